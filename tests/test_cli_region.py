"""jpezy_decode --region=WxH+X+Y: the window as a P3 file whose header is w x h and whose pixels are the model's slice
(tests/region_model.py); a malformed geometry is the usage error, a well-formed one outside the picture exits 1 with the library's
message; neither writes a file."""
import subprocess
from pathlib import Path

import pytest

import region_model as R

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "jpezy_amd" / "bin"


@pytest.fixture(scope="module")
def dec():
    from jpezy_amd import _build
    _build.build_all()
    exe = BIN / "jpezy_decode"
    assert exe.exists()
    return exe


def _run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_malformed_region_is_the_usage_error(dec, tmp_path):
    forms = ["--region=", "--region=10x10", "--region=10x10+1", "--region=0x5+0+0", "--region=-3x4+0+0", "--region=10x10+1+2junk",
             "--region=10x10+1+2+3", "--region=10X10+1+2", "--region=x10+1+2", "--region=10x10+-1+2"]
    for form in forms:
        for opts in ([form], ["--gray", form], [form, "--scale=2"], ["--scale=2", "--gray", form]):
            p = _run(dec, tmp_path / "x.jpg", tmp_path / "y.ppm", *opts)
            assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode <input.(jpg | jpeg)>"), opts
            assert "--region=WxH+X+Y" in p.stderr and "by roki" not in p.stdout and not (tmp_path / "y.ppm").exists()
    p = _run(dec, tmp_path / "x.jpg", tmp_path / "y.ppm", "--gray", "--scale=2", "--region=1x1+0+0", "--gray")      # one argument too many
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode <input.(jpg | jpeg)>") and not (tmp_path / "y.ppm").exists()


@pytest.mark.gpu
def test_region_ppm(dec, oracle, tmp_path):
    """100 x 37: 40x20+33+9 lies inside the full-size picture and outside the half-size one (50 x 19), where 20x10+16+4 is used"""
    import jpezy_amd as J
    W, H = 100, 37
    r, g, b = oracle.synth_rgb(W, H, frame=21)
    data = oracle.encode_jpeg(r, g, b, W, H)
    jpg = tmp_path / "x.jpg"
    jpg.write_bytes(data)
    info, co = J.read_jpeg(data)
    full, half = "--region=40x20+33+9", "--region=20x10+16+4"
    cases = [([full], (33, 9, 40, 20), 1, False), ([full, "--gray"], (33, 9, 40, 20), 1, True), (["--gray", full], (33, 9, 40, 20), 1, True),
             ([half, "--scale=2"], (16, 4, 20, 10), 2, False), (["--scale=2", half], (16, 4, 20, 10), 2, False),
             (["--scale=2", "--gray", half], (16, 4, 20, 10), 2, True), ([half, "--scale=2", "--gray"], (16, 4, 20, 10), 2, True),
             (["--gray", half, "--scale=2"], (16, 4, 20, 10), 2, True), (["--region=100x37+0+0"], (0, 0, 100, 37), 1, False),
             (["--scale=8", "--region=1x1+12+4"], (12, 4, 1, 1), 8, False)]
    for opts, region, scale, gray in cases:
        ppm = tmp_path / "y.ppm"
        p = _run(dec, jpg, ppm, *opts)
        assert p.returncode == 0, (opts, p.stderr)
        want = R.decode_region(co, info, region, scale, gray)
        assert len({a.tobytes() for a in want}) == (1 if gray else 3) or region[2] == 1
        assert ppm.read_bytes() == oracle.format_ppm_p3(region[2], region[3], *(a.reshape(-1) for a in want)), opts
        assert f"Loaded JPEG: {W}x{H}, presicion 8" in p.stdout
        assert f"Decoded image: Netpbm image data, size = {region[2]} x {region[3]}, pixmap, ASCII text" in p.stdout
        ppm.unlink()
    for opts, named in (([full, "--scale=2"], "40x20+33+9"), (["--scale=2", "--gray", full], "50 x 19"), (["--region=1x1+100+0"], "1x1+100+0"),
                        (["--region=100x38+0+0"], "100 x 37")):
        p = _run(dec, jpg, tmp_path / "z.ppm", *opts)
        assert p.returncode == 1 and named in p.stderr and "Usage" not in p.stderr, (opts, p.stderr)
        assert not (tmp_path / "z.ppm").exists()
