"""jpezy_decode --scale=N: the reduced picture as a P3 file whose header is the scaled size and whose pixels are the model's
(tests/scaled_model.py); a denominator outside 1, 2, 4, 8 is the usage error."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import scaled_model as M

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


def test_bad_scale_is_the_usage_error(dec, tmp_path):
    for opt in (["--scale=3"], ["--gray", "--scale=0"], ["--scale=16", "--gray"], ["--scale="], ["--scale=4x"]):
        p = _run(dec, tmp_path / "x.jpg", tmp_path / "y.ppm", *opt)
        assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode <input.(jpg | jpeg)>"), opt
        assert "--scale" in p.stderr and "by roki" not in p.stdout and not (tmp_path / "y.ppm").exists()


@pytest.mark.gpu
def test_scaled_ppm(dec, oracle, tmp_path):
    import jpezy_amd as J
    W, H = 100, 37
    r, g, b = oracle.synth_rgb(W, H, frame=21)
    data = oracle.encode_jpeg(r, g, b, W, H)
    jpg = tmp_path / "x.jpg"
    jpg.write_bytes(data)
    info, co = J.read_jpeg(data)
    ws, hs = M.scaled_size(W, H, 4)
    for opts, gray in ((["--scale=4"], False), (["--scale=4", "--gray"], True), (["--gray", "--scale=4"], True)):
        ppm = tmp_path / "y.ppm"
        p = _run(dec, jpg, ppm, *opts)
        assert p.returncode == 0, p.stderr
        want = M.decode_planes(co, info, 4, gray)
        assert ppm.read_bytes() == oracle.format_ppm_p3(ws, hs, *want)
        assert f"Loaded JPEG: {W}x{H}, presicion 8" in p.stdout
        assert f"Decoded image: Netpbm image data, size = {ws} x {hs}, pixmap, ASCII text" in p.stdout
    p = _run(dec, jpg, tmp_path / "z.ppm", "--scale=1")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "z.ppm").read_bytes() == oracle.format_ppm_p3(W, H, *oracle.decode_jpeg(data, False)[1:])
