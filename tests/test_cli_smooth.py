"""jpezy_decode --upsampling=smooth|nearest, the rules that need no GPU: a malformed value is the usage error, smooth together with
--scale= other than 1, --region= or --i420 is one rule line without usage text, and neither writes a file.  tests/test_gpu_smooth.py
decodes with it."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "jpezy_amd" / "bin"
RULE = "--upsampling=smooth writes whole pictures at full size"


@pytest.fixture(scope="module")
def dec():
    from jpezy_amd import _build
    _build.build_all()
    exe = BIN / "jpezy_decode"
    assert exe.exists()
    return exe


def _run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_malformed_upsampling_is_the_usage_error(dec, tmp_path):
    out = tmp_path / "y.ppm"
    for form in ("--upsampling=", "--upsampling=fancy", "--upsampling=smoothx", "--upsampling=Smooth", "--upsampling=1"):
        for opts in ([form], ["--gray", form], [form, "--scale=2"], ["--scale=2", "--gray", form]):
            p = _run(dec, tmp_path / "x.jpg", out, *opts)
            assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode <input.(jpg | jpeg)>"), opts
            assert "--upsampling=(smooth | nearest)" in p.stderr and "by roki" not in p.stdout and not out.exists()
    p = _run(dec, "--i420", tmp_path / "x.jpg", tmp_path / "y.yuv", "--upsampling=fancy")
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode <input.(jpg | jpeg)>") and not (tmp_path / "y.yuv").exists()


def test_usage_text_keeps_its_beginning(dec, tmp_path):
    p = _run(dec, tmp_path / "x.jpg")
    assert p.returncode == 1
    assert p.stderr.startswith("Usage: jpezy_decode <input.(jpg | jpeg)> ( <output.ppm | [OPT: --gray]> | -v ) [OPT: --scale=(1 | 2 | 4 | 8)] "
                               "[OPT: --region=WxH+X+Y]")
    assert p.stderr.rstrip().endswith("[OPT: --upsampling=(smooth | nearest)]")


def test_cli_upsampling_rules(dec, tmp_path):
    out = tmp_path / "y.ppm"
    for opts in (["--upsampling=smooth", "--scale=2"], ["--scale=8", "--upsampling=smooth"], ["--gray", "--scale=4", "--upsampling=smooth"],
                 ["--upsampling=smooth", "--region=4x4+0+0"], ["--region=4x4+0+0", "--upsampling=smooth", "--scale=2"],
                 ["--region=4x4+0+0", "--scale=1", "--upsampling=smooth"]):
        p = _run(dec, tmp_path / "x.jpg", out, *opts)
        assert p.returncode == 1 and RULE in p.stderr and "Usage" not in p.stderr and not out.exists(), opts
        assert p.stderr.count("\n") == 1 and "by roki" not in p.stdout
    yuv = tmp_path / "y.yuv"
    p = _run(dec, "--i420", tmp_path / "x.jpg", yuv, "--upsampling=smooth")
    assert p.returncode == 1 and RULE in p.stderr and "Usage" not in p.stderr and not yuv.exists()
    # nearest is the default and combines with everything: these get past the rules (and fail on the missing file)
    for opts in (["--upsampling=nearest", "--scale=2"], ["--upsampling=nearest", "--region=4x4+0+0"], ["--upsampling=smooth", "--scale=1"],
                 ["--upsampling=smooth", "--gray"]):
        p = _run(dec, tmp_path / "x.jpg", out, *opts)
        assert p.returncode == 1 and RULE not in p.stderr and "Usage" not in p.stderr and not out.exists(), opts
