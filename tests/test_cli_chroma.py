"""jpezy_encode --chroma=average|point: the rules that need no GPU -- the spellings that are usage errors, and the combinations that the
one-line rule refuses (exit 1, no usage text, no output file).  What the flag writes is tests/test_gpu_chroma_average.py's."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "jpezy_amd" / "bin"
RULE = "--chroma=average averages the 4:2:0 chroma of colour files from RGB input on one GPU"


@pytest.fixture(scope="module")
def enc():
    from jpezy_amd import _build
    _build.build_all()
    exe = BIN / "jpezy_encode"
    assert exe.exists()
    return exe


@pytest.fixture
def files(tmp_path):
    ppm = tmp_path / "x.ppm"
    ppm.write_text("P3\n2 2\n255\n" + "1 2 3 " * 4 + "\n")
    yuv = tmp_path / "x.yuv"
    yuv.write_bytes(bytes(6))
    return ppm, yuv, tmp_path / "y.jpg"


def _run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("form", ["--chroma=", "--chroma=avg", "--chroma=Average", "--chroma=averagex"])
def test_other_spellings_are_the_usage_error(enc, files, form):
    ppm, yuv, out = files
    p = _run(enc, ppm, out, form)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists()
    p = _run(enc, ppm, out, "--quality=90", form)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists()
    p = _run(enc, "--i420=2x2", yuv, out, form)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists()
    p = _run(enc, "--gpus", 1, form, ppm, out)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists()


@pytest.mark.parametrize("opts", [["--gray", "--chroma=average"], ["--chroma=average", "--gray"], ["--optimize", "--gray", "--chroma=average"],
                                  ["--sampling=444", "--chroma=average"], ["--chroma=average", "--sampling=444"],
                                  ["--chroma=average", "--quality=90", "--sampling=444"]])
def test_average_is_refused_with_gray_and_444(enc, files, opts):
    ppm, _, out = files
    p = _run(enc, ppm, out, *opts)
    assert p.returncode == 1 and RULE in p.stderr and "Usage" not in p.stderr and not out.exists()
    assert len(p.stderr.strip().splitlines()) == 1


def test_average_is_refused_with_i420_and_several_gpus(enc, files):
    ppm, yuv, out = files
    for cmd in ([enc, "--i420=2x2", yuv, out, "--chroma=average"], [enc, "--i420=2x2", yuv, out, "--quality=90", "--chroma=average"],
                [enc, "--gpus", 2, "--chroma=average", ppm, out], [enc, "--gpus", 1, "--gray", "--chroma=average", ppm, out],
                [enc, "--gpus", 1, "--sampling=444", "--chroma=average", ppm, out]):
        p = _run(*cmd)
        assert p.returncode == 1 and RULE in p.stderr and "Usage" not in p.stderr and not out.exists(), cmd[1:]


def test_the_rules_of_444_stand(enc, files):
    """--chroma=point beside a refused --sampling=444 combination changes nothing: the sampling rule speaks"""
    ppm, _, out = files
    p = _run(enc, ppm, out, "--gray", "--sampling=444", "--chroma=point")
    assert p.returncode == 1 and "--sampling=444 writes colour files from RGB input on one GPU" in p.stderr and not out.exists()
    # a PPM output takes no codec flag: the usage error, as for --sampling=444
    p = _run(enc, ppm, out.with_suffix(".ppm"), "--chroma=average")
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode")
