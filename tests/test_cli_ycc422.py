"""jpezy_encode --yuy2=WxH | --uyvy=WxH and jpezy_decode --yuy2 | --uyvy (raw packed YCbCr 4:2:2, ffmpeg's rawvideo yuyv422 / uyvy422):
the combinations that are usage errors need no GPU; the files the two write are compared with the library's own entries on one."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ycc422_model as M

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "jpezy_amd" / "bin"


@pytest.fixture(scope="module")
def exes():
    from jpezy_amd import _build
    _build.build_all()
    assert (BIN / "jpezy_encode").exists() and (BIN / "jpezy_decode").exists()
    return BIN / "jpezy_encode", BIN / "jpezy_decode"


def _run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flag", ["--yuy2", "--uyvy"])
@pytest.mark.parametrize("opt", ["--gray", "--sampling=422", "--sampling=420", "--sampling=444", "--chroma=average", "--chroma=point", "--i420=2x2",
                                 "--scale=2", "--gpus", "--quality=0", "--restart=x", "--yuy2=2x2"])
def test_encode_combinations_are_usage_errors(exes, tmp_path, flag, opt):
    enc, _ = exes
    yuv, out = tmp_path / "x.yuv", tmp_path / "y.jpg"
    yuv.write_bytes(bytes(4 * 2))
    p = _run(enc, f"{flag}=2x2", yuv, out, opt)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode --yuy2=WxH | --uyvy=WxH") and not out.exists()
    p = _run(enc, f"{flag}=2x2", yuv, out, "--optimize", opt)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists()


@pytest.mark.parametrize("dims", ["", "2", "2x", "x2", "0x2", "2x65536", "axb"])
def test_encode_malformed_sizes_are_usage_errors(exes, tmp_path, dims):
    enc, _ = exes
    yuv, out = tmp_path / "x.yuv", tmp_path / "y.jpg"
    yuv.write_bytes(bytes(8))
    p = _run(enc, f"--uyvy={dims}", yuv, out)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists()


@pytest.mark.parametrize("flag", ["--yuy2", "--uyvy"])
@pytest.mark.parametrize("opt", ["--gray", "--scale=2", "--region=1x1+0+0", "--upsampling=smooth", "--upsampling=nearest", "--orient", "--i420", "-v"])
def test_decode_combinations_are_usage_errors(exes, tmp_path, flag, opt):
    _, dec = exes
    out = tmp_path / "y.yuv"
    p = _run(dec, flag, tmp_path / "x.jpg", out, opt)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode --yuy2 | --uyvy") and not out.exists()
    p = _run(dec, flag, tmp_path / "x.jpg")
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode") and not out.exists()


def test_the_old_usage_texts_and_rules_stand(exes, tmp_path):
    enc, dec = exes
    assert _run(enc).stderr.startswith("Usage: jpezy_encode <input.ppm>")
    assert _run(dec).stderr.startswith("Usage: jpezy_decode")
    ppm, out = tmp_path / "x.ppm", tmp_path / "y.jpg"
    ppm.write_text("P3\n2 2\n255\n" + "1 2 3 " * 4 + "\n")
    p = _run(enc, ppm, out, "--sampling=422")
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists()


@pytest.mark.gpu
@pytest.mark.parametrize("flag,fmt", [("--yuy2", M.YUY2), ("--uyvy", M.UYVY)])
def test_round_trip_equals_the_library(exes, tmp_path, flag, fmt):
    import jpezy_amd as J
    enc, dec = exes
    W, H = 37, 19
    img = M.pack(*M.random_planes(W, H), fmt, fill=0)
    yuv, jpg, back = tmp_path / "in.yuv", tmp_path / "out.jpg", tmp_path / "back.yuv"
    yuv.write_bytes(img.tobytes())
    p = _run(enc, f"{flag}={W}x{H}", yuv, jpg, "--optimize", "--restart=3", "--quality=90")
    assert p.returncode == 0, p.stderr
    ctx = J.Context(0)
    try:
        ctx.set_huffman_optimize(1)
        ctx.set_restart_interval(3)
        ctx.set_quality(90)
        assert jpg.read_bytes() == ctx.encode_jpeg_yuv422(img, W=W, format=fmt)
        p = _run(dec, flag, jpg, back)
        assert p.returncode == 0, p.stderr
        want = ctx.decode_jpeg_yuv422(jpg.read_bytes(), format=fmt)[1]
        assert np.array_equal(np.frombuffer(back.read_bytes(), np.uint8).reshape(H, M.row_bytes(W)), want)
    finally:
        ctx.close()
    short = tmp_path / "short.yuv"
    short.write_bytes(img.tobytes()[:-1])
    p = _run(enc, f"{flag}={W}x{H}", short, tmp_path / "no.jpg")
    assert p.returncode == 1 and "must hold" in p.stderr and not (tmp_path / "no.jpg").exists()
