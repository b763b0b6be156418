"""jpezy_tran in.jpg out.jpg (--rotate=90|180|270 | --flip=h|v | --transpose | --transverse | --none) [--trim] [--optimize] [--restart=N]:
exactly one operation, anything else is the usage error (exit 1, nothing loaded, no file written); on the GPU the output is
Context.transform_jpeg's, and a file the library refuses prints its reason."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "jpezy_amd" / "bin"

OPTIONS = ["--none", "--flip=h", "--flip=v", "--transpose", "--transverse", "--rotate=90", "--rotate=180", "--rotate=270"]      # by XFORM_* value


@pytest.fixture(scope="module")
def tran():
    from jpezy_amd import _build
    _build.build_all()
    exe = BIN / "jpezy_tran"
    assert exe.exists()
    return exe


def _run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_argument_rules(tran, tmp_path):
    src, dst = tmp_path / "x.jpg", tmp_path / "y.jpg"
    bad = [
        [],                                                               # no operation
        ["--trim"], ["--optimize", "--restart=4"],
        ["--rotate=90", "--flip=h"], ["--none", "--none"], ["--transpose", "--transverse"], ["--rotate=90", "--rotate=90"],    # two operations
        ["--rotate=45"], ["--rotate="], ["--rotate=90x"], ["--rotate"], ["--flip=x"], ["--flip="], ["--flip=hv"], ["--flip"],     # bad values
        ["--none", "--restart=65536"], ["--none", "--restart=-1"], ["--none", "--restart="], ["--none", "--restart=4k"],
        ["--none", "--trim", "--trim"], ["--none", "--optimize", "--optimize"], ["--none", "--restart=1", "--restart=2"],
        ["--none", "--gray"], ["--nonesuch"], ["--none", "--trim", "--optimize", "--restart=3", "--trim"],
    ]
    for opts in bad:
        p = _run(tran, src, dst, *opts)
        assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_tran <input.(jpg | jpeg)> <output.(jpg | jpeg)>"), (opts, p.stderr)
        assert "by roki" not in p.stdout and not dst.exists(), opts
    for names in ((tmp_path / "x.ppm", dst), (src, tmp_path / "y.ppm")):
        p = _run(tran, *names, "--none")
        assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_tran")
    p = _run(tran)
    assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_tran")


@pytest.mark.gpu
@pytest.mark.parametrize("op", range(8))
def test_cli_writes_what_the_library_writes(tran, oracle, tmp_path, op):
    import jpezy_amd as J
    W, H = 48, 32
    ctx = J.Context(0)
    try:
        data = ctx.encode_jpeg(*oracle.synth_rgb(W, H, frame=11), W, H)
        src, dst = tmp_path / "x.jpg", tmp_path / "y.jpg"
        src.write_bytes(data)
        want, info = ctx.transform_jpeg(data, op)
        p = _run(tran, src, dst, OPTIONS[op])
        assert p.returncode == 0, p.stderr
        assert dst.read_bytes() == want
        assert f"Transformed image: JPEG image data, size = {info.width} x {info.height}, {len(want)} bytes" in p.stdout and "by roki" in p.stdout
        if op == J.XFORM_ROT90:                                           # the options reach the context; a refused file prints the reason
            ctx.set_huffman_optimize(True)
            ctx.set_restart_interval(2)
            want, _ = ctx.transform_jpeg(data, op)
            p = _run(tran, src, dst, "--optimize", OPTIONS[op], "--restart=2")
            assert p.returncode == 0 and dst.read_bytes() == want, p.stderr
            ctx.set_huffman_optimize(False)
            ctx.set_restart_interval(0)
            part, out = tmp_path / "p.jpg", tmp_path / "q.jpg"
            part.write_bytes(ctx.encode_jpeg(*oracle.synth_rgb(40, 24, frame=1), 40, 24))
            p = _run(tran, part, out, OPTIONS[op])
            assert p.returncode == 1 and "height" in p.stderr and "Usage" not in p.stderr and not out.exists(), p.stderr
            p = _run(tran, part, out, OPTIONS[op], "--trim")
            assert p.returncode == 0 and out.read_bytes() == ctx.transform_jpeg(part.read_bytes(), op, trim=True)[0], p.stderr
    finally:
        ctx.close()
