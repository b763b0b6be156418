"""What the encoder's entries and the three fused decode entries of the C-ABI answer to a fixed table of calls
(tests/fused_entry_table.py): status, message and -- for a call that succeeds -- the SHA-256 of everything it wrote, equal to
tests/golden/fused_entry_errors.json, which tools/gen/record_fused_entry_errors.py recorded from the commit before the encoder's host
layer got its one pixel source, one transform core and one file-encode driver.  The order of an entry's checks is observable (which
of two bad arguments is named), and so is what a forwarded call says; this pins both, and the bytes.  The null-context half needs no GPU."""
import json
from pathlib import Path

import pytest

import fused_entry_table as T

FIXTURE = Path(__file__).resolve().parent / "golden" / "fused_entry_errors.json"


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())


def _compare(got, want):
    assert [(r["entry"], r["case"]) for r in got] == [(r["entry"], r["case"]) for r in want], \
        "the table and the fixture list different calls: record the fixture again from the parent build"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} calls answer differently; the first: got {wrong[0][0]}, recorded {wrong[0][1]}"


def test_null_context_half(J, recorded):
    _compare(T.Env(J).record("null_context"), recorded["null_context"])


@pytest.mark.gpu
def test_real_context_half(J, recorded):
    ctx = J.Context(0)
    try:
        _compare(T.Env(J, ctx._h).record("real_context"), recorded["real_context"])
    finally:
        ctx.close()


def test_the_table_covers_every_entry(J, recorded):
    """every entry refuses at least once and succeeds at least once (with a context), every succeeding call has its bytes pinned, and
    api.ABI names no transform-encode or file-encode entry the table lacks"""
    assert len(T.ENTRIES) == 15 and len(set(T.ENTRIES)) == 15
    for half in ("null_context", "real_context"):
        keys = [(e, c) for e, c, _ in T.table(half)]
        assert len(set(keys)) == len(keys), f"{half}: a case is listed twice"
        assert keys == [(r["entry"], r["case"]) for r in recorded[half]], half
    assert all(r["status"] < 0 for r in recorded["null_context"])
    for r in recorded["real_context"]:
        assert (r["status"] >= 0) == ("sha256" in r), r
        if r["case"].startswith("ok"):
            assert r["status"] >= 0, r
    for e in T.ENTRIES:
        assert any(r["entry"] == e and r["status"] < 0 for r in recorded["real_context"]), f"{e}: no refusing case"
        assert any(r["entry"] == e and r["status"] >= 0 for r in recorded["real_context"]), f"{e}: no succeeding case"
    names = {n for n, _, _ in J.api.ABI}
    for name in names:
        if name.startswith("jpezy_fdct_quant") or name.startswith("jpezy_encode_jpeg"):
            assert name[len("jpezy_"):] in T.ENTRIES, f"{name} is an encode entry of the ABI that the table does not drive"
    assert all("jpezy_" + e in names for e in T.ENTRIES)
