"""What every decode entry of the C-ABI answers to a fixed table of calls (tests/decode_entry_table.py): status and message, equal to
tests/golden/decode_entry_errors.json, which tools/gen/record_decode_entry_errors.py recorded from the commit before the host layer got
its one driver.  The order of an entry's checks is observable (which of two bad arguments is named), and so is what a forwarded call
says; this pins both.  The null-context half needs no GPU."""
import json
from pathlib import Path

import pytest

import decode_entry_table as T

FIXTURE = Path(__file__).resolve().parent / "golden" / "decode_entry_errors.json"


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def recorded():
    return json.loads(FIXTURE.read_text())


def _compare(got, want):
    assert [(r["entry"], r["file"], r["case"]) for r in got] == [(r["entry"], r["file"], r["case"]) for r in want], \
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


def test_the_table_covers_every_decode_entry(J, recorded):
    """every entry refuses at least once and succeeds at least once (with a context), and api.ABI names no decode entry the table lacks"""
    assert len(T.ENTRIES) == 17
    for half in ("null_context", "real_context"):
        assert [(e, f, c) for e, f, c, _ in T.table(half)] == [(r["entry"], r["file"], r["case"]) for r in recorded[half]], half
    rows = recorded["null_context"] + recorded["real_context"]
    for e in T.ENTRIES:
        assert any(r["entry"] == e and r["status"] < 0 for r in rows), f"{e}: no refusing case"
        assert any(r["entry"] == e and r["status"] == 0 and r["case"].startswith("ok") for r in recorded["real_context"]), f"{e}: no succeeding case"
    for name, _, _ in J.api.ABI:
        decode_entry = name.startswith("jpezy_decode_jpeg") or (name.startswith("jpezy_dequant_idct_") and name.endswith("_dev"))
        if decode_entry and name not in T.NOT_IN_TABLE:
            assert name[len("jpezy_"):] in T.ENTRIES, f"{name} is a decode entry of the ABI that the table does not drive"
    assert all("jpezy_" + e in {n for n, _, _ in J.api.ABI} for e in T.ENTRIES)
