"""The constructions of tests/huffdec_seams_model.py, proved without a device: every file the GPU test
(tests/test_gpu_huffdec_seams.py) decodes lands where it says, its entropy-coded segment is the model's stream with the 0xFF00
stuffing put in, and the host decoder returns exactly the coefficients it was built from."""
import numpy as np
import pytest

import huffdec_seams_model as S


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def test_geometry_constants_are_the_ones_the_constructions_were_written_for():
    assert S.read_geometry() == S.EXPECTED_GEOMETRY


def test_symbol_table_against_entropy_model():
    """the model's stream of an own-layout frame is entropy_model's, and the state it reports is the one a walk arrives in"""
    b = S.Builder(S.LAYOUTS["own420"], seed=2)
    b.noise_blocks(60)
    co = np.stack(b.blocks).reshape(-1, 6, 64)
    assert b.stream() == S.M.unstuffed_stream(co, pad_bit=S.PAD_BIT)
    sym = S.symbol_starts(co, b.L)
    assert sym.starts == b.starts and sym.recs == b.recs and sym.total_bits == int(S.M.block_lengths(co).sum())
    ends = np.cumsum(S.M.block_lengths(co))
    for pos in (0, 1, 517, 1024, 2048, int(ends[10]), int(ends[10]) - 1, sym.total_bits):
        p, blk, k, done = sym.state_at(pos)
        assert done == int(np.searchsorted(ends, pos + p, side="right"))
        assert pos + p in sym.starts + [sym.total_bits]
        if k == 0:
            assert pos + p in [0] + ends.tolist() and done == ([0] + ends.tolist()).index(pos + p) and blk == done % 6
    assert S.stuffed(b"\x01\xff\xff\x02") == b"\x01\xff\x00\xff\x00\x02"
    assert [S.removed_before(b"\x01\xff\xff\x02", q) for q in range(7)] == [0, 0, 0, 1, 1, 2, 2]


def _recheck(c):
    """the landings once more, from a symbol table built afresh from the coefficients"""
    sym = S.symbol_starts(c.coeffs, c.layout, zrl_blocks=getattr(c, "zrl_blocks", ()))
    assert sym.total_bits == c.total_bits
    aimed = [l for l in c.landed if "boundary" in l]
    for l in aimed:
        again = S.check_landing(sym, l["kind"], l["boundary"], l["amount"], l["nbits"], l["symbol"], c.layout.bpm)
        assert again == l
    return len(aimed)


@pytest.mark.parametrize("name", list(S.REGISTRY))
def test_construction(J, name):
    c = S.case(name)
    data = S.file_of(J, name)
    assert c.landed, "a construction says where it landed"
    if isinstance(c, S.Case):
        n = _recheck(c)
        if S.REGISTRY[name][1] is S.straddle_for:
            assert n == len(c.landed) >= 2
            assert ("own" in name) == (c.layout.writer != "synth")
            bk = name.split("-")[0]
            for l in c.landed:
                sub, rem = divmod(l["boundary"], S.SUBSEQ_BITS)
                assert {"interior": rem == 0 and sub % S.EMIT_SUBS != 0, "quarter": rem in (S.PART_BITS, 2 * S.PART_BITS, 3 * S.PART_BITS),
                        "emit_wg": rem == 0 and sub % S.EMIT_SUBS == 0 and sub % S.WGS != 0, "sync_wg": rem == 0 and sub % S.WGS == 0}[bk], l
        assert S.entropy_segment(data) == S.stuffed(c.stream)
    elif isinstance(c, S.RestartCase):
        assert S.entropy_segment(data) == c.segment()
    info, co = J.read_jpeg(data)
    assert (info.width, info.height, info.blocks_per_mcu) == (c.W, c.H, c.layout.bpm)
    assert np.array_equal(co.reshape(c.coeffs.shape), c.coeffs)


def test_every_pair_lands_on_every_kind_of_boundary():
    """interior and quarter files hold every (kind, amount) of their layout; at the two workgroup seams the five Annex-K files
    together hold seam_pairs() -- the 26-bit symbol at every amount, every kind -- and the two wide-table files every amount of the
    31-bit symbol"""
    for bk in S.BOUNDARY_KINDS:
        seen = {}
        for lay in S.STRADDLE_LAYOUTS:
            seen[lay] = {(l["kind"], l["amount"]) for l in S.case(f"{bk}-{lay}").landed}
            if bk in ("interior", "quarter"):
                assert seen[lay] == set(S.kind_amounts(lay)), (bk, lay)
        if bk in ("emit_wg", "sync_wg"):
            annex = sorted(p for l in S.ANNEX_LAYOUTS for p in seen[l])
            assert annex == sorted(S.seam_pairs()), bk
            assert {a for k, a in annex if k == "ac"} == set(range(26))
            assert {a for k, a in annex if k == "eob"} == set(range(4)) and {a for k, a in annex if k == "zrl"} == set(range(11))
            assert all(seen[l] for l in S.ANNEX_LAYOUTS)
            if bk == "sync_wg":          # every kind where the table sequence has a period (b wraps at the end of an MCU)
                assert {k for k, a in seen["own420"]} == set(S.TARGET_KINDS) == {k for k, a in seen["s444"]}
                last = [l for l in S.case("sync_wg-own420").landed if l["kind"].startswith("mcu_last")]
                assert len(last) == 2 and all(l["block"] % 6 == 5 and l["state"][1:] == (0, 0) for l in last), last      # b wraps 5 -> 0
            assert {a for k, a in seen["wide444"] | seen["long_one"] if k == "ac"} == set(range(31))
    assert {l["nbits"] for l in S.case("interior-wide444").landed if l["kind"] in ("ac", "dc")} == {31}


def test_light_filler_finds_the_mcu_phase_within_one_subsequence():
    """the model of the speculation walk behind two choices of the builders: with the light filler of the period-6 layouts fewer than
    half of the lanes start wrong even at a speculation distance of one subsequence (blocks of 100 bits and more: more than half,
    which scan_hopeless hands to the host decoder), and the flat frame of the exception table keeps nearly every lane in a wrong parse"""
    L = S.LAYOUTS["own420"]
    light = S.Builder(L, seed=3)
    light.noise_to(60 * S.SUBSEQ_BITS)
    heavy = S.Builder(L, seed=3)
    heavy.light = False
    heavy.noise_to(60 * S.SUBSEQ_BITS)
    miss = [float(S.speculation_misses(b.stream(), L, b.symbols(), overflow=1).mean()) for b in (light, heavy)]
    print("lanes that start wrong at distance 1: light filler %.2f, blocks of 150 bits %.2f" % tuple(miss))
    assert miss[0] < 0.35 and miss[1] > 0.5, miss
    flat = S.FlatCase(W=2032, H=128)
    sym = S.symbol_starts(flat.coeffs, L)
    stream = S.M.unstuffed_stream(flat.coeffs, pad_bit=S.PAD_BIT)
    # (the first OVERFLOW_DEFAULT + 1 lanes start from the scan's own start state, not from a guess)
    assert S.speculation_misses(stream, L, sym)[S.OVERFLOW_DEFAULT + 1:].mean() > 0.9


def test_refused_zrl_is_refused_by_the_host_decoder(J):
    c = S.zrl_case(65)
    with pytest.raises(J.JpezyError):
        J.read_jpeg(S.raw_file(c))


@pytest.mark.parametrize("nmcu", [S.DC_PASS_MCUS[0], S.DC_PASS_MCUS[-1]])
def test_dc_pass_files(J, nmcu):
    data, co = S.dc_pass_file(nmcu)
    assert (np.diff(co[:, 4, 0].astype(np.int64)) != 0).all()
    sym = S.symbol_starts(co, S.Layout("420", S.YUV420))
    assert sym.nblocks == 6 * nmcu
    info, back = J.read_jpeg(data)
    assert np.array_equal(back.reshape(co.shape), co)
