"""The workgroup forms of the f32 encode launch for planar frames (jpezy_ctx_set_encode_groups): {4 waves, cooperative 256-byte row
pieces}, {2 waves, cooperative 128-byte row pieces}, {2 waves, direct loads}.  Every legal form of a frame, forced, must give the
CPU oracle's coefficients bit for bit -- and therefore each other's -- at the smallest shapes where the two-wave cooperative load can
go wrong: one full group, a group whose second wave has no quad, an odd quad count, replicated bottom rows, clamped pieces, the
30-quad row of a 1920-wide frame, several frames with padding between them, the rare paths forced.  A form that is not legal for a
frame is refused with JPEZY_E_BADARG and launches nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BADARG = -1


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()       # fails loudly if the extension is missing
    return jpezy_amd


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)               # encode variant 1 (the default): the only launch the setting acts on
    yield c
    c.close()


@pytest.fixture(scope="module")
def forms(J):
    return {"4coop": J.ENCODE_GROUPS_4_COOP, "2coop": J.ENCODE_GROUPS_2_COOP, "2direct": J.ENCODE_GROUPS_2_DIRECT, "auto": J.ENCODE_GROUPS_AUTO}


def legal(W, H, name):
    """include/jpezy_hip.h: the cooperative forms need W % 16 == 0 (the host entry stages into aligned planes), four waves also a row
    of quads that divides by four"""
    quads = ((W + 15) // 16 + 3) // 4
    return {"4coop": W % 16 == 0 and quads % 4 == 0, "2coop": W % 16 == 0, "2direct": True, "auto": True}[name]


# the issue's shapes, then two where the four-wave form is legal too (one group; three groups with a replicated bottom band) and one
# whose last quad holds a single MCU (208 = 13 MCUs: pieces clamped inside the last group)
SHAPES = [(128, 16), (64, 16), (192, 16), (320, 24), (128, 8), (1920, 32), (256, 16), (768, 24), (208, 16)]

_cache = {}


def case(oracle, W, H, gray):
    """(pixels, oracle coefficients) of a shape, computed once"""
    key = (W, H, gray)
    if key not in _cache:
        r, g, b = oracle.synth_rgb(W, H, frame=W * 1000 + H + 26)
        _cache[key] = ((r, g, b), oracle.encode_coeffs(r, g, b, W, H, gray))
    return _cache[key]


@pytest.mark.parametrize("gray", [False, True], ids=["colour", "gray"])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_legal_form_matches_the_oracle(J, ctx, forms, oracle, size, gray):
    W, H = size
    (r, g, b), want = case(oracle, W, H, gray)
    ran = []
    try:
        for name, form in forms.items():
            if not legal(W, H, name):
                continue
            ctx.set_encode_groups(form)
            assert ctx.encode_groups() == form
            got = ctx.fdct_quant(r, g, b, W, H, gray=gray)
            assert got.shape == want.shape and np.array_equal(got, want), f"{name} differs from the oracle at {W}x{H} gray={gray}"
            ran.append(name)
    finally:
        ctx.set_encode_groups(J.ENCODE_GROUPS_AUTO)
    assert {"2coop", "2direct", "auto"} <= set(ran)


@pytest.mark.parametrize("gray", [False, True], ids=["colour", "gray"])
def test_frames_with_padding_between_them(J, ctx, forms, oracle, gray):
    """n_frames = 2 on the device entry with plane_stride > W * H: the second frame's rows lie behind padding, which no form reads
    into the picture (the padding holds 0xA5, the clamped rows and pieces must come from the frame)"""
    import torch
    W, H, F = 192, 24, 2
    stride = W * H + 4096 + 16
    frames = [oracle.synth_rgb(W, H, frame=2600 + f) for f in range(F)]
    want = np.stack([oracle.encode_coeffs(*fr, W, H, gray) for fr in frames])
    dev = torch.device("cuda", 0)
    d = []
    for k in range(3):
        t = torch.full((F * stride,), 0xA5, dtype=torch.uint8, device=dev)
        t.view(F, stride)[:, : W * H] = torch.from_numpy(np.stack([fr[k] for fr in frames])).to(dev)
        d.append(t)
    try:
        for name in ("2coop", "2direct", "auto"):
            ctx.set_encode_groups(forms[name])
            dco = torch.zeros(F * J.coeff_count(W, H, gray), dtype=torch.int16, device=dev)
            ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, dco, gray=gray, n_frames=F, plane_stride=stride)
            torch.cuda.synchronize()
            assert np.array_equal(dco.cpu().numpy().reshape(want.shape), want), name
    finally:
        ctx.set_encode_groups(J.ENCODE_GROUPS_AUTO)


@pytest.mark.parametrize("force", [1, 2, 3])
def test_forced_rare_paths_in_every_form(J, ctx, forms, oracle, force):
    """force_exact on: the forms differ in the pixel load alone, so the rare paths behind it must see the same pixels"""
    try:
        ctx.set_force_exact(force)
        for (W, H) in ((192, 16), (256, 16)):
            for gray in (False, True):
                (r, g, b), want = case(oracle, W, H, gray)
                for name, form in forms.items():
                    if legal(W, H, name):
                        ctx.set_encode_groups(form)
                        assert np.array_equal(ctx.fdct_quant(r, g, b, W, H, gray=gray), want), (name, W, H, gray, force)
    finally:
        ctx.set_force_exact(0)
        ctx.set_encode_groups(J.ENCODE_GROUPS_AUTO)


def test_illegal_forms_are_refused(J, ctx, forms, oracle):
    lib = J.load_library()
    assert lib.jpezy_ctx_set_encode_groups(ctx._h, 4) == BADARG and lib.jpezy_ctx_set_encode_groups(ctx._h, -1) == BADARG
    assert lib.jpezy_ctx_set_encode_groups(None, 0) == BADARG and lib.jpezy_ctx_encode_groups(None) == BADARG
    assert ctx.encode_groups() == J.ENCODE_GROUPS_AUTO            # a refused value changes nothing
    try:
        # four waves where the quads of a row do not divide by four; either cooperative form where a row is no whole number of pieces
        for (W, H, name) in ((1920, 32, "4coop"), (192, 16, "4coop"), (64, 16, "4coop"), (100, 16, "4coop"), (100, 16, "2coop")):
            assert not legal(W, H, name)
            r, g, b = oracle.synth_rgb(W, H, frame=1)
            ctx.set_encode_groups(forms[name])
            with pytest.raises(J.JpezyError, match="status -1"):
                ctx.fdct_quant(r, g, b, W, H)
            ctx.set_encode_groups(forms["2direct"])                 # ... and the context stays usable
            assert np.array_equal(ctx.fdct_quant(r, g, b, W, H), oracle.encode_coeffs(r, g, b, W, H, False))
    finally:
        ctx.set_encode_groups(J.ENCODE_GROUPS_AUTO)


def test_other_launches_do_not_consult_the_setting(J, ctx, forms, oracle):
    """encode variant 0 (the FP64 kernel) has one form: a forced form of variant 1 neither reaches nor refuses it"""
    W, H = 100, 16
    r, g, b = oracle.synth_rgb(W, H, frame=3)
    c0 = J.Context(0)
    try:
        c0.set_variant(0)
        c0.set_encode_groups(forms["4coop"])
        assert np.array_equal(c0.fdct_quant(r, g, b, W, H), oracle.encode_coeffs(r, g, b, W, H, False))
    finally:
        c0.close()
