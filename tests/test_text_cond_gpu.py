"""The text-conditioning branch beyond the one-token, all-kept call of the reference: csrc/text_build.inc, kernels_text.hip
and Unet.text_cond.

1. The small kernels through their pass-through entries (include/kd_engine.h: kd_text_select, kd_add_rows_bcast,
   kd_mean_rows, kd_copy_rows, kd_cfg_combine) against the torch expression of the same operation.  Every output sits in a
   NaN-filled buffer with NaN guard rows before and after the written region: a write outside it destroys a NaN, an
   element left out stays one.  The kernels that move data or add once must be bit-equal to torch; the mean and the
   guidance combine have worked-out fp32 bounds against fp64.
2. Unet.text_cond against the oracle's Unet.text_conditioning (oracle/imagen_ref.py) in fp64: token counts 1 .. beyond
   max_text_len, ragged masks, holes, bool / float masks, text_mask=None, drop, two text_embed_dim, qk-norm.

Bound of part 2 (BRANCH_FACTOR, CONV_REL): the fp32 oracle's own rel-L2 against the fp64 oracle, times 3 (the margin
test_conv_igemm gives a differently ordered fp32 sum), floor 2e-6.  The fp32 oracle itself measures 4e-7 .. 6e-7 (tokens) and
1e-7 .. 2e-7 (hiddens) in every case, so the bound is the floor throughout; every case prints its engine error / bound
(worst measured: 0.274, next to BRANCH_FACTOR).  The kernel bounds: mean_rows uses at most 0.24 of its bound, cfg_combine 0.66.
"""
import copy
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import helpers as H

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24   # one fp32 rounding, relative
GUARD = 256        # floats of NaN before and after every output region (keeps the region 1 KB aligned)
NAN = float("nan")


@pytest.fixture(scope="module")
def E():
    """The binding module (ptr, check, current_stream); E.load() is the library."""
    from imagen_pytorch import _engine

    return _engine


def guarded(n, device, fill=None):
    """(buffer, region): n floats between two NaN guards; the region is NaN too unless `fill` [n] is given."""
    buf = torch.full((GUARD + n + GUARD,), NAN, device=device)
    region = buf[GUARD:GUARD + n]
    if fill is not None:
        region.copy_(fill.reshape(-1).to(device))
    return buf, region


def read_guarded(buf, n, what):
    """The region on the host, after checking that the guards are untouched and the region fully written."""
    host = buf.cpu()
    assert torch.isnan(host[:GUARD]).all(), f"{what}: wrote before the output"
    assert torch.isnan(host[GUARD + n:]).all(), f"{what}: wrote past the output"
    region = host[GUARD:GUARD + n]
    assert torch.isfinite(region).all(), f"{what}: output not written everywhere"
    return region


def bit_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def fptr(t, offset_floats=0):
    """Device address `offset_floats` into a contiguous fp32 tensor."""
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    return C.c_void_p(t.data_ptr() + 4 * offset_floats)


# ------------------------------------------------------------------------------------------------ text_select
def _hole_row(L):
    """Zeros at the first, the last and (from L = 5) an interior position; one kept position holds 0.5, which counts as kept."""
    m = torch.ones(L)
    if L >= 2:
        m[L - 1] = 0.0
    if L >= 3:
        m[0] = 0.0
    if L >= 5:
        m[L // 2] = 0.0
    m[1 if L >= 3 else 0] = 0.5
    return m


def _select_mask(kind, B, L):
    """[B, L] float mask.  "mixed" cycles the rows through (holes + a 0.5, all false, all true), "mixed-rot" starts the
    cycle at the all-false row, so every pattern meets every batch index a shape has."""
    if kind == "none":
        return None
    if kind == "all-true":
        return torch.ones(B, L)
    rows = [_hole_row(L), torch.zeros(L), torch.ones(L)]
    start = {"mixed": 0, "mixed-rot": 1}[kind]
    return torch.stack([rows[(start + b) % 3] for b in range(B)])


SELECT_SHAPES = [(3, 1, 8, 32), (2, 3, 8, 32), (2, 8, 8, 32), (2, 77, 256, 512), (1, 256, 256, 64)]   # (B, L, P, C)


def test_select_masks_hold_the_patterns_they_claim():
    m = _select_mask("mixed", 3, 8)
    assert m[0].tolist() == [0.0, 0.5, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0] and not m[1].any() and m[2].all()
    assert _select_mask("mixed-rot", 1, 77).sum() == 0 and _select_mask("mixed", 1, 1).tolist() == [[0.5]]
    assert _hole_row(3).tolist() == [0.0, 0.5, 0.0]


@pytest.mark.parametrize("kind", ["all-true", "mixed", "mixed-rot", "none"])
@pytest.mark.parametrize("B,L,P,Cd", SELECT_SHAPES)
def test_text_select_is_bit_equal_to_where(E, device, B, L, P, Cd, kind):
    """out[b][p] = tok[b][p] where p < L, mask[b][p] != 0 and not drop, else null_embed[p]; without a mask (text_mask=None)
    the L tokens are kept and the rows from L on are the zero padding.  tok has no rows past L, null_embed is random per
    position."""
    lib = E.load()
    tok = torch.randn(B, L, Cd, generator=H.gen(1))
    null = torch.randn(P, Cd, generator=H.gen(2))
    mask = _select_mask(kind, B, L)
    # tok and mask lie at the very end of their allocations' used part, NaN behind them: a read of row L poisons the output
    tbuf, tdev = guarded(B * L * Cd, device, tok)
    ndev = null.to(device)
    mdev = None
    if mask is not None:
        mbuf, mdev = guarded(B * L, device, mask)
    tokp = F.pad(tok, (0, 0, 0, P - L))
    for drop in (0, 1):
        obuf, out = guarded(B * P * Cd, device)
        E.check(lib.kd_text_select(E.ptr(tdev), E.ptr(mdev), E.ptr(ndev), E.ptr(out), B, L, P, Cd, drop, E.current_stream()))
        got = read_guarded(obuf, B * P * Cd, f"text_select {kind} drop {drop}").view(B, P, Cd)
        if drop:
            ref = null[None].expand(B, P, Cd)
        elif mask is None:
            ref = tokp
        else:
            keep = F.pad(mask != 0, (0, P - L), value=False)
            ref = torch.where(keep[:, :, None], tokp, null[None])
        assert bit_equal(got, ref), (kind, drop, int((got != ref).sum()))


def test_text_select_rejects_more_tokens_than_positions(E, device):
    lib = E.load()
    t = torch.zeros(256, device=device)
    for L, P in ((0, 8), (9, 8)):
        assert lib.kd_text_select(E.ptr(t), E.ptr(t), E.ptr(t), E.ptr(t), 1, L, P, 4, 0, E.current_stream()) != 0
        assert b"kd_text_select" in lib.kd_last_error()


# ------------------------------------------------------------------------------------------------ add_rows_bcast
# the last shape has B R C > 4096 * 256 elements: the capped grid of kernels_text.hip takes a second trip
@pytest.mark.parametrize("B,R,Cd", [(1, 8, 32), (3, 256, 512), (5, 256, 1024)])
def test_add_rows_bcast_is_bit_equal_to_torch(E, device, B, R, Cd):
    lib = E.load()
    assert (B, R, Cd) != (5, 256, 1024) or B * R * Cd > 4096 * 256
    x = torch.randn(B, R, Cd, generator=H.gen(3))
    add = torch.randn(R, Cd, generator=H.gen(4))   # random per row: an index taken % C instead of % (R C) shows
    n = B * R * Cd
    obuf, out = guarded(n, device)
    xd, ad = x.to(device), add.to(device)
    E.check(lib.kd_add_rows_bcast(E.ptr(xd), E.ptr(ad), E.ptr(out), B, R, Cd, E.current_stream()))
    got = read_guarded(obuf, n, "add_rows_bcast").view(B, R, Cd)
    assert bit_equal(got, x + add[None])


# ------------------------------------------------------------------------------------------------ mean_rows
# (3, 7, 100): B C = 300 is no multiple of the 256-thread block; (2, 36, 512) the plan's mean over the pooled tokens
@pytest.mark.parametrize("B,R,Cd", [(1, 1, 32), (3, 8, 32), (2, 256, 512), (2, 36, 512), (3, 7, 100)])
def test_mean_rows_matches_fp64(E, device, B, R, Cd):
    """Sequential fp32 summation of R terms: |error of the sum| <= (R - 1) 2^-24 sum|x| to first order, so the mean is within
    R 2^-24 mean|x|, plus one rounding of the result (the division)."""
    lib = E.load()
    x = torch.randn(B, R, Cd, generator=H.gen(5)) + 0.5
    obuf, out = guarded(B * Cd, device)
    xd = x.to(device)
    E.check(lib.kd_mean_rows(E.ptr(xd), E.ptr(out), B, R, Cd, E.current_stream()))
    got = read_guarded(obuf, B * Cd, "mean_rows").view(B, Cd).double()
    ref = x.double().mean(dim=1)
    bound = R * U24 * x.double().abs().mean(dim=1) + U24 * ref.abs()
    worst = float(((got - ref).abs() / bound).max())
    print(f"mean_rows B{B} R{R} C{Cd}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ copy_rows
def test_copy_rows_broadcasts_the_latents_behind_the_mean_pooled_rows(E, device):
    """The launch form text_build.inc uses for the learned latents: n_lat rows from one source block (batch stride 0) into
    every batch element's block of ntok rows, behind a row offset; the rows before the offset are not touched.  The offset
    n_mp is this test's own argument: it checks the kernel's addressing, not that the plan passes n_mp - a plan that copied
    to row 0 is seen only by test_text_cond_matches_fp64_oracle."""
    lib = E.load()
    B, n_mp, n_lat, Cd = 3, 4, 32, 64
    ntok = n_mp + n_lat
    lat = torch.randn(n_lat, Cd, generator=H.gen(6))
    obuf, out = guarded(B * ntok * Cd, device)
    ld = lat.to(device)
    E.check(lib.kd_copy_rows(E.ptr(ld), 0, Cd, fptr(out, n_mp * Cd), ntok * Cd, Cd, n_lat, Cd, B, E.current_stream()))
    host = obuf.cpu()
    assert torch.isnan(host[:GUARD]).all() and torch.isnan(host[GUARD + B * ntok * Cd:]).all(), "guards"
    got = host[GUARD:GUARD + B * ntok * Cd].view(B, ntok, Cd)
    assert torch.isnan(got[:, :n_mp]).all(), "rows before the row offset were written"
    assert bit_equal(got[:, n_mp:], lat[None].expand(B, n_lat, Cd))


def test_copy_rows_with_unequal_row_and_batch_strides(E, device):
    lib = E.load()
    B, rows, Cd, lds, ldd = 3, 5, 24, 32, 28
    sbs, dbs = rows * lds + 16, rows * ldd + 8
    src = torch.randn(B * sbs, generator=H.gen(7))
    obuf, out = guarded(B * dbs, device)
    sd = src.to(device)
    E.check(lib.kd_copy_rows(E.ptr(sd), sbs, lds, E.ptr(out), dbs, ldd, rows, Cd, B, E.current_stream()))
    host = obuf.cpu()
    assert torch.isnan(host[:GUARD]).all() and torch.isnan(host[GUARD + B * dbs:]).all(), "guards"
    got = host[GUARD:GUARD + B * dbs].view(B, dbs)
    ref = torch.full((B, dbs), NAN)
    for b in range(B):
        for r in range(rows):
            ref[b, r * ldd:r * ldd + Cd] = src[b * sbs + r * lds:b * sbs + r * lds + Cd]
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "wrote outside the rows' C columns, or left some out"
    assert bit_equal(torch.nan_to_num(got), torch.nan_to_num(ref))


@pytest.mark.parametrize("bcast", [False, True])
def test_copy_rows_of_one_row(E, device, bcast):
    """The text hiddens' last launch: one row of time_cond_dim per batch element, from the plan's own rows or - under
    drop - from null_text_hidden with batch stride 0."""
    lib = E.load()
    B, Cd = 3, 128
    src = torch.randn(1 if bcast else B, Cd, generator=H.gen(8))
    obuf, out = guarded(B * Cd, device)
    sd = src.to(device)
    E.check(lib.kd_copy_rows(E.ptr(sd), 0 if bcast else Cd, Cd, E.ptr(out), Cd, Cd, 1, Cd, B, E.current_stream()))
    got = read_guarded(obuf, B * Cd, "copy_rows rows=1").view(B, Cd)
    assert bit_equal(got, src.expand(B, Cd))


@pytest.mark.parametrize("rows,Cd,B", [(0, 16, 2), (4, 0, 2), (4, 16, 0)])
def test_copy_rows_of_nothing_writes_nothing(E, device, rows, Cd, B):
    lib = E.load()
    src = torch.randn(256, generator=H.gen(9)).to(device)
    obuf, out = guarded(256, device)
    E.check(lib.kd_copy_rows(E.ptr(src), 64, 16, E.ptr(out), 64, 16, rows, Cd, B, E.current_stream()))
    assert torch.isnan(obuf.cpu()).all()


# ------------------------------------------------------------------------------------------------ cfg_combine
CFG_SCALES = (0.0, 1.0, 2.5, -1.0)


@pytest.mark.parametrize("alias", [False, True], ids=["out-distinct", "out-is-cond"])
@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 13])
def test_cfg_combine_matches_fp64(E, device, n, alias):
    """out = null + (cond - null) * scale: three fp32 roundings (difference, product, sum; two under a contracted
    multiply-add), each at most 2^-24 of a term no larger than |null| + |scale| |cond - null|.  Scale 0 returns null."""
    lib = E.load()
    cond = torch.randn(n, generator=H.gen(10))
    null = torch.randn(n, generator=H.gen(11)) * 0.7 + 0.2
    nd = null.to(device)
    c64, n64 = cond.double(), null.double()
    for scale in CFG_SCALES:
        cbuf, cdev = guarded(n, device, cond)
        obuf, out = (cbuf, cdev) if alias else guarded(n, device)
        E.check(lib.kd_cfg_combine(E.ptr(cdev), E.ptr(nd), E.ptr(out), scale, n, E.current_stream()))
        got = read_guarded(obuf, n, f"cfg_combine scale {scale}")
        if not alias:
            assert bit_equal(read_guarded(cbuf, n, "cond"), cond), "cond was written"
        ref = n64 + (c64 - n64) * scale
        bound = 3 * U24 * (n64.abs() + abs(scale) * (c64 - n64).abs())
        worst = float(((got.double() - ref).abs() / bound).max())
        print(f"cfg_combine n {n} scale {scale} {'in place' if alias else 'out of place'}: worst error / bound {worst:.3f}")
        assert worst <= 1.0, (scale, worst)
        if scale == 0.0:
            assert bit_equal(got, null), "scale 0 must return null bit for bit"
    assert bit_equal(nd.cpu(), null)


# ------------------------------------------------------------------------------------------------ the branch against the oracle
CONV_REL = 2e-6          # floor of the bound (tests/test_kernels_gpu.py)
BRANCH_FACTOR = 3.0      # engine error <= 3 x the fp32 oracle's own error against fp64
                         # measured on an MI355X: worst engine error / bound 0.274 (5.49e-07 against 2e-6: tokens, text_embed_dim
                         # 16, L 11 of 8, all kept); over all cases the engine's token errors are 4.8e-07 .. 5.5e-07, the fp32 oracle's 4.1e-07 .. 5.2e-07
SENSITIVITY = 100.0      # one flipped mask bit must move the fp64 tokens by 100 x the bound: holds for every ragged / hole case,
                         # max_text_len 256 included (least: 5e-3 against 2e-4, L 256 ragged); the per-position select is also
                         # checked exactly at text_select level (SELECT_SHAPES: L 77 and 256 of P 256)

SEG_KW = dict(dim=32, dim_mults=(1, 2, 3, 4), cond_dim=64, num_resnet_blocks=2, layer_attns=(False, True, True, True),
              layer_cross_attns=(False, True, True, True), cond_images_channels=4)   # tests/test_unet_gpu.py _seg_pair
BATCH, SIZE = 3, 16


@pytest.fixture(scope="module")
def pairs(device):
    """pairs(ted, P, qk=0) -> (oracle fp32, oracle fp64, product UNet on the device) with the same randomised weights, built
    once per key; the UNets and their engine plans are released when the module is done."""
    import imagen_pytorch as ip
    from oracle import imagen_ref as R

    cache = {}

    def get(ted, P, qk=0):
        key = (ted, P, qk)
        if key not in cache:
            ou = H.randomize_(R.Unet(**SEG_KW, text_embed_dim=ted, max_text_len=P, cond_on_text=True, attn_qk_norm=qk),
                              40 + ted + P + qk).eval()
            pu = ip.Unet(**ou._locals)
            pu.load_state_dict(ou.state_dict(), strict=True)
            assert pu.attn_qk_norm == qk and pu.max_text_len == P
            cache[key] = (ou, copy.deepcopy(ou).double(), pu.to(device))
        return cache[key]

    yield get
    for _, _, pu in cache.values():
        pu.invalidate_engine()
    cache.clear()


def _branch_mask(kind, L, P):
    """bool [3, L] or None.  ragged: lengths [L, 1, 0] (sample 2 all false); hole: sample 0 misses an interior token,
    sample 1 its first, sample 2 is whole."""
    if kind == "none":
        return None
    m = torch.ones(BATCH, L, dtype=torch.bool)
    if kind == "ragged":
        m[1, 1:] = False
        m[2] = False
    elif kind == "hole":
        assert L >= 3
        m[0, L // 2] = False
        m[1, 0] = False
    else:
        assert kind == "true"
    return m


def _flip_one_bit(kind, mask, P):
    """The mask with one bit flipped inside the first max_text_len positions: ragged loses sample 0's last kept token, hole
    gets its interior token back."""
    f = mask.clone()
    p = min(mask.shape[1], P) - 1 if kind == "ragged" else mask.shape[1] // 2
    f[0, p] = ~f[0, p]
    return f


def _oracle(u, text, mask, drop):
    with torch.no_grad():
        return u.text_conditioning(text.to(next(u.parameters()).dtype), mask, 1.0 if drop else 0.0)


def _engine(pu, device, text, mask, drop):
    h = pu.engine(BATCH, SIZE, device, with_text=True)
    with torch.cuda.device(device):
        tok, hid = pu.text_cond(h, text.to(device), None if mask is None else mask.to(device), drop, device)
    return tok.cpu(), hid.cpu()


def _check_against_oracle(pairs, device, ted, P, L, kind, qk=0):
    ou, ou64, pu = pairs(ted, P, qk)
    text = torch.randn(BATCH, L, ted, generator=H.gen(100 + L))
    mask = _branch_mask(kind, L, P)
    for drop in (False, True):
        tok64, hid64 = _oracle(ou64, text, mask, drop)
        tok32, hid32 = _oracle(ou, text, mask, drop)
        tok, hid = _engine(pu, device, text, mask, drop)
        assert tok.shape == tok64.shape and hid.shape == hid64.shape
        assert torch.isfinite(tok).all() and torch.isfinite(hid).all()
        for name, got, r32, r64 in (("tokens", tok, tok32, tok64), ("hiddens", hid, hid32, hid64)):
            e32, e = H.rel_l2(r32, r64), H.rel_l2(got, r64)
            bound = max(BRANCH_FACTOR * e32, CONV_REL)
            print(f"text_cond ted {ted} P {P} L {L} {kind} qk {qk} drop {int(drop)} {name}: engine {e:.2e}, fp32 oracle "
                  f"{e32:.2e}, bound {bound:.2e}, ratio {e / bound:.3f}")
            assert e <= bound, (name, drop, e, e32, bound)
        if drop:
            # cond_drop_prob = 1: the learned null hidden itself, and the tokens of a mask that keeps nothing
            null_hidden = pu.null_text_hidden.detach().cpu().expand_as(hid)
            assert bit_equal(hid, null_hidden), "dropped hiddens must be null_text_hidden bit for bit"
            tok_f, _ = _engine(pu, device, text, torch.zeros(BATCH, L, dtype=torch.bool), False)
            assert bit_equal(tok, tok_f), "dropped tokens must equal those of the all-false mask"
        elif mask is not None:
            # a float mask of the same pattern (kept entries 1 or 0.5) is the same mask
            fm = mask.float()
            fm[:, ::2] *= 0.5
            tok_fl, hid_fl = _engine(pu, device, text, fm, False)
            assert bit_equal(tok, tok_fl) and bit_equal(hid, hid_fl), "bool and float masks of one pattern differ"
        if not drop and kind in ("ragged", "hole"):
            # can this case see a one-token error?  (fp64 on the host, no engine involved)
            tok_flip, _ = _oracle(ou64, text, _flip_one_bit(kind, mask, P), False)
            moved = H.rel_l2(tok_flip, tok64)
            need = SENSITIVITY * max(BRANCH_FACTOR * H.rel_l2(tok32, tok64), CONV_REL)
            print(f"text_cond ted {ted} P {P} L {L} {kind}: one flipped mask bit moves the fp64 tokens by {moved:.2e} "
                  f"(100 x bound = {need:.2e})")
            assert moved >= need, (moved, need)


BRANCH_LP = [(8, 1), (8, 3), (8, 8), (8, 11), (256, 77), (256, 256)]   # (max_text_len, L); L = 11 is truncated to 8
BRANCH_CASES = [pytest.param(P, L, kind, id=f"P{P}-L{L}-{kind}") for P, L in BRANCH_LP
                for kind in ("true", "ragged", "hole", "none") if not (kind == "hole" and L < 3)]   # one token has no interior


@pytest.mark.parametrize("P,L,kind", BRANCH_CASES)
@pytest.mark.parametrize("ted", [3, 16])
def test_text_cond_matches_fp64_oracle(pairs, device, ted, P, L, kind):
    _check_against_oracle(pairs, device, ted, P, L, kind)


@pytest.mark.parametrize("qk", [0, 1])
def test_text_cond_ragged_under_qk_norm(pairs, device, qk):
    """The PerceiverResampler's attention takes the attn_qk_norm switch of the UNet: one ragged case for each form."""
    _check_against_oracle(pairs, device, 16, 8, 3, "ragged", qk=qk)


def test_text_mask_none_keeps_the_zero_padding(pairs, device):
    """The library pads the projected tokens with zeros up to max_text_len and selects against null_text_embed only
    where there is a mask.  Without one the padding stays: text_mask=None is NOT a mask of ones (which would put
    null_text_embed into the rows from L on)."""
    ted, P, L = 3, 8, 3
    ou, ou64, pu = pairs(ted, P)
    text = torch.randn(BATCH, L, ted, generator=H.gen(100 + L))
    tok_none, hid_none = _engine(pu, device, text, None, False)
    tok_ones, hid_ones = _engine(pu, device, text, torch.ones(BATCH, L, dtype=torch.bool), False)
    r_none, _ = _oracle(ou64, text, None, False)
    r_ones, _ = _oracle(ou64, text, torch.ones(BATCH, L, dtype=torch.bool), False)
    gap = H.rel_l2(r_ones, r_none)
    print(f"text_mask=None against a mask of ones, L {L} of {P}: the fp64 oracle's tokens differ by {gap:.2e}; engine vs "
          f"oracle {H.rel_l2(tok_none, r_none):.2e} (None), {H.rel_l2(tok_ones, r_ones):.2e} (ones)")
    assert gap > 1e-2, "the two calls must be different functions for this test to mean anything"
    assert H.rel_l2(tok_none, r_none) < 1e-4 * gap and H.rel_l2(tok_ones, r_ones) < 1e-4 * gap
    # at L == max_text_len there is no padding and the two calls are one
    text8 = torch.randn(BATCH, P, ted, generator=H.gen(108))
    a = _engine(pu, device, text8, None, False)
    b = _engine(pu, device, text8, torch.ones(BATCH, P, dtype=torch.bool), False)
    assert bit_equal(a[0], b[0]) and bit_equal(a[1], b[1])
