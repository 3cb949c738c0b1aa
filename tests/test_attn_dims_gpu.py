"""`Unet(attn_dim_head=32 | 128, layer_attns_depth > 1)` on the MI355X: the attention core and the qk-norm at D = 32 and 128
through kd_attention_ex_d / kd_l2norm_heads_d against fp64 torch (the forms of tests/test_attention_gpu.py, restated with D
as a parameter), D = 64 bit-equal to the entries without the argument, the UNet forward and the samplers against
oracle.imagen_ref.Unet on identical weights, a default plan through kd_unet_create_ext3, and a strict ImagenTrainer.load.

Every tensor of an attention launch sits in a NaN-filled buffer with padded row strides: a read outside a slice poisons the
output, a write outside it destroys a NaN.  Key counts are placed around KT(D) = kd_attention_key_tile(D), the keys per LDS
tile of the D-wide instantiations (64, 64, 32).

Tolerance of the attention core: test_attention_gpu.py's rtol 1e-4, atol 2e-5 for both D (every test prints the share of
it that it uses, and the share fp32 torch attention on the CPU uses on the same inputs)."""
import ctypes as C
import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

import attention_cases as AC
import elucidated_ref as ER
import helpers as H
from oracle import imagen_ref as R
from oracle import sampler_ref as RS

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5   # test_kernels_gpu.py::test_attention
FWD_REL_L2 = 2e-5
SAMPLE_ABS = 2e-3
DS = [32, 128]
NAN = float("nan")


engine = H.engine   # (H is the head count inside some functions below)


@pytest.fixture(scope="module")
def lib():
    return engine().load()


QSHAPES = {"vec70": (2, 70, 4),      # Nq < 128: attention_kernel<4, D, DS>
           "mfma200": (2, 200, 4)}   # 16 blocks of 128 queries, the last wave a quarter full: attention_mfma_kernel<D>


def test_query_shapes_reach_both_kernels_and_tiles_are_known(lib):
    assert [AC.is_mfma(*QSHAPES[n]) for n in ("vec70", "mfma200")] == [False, True]
    assert [lib.kd_attention_key_tile(d) for d in (32, 64, 128)] == [64, 64, 32]


# ------------------------------------------------------------------------------------------------ device buffers
class _Bufs:
    """The NaN-filled device buffers of one launch.  "self" (Hkv = 1, transformer()): q | k | v are columns of one buffer of
    row stride ldq = ld1 = inner + 2 D + 4, the context k | v rows of stride ld0 = 2 D + 8.  "cross" (Hkv = H, cross_attn() and
    the Perceiver): q rows of stride inner + 4, k | v rows of stride 2 inner + 8.  Output rows of stride ldo = inner + 4 and one
    guard row."""

    def __init__(self, device, D, q, nkv, k0, v0, k1, v1):
        B, Nq, H, _ = q.shape
        Hkv, n0, n1 = k0.shape[2], k0.shape[1], k1.shape[1]
        inner = H * D
        self.D, self.B, self.Nq, self.H, self.Hkv, self.n0, self.n1, self.inner = D, B, Nq, H, Hkv, n0, n1, inner
        nan = lambda rows, cols: torch.full((max(rows, 1), cols), NAN, device=device)
        if Hkv == 1:
            self.ldq = self.ld1 = inner + 2 * D + 4
            self.qkv = nan(B * max(Nq, n1), self.ldq)
            self.qkv[:B * Nq, :inner] = q.reshape(B * Nq, inner).to(device)
            self.qkv[:B * n1, inner:inner + D] = k1.reshape(B * n1, D).to(device)
            self.qkv[:B * n1, inner + D:inner + 2 * D] = v1.reshape(B * n1, D).to(device)
            self.q_ptr, self.k1_ptr, self.v1_ptr = (self.qkv.data_ptr() + 4 * off for off in (0, inner, inner + D))
            self.ld0 = 2 * D + 8
            self.ckv = nan(B * n0, self.ld0)
            self.ckv[:B * n0, :D] = k0.reshape(B * n0, D).to(device)
            self.ckv[:B * n0, D:2 * D] = v0.reshape(B * n0, D).to(device)
            self.k0_ptr, self.v0_ptr = self.ckv.data_ptr(), self.ckv.data_ptr() + 4 * D
        else:
            assert Hkv == H
            self.ldq = inner + 4
            self.qb = nan(B * Nq, self.ldq)
            self.qb[:, :inner] = q.reshape(B * Nq, inner).to(device)
            self.q_ptr = self.qb.data_ptr()
            self.ld0 = self.ld1 = 2 * inner + 8
            self.kv0, self.kv1 = nan(B * n0, self.ld0), nan(B * n1, self.ld1)
            for buf, k, v, n in ((self.kv0, k0, v0, n0), (self.kv1, k1, v1, n1)):
                buf[:B * n, :inner] = k.reshape(B * n, inner).to(device)
                buf[:B * n, inner:2 * inner] = v.reshape(B * n, inner).to(device)
            self.k0_ptr, self.v0_ptr = self.kv0.data_ptr(), self.kv0.data_ptr() + 4 * inner
            self.k1_ptr, self.v1_ptr = self.kv1.data_ptr(), self.kv1.data_ptr() + 4 * inner
        self.nkv = nkv.contiguous().to(device) if nkv is not None else None
        self.ldo = inner + 4
        self.out = nan(B * Nq + 1, self.ldo)   # (+ one guard row)

    def launch(self, lib, scale, D=None, plain_entry=False):
        E = engine()
        p = lambda a, n: C.c_void_p(a) if n else None   # an empty segment goes in as NULL pointers
        head = (C.c_void_p(self.q_ptr), self.ldq, E.ptr(self.nkv), p(self.k0_ptr, self.n0), p(self.v0_ptr, self.n0), self.ld0,
                self.n0, p(self.k1_ptr, self.n1), p(self.v1_ptr, self.n1), self.ld1, self.n1, E.ptr(self.out), self.ldo, self.B,
                self.Nq, self.H, self.Hkv)
        if plain_entry:
            return lib.kd_attention_ex(*head, scale, E.current_stream())
        return lib.kd_attention_ex_d(*head, self.D if D is None else D, scale, E.current_stream())

    def result(self):
        """The output slice - all D columns of every head - after checking that nothing outside it was written and
        everything inside it was."""
        out = self.out.cpu()
        rows = self.B * self.Nq
        assert bool(out[:rows, self.inner:].isnan().all()) and bool(out[rows:].isnan().all()), "a write outside the output slice"
        got = out[:rows, :self.inner]
        assert bool(got.isfinite().all()), "an element of the output slice was not written, or a read left the input slices"
        return got.reshape(self.B, self.Nq, self.H, self.D).double()


def _used(got, ref):
    return float(((got.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def _check(lib, device, D, family, qshape, Hkv_is_H, null, n0, n1, seed, marker=None, tag=""):
    B, Nq, H = qshape
    Hkv = H if Hkv_is_H else 1
    args = AC.inputs(D, family, B, Nq, H, Hkv, null, n0, n1, seed, marker)
    bufs = _Bufs(device, D, *args[:6])
    engine().check(bufs.launch(lib, args[6]))
    got = bufs.result()
    ref = AC.reference(*args)
    used, used32 = _used(got, ref), _used(AC.reference(*args, dtype=torch.float32), ref)
    print(f"attention D{D} {family}{tag} B{B} Nq{Nq} H{H} Hkv{Hkv} keys {int(null)}+{n0}+{n1} "
          f"{'mfma' if AC.is_mfma(B, Nq, H) else 'vec'}: max|err| {float((got - ref).abs().max()):.2e}, {used:.3f} of the bound "
          f"(fp32 torch: {used32:.3f})")
    assert torch.allclose(got, ref, rtol=RTOL, atol=ATOL), used
    return used


# ------------------------------------------------------------------------------------------------ key counts and boundaries
def _keys(KT):
    """(null, n0, n1): null + n0 + n1 keys in tiles of KT; segment 1 starts at key null + n0."""
    return [
        (True, 0, 0),                 # 1: the null key alone, both segments empty
        (True, 1, 0),                 # 2
        (True, 0, 1),                 # 2, segment 0 empty
        (False, 0, KT - 1),           # KT - 1 without the null key, segment 0 empty
        (True, 2, KT - 4),            # KT - 1
        (True, KT - 2, 1),            # KT: segment 1 is the last row of the tile
        (True, KT - 1, 1),            # KT + 1: segment 1 starts at the first row of the second tile
        (True, KT, 0),                # KT + 1, segment 1 empty
        (True, KT - 1, KT + 1),       # 2 KT + 1: boundary at a tile's first row
        (True, KT - 2, KT + 2),       # 2 KT + 1: boundary at a tile's last row
        (True, KT // 2 - 2, 2 * KT - KT // 2 + 2),   # 2 KT + 1: boundary inside a tile
        (False, KT, KT + 1),          # 2 KT + 1 without the null key: boundary at a tile's first row
        (False, 2 * KT + 1, 0),       # 2 KT + 1 in segment 0 alone
    ]


@pytest.mark.parametrize("case", range(13))
@pytest.mark.parametrize("qname", list(QSHAPES))
@pytest.mark.parametrize("Hkv_is_H", [False, True])
@pytest.mark.parametrize("D", DS)
def test_key_counts_and_segment_boundaries(lib, device, D, Hkv_is_H, qname, case):
    """Both kernels, Hkv = 1 and H, with and without the null key, over 1, 2, KT - 1, KT, KT + 1 and 2 KT + 1 keys with the
    segment boundary at a tile's first row, last row and inside it, and either segment empty; the three dense input
    families; padded strides whose spare columns stay NaN."""
    KT = lib.kd_attention_key_tile(D)
    keys = _keys(KT)
    assert len(keys) == 13 and sorted({int(a) + b + c for a, b, c in keys}) == [1, 2, KT - 1, KT, KT + 1, 2 * KT + 1]
    null, n0, n1 = keys[case]
    for family in ("plain", "cos16", "ascending"):
        _check(lib, device, D, family, QSHAPES[qname], Hkv_is_H, null, n0, n1, 202 + case)


# ------------------------------------------------------------------------------------------------ one key that matters
@pytest.mark.parametrize("where", ["null", "seg0_last", "seg1_first", "tile_rowKT"])
@pytest.mark.parametrize("qname", list(QSHAPES))
@pytest.mark.parametrize("Hkv_is_H", [False, True])
@pytest.mark.parametrize("D", DS)
def test_marker_key(lib, device, D, Hkv_is_H, qname, where):
    """One key holds most of the softmax and has a value row of its own (3 + d / 16: every one of the D columns differs): a
    key that is dropped, read twice or taken from the wrong segment, or an output column that is not the key's, moves the
    output by O(1).  Keys 1 + 20 + (2 KT + 30): the boundary (key 21) inside the first tile, four or more tiles."""
    KT = lib.kd_attention_key_tile(D)
    marker = {"null": 0, "seg0_last": 20, "seg1_first": 21, "tile_rowKT": KT}[where]
    _check(lib, device, D, "marker", QSHAPES[qname], Hkv_is_H, True, 20, 2 * KT + 30, 404, marker=marker, tag=f"@{where}")


def test_marker_moves_every_output_column(lib, device):
    """The marker family does what it is for: the reference output of a marked key list is, in every column of every head,
    far outside the tolerance from the reference with the marker's value row zeroed in its upper half (a kernel that
    wrote only the first 64 of 128 columns, or took them from another key, would be caught)."""
    args = list(AC.inputs(128, "marker", 2, 70, 4, 1, True, 20, 94, 404, marker=32))
    ref = AC.reference(*args)
    args[5] = args[5].clone()   # v1: key 32 of the list is row 32 - 1 - 20 of segment 1
    args[5][:, 32 - 21, :, 64:] = 0
    other = AC.reference(*args)
    assert bool(((ref - other).abs()[..., 64:] > 1.0).all()) and bool(((ref - other).abs()[..., :64] < 1e-9).all())


# ------------------------------------------------------------------------------------------------ D = 64 and refusals
@pytest.mark.parametrize("qname", list(QSHAPES))
def test_d64_through_the_new_entry_is_bit_equal_to_kd_attention_ex(lib, device, qname):
    B, Nq, H = QSHAPES[qname]
    for Hkv in (1, H):
        args = AC.inputs(64, "ascending", B, Nq, H, Hkv, True, 30, 98, 303)
        a, b = _Bufs(device, 64, *args[:6]), _Bufs(device, 64, *args[:6])
        engine().check(a.launch(lib, args[6], plain_entry=True))
        engine().check(b.launch(lib, args[6]))
        assert torch.equal(a.result(), b.result())
        assert torch.allclose(a.result(), AC.reference(*args), rtol=RTOL, atol=ATOL)


def test_other_head_widths_are_refused(lib, device):
    args = AC.inputs(32, "plain", 1, 8, 4, 4, True, 4, 4, 7)
    bufs = _Bufs(device, 32, *args[:6])
    assert bufs.launch(lib, args[6]) == 0
    for bad in (48, 256, 0):
        assert bufs.launch(lib, args[6], D=bad) != 0
        assert all(v in lib.kd_last_error() for v in (b"32", b"64", b"128")), lib.kd_last_error()
    x = torch.zeros(4, 256, device=device)
    assert lib.kd_l2norm_heads_d(engine().ptr(x), 256, 4, 1, 48, None, engine().current_stream()) != 0
    assert all(v in lib.kd_last_error() for v in (b"32", b"64", b"128"))
    assert lib.kd_l2norm_heads_d(engine().ptr(x), 256, 4, 3, 128, None, engine().current_stream()) != 0   # ld < heads * D
    q = torch.zeros(1, 4, 2, 48, device=device)
    assert lib.kd_attention(engine().ptr(q), engine().ptr(q), engine().ptr(q), engine().ptr(q.clone()), 1, 4, 4, 2, 2, 48,
                            engine().current_stream()) != 0
    assert b"32, 64 and 128" in lib.kd_last_error()


@pytest.mark.parametrize("D", DS)
def test_kd_attention_takes_the_three_widths(lib, device, D):
    E = engine()
    gen = H.gen(D)
    q, k, v = (torch.randn(2, n, 4, D, generator=gen) for n in (70, 90, 90))
    out = torch.full((2, 70, 4, D), NAN, device=device)
    qd, kd, vd = q.to(device), k.to(device), v.to(device)
    E.check(lib.kd_attention(E.ptr(qd), E.ptr(kd), E.ptr(vd), E.ptr(out), 2, 70, 90, 4, 4, D, E.current_stream()))
    torch.cuda.synchronize()
    ref = AC.reference(q, None, k, v, k[:, :0], v[:, :0], 1.0)
    assert torch.allclose(out.cpu().double(), ref, rtol=RTOL, atol=ATOL), _used(out.cpu(), ref)


# ------------------------------------------------------------------------------------------------ qk-norm
L2_REL = 1e-6   # test_attention_gpu.py: fp32 torch is 5e-8 from fp64 on such inputs, an order of magnitude for the summation order
SENTINEL = 777.0


@pytest.mark.parametrize("heads,extra,rows", [
    (1, 0, 7),      # 7 segments: the last block is not full (8 segments a block at D = 32, 4 at 64 and 128)
    (1, 12, 9),     # strided rows
    (3, 8, 5),      # 15 segments
    (3, 0, 11),     # 33 segments, dense rows
])
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("D", DS)
def test_l2norm_heads(lib, device, D, heads, extra, rows, with_scale):
    """kd_l2norm_heads_d against fp64 F.normalize(x, dim=-1, eps=1e-12) * scale_vec per D-wide head segment: strided rows
    whose other columns keep their sentinel, a segment count that does not fill the last block, an all-zero segment (0, not
    NaN) and a segment of norm 1e-13, below the floor (x / 1e-12, not a unit vector)."""
    E = engine()
    gen = H.gen(17 + heads + rows + D)
    ld = heads * D + extra
    x = torch.randn(rows, heads, D, generator=gen) * torch.logspace(-3, 3, rows * heads).reshape(rows, heads, 1)
    zero_at, tiny_at = (1, 0), (rows - 1, heads - 1)
    x[zero_at] = 0
    x[tiny_at] = torch.randn(D, generator=gen) * (1e-13 / math.sqrt(D))
    sv = 1 + 0.3 * torch.randn(D, generator=gen) if with_scale else None
    ref = F.normalize(x.double(), dim=-1, eps=1e-12) * (sv.double() if with_scale else 1.0)
    buf = torch.full((rows + 1, ld), SENTINEL)   # (+ one guard row)
    buf[:rows, :heads * D] = x.reshape(rows, heads * D)
    buf = buf.to(device)
    svd = sv.to(device) if with_scale else None
    E.check(lib.kd_l2norm_heads_d(E.ptr(buf), ld, rows, heads, D, E.ptr(svd), E.current_stream()))
    out = buf.cpu()
    assert bool((out[:, heads * D:] == SENTINEL).all()) and bool((out[rows:] == SENTINEL).all()), "a write outside the head segments"
    got = out[:rows, :heads * D].reshape(rows, heads, D)
    assert bool((got[zero_at] == 0).all())
    tiny_norm = float(x[tiny_at].double().norm())   # below the floor: x / 1e-12, a vector of norm 0.1, not a unit vector
    assert 0.5e-13 < tiny_norm < 2e-13
    assert abs(float((got[tiny_at].double() / (sv.double() if with_scale else 1.0)).norm()) - tiny_norm / 1e-12) < 1e-6
    err = AC.rel(got, ref)
    worst = max(AC.rel(got[r, h], ref[r, h]) for r in range(rows) for h in range(heads) if (r, h) != zero_at)
    print(f"l2norm D{D} heads {heads} ld {ld} rows {rows} scale {with_scale}: rel-L2 {err:.2e}, worst segment {worst:.2e}")
    assert err < L2_REL and worst < L2_REL


@pytest.mark.parametrize("D", DS)
def test_l2norm_heads_of_the_null_key(lib, device, D):
    """null_kv_of (engine.hip): the [2][D] null key / value as one row of stride 2 D with one head - the value stays."""
    E = engine()
    nkv = torch.randn(2, D, generator=H.gen(23)) * 3
    sv = 1 + 0.3 * torch.randn(D, generator=H.gen(24))
    buf, svd = nkv.to(device), sv.to(device)
    E.check(lib.kd_l2norm_heads_d(E.ptr(buf), 2 * D, 1, 1, D, E.ptr(svd), E.current_stream()))
    out = buf.cpu()
    assert torch.equal(out[1], nkv[1])
    assert AC.rel(out[0], F.normalize(nkv[0].double(), dim=-1, eps=1e-12) * sv.double()) < L2_REL


def test_l2norm_d64_through_the_new_entry_is_bit_equal(lib, device):
    E = engine()
    x = torch.randn(37, 3 * 64 + 8, generator=H.gen(5))
    a, b = x.to(device), x.to(device)
    E.check(lib.kd_l2norm_heads(E.ptr(a), 200, 37, 3, None, E.current_stream()))
    E.check(lib.kd_l2norm_heads_d(E.ptr(b), 200, 37, 3, 64, None, E.current_stream()))
    assert torch.equal(a, b) and not torch.equal(a.cpu(), x)


# ------------------------------------------------------------------------------------------------ the UNet forward
# attention at 16 x 16 (256 tokens x 4 heads x 2 images = 16 blocks of 128 queries: the matrix cores) and at 8 x 8 (64 tokens:
# the vector kernel); mid_attn at 8 x 8; the cross-attention of mid_block1 / mid_block2 keeps the library's 8 heads of 64
BASE = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, True, True),
            layer_cross_attns=(False, True, True), attn_heads=4)
TEXT = dict(dim=32, dim_mults=(1, 2, 4), cond_dim=64, text_embed_dim=3, num_resnet_blocks=1, layer_attns=(False, True, True),
            layer_cross_attns=(False, True, True))   # tests/test_combine_fmaps_gpu.py
_ref_unet = functools.partial(H.ref_unet, R.Unet)



@pytest.mark.parametrize("name,kw,extra", [
    ("D32", BASE, dict(attn_dim_head=32)),
    ("D128", BASE, dict(attn_dim_head=128)),
    ("depth2", BASE, dict(layer_attns_depth=2)),
    ("depth123 D32", BASE, dict(layer_attns_depth=(1, 2, 3), attn_dim_head=32)),
    ("memory_efficient depth2", BASE, dict(layer_attns_depth=2, memory_efficient=True, init_conv_to_final_conv_residual=True)),
    ("lowres D128 depth2", BASE, dict(lowres_cond=True, attn_dim_head=128, layer_attns_depth=2)),
    ("lowres D32", BASE, dict(lowres_cond=True, attn_dim_head=32)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_unet_forward_matches_the_oracle(device, name, kw, extra):
    ou = _ref_unet(kw, seed=11, **extra)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3))
    print(f"forward {name}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2
    labels = H.plan_csv(pu, 2, 32, device)
    depths = pu._plan["layer_attns_depth"]
    # self-attention launches: the down and the up block of the two levels, mid_attn
    assert len(re.findall(r"(?<![a-z])attn N\d+", labels)) == 2 * (depths[1] + depths[2]) + 1


@pytest.mark.parametrize("D", DS)
def test_unet_forward_with_text_runs_the_perceiver_and_the_cross_attention_at_d(device, D):
    ou = _ref_unet(TEXT, seed=15, text=True, attn_dim_head=D, layer_attns_depth=(1, 1, 2))
    e, _ = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3))
    print(f"forward text D{D}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("D", DS)
def test_unet_forward_with_qk_norm(device, D, mode):
    """attn_qk_norm 1 (cosine-sim) and 2 (learned q_scale / k_scale [D]; [64] in the two middle ResnetBlocks) on the text
    config: self-attention, cross-attention, the Perceiver and the null keys normalised at plan build."""
    ou = _ref_unet(TEXT, seed=19 + mode, text=True, attn_dim_head=D, attn_qk_norm=mode, layer_attns_depth=(1, 2, 1))
    if mode == 2:
        assert tuple(ou.state_dict()["downs.1.3.layers.1.0.q_scale"].shape) == (D,)
    e, pu = H.forward_err(ou, device, *H.unet_inputs(ou, 2, 32, seed=3))
    assert pu.attn_qk_norm == mode
    print(f"forward text D{D} qk-norm {mode}: rel-L2 {e:.2e}")
    assert e < FWD_REL_L2


def _layer_macs(B, N, dim, H, D, Nc, cd, ff_mult=2):
    """MACs of one (attention, feed-forward) pair as kd_unet_macs counts them: the q | kv and context kv projections, QK^T and
    PV over 1 + Nc + N keys, to_out, the two feed-forward GEMMs."""
    inner, hidden = H * D, int(dim * ff_mult)
    return B * N * dim * (inner + 2 * D) + B * Nc * cd * 2 * D + B * H * N * (N + Nc + 1) * D * 2 + B * N * inner * dim \
        + 2 * B * N * dim * hidden


def test_depth_adds_the_further_layers_macs_and_launches(device):
    """Depth 2 and (1, 2, 3) against depth 1 on the same config: kd_unet_macs grows by exactly the further layers' MACs, and
    the launch count grows with them (a plan that ran layer 0 twice would also pass this - the forward tests, whose layers.1
    weights differ from layers.0's, would not)."""
    lib = engine().load()
    stats = {}
    for dep in (1, 2, (1, 2, 3)):
        pu = H.product_like(_ref_unet(BASE, seed=5, layer_attns_depth=dep), device)
        h = pu.engine(2, 32, device, with_text=False)
        stats[dep] = (lib.kd_unet_macs(h), lib.kd_unet_num_launches(h))
    B, H_, D, Nc, cd = 2, 4, 64, 2, 32
    # level 1: 256 tokens, widths 32 (down) and 64 (up); level 2: 64 tokens, widths 64 and 128
    l1 = _layer_macs(B, 256, 32, H_, D, Nc, cd) + _layer_macs(B, 256, 64, H_, D, Nc, cd)
    l2 = _layer_macs(B, 64, 64, H_, D, Nc, cd) + _layer_macs(B, 64, 128, H_, D, Nc, cd)
    print(f"macs / launches: {stats}; further layers: level 1 {l1}, level 2 {l2}")
    assert stats[2][0] - stats[1][0] == l1 + l2
    assert stats[(1, 2, 3)][0] - stats[1][0] == l1 + 2 * l2
    # four further layers / six: each at least 2 LayerNorm passes, 4 GEMMs and the attention
    assert stats[2][1] - stats[1][1] >= 4 * 7 and stats[(1, 2, 3)][1] - stats[2][1] >= 2 * 7


# ------------------------------------------------------------------------------------------------ the default plan
def test_default_unet_through_create_ext3_keeps_its_plan(device):
    """A D = 64, depth-1 UNet through kd_unet_create_ext3 with ext3 = NULL, with all-zero and with all-one depths: the
    launches and the bits of the plan kd_unet_create_ext2 builds (the entry Unet.engine() takes for such a UNet)."""
    lib = engine().load()
    ou = _ref_unet(H.UNET_KW["small2"], seed=4, lowres_cond=True)
    gen = H.gen(5)
    x, t = torch.randn(2, 3, 32, 32, generator=gen), torch.randn(2, generator=gen)
    kw = dict(lowres_cond_img=torch.randn(2, 3, 32, 32, generator=gen), lowres_noise_times=torch.full((2,), 1.5),
              cond_images=torch.rand(2, 3, 32, 32, generator=gen))
    dv = {k: v.to(device) for k, v in kw.items()}
    E = engine()
    ones = E.kd_unet_ext3_t()
    for i in range(E.KD_MAX_LEVELS):
        ones.layer_attns_depth[i] = 1
    zeros = E.kd_unet_ext3_t()
    orig, ext3_entry = lib.kd_unet_create_ext2, lib.kd_unet_create_ext3
    seen = []
    forms = {
        "ext2": orig,
        "null": lambda cfg, arr, n, share, ext, ext2, out: ext3_entry(cfg, arr, n, share, ext, ext2, None, out),
        "zeros": lambda cfg, arr, n, share, ext, ext2, out: ext3_entry(cfg, arr, n, share, ext, ext2, C.byref(zeros), out),
        "ones": lambda cfg, arr, n, share, ext, ext2, out: ext3_entry(cfg, arr, n, share, ext, ext2, C.byref(ones), out),
    }
    res = {}
    for name, fn in forms.items():
        pu = H.product_like(ou, device)
        lib.kd_unet_create_ext2 = lambda *a, fn=fn, name=name: (seen.append(name), fn(*a))[1]
        try:
            h = pu.engine(2, 32, device, with_text=False)
        finally:
            lib.kd_unet_create_ext2 = orig
        res[name] = (lib.kd_unet_num_launches(h), lib.kd_unet_macs(h), pu(x.to(device), t.to(device), **dv).cpu())
    assert seen == list(forms)
    for name in ("null", "zeros", "ones"):
        assert res[name][:2] == res["ext2"][:2], name
        assert torch.equal(res[name][2], res["ext2"][2]), name


def test_engine_refuses_what_python_refuses(device):
    """The plan builder's own refusals, reached past the Python checks: dim_head 48, and a depth on a linear-attention level."""
    pu = H.product_like(_ref_unet(BASE, seed=1), device)
    pu._plan["attn_dim_head"] = 48
    with pytest.raises(engine().EngineError, match="32, 64 and 128"):
        pu.engine(2, 32, device, with_text=False)
    import imagen_pytorch as ip

    lu = ip.Unet(**{**BASE, "layer_attns": (False, False, True)}, use_linear_attn=True, **H.NOTEXT).to(device)
    lu._plan["layer_attns_depth"] = (1, 2, 1)
    with pytest.raises(engine().EngineError, match="linear-attention level"):
        lu.engine(2, 32, device, with_text=False)


# ------------------------------------------------------------------------------------------------ sampling
def test_ddpm_text_guided_sampling_matches_the_oracle_and_graph_equals_eager(device):
    """Three DDPM steps with cond_scale = 3 on the text config at D = 128, depths (1, 2, 1)."""
    ou = _ref_unet(TEXT, seed=17, text=True, attn_dim_head=128, layer_attns_depth=(1, 2, 1))
    oim, pim = H.imagen_pair(device, RS.Imagen, "Imagen", [ou], image_sizes=(32,), timesteps=(3,), text_embed_dim=3)
    text = torch.tensor([[0.0, 0.5, 0.2], [0.3, -0.4, 0.9]]).reshape(2, 1, 3)
    nf = RS.generator_noise_fn(5)
    ref = oim.sample(noise_fn=nf, text_embeds=text, cond_scale=3.0)
    got = pim.sample(noise_fn=nf, text_embeds=text.to(device), cond_scale=3.0, device=device)
    err = float((got.cpu() - ref).abs().max())
    print(f"DDPM text D128 depth (1, 2, 1), cond_scale 3, T=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert torch.equal(got, pim.sample(noise_fn=nf, text_embeds=text.to(device), cond_scale=3.0, use_graph=False, device=device))


def test_ddpm_inpainting_matches_the_oracle_and_graph_equals_eager(device):
    """Three DDPM steps with inpainting, 2 resamples, at D = 32, depth 2."""
    ou = _ref_unet(BASE, seed=21, attn_dim_head=32, layer_attns_depth=2)
    oim, pim = H.imagen_pair(device, RS.Imagen, "Imagen", [ou], image_sizes=(32,), timesteps=(3,), condition_on_text=False)
    gen = H.gen(3)
    inp = torch.rand(2, 3, 32, 32, generator=gen)
    mask = torch.zeros(2, 32, 32, dtype=torch.bool)
    mask[:, 4:20, 6:30] = True
    nf = RS.generator_noise_fn(7)
    kw = dict(batch_size=2, inpaint_resample_times=2)
    ref = oim.sample(noise_fn=nf, inpaint_images=inp, inpaint_masks=mask, **kw)
    got = pim.sample(noise_fn=nf, inpaint_images=inp.to(device), inpaint_masks=mask.to(device), device=device, **kw)
    err = float((got.cpu() - ref).abs().max())
    print(f"DDPM D32 depth 2, inpainting R=2, T=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert torch.equal(got, pim.sample(noise_fn=nf, inpaint_images=inp.to(device), inpaint_masks=mask.to(device), use_graph=False,
                                       device=device, **kw))


def test_edm_sampling_matches_the_restatement_and_graph_equals_eager(device):
    """ElucidatedImagen, N = 3, at D = 128, depth (1, 1, 2)."""
    ou = _ref_unet(BASE, seed=23, attn_dim_head=128, layer_attns_depth=(1, 1, 2))
    oim, pim = H.imagen_pair(device, ER.ElucidatedImagen, "ElucidatedImagen", [ou], image_sizes=(32,), condition_on_text=False,
                             num_sample_steps=3)
    nf = RS.generator_noise_fn(13)
    ref = oim.sample(noise_fn=nf, batch_size=2)
    got = pim.sample(noise_fn=nf, batch_size=2, device=device)
    err = float((got.cpu() - ref).abs().max())
    print(f"EDM D128 depth (1, 1, 2), N=3: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    assert torch.equal(got, pim.sample(noise_fn=nf, batch_size=2, use_graph=False, device=device))


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_loads_a_d32_depth2_checkpoint_strictly_and_samples_from_it(device, tmp_path, capsys):
    import imagen_pytorch as ip

    kw = dict(image_sizes=(32,), timesteps=(3,), condition_on_text=False)
    online, ema_u = (_ref_unet(BASE, seed=s, attn_dim_head=32, layer_attns_depth=2) for s in (31, 32))
    oim_online, oim_ema = RS.Imagen([online], **kw), RS.Imagen([ema_u], **kw)
    ema = {f"0.ema_model.{k}": v for k, v in ema_u.state_dict().items()}
    path = tmp_path / "ckpt.pt"
    torch.save({"model": oim_online.state_dict(), "ema": ema, "version": ip.__version__, "steps": torch.tensor([3])}, path)
    pim = ip.Imagen([ip.Unet(**online._locals)], **kw).to(device)
    trainer = ip.ImagenTrainer(imagen=pim)
    capsys.readouterr()
    trainer.load(str(path), strict=True)
    out = capsys.readouterr().out
    assert "Trying partial load" not in out and "library fork" not in out, out
    got_sd = trainer.imagen.unets[0].state_dict()
    assert all(torch.equal(got_sd[k].cpu(), v) for k, v in online.state_dict().items())
    nf = RS.generator_noise_fn(11)
    ref = oim_ema.sample(noise_fn=nf, batch_size=2)
    got = trainer.sample(batch_size=2, noise_fn=nf).cpu()
    err = float((got - ref).abs().max())
    print(f"trainer.sample from the EMA weights, D32 depth 2: max|diff| {err:.2e}")
    assert err < SAMPLE_ABS
    # a default UNet does not take the checkpoint silently
    plain = ip.ImagenTrainer(imagen=ip.Imagen([ip.Unet(**{**online._locals, "layer_attns_depth": 1})], **kw))
    capsys.readouterr()
    try:
        plain.load(str(path), strict=True)
    except RuntimeError:
        return
    assert "Trying partial load" in capsys.readouterr().out
