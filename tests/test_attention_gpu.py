"""The attention core and the qk-norm as the plan launches them, through kd_attention_ex / kd_l2norm_heads
(include/kd_engine.h), against fp64 torch on the same fp32 inputs.

kd_attention (test_kernels_gpu.py::test_attention) reaches launch_attention with one dense K/V segment, no null key and
scale 1.  The plan's launches look different (engine.hip transformer() / cross_attn(), text_build.inc): a learned null
key in front of the key list, two K/V segments with their own row strides, q and k | v as column slices of one fused
buffer, one shared K/V head or H of them, and a scale of 1/8, 16 or 8.  Here every tensor sits in a NaN-filled buffer
with the plan's row stride: a read outside a slice poisons the output, a write outside it destroys a NaN.

Layouts (inner = H * 64):
  "self"   transformer(): Hkv = 1.  q | k | v are columns [0, inner) | [inner, inner + 64) | [inner + 64, inner + 128) of
           one buffer of row stride inner + 128 (segment 1: the feature tokens); the context tokens' k | v are the two
           halves of rows of stride 128 (segment 0); null key.
  "cross"  cross_attn(): Hkv = H.  q dense (stride inner); k | v the two halves of rows of stride 2 * inner
           (segment 0); null key; no segment 1.
  "text"   the PerceiverResampler of text_build.inc: as "cross" without the null key and with the latents' k | v, same
           form, as segment 1.
The sweeps below also run "cross" buffers with a second segment and a null key: not a launch of the plan, but the
Hkv = H addressing of both segments.  `pad` extra NaN columns can follow every row (stride = the plan's + pad); the
output buffer always has 8, and one guard row.

Tolerance: test_attention's rtol 1e-4, atol 2e-5 for every case, no family needs more (measured on an MI355X: the
worst of the 224 launches of this file uses 0.09 of it, the fp32 torch evaluation of the same inputs 0.11; every test
prints its figure).
"""
import pytest
import torch
import torch.nn.functional as F

import attention_cases as AC
import helpers as H

pytestmark = pytest.mark.gpu

D = 64
RTOL, ATOL = 1e-4, 2e-5   # test_kernels_gpu.py::test_attention


engine = H.engine   # (H is the head count inside the functions below)


@pytest.fixture(scope="module")
def lib():
    return engine().load()


# (B, Nq, H): which kernel launch_attention picks (kernels_attn.hip: matrix cores from Nq >= 128 and at least 16 blocks
# of 128 queries, else attention_kernel<4>)
QSHAPES = {
    "vec70": (2, 70, 4),      # Nq < 128
    "vec130": (1, 130, 2),    # Nq >= 128 but 4 blocks
    "mfma200": (2, 200, 4),   # 16 blocks; Nq % 128 != 0 and Nq % 32 != 0 (last wave a quarter full)
    "mfma256": (1, 256, 8),   # 16 blocks, all full
}


def test_query_shapes_reach_both_kernels():
    assert [AC.is_mfma(*QSHAPES[n]) for n in ("vec70", "vec130", "mfma200", "mfma256")] == [False, False, True, True]
    assert AC.is_mfma(1, 4096, 8) and not AC.is_mfma(1, 64, 8)


# ------------------------------------------------------------------------------------------------ device buffers
NAN = float("nan")


class _Bufs:
    """The NaN-filled device buffers of one launch and the slices the kernel may touch."""

    def __init__(self, device, layout, q, nkv, k0, v0, k1, v1, pad):
        B, Nq, H, _ = q.shape
        Hkv, n0, n1 = k0.shape[2], k0.shape[1], k1.shape[1]
        inner = H * D
        self.B, self.Nq, self.H, self.Hkv, self.n0, self.n1, self.inner = B, Nq, H, Hkv, n0, n1, inner
        nan = lambda rows, cols: torch.full((max(rows, 1), cols), NAN, device=device)
        if layout == "self":
            assert Hkv == 1
            self.ldq = self.ld1 = inner + 2 * D + pad
            self.qkv = nan(B * max(Nq, n1), self.ldq)
            self.qkv[:B * Nq, :inner] = q.reshape(B * Nq, inner).to(device)
            self.qkv[:B * n1, inner:inner + D] = k1.reshape(B * n1, D).to(device)
            self.qkv[:B * n1, inner + D:inner + 2 * D] = v1.reshape(B * n1, D).to(device)
            self.q_ptr, self.k1_ptr, self.v1_ptr = (self.qkv.data_ptr() + 4 * off for off in (0, inner, inner + D))
            self.ld0 = 2 * D + pad
            self.ckv = nan(B * n0, self.ld0)
            self.ckv[:B * n0, :D] = k0.reshape(B * n0, D).to(device)
            self.ckv[:B * n0, D:2 * D] = v0.reshape(B * n0, D).to(device)
            self.k0_ptr, self.v0_ptr = self.ckv.data_ptr(), self.ckv.data_ptr() + 4 * D
        else:
            assert layout == "cross" and Hkv == H
            self.ldq = inner + pad
            self.qb = nan(B * Nq, self.ldq)
            self.qb[:, :inner] = q.reshape(B * Nq, inner).to(device)
            self.q_ptr = self.qb.data_ptr()
            self.ld0 = self.ld1 = 2 * inner + pad
            self.kv0, self.kv1 = nan(B * n0, self.ld0), nan(B * n1, self.ld1)
            for buf, k, v, n in ((self.kv0, k0, v0, n0), (self.kv1, k1, v1, n1)):
                buf[:B * n, :inner] = k.reshape(B * n, inner).to(device)
                buf[:B * n, inner:2 * inner] = v.reshape(B * n, inner).to(device)
            self.k0_ptr, self.v0_ptr = self.kv0.data_ptr(), self.kv0.data_ptr() + 4 * inner
            self.k1_ptr, self.v1_ptr = self.kv1.data_ptr(), self.kv1.data_ptr() + 4 * inner
        self.nkv = nkv.contiguous().to(device) if nkv is not None else None
        self.ldo = inner + 8
        self.out = nan(B * Nq + 1, self.ldo)   # (+ one guard row)

    def launch(self, lib, scale):
        import ctypes as C

        E = engine()
        p = lambda a, n: C.c_void_p(a) if n else None   # an empty segment goes in as NULL pointers
        return lib.kd_attention_ex(C.c_void_p(self.q_ptr), self.ldq, E.ptr(self.nkv), p(self.k0_ptr, self.n0),
                                   p(self.v0_ptr, self.n0), self.ld0, self.n0, p(self.k1_ptr, self.n1), p(self.v1_ptr, self.n1),
                                   self.ld1, self.n1, E.ptr(self.out), self.ldo, self.B, self.Nq, self.H, self.Hkv, scale,
                                   E.current_stream())

    def result(self):
        """The output slice, after checking that nothing outside it was written and everything inside it was."""
        out = self.out.cpu()
        rows = self.B * self.Nq
        assert bool(out[:rows, self.inner:].isnan().all()) and bool(out[rows:].isnan().all()), "a write outside the output slice"
        got = out[:rows, :self.inner]
        assert bool(got.isfinite().all()), "an element of the output slice was not written, or a read left the input slices"
        return got.reshape(self.B, self.Nq, self.H, D).double()


def _check(lib, device, layout, family, qshape, Hkv_is_H, null, n0, n1, pad, seed, marker=None, tag=""):
    B, Nq, H = qshape
    Hkv = H if Hkv_is_H else 1
    q, nkv, k0, v0, k1, v1, scale = AC.inputs(D, family, B, Nq, H, Hkv, null, n0, n1, seed, marker)
    bufs = _Bufs(device, layout, q, nkv, k0, v0, k1, v1, pad)
    engine().check(bufs.launch(lib, scale))
    got = bufs.result()
    ref = AC.reference(q, nkv, k0, v0, k1, v1, scale)
    used = float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())
    print(f"attention {layout} {family}{tag} B{B} Nq{Nq} H{H} Hkv{Hkv} keys {int(null)}+{n0}+{n1} "
          f"{'mfma' if AC.is_mfma(B, Nq, H) else 'vec4'}: max|err| {float((got - ref).abs().max()):.2e}, {used:.3f} of the bound")
    assert torch.allclose(got, ref, rtol=RTOL, atol=ATOL), used


# ------------------------------------------------------------------------------------------------ the plan's launch forms
@pytest.mark.parametrize("form,qshape,null,n0,n1", [
    # transformer() of the 64 x 64 level of the base UNet: 4096 feature tokens, 2 time tokens as context, 1 + 2 + 4096 keys
    ("self", (1, 4096, 8), True, 2, 4096),
    ("self", (1, 64, 8), True, 2, 4096),        # the same key list under the vector kernel
    ("self", (2, 256, 8), True, 2, 256),        # a 16 x 16 level, batch 2
    ("self", (2, 64, 8), True, 0, 64),          # transformer() without context: segment 0 empty, NULL pointers
    ("cross", (2, 1024, 8), True, 2, 0),        # cross_attn(): 3 keys, matrix cores
    ("cross", (1, 64, 8), True, 34, 0),         # ... to pooled text tokens, vector kernel
    ("text", (2, 34, 8), False, 77, 34),        # PerceiverResampler: text tokens, then the latents themselves
    ("text", (2, 34, 8), False, 77, 0),
])
@pytest.mark.parametrize("family", ["plain", "cos16"])
def test_plan_launch_forms(lib, device, form, qshape, null, n0, n1, family):
    """Self-attention with context (transformer()), cross-attention (cross_attn()) and text pooling (text_build.inc)
    with the plan's own strides (pad = 0): ldq = ld1 = inner + 128 and ld0 = 128; ldq = inner and ld0 = 2 inner."""
    layout = "self" if form == "self" else "cross"
    _check(lib, device, layout, family, qshape, form != "self", null, n0, n1, 0, 101)


# ------------------------------------------------------------------------------------------------ key counts and boundaries
# (null, n0, n1): the key list has null + n0 + n1 keys in tiles of 64; segment 1 starts at key null + n0
KEYS = [
    (True, 0, 0),       # 1: the null key alone, both segments empty
    (True, 1, 0),       # 2
    (True, 0, 1),       # 2, segment 0 empty
    (True, 1, 1),       # 3
    (True, 2, 60),      # 63
    (True, 62, 1),      # 64: segment 1 is the last row of the tile
    (True, 63, 1),      # 65: segment 1 starts at the first row of the second tile
    (True, 2, 124),     # 127
    (True, 127, 0),     # 128, segment 1 empty
    (True, 63, 64),     # 128: boundary at a tile's first row
    (True, 62, 66),     # 129: boundary at a tile's last row
    (True, 30, 98),     # 129: boundary inside a tile
    (False, 64, 65),    # 129 without the null key: boundary at a tile's first row
    (False, 0, 63),     # 63, no null key, segment 0 empty
]


@pytest.mark.parametrize("null,n0,n1", KEYS)
@pytest.mark.parametrize("qname", ["vec70", "mfma200"])
@pytest.mark.parametrize("Hkv_is_H", [False, True])
def test_key_counts_and_segment_boundaries(lib, device, null, n0, n1, qname, Hkv_is_H):
    """Both kernels, Hkv = 1 and H, over key counts 1, 2, 3, 63, 64, 65, 127, 128, 129 with the segment boundary at a
    tile's first row, last row and inside it, and either segment empty; the three dense input families, strides padded."""
    for family in ("plain", "cos16", "ascending"):
        _check(lib, device, "cross" if Hkv_is_H else "self", family, QSHAPES[qname], Hkv_is_H, null, n0, n1, 4, 202)


@pytest.mark.parametrize("qname", ["vec130", "mfma256"])
@pytest.mark.parametrize("Hkv_is_H", [False, True])
def test_other_query_counts(lib, device, qname, Hkv_is_H):
    """Nq >= 128 on too few blocks for the matrix cores, and a launch of full 128-query blocks."""
    for family in ("plain", "ascending"):
        _check(lib, device, "cross" if Hkv_is_H else "self", family, QSHAPES[qname], Hkv_is_H, True, 30, 98, 4, 303)


# ------------------------------------------------------------------------------------------------ one key that matters
# keys 1 + 40 + 150 = 191: three tiles, the boundary (key 41) inside the first
MARKERS = {"null": 0, "seg0_last": 40, "seg1_first": 41, "seg1_last": 190, "tile_row63": 63, "tile_row64": 64}


@pytest.mark.parametrize("where", list(MARKERS))
@pytest.mark.parametrize("qname", ["vec70", "mfma200"])
@pytest.mark.parametrize("Hkv_is_H", [False, True])
def test_marker_key(lib, device, where, qname, Hkv_is_H):
    """One key holds most of the softmax and has a value row of its own: a key that is dropped, read twice or taken from
    the wrong segment moves the output by O(1) however long the key list is."""
    _check(lib, device, "cross" if Hkv_is_H else "self", "marker", QSHAPES[qname], Hkv_is_H, True, 40, 150, 4, 404,
           marker=MARKERS[where], tag=f"@{where}")


@pytest.mark.parametrize("where,marker", [("seg0_last", 2), ("seg1_first", 3), ("seg1_last", 4098)])
@pytest.mark.parametrize("qshape", [(1, 4096, 2), (1, 64, 2)])
def test_marker_key_at_plan_size(lib, device, where, marker, qshape):
    """The same at 1 + 2 + 4096 keys, on both kernels."""
    _check(lib, device, "self", "marker", qshape, False, True, 2, 4096, 0, 505, marker=marker, tag=f"@{where}")


# ------------------------------------------------------------------------------------------------ refusals
def test_attention_ex_refuses_what_the_kernels_cannot_do(lib, device):
    E = engine()
    B, Nq, H = 1, 8, 8
    q, nkv, k0, v0, k1, v1, scale = AC.inputs(D, "plain", B, Nq, H, H, True, 4, 4, 7)
    bufs = _Bufs(device, "cross", q, nkv, k0, v0, k1, v1, 0)
    assert bufs.launch(lib, scale) == 0
    bufs.Hkv = 3
    assert bufs.launch(lib, scale) != 0 and b"Hkv must be 1" in lib.kd_last_error()
    bufs.Hkv = H
    for name in ("ldq", "ld0", "ld1", "ldo"):
        keep = getattr(bufs, name)
        setattr(bufs, name, keep + 2)
        assert bufs.launch(lib, scale) != 0 and b"strides % 4" in lib.kd_last_error(), name
        setattr(bufs, name, keep)
    bufs.n0 = bufs.n1 = 0
    bufs.nkv = None
    assert bufs.launch(lib, scale) != 0 and b"attention: empty" in lib.kd_last_error()
    bufs.out = bufs.out.clone()
    bufs.nkv = nkv.to(device)   # one key is enough
    E.check(bufs.launch(lib, scale))
    assert torch.allclose(bufs.result(), nkv[1].double().expand(B, Nq, H, D), rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ qk-norm
L2_REL = 1e-6   # fp32 torch is 5e-8 from fp64 on such inputs: an order of magnitude for the shuffle tree's summation order
SENTINEL = 777.0


@pytest.mark.parametrize("heads,extra,rows", [
    (1, 0, 7),      # rows * heads = 7: the last block has one idle wave
    (1, 12, 9),     # strided rows
    (3, 8, 5),      # 15 segments
    (8, 0, 6),      # dense [rows][512]
    (8, 128, 33),   # the q slice of the fused q | k | v buffer
    (1, 512 + 64, 37),   # its k slice: one head at stride inner + 128, in front of v
])
@pytest.mark.parametrize("with_scale", [False, True])
def test_l2norm_heads(lib, device, heads, extra, rows, with_scale):
    """kd_l2norm_heads against fp64 F.normalize(x, dim=-1, eps=1e-12) * scale_vec per 64-wide head segment: strided rows
    whose other columns keep their sentinel, a segment count that does not fill the last block, an all-zero segment (0, not
    NaN) and a segment of norm 1e-13, below the floor (x / 1e-12, not a unit vector)."""
    E = engine()
    gen = H.gen(17 + heads + rows)
    ld = heads * D + extra
    x = torch.randn(rows, heads, D, generator=gen) * torch.logspace(-3, 3, rows * heads).reshape(rows, heads, 1)
    zero_at, tiny_at = (1, 0), (rows - 1, heads - 1)
    x[zero_at] = 0
    x[tiny_at] = torch.randn(D, generator=gen) * (1e-13 / 8)
    sv = 1 + 0.3 * torch.randn(D, generator=gen) if with_scale else None
    ref = F.normalize(x.double(), dim=-1, eps=1e-12) * (sv.double() if with_scale else 1.0)
    buf = torch.full((rows, ld), SENTINEL)
    buf[:, :heads * D] = x.reshape(rows, heads * D)
    buf = buf.to(device)
    svd = sv.to(device) if with_scale else None
    E.check(lib.kd_l2norm_heads(E.ptr(buf), ld, rows, heads, E.ptr(svd), E.current_stream()))
    out = buf.cpu()
    assert bool((out[:, heads * D:] == SENTINEL).all()), "a write outside the head segments"
    got = out[:, :heads * D].reshape(rows, heads, D)
    assert bool((got[zero_at] == 0).all())
    tiny_norm = float(x[tiny_at].double().norm())   # below the floor: x / 1e-12, a vector of norm 0.1, not a unit vector
    assert 0.5e-13 < tiny_norm < 2e-13
    assert abs(float((got[tiny_at].double() / (sv.double() if with_scale else 1.0)).norm()) - tiny_norm / 1e-12) < 1e-6
    err, err_tiny = AC.rel(got, ref), AC.rel(got[tiny_at], ref[tiny_at])
    worst = max(AC.rel(got[r, h], ref[r, h]) for r in range(rows) for h in range(heads) if (r, h) != zero_at)
    print(f"l2norm heads {heads} ld {ld} rows {rows} scale {with_scale}: rel-L2 {err:.2e}, worst segment {worst:.2e}, "
          f"below the floor {err_tiny:.2e}")
    assert err < L2_REL and worst < L2_REL


def test_l2norm_heads_of_the_null_key(lib, device):
    """null_kv_of (engine.hip): the [2][64] null key / value as one row of stride 128 with one head - the value stays."""
    E = engine()
    nkv = torch.randn(2, D, generator=H.gen(23)) * 3
    sv = 1 + 0.3 * torch.randn(D, generator=H.gen(24))
    buf, svd = nkv.to(device), sv.to(device)
    E.check(lib.kd_l2norm_heads(E.ptr(buf), 2 * D, 1, 1, E.ptr(svd), E.current_stream()))
    out = buf.cpu()
    assert torch.equal(out[1], nkv[1])
    assert AC.rel(out[0], F.normalize(nkv[0].double(), dim=-1, eps=1e-12) * sv.double()) < L2_REL


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("qshape", [(2, 70, 4), (2, 200, 4)])
def test_qk_norm_then_attention_is_cosine_sim_attention(lib, device, qshape):
    """transformer() under attn_qk_norm = 1: kd_l2norm_heads in place on the q slice (H heads) and the k slices (one head)
    of the fused buffers and on the null key, then kd_attention_ex with scale 16, against fp64 cosine-similarity attention
    of the raw inputs."""
    import ctypes as C

    E = engine()
    B, Nq, H = qshape
    n0, n1 = 2, Nq
    q, nkv, k0, v0, k1, v1, _ = AC.inputs(D, "ascending", B, Nq, H, 1, True, n0, n1, 606)
    bufs = _Bufs(device, "self", q, nkv, k0, v0, k1, v1, 0)
    s = E.current_stream()
    E.check(lib.kd_l2norm_heads(C.c_void_p(bufs.q_ptr), bufs.ldq, B * Nq, H, None, s))
    E.check(lib.kd_l2norm_heads(C.c_void_p(bufs.k1_ptr), bufs.ld1, B * n1, 1, None, s))
    E.check(lib.kd_l2norm_heads(C.c_void_p(bufs.k0_ptr), bufs.ld0, B * n0, 1, None, s))
    E.check(lib.kd_l2norm_heads(E.ptr(bufs.nkv), 2 * D, 1, 1, None, s))
    E.check(bufs.launch(lib, 16.0))
    got = bufs.result()
    nrm = lambda t: F.normalize(t.double(), dim=-1, eps=1e-12)
    ref = AC.reference(nrm(q), torch.stack([nrm(nkv[0]), nkv[1].double()]), nrm(k0), v0, nrm(k1), v1, 16.0)
    used = float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())
    print(f"qk-norm + attention B{B} Nq{Nq} H{H}: {used:.3f} of the bound")
    assert torch.allclose(got, ref, rtol=RTOL, atol=ATOL), used
    # v and the columns the norm must not touch: still what went in
    inner = H * D
    assert torch.equal(bufs.qkv[:B * n1, inner + D:inner + 2 * D].cpu(), v1.reshape(B * n1, D))
    assert torch.equal(bufs.ckv[:B * n0, D:].cpu(), v0.reshape(B * n0, D))
