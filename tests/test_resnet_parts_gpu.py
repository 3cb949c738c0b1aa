"""GPU parity of the pieces a ResnetBlock of the plan is joined from - the skinny linears, the GlobalContext gate, the gated
residual add with its GroupNorm partials, the GroupNorm fold from segment partials and the F(4x4,3x3) conv with the
GroupNorm / FiLM / SiLU affine folded into its input transform - each through its C ABI entry (include/kd_engine.h) against
plain torch in fp64 on the host.  Inside a whole UNet forward these only answer to one rel-L2 of the final output; here every
unit answers for itself, at the shapes the benchmarked plan runs them."""
import math

import pytest
import torch
import torch.nn.functional as F

import helpers as H

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24   # one fp32 rounding, relative


engine, g, dp, nan_dev = H.engine, H.gen, H.dev_ptr, H.nan_dev   # (H is the image height in the tests below)


@pytest.fixture(scope="module")
def lib():
    return engine().load()


def act64(v, act):
    return {0: lambda t: t, 1: F.silu, 2: lambda t: F.gelu(t), 3: torch.sigmoid}[act](v)


# ---------------------------------------------------------------------------------------------------- skinny linears
# (M, K, N, ldx, ldy, x offset in floats, in_act, act): every branch of launch_linear_skinny's dispatch
SKINNY = [
    pytest.param(1, 1024, 1024, 0, 0, 0, 1, 0, id="gemv-M1"),
    pytest.param(1, 100, 37, 0, 0, 0, 0, 3, id="gemv-M1-ragged-N-sigmoid"),
    pytest.param(16, 256, 96, 0, 0, 0, 1, 1, id="mfma-KW1-silu-silu"),
    pytest.param(16, 480, 3, 0, 0, 0, 0, 2, id="mfma-KW1-N3-gelu"),
    pytest.param(16, 512, 37, 0, 0, 0, 1, 0, id="mfma-KW4-N37"),
    pytest.param(16, 1028, 200, 0, 0, 0, 0, 3, id="mfma-KW4-K-not-per-wave-multiple"),
    pytest.param(32, 640, 64, 0, 0, 0, 0, 2, id="mfma-M32"),
    pytest.param(33, 512, 96, 0, 0, 0, 1, 1, id="mfma-M33-second-row-tile"),
    pytest.param(16, 512, 96, 520, 100, 0, 0, 0, id="mfma-strided-ldx-ldy"),
    pytest.param(4, 130, 40, 0, 0, 0, 1, 2, id="valu-K-odd"),
    pytest.param(8, 256, 64, 0, 0, 1, 0, 1, id="valu-x-offset-one-float"),
    pytest.param(33, 99, 37, 101, 41, 1, 1, 3, id="valu-M33-strided"),
    # the C3 UNet's real shapes (batch 16): the learned-sinusoid MLP, the time-conditioning / time-token projections, the
    # GlobalContext FCs of the pooling path, and the widest - every ResnetBlock's time MLP stacked into one launch
    pytest.param(16, 17, 1024, 0, 0, 0, 0, 1, id="c3-sinu-mlp"),
    pytest.param(16, 1024, 1024, 0, 0, 0, 0, 0, id="c3-time-cond"),
    pytest.param(16, 1024, 256, 0, 0, 0, 0, 0, id="c3-time-tokens"),
    pytest.param(16, 1024, 512, 0, 0, 0, 0, 1, id="c3-gca-fc1"),
    pytest.param(16, 512, 1024, 0, 0, 0, 0, 3, id="c3-gca-fc2"),
    pytest.param(16, 1024, "c3", 0, 0, 0, 1, 0, id="c3-stacked-time-mlps"),
    # text_to_cond (text_build.inc), the one launch whose row count grows with the input: M = B L tokens, K = text_embed_dim,
    # N = cond_dim.  K = 3 runs on the VALU kernel, K = 16 and 768 on the matrix cores with 8 and 16 row tiles
    pytest.param(231, 3, 64, 0, 0, 0, 0, 0, id="text-to-cond-M231-K3"),
    pytest.param(512, 3, 512, 0, 0, 0, 0, 0, id="text-to-cond-M512-K3"),
    pytest.param(231, 768, 64, 0, 0, 0, 0, 0, id="text-to-cond-M231-K768"),
    pytest.param(512, 16, 512, 0, 0, 0, 0, 0, id="text-to-cond-M512-K16"),
]


def _c3_stacked_time_mlp_width():
    """N of the plan's stacked time-MLP launch, read off the C3 UNet's parameter tree (engine.hip collect_time_mlps)."""
    import bench

    u = bench.build_unet(0)
    sd = u.state_dict()
    tcd = next(v.shape[1] for k, v in sd.items() if k.endswith(".time_mlp.1.weight"))
    assert tcd == 1024
    return sum(v.shape[0] for k, v in sd.items() if k.endswith(".time_mlp.1.weight"))


@pytest.mark.parametrize("M,K,N,ldx,ldy,xoff,in_act,act", SKINNY)
def test_linear_skinny_matches_fp64(lib, device, M, K, N, ldx, ldy, xoff, in_act, act):
    E = engine()
    if N == "c3":
        N = _c3_stacked_time_mlp_width()
        assert N == 27648, N   # (the plan's label "skinny M16 K1024 N27648")
    ldx, ldy = ldx or K, ldy or N
    x = torch.randn(M, ldx, generator=g(1)) * 1.5
    w = torch.randn(N, K, generator=g(2)) * K ** -0.5
    b = torch.randn(N, generator=g(3)) * 0.3
    xbuf = torch.zeros(M * ldx + 4, device=device)
    xv = xbuf[xoff:xoff + M * ldx].view(M, ldx)
    xv.copy_(x.to(device))
    wd, bd = w.to(device), b.to(device)
    y = nan_dev(M, ldy)
    E.check(lib.kd_linear_skinny(dp(xv), ldx, dp(wd), dp(bd), dp(y), ldy, M, K, N, in_act, act, E.current_stream()))
    got = y.cpu().double()
    assert torch.isnan(got[:, N:]).all(), "wrote past N in a row"
    got = got[:, :N]
    assert torch.isfinite(got).all(), "output not written everywhere"
    fx = act64(x[:, :K].double(), in_act)
    z = fx @ w.double().T + b.double()
    ref = act64(z, act)
    f32 = act64(act64(x[:, :K], in_act) @ w.T + b, act).double()
    # |err| per element against what it scales with: sum_k |f(x)| |w| + |bias| (the activation's slope is at most 1.13) and
    # the output itself (the activation's own rounding)
    scale = (fx.abs() @ w.double().abs().T + b.double().abs()) + ref.abs()
    e_k = float(((got - ref).abs() / scale).max())
    e_32 = float(((f32 - ref).abs() / scale).max())
    print(f"skinny M{M} K{K} N{N} in_act {in_act} act {act}: max err / scale {e_k:.2e} (fp32 torch {e_32:.2e})")
    # bound: twice fp32 torch's error, or 4 fp32 roundings of the scale where that is below it (short K: another summation
    # order shows)
    assert e_k <= max(2.0 * e_32, 4 * U24), (e_k, e_32)


def test_linear_skinny_rejects_unsupported_shapes(lib, device):
    E = engine()
    t = torch.zeros(64, device=device)
    for M, K, N, ldx, ldy, ia, a in [(0, 16, 16, 16, 16, 0, 0), (4, 16, 16, 8, 16, 0, 0), (4, 16, 16, 16, 8, 0, 0),
                                     (4, 16, 16, 16, 16, 4, 0), (4, 16, 16, 16, 16, 0, -1)]:
        rc = lib.kd_linear_skinny(dp(t), ldx, dp(t), None, dp(t), ldy, M, K, N, ia, a, E.current_stream())
        assert rc != 0 and b"kd_linear_skinny" in lib.kd_last_error()


# ---------------------------------------------------------------------------------------------------- GlobalContext
# (B, HW, C): the C3 / unet3 plans' levels - 256^2 x 128 takes the C4 == 32 <1,2> template, 64^2 x 256 and 32^2 x 512
# (the largest C of the fused gate), 16^2 x 1024 (the pooling path), one 512^2 patch (exactly 1024 chunks, the merge
# kernels' se[1024]), a ragged map; 384^2 at batch 1: 576 chunks of 256 pixels, 1152 of 128 - the chunk count once went
# past se[1024] there (gca_rows)
GCA_SHAPES = [(16, 256 * 256, 128), (16, 64 * 64, 256), (16, 32 * 32, 512), (16, 16 * 16, 1024), (1, 512 * 512, 128),
              (3, 100, 96), pytest.param(1, 384 * 384, 128, id="chunks-past-1024-regression")]
_gca_x = {}


def _gca_input(B, HW, C):
    if (B, HW, C) not in _gca_x:
        gen = g(11)
        x = torch.randn(B, HW, C, generator=gen) + 0.3 * torch.randn(1, 1, C, generator=gen)
        _gca_x[B, HW, C] = x
    return _gca_x[B, HW, C]


def _gca_ref(x, wk, bk, w0, b0, w2, b2):
    logits = x @ wk + bk                                   # [B, HW]
    p = torch.softmax(logits, dim=-1)
    pooled = torch.einsum("bp,bpc->bc", p, x)
    hidden = F.silu(pooled @ w0.T + b0)
    return torch.sigmoid(hidden @ w2.T + b2), pooled, p


@pytest.mark.parametrize("B,HW,C", GCA_SHAPES)
@pytest.mark.parametrize("logits", ["plain", "peaked", "uniform"])
def test_global_context_gate_matches_fp64(lib, device, B, HW, C, logits):
    E = engine()
    hid = max(3, C // 2)
    x = _gca_input(B, HW, C)
    gen = g(12)
    wk = torch.randn(C, generator=gen) * C ** -0.5
    bk = torch.randn(1, generator=gen) * 0.1
    w0 = torch.randn(hid, C, generator=gen) * C ** -0.5
    b0 = torch.randn(hid, generator=gen) * 0.1
    w2 = torch.randn(C, hid, generator=gen) * hid ** -0.5
    b2 = torch.randn(C, generator=gen) * 0.5
    xd64 = x.double()
    if logits == "peaked":     # logits spanning +-80: a softmax on a handful of pixels, exp() down to e^-160 for the rest
        lg = xd64 @ wk.double()
        wk = (wk.double() * (80.0 / float(lg.abs().max()))).float()
    elif logits == "uniform":  # wk = 0: every pixel weighs the same, pooled = the mean over every chunk
        wk = torch.zeros(C)
    args64 = [t.double() for t in (wk, bk, w0, b0, w2, b2)]
    ref, pooled_ref, p = _gca_ref(xd64, *args64)
    g32, pooled32, _ = _gca_ref(x, wk, bk, w0, b0, w2, b2)
    # what the pooled vector's error scales with: sum_p p |x| (the weights' own error is relative)
    pscale = torch.einsum("bp,bpc->bc", p, xd64.abs())
    e32_pool = float(((pooled32.double() - pooled_ref).abs() / pscale).max())
    e32_gate = float((g32.double() - ref).abs().max())
    xd = x.to(device)
    dev = [t.to(device) for t in (wk, bk, w0, b0, w2, b2)]
    fused_ok = C <= 512 and hid <= 256
    outs = {}
    for path in ([1, 2] if fused_ok else [1]) + [0]:
        gate = nan_dev(B, C)
        pooled = nan_dev(B, C) if path == 1 else None
        E.check(lib.kd_global_context_gate(dp(xd), B, HW, C, dp(dev[0]), dp(dev[1]), dp(dev[2]), dp(dev[3]), hid, dp(dev[4]),
                                           dp(dev[5]), dp(gate), dp(pooled), path, E.current_stream()))
        got = gate.cpu().double()
        assert torch.isfinite(got).all(), f"path {path}: gate not written everywhere"
        outs[path] = gate.cpu()
        e_gate = float((got - ref).abs().max())
        msg = f"GlobalContext B{B} HW{HW} C{C} {logits} path {path}: gate max err {e_gate:.2e} (fp32 torch {e32_gate:.2e})"
        if path == 1:
            pg = pooled.cpu().double()
            assert torch.isfinite(pg).all(), "pooled not written everywhere"
            e_pool = float(((pg - pooled_ref).abs() / pscale).max())
            msg += f", pooled max err / sum p|x| {e_pool:.2e} (fp32 torch {e32_pool:.2e})"
            # fp32 online softmax over chunks of <= 256 rows merged over <= 1024 chunks: 4x fp32 torch's error, or 16 fp32
            # roundings of sum p |x| where that is below it
            assert e_pool <= max(4.0 * e32_pool, 16 * U24), (e_pool, e32_pool)
        print(msg)
        # the gate in (0, 1): 4x fp32 torch's error of the same chain, or 8 fp32 roundings of 1 where that is below it
        assert e_gate <= max(4.0 * e32_gate, 8 * U24), (path, e_gate, e32_gate)
    if 2 in outs:   # the two forms of the gate agree with each other to the same bound
        assert float((outs[1] - outs[2]).abs().max()) <= 2 * max(4.0 * e32_gate, 8 * U24)
    plan = 2 if fused_ok and B > 1 else 1   # path 0 is the plan's choice, bit for bit
    assert torch.equal(outs[0], outs[plan])


def test_global_context_gate_rejects_unsupported_shapes(lib, device):
    E = engine()
    t = torch.zeros(4096, device=device)
    for B, HW, C, hid, path in [(2, 16, 1024, 512, 2), (2, 16, 640, 320, 2), (2, 16, 64, 32, 3), (2, 16, 66, 33, 1),
                                (2, 16, 4096, 2048, 1), (0, 16, 64, 32, 1)]:
        rc = lib.kd_global_context_gate(dp(t), B, HW, C, dp(t), dp(t), dp(t), dp(t), hid, dp(t), dp(t), dp(t), None, path,
                                        E.current_stream())
        assert rc != 0 and b"kd_global_context_gate" in lib.kd_last_error()


# ---------------------------------------------------------------------------------------------------- gate_add
def _gate_add_rows_per_chunk(B, HW):
    """Pixel rows per partial chunk of launch_gate_add (kernels_norm.hip gate_add_rpb): the layout of its partials."""
    return min(64, max(8, (B * HW + 2047) // 2048))


@pytest.mark.parametrize("B,HW,C,gate,ldr,ldy", [
    (1, 1000, 64, True, 0, 0),          # C = 64: sixteen columns, sixteen rows per pass; HW not a multiple of the chunk
    (16, 1024, 512, True, 1024, 1024),  # the C3 32 x 32 level: r and y channel slices of concat buffers
    (16, 256, 1024, True, 0, 2048),     # 16 x 16 level, y into the first half of a concat
    (2, 300, 2048, True, 2560, 0),      # two column passes of 256 float4, ragged HW
    (1, 16384, 128, False, 0, 256),     # no gate (the plain residual add), batch 1
    (16, 4096, 256, True, 0, 0),        # the 64 x 64 level at batch 16
    (3, 77, 1280, True, 1280 + 64, 1280 + 128),   # 320 float4: a partial second pass
])
def test_gate_add_and_its_partials_match_fp64(lib, device, B, HW, C, gate, ldr, ldy):
    E = engine()
    ldr, ldy = ldr or C, ldy or C
    gen = g(21)
    a = torch.randn(B, HW, C, generator=gen)
    gt = torch.rand(B, C, generator=gen) if gate else None
    rbuf = torch.randn(B, HW, ldr, generator=gen) + 0.5
    r = rbuf[..., :C]
    ad, gd, rd = a.to(device), gt.to(device) if gate else None, rbuf.to(device)
    ybuf = nan_dev(B, HW, ldy)
    nch = lib.kd_gate_add_chunks(B, HW)
    rpc = _gate_add_rows_per_chunk(B, HW)
    assert nch == (HW + rpc - 1) // rpc
    seg = nan_dev(B, C // 16, nch, 2, dtype=torch.float64)
    E.check(lib.kd_gate_add_nhwc(dp(ad), dp(gd), dp(rd), ldr, dp(ybuf), ldy, dp(seg), B, HW, C, E.current_stream()))
    yb = ybuf.cpu()
    got = yb[..., :C].double()
    assert torch.isfinite(got).all(), "y not written everywhere"
    assert torch.isnan(yb[..., C:]).all(), "wrote past C in a row"
    prod = a.double() * (gt.double()[:, None, :] if gate else 1.0)
    ref = prod + r.double()
    # one fp32 rounding of the product and one of the sum (or one in all, fused)
    assert bool(((got - ref).abs() <= U24 * (prod.abs() + ref.abs())).all()), float((got - ref).abs().max())
    # partials: fp64 (sum, sum of squares) of the RETURNED y per (image, 16-channel segment, chunk of rpc pixels)
    pad = nch * rpc - HW
    yp = F.pad(got, (0, 0, 0, pad)).reshape(B, nch, rpc, C // 16, 16)
    s1 = yp.sum(dim=(2, 4)).permute(0, 2, 1)
    s2 = (yp * yp).sum(dim=(2, 4)).permute(0, 2, 1)
    sg = seg.cpu()
    assert torch.isfinite(sg).all(), "partials not written everywhere"
    a1 = yp.abs().sum(dim=(2, 4)).permute(0, 2, 1)
    # fp64 sums of fp32 values in another order: 1e-13 of sum |y| (fp64 rounding is 1.1e-16)
    e1 = float(((sg[..., 0] - s1).abs() / a1.clamp_min(1e-30)).max())
    e2 = float(((sg[..., 1] - s2).abs() / s2.clamp_min(1e-30)).max())
    print(f"gate_add B{B} HW{HW} C{C}: partials rel err {e1:.1e} / {e2:.1e}")
    assert e1 <= 1e-13 and e2 <= 1e-13, (e1, e2)
    # per group of 128 channels (G = C / 128 ... as the GroupNorm reading them sums): the group statistics
    G = max(1, C // 128)
    grp1 = sg[..., 0].reshape(B, G, -1).sum(-1)
    ref1 = got.reshape(B, HW, G, -1).sum(dim=(1, 3))
    assert torch.allclose(grp1, ref1, rtol=0, atol=1e-13 * float(got.abs().sum()))


def test_gate_add_rejects_unsupported_shapes(lib, device):
    E = engine()
    t = torch.zeros(4096, device=device)
    s = torch.zeros(64, dtype=torch.float64, device=device)
    for C, ldr, ldy, seg, off in [(62, 0, 0, False, 0), (40, 0, 0, True, 0), (64, 32, 0, False, 0), (64, 0, 66, False, 0),
                                  (64, 0, 0, False, 1)]:
        rc = lib.kd_gate_add_nhwc(dp(t[off:]), None, dp(t), ldr, dp(t), ldy, dp(s) if seg else None, 1, 8, C,
                                  E.current_stream())
        assert rc != 0 and b"kd_gate_add_nhwc" in lib.kd_last_error()


# ---------------------------------------------------------------------------------------------------- gn_fold_seg
def _partials(x, nchunk):
    """fp64 (sum, sum of squares) of x [B, HW, C] per image, 16-channel segment and chunk of HW / nchunk pixels:
    [B][C / 16][nchunk][2] - the producers' layout (SegSrc)."""
    B, HW, C = x.shape
    xs = x.double().reshape(B, nchunk, HW // nchunk, C // 16, 16)
    return torch.stack([xs.sum(dim=(2, 4)), (xs * xs).sum(dim=(2, 4))], dim=-1).permute(0, 2, 1, 3).contiguous()


def _gn_ref(xcat, G, eps):
    B, HW, C = xcat.shape
    grp = xcat.double().reshape(B, HW, G, C // G)
    mean = grp.mean(dim=(1, 3))
    var = grp.var(dim=(1, 3), unbiased=False)
    return mean, (var + eps).rsqrt()


@pytest.mark.parametrize("B,HW,C0,C1,nch0,nch1,G,scale1,abm,film,offset", [
    pytest.param(2, 256, 512, 0, 16, 0, 8, 1.0, 1.0, False, 0.0, id="one-source"),
    pytest.param(2, 256, 512, 0, 16, 0, 8, 1.0, 1.0, True, 0.0, id="one-source-film"),
    pytest.param(2, 256, 768, 512, 16, 64, 8, 2 ** -0.5, 1.0, True, 0.0, id="straddle-scaled-skip-abmul1"),
    pytest.param(2, 256, 768, 512, 16, 64, 8, 2 ** -0.5, 2 ** -0.5, True, 0.0, id="straddle-scaled-skip-abmul-scale"),
    pytest.param(3, 1024, 128, 128, 64, 16, 8, 1.0, 1.0, False, 0.0, id="two-sources-scale1"),
    pytest.param(1, 32768, 32, 0, 32768, 0, 2, 1.0, 1.0, False, 0.0, id="32768-partials-per-segment"),
    pytest.param(1, 32767, 16, 16, 32767, 32767, 1, 2 ** -0.5, 2 ** -0.5, False, 0.0, id="32767-partials-tail"),
    pytest.param(2, 512, 256, 256, 32, 8, 8, 2 ** -0.5, 2 ** -0.5, True, 36.0, id="mean-30x-std"),
])
def test_gn_fold_seg_matches_fp64(lib, device, B, HW, C0, C1, nch0, nch1, G, scale1, abm, film, offset):
    E = engine()
    C = C0 + C1
    gen = g(31)
    x0 = torch.randn(B, HW, C0, generator=gen) * 1.3 + 0.2 + offset
    x1 = torch.randn(B, HW, C1, generator=gen) * 0.7 - 0.4 + offset if C1 else None
    p0 = _partials(x0, nch0).to(device)
    p1 = _partials(x1, nch1).to(device) if C1 else None
    gamma = 1.0 + 0.2 * torch.randn(C, generator=gen)
    beta = 0.1 * torch.randn(C, generator=gen)
    ld_ss, col = 2 * C + 40, 24   # FiLM rows inside wider rows, at a column offset (the plan's stacked time MLPs)
    ssbuf = torch.randn(B, ld_ss, generator=gen) * 0.3
    ss = ssbuf[:, col:col + 2 * C]
    ssd = ssbuf.to(device)
    eps = 1e-5
    ab = nan_dev(B, C, 2)
    stats = nan_dev(B, G, 2)
    gd, bd = gamma.to(device), beta.to(device)
    E.check(lib.kd_gn_fold_seg(dp(p0), C0 // 16, nch0, 1.0, 1.0, dp(p1), C1 // 16, nch1, scale1, abm, dp(gd), dp(bd),
                               dp(ssd[:, col:]) if film else None, ld_ss, dp(ab), dp(stats), B, HW, C, G, eps,
                               E.current_stream()))
    xcat = torch.cat([x0.double()] + ([x1.double() * scale1] if C1 else []), dim=-1)
    mean, rstd = _gn_ref(xcat, G, eps)
    st = stats.cpu().double()
    assert torch.isfinite(st).all()
    em = float(((st[..., 0] - mean).abs() / (mean.abs() + 1.0 / rstd)).max())
    er = float(((st[..., 1] - rstd).abs() / rstd).max())
    # fp64 from the partials, rounded once to fp32 (mean relative to |mean| + std: its scale in the normalisation)
    assert em <= U24 and er <= 2 * U24, (em, er)
    # the affine as the fused kernel takes it: times WF_AB_SCALE = -log2(e)
    wf = lib.kd_wf_ab_scale()
    assert abs(wf + 1.0 / math.log(2.0)) < 1e-7
    m32, r32 = st[..., 0], st[..., 1]   # (what the kernel folds: its fp32 statistics)
    cg = torch.arange(C) // (C // G)
    a = r32[:, cg] * gamma.double()
    bb = beta.double() - m32[:, cg] * a
    if film:
        sc = ss[:, :C].double() + 1.0
        a, bb = a * sc, bb * sc + ss[:, C:].double()
    mul = torch.ones(C, dtype=torch.float64)
    mul[C0:] = abm
    A_ref, B_ref = a * mul * wf, bb * wf
    got = ab.cpu().double()
    assert torch.isfinite(got).all()
    # errors relative to the terms' magnitudes: sc = scale + 1 is itself rounded relative to |scale| + 1
    scm = (ss[:, :C].double().abs() + 1.0) if film else 1.0
    a0 = r32[:, cg] * gamma.double()
    ascale = (a0 * mul * wf).abs() * scm
    bscale = ((beta.double().abs() + (m32[:, cg] * a0).abs()) * scm + (ss[:, C:].double().abs() if film else 0.0)) * abs(wf)
    eA = float(((got[..., 0] - A_ref).abs() / ascale).max())
    eB = float(((got[..., 1] - B_ref).abs() / bscale).max())
    print(f"gn_fold_seg B{B} HW{HW} C{C0}+{C1} G{G}: mean {em:.1e} rstd {er:.1e} A {eA:.1e} B {eB:.1e}")
    # A: roundings of rstd gamma, scale + 1, the product, ab_mul, WF_AB_SCALE; B: of mean a, beta - mean a, sc, shift, WF
    assert eA <= 6 * U24 and eB <= 8 * U24, (eA, eB)


def test_gn_fold_seg_rejects_unsupported_shapes(lib, device):
    E = engine()
    t = torch.zeros(4096, device=device)
    s = torch.zeros(4096, dtype=torch.float64, device=device)
    for nseg0, nseg1, C, G, seg1, ld_ss in [(4, 0, 64, 8, False, 0), (4, 0, 48, 1, False, 0), (2, 2, 64, 2, False, 0),
                                            (2, 1, 64, 2, True, 0), (4, 0, 64, 2, False, 100)]:
        rc = lib.kd_gn_fold_seg(dp(s), nseg0, 4, 1.0, 1.0, dp(s) if seg1 else None, nseg1, 4, 1.0, 1.0, dp(t), dp(t),
                                dp(t) if ld_ss else None, ld_ss, dp(t), dp(t), 1, 64, C, G, 1e-5, E.current_stream())
        assert rc != 0 and b"kd_gn_fold_seg" in lib.kd_last_error()


# ---------------------------------------------------------------------------------------------------- F(4x4,3x3) chain
# The 56 F(4x4,3x3) ResnetBlock convs of the benchmarked plan (C3 SR UNet, batch 16; kd_unet_profile labels
# "wino4_in[3] M<B HW> Cin<..> Cout<..>"), by (H, Cin, Cout, channels of x, skip channels, skip scale) with their count:
#   256^2 128 -> 128 (3)   256 -> 128 = x 128 + the init conv's residual 128, unscaled (1, final_res_block)
#   128^2 128 -> 128 (9)   256 -> 128 = 128 + skip 128 x 2^-1/2 (3)
#    64^2 256 -> 256 (9)   512 -> 256 = 256 + 256 x 2^-1/2 (3)
#    32^2 512 -> 512 (9)  1024 -> 512 = 512 + 512 x 2^-1/2 (3)
#    16^2 1024 -> 1024 (13) 2048 -> 1024 = 1024 + 1024 x 2^-1/2 (3)
# gemm_mode the plan gives each (wino4_block: V as fp32 where Cin Cout < 40 (6 Cin + 4 Cout), planes elsewhere) and -1
# (fp32 MFMA); batch: the smallest the plan's tile rule (B (H/4) (W/4) % 256 == 0) allows.  Each case runs block1 of a
# ResnetBlock - GroupNorm(cat(x, skip s)) -> SiLU -> conv - from host-built fp64 partials of x and skip, then block2 -
# GroupNorm of block1's output from its own partials -> FiLM -> SiLU -> conv + residual.
WINO4_REL = 8e-6   # tests/test_kernels_gpu.py: F(4x4,3x3) re-association, fp32 (per conv rel-L2 against fp64)
SQ = 2 ** -0.5
CHAIN = [  # (B, H, Cx, Cskip, skip scale, Cout, gemm_mode, images_per_set)
    (1, 256, 128, 0, 1.0, 128, 2, 0),
    (1, 256, 128, 0, 1.0, 128, -1, 0),
    (1, 256, 128, 128, 1.0, 128, 2, 0),
    (1, 256, 128, 128, 1.0, 128, -1, 0),
    (1, 128, 128, 0, 1.0, 128, 2, 0),
    (1, 128, 128, 0, 1.0, 128, -1, 0),
    (1, 128, 128, 128, SQ, 128, 2, 0),
    (1, 128, 128, 128, SQ, 128, -1, 0),
    (2, 64, 256, 0, 1.0, 256, 2, 1),    # two sets of one image
    (2, 64, 256, 0, 1.0, 256, -1, 1),
    (1, 64, 256, 256, SQ, 256, 2, 0),
    (1, 64, 256, 256, SQ, 256, -1, 0),
    (4, 32, 512, 0, 1.0, 512, 1, 0),
    (4, 32, 512, 0, 1.0, 512, -1, 2),   # two sets of two images
    (4, 32, 512, 512, SQ, 512, 1, 0),
    (4, 32, 512, 512, SQ, 512, -1, 0),
    (16, 16, 1024, 0, 1.0, 1024, 1, 0),
    (16, 16, 1024, 0, 1.0, 1024, -1, 8),
    (16, 16, 1024, 1024, SQ, 1024, 1, 0),
    (16, 16, 1024, 1024, SQ, 1024, -1, 8),
]
_chain_ref = {}


def _block_ref(xin64, gamma, beta, G, ss, w, b, res):
    """conv3x3(SiLU(FiLM(GroupNorm(x)))) + b (+ res) in fp64, x NHWC [B, H, W, C]."""
    xn = F.group_norm(xin64.permute(0, 3, 1, 2), G, gamma.double(), beta.double(), eps=1e-5)
    if ss is not None:
        C = xin64.shape[-1]
        xn = xn * (ss[:, :C].double() + 1.0)[:, :, None, None] + ss[:, C:].double()[:, :, None, None]
    y = F.conv2d(F.silu(xn), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    return y + res.double() if res is not None else y


def _check_conv(tag, got, ref):
    err = float((got - ref).norm() / ref.norm())
    mx = float((got - ref).abs().max() / ref.abs().max())
    print(f"{tag}: rel-L2 {err:.2e}, max {mx:.2e}")
    assert err <= WINO4_REL, (tag, err)
    assert mx <= 5e-5, (tag, "element-wise outlier", mx)   # (5e-5 max|ref|: test_conv3x3_winograd4_matches_direct)


def _check_out_seg(tag, seg, y):
    """The output transform's partials [B][C/16][(H/4)(W/4)][2] against fp64 sums of the returned y."""
    B, H, W, C = y.shape
    yt = y.reshape(B, H // 4, 4, W // 4, 4, C // 16, 16)
    s1 = yt.sum(dim=(2, 4, 6)).permute(0, 3, 1, 2).reshape(B, C // 16, -1)
    s2 = (yt * yt).sum(dim=(2, 4, 6)).permute(0, 3, 1, 2).reshape(B, C // 16, -1)
    a1 = yt.abs().sum(dim=(2, 4, 6)).permute(0, 3, 1, 2).reshape(B, C // 16, -1)
    sg = seg.cpu()
    assert torch.isfinite(sg).all(), (tag, "partials not written everywhere")
    # each thread sums its 32 values in fp32 (then fp64): 32 fp32 roundings of sum |y| at most; per entry
    e1 = float(((sg[..., 0] - s1).abs() / a1).max())
    e2 = float(((sg[..., 1] - s2).abs() / s2).max())
    assert e1 <= 32 * U24 and e2 <= 32 * U24, (tag, e1, e2)
    return e1, e2


@pytest.mark.parametrize("B,H,Cx,Cs,sscale,Cout,mode,ips", CHAIN)
def test_resnet_block_winograd4_chain_matches_fp64(lib, device, B, H, Cx, Cs, sscale, Cout, mode, ips):
    E = engine()
    W, Cin, G, eps = H, Cx + Cs, 8, 1e-5
    key = (B, H, Cx, Cs, sscale, Cout)
    gen = g(41)
    ldx = Cin + 64                       # x a channel slice of a wider buffer (a skip slot of a concat)
    xbuf = torch.randn(B, H, W, ldx, generator=gen) * 0.8
    xbuf[..., :Cx] += 1.5                # a mean offset; the skip half keeps its own
    x, skip = xbuf[..., :Cx], xbuf[..., Cx:Cin]
    gamma1, beta1 = 1.0 + 0.2 * torch.randn(Cin, generator=gen), 0.1 * torch.randn(Cin, generator=gen)
    gamma2, beta2 = 1.0 + 0.2 * torch.randn(Cout, generator=gen), 0.1 * torch.randn(Cout, generator=gen)
    w1 = torch.randn(Cout, Cin, 3, 3, generator=gen) * (Cin * 9) ** -0.5
    w2 = torch.randn(Cout, Cout, 3, 3, generator=gen) * (Cout * 9) ** -0.5
    # biases ~ N(0, 1) as in test_conv3x3_winograd4_matches_direct, the test WINO4_REL was set on (the rel-L2 counts them in
    # its norm: with biases of 0.1 the fp32-MFMA GEMMs at Cin = 2048 measure 8.3e-6 against the bias-free output)
    b1, b2 = torch.randn(Cout, generator=gen), torch.randn(Cout, generator=gen)
    ld_ss, col = 2 * Cout + 96, 32       # per-image FiLM rows (distinct times) inside the stacked time-MLP rows
    ssbuf = torch.randn(B, ld_ss, generator=gen) * 0.3
    ss = ssbuf[:, col:col + 2 * Cout]
    # residual of block2: x itself where Cin == Cout (the plan's ResnetBlock without a skip conv: rows of stride ldx), else
    # a map with rows wider than Cout
    if Cin == Cout:
        res, ldres = x, ldx
        resbuf = xbuf
    else:
        ldres = Cout + 32
        resbuf = torch.randn(B, H, W, ldres, generator=gen)
        res = resbuf[..., :Cout]
    xcat = torch.cat([x.double()] + ([skip.double() * sscale] if Cs else []), dim=-1)
    if key not in _chain_ref:
        _chain_ref.clear()
        _chain_ref[key] = _block_ref(xcat, gamma1, beta1, G, None, w1, b1, None)
    ref1 = _chain_ref[key]
    dv = lambda t: t.contiguous().to(device)
    xd, resd, ssd = dv(xbuf), dv(resbuf), dv(ssbuf)
    g1d, be1d, g2d, be2d, w1d, w2d, b1d, b2d = map(dv, (gamma1, beta1, gamma2, beta2, w1, w2, b1, b2))
    # block1's GroupNorm statistics from host-built fp64 partials of x (chunks of 16 pixels) and the UNSCALED skip (chunks of
    # 64 pixels; the fold applies its scale), as the producers of a concat leave them
    HW = H * W
    p0 = _partials(x.reshape(B, HW, Cx), HW // 16).to(device)
    p1 = _partials(skip.reshape(B, HW, Cs), HW // 64).to(device) if Cs else None
    stats1 = nan_dev(B, G, 2)
    E.check(lib.kd_gn_fold_seg(dp(p0), Cx // 16, HW // 16, 1.0, 1.0, dp(p1), Cs // 16, HW // 64, sscale, sscale, dp(g1d),
                               dp(be1d), None, 0, None, dp(stats1), B, HW, Cin, G, eps, E.current_stream()))
    nch = (H // 4) * (W // 4)
    y1 = nan_dev(B, H, W, Cout)
    seg1 = nan_dev(B, Cout // 16, nch, 2, dtype=torch.float64)
    skip_c0 = Cx if Cs and sscale != 1.0 else -1   # (the init-conv residual joins unscaled: nothing to fold)
    E.check(lib.kd_gn_conv3x3_winograd4_nhwc(dp(xd), ldx, dp(stats1), dp(g1d), dp(be1d), None, 0, skip_c0, sscale, dp(w1d),
                                             dp(b1d), None, 0, dp(y1), dp(seg1), B, H, W, Cin, Cout, G, mode, ips,
                                             E.current_stream()))
    got1 = y1.cpu().double()
    assert torch.isfinite(got1).all(), "block1: y not written everywhere"
    tag = f"B{B} {H}x{W} {Cx}+{Cs}->{Cout} mode {mode} ips {ips}"
    _check_conv(tag + " block1", got1, ref1)
    s1e = _check_out_seg(tag + " block1", seg1, got1)
    # block2: statistics of y1 from its own partials, FiLM per image, residual
    stats2 = nan_dev(B, G, 2)
    E.check(lib.kd_gn_fold_seg(dp(seg1), Cout // 16, nch, 1.0, 1.0, None, 0, 0, 1.0, 1.0, dp(g2d), dp(be2d),
                               dp(ssd[:, col:]), ld_ss, None, dp(stats2), B, HW, Cout, G, eps, E.current_stream()))
    m2, r2 = _gn_ref(got1.reshape(B, HW, Cout), G, eps)
    st2 = stats2.cpu().double()
    assert float(((st2[..., 0] - m2).abs() * r2).max()) <= 64 * U24 and float(((st2[..., 1] - r2).abs() / r2).max()) <= 64 * U24
    y2 = nan_dev(B, H, W, Cout)
    seg2 = nan_dev(B, Cout // 16, nch, 2, dtype=torch.float64)
    E.check(lib.kd_gn_conv3x3_winograd4_nhwc(dp(y1), 0, dp(stats2), dp(g2d), dp(be2d), dp(ssd[:, col:]), ld_ss, -1, 1.0,
                                             dp(w2d), dp(b2d), dp(resd), ldres, dp(y2), dp(seg2), B, H, W, Cout, Cout, G,
                                             mode, ips, E.current_stream()))
    got2 = y2.cpu().double()
    assert torch.isfinite(got2).all(), "block2: y not written everywhere"
    ref2 = _block_ref(got1, gamma2, beta2, G, ss, w2, b2, res)   # (per conv: from block1's returned output)
    _check_conv(tag + " block2", got2, ref2)
    s2e = _check_out_seg(tag + " block2", seg2, got2)
    print(f"{tag}: out partials rel err {s1e[0]:.1e}/{s1e[1]:.1e}, {s2e[0]:.1e}/{s2e[1]:.1e}")


def test_gn_conv3x3_winograd4_rejects_unsupported_shapes(lib, device):
    E = engine()
    t = torch.zeros(4096, device=device)
    for B, H, Cin, Cout, mode, ips, ldx, skip_c0 in [
            (1, 18, 128, 128, -1, 0, 0, -1),     # H % 4
            (1, 16, 128, 128, -1, 0, 0, -1),     # B (H/4) (W/4) = 16 tiles: not a 128-row slab
            (8, 16, 48, 128, -1, 0, 0, -1),      # Cin % 32
            (8, 16, 128, 96, -1, 0, 0, -1),      # Cout % 64
            (8, 16, 128, 128, 1, 0, 0, -1),      # 128 tiles: below the bf16x3 GEMM's 256-row tile
            (16, 16, 128, 192, 2, 0, 0, -1),     # Cout % 128 for bf16x3
            (16, 16, 128, 128, -1, 3, 0, -1),    # images_per_set does not divide B
            (16, 16, 128, 128, 0, 0, 0, -1),     # unknown gemm_mode
            (16, 16, 128, 128, -1, 0, 120, -1),  # ldx < Cin
            (16, 16, 128, 128, -1, 0, 0, 130)]:  # skip_c0 past Cin
        rc = lib.kd_gn_conv3x3_winograd4_nhwc(dp(t), ldx, dp(t), dp(t), dp(t), None, 0, skip_c0, 1.0, dp(t), dp(t), None, 0,
                                              dp(t), None, B, H, H, Cin, Cout, 8, mode, ips, E.current_stream())
        err = lib.kd_last_error()
        assert rc != 0 and (b"kd_gn_conv3x3_winograd4_nhwc" in err or b"F(4x4,3x3)" in err or b"bf16x3" in err), err
