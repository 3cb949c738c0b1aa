"""The Winograd F(4x4,3x3) transforms (csrc/kernels_wino4.hip) through the plan's own launch form,
kd_gn_conv3x3_winograd4_nhwc - input transform with the GroupNorm / FiLM / SiLU affine folded, the 36 position GEMMs, output
transform with bias, residual and the GroupNorm partials of y - against an fp64 convolution on the host.

What these cases are about is the map from workgroups to (tile, channel pair): which workgroup takes which tiles is free to
change (the output transform walks its blocks XCD by XCD), and a wrong map shows as tiles written twice, never, or with another
tile's pixels.  The shapes are the smallest the bf16x3 GEMM accepts (B (H/4) (W/4) a multiple of 256) at which the maps differ:
four tiles, two tiles or a sixteenth of a tile per wave, every tile on an image edge, a non-square map, two column tiles of the
GEMM.  Every shape runs with V as fp32 and as bf16 planes, plain and with everything the plan can ask of the transforms at once:
a residual, x a channel slice of a wider buffer whose upper half is an unscaled skip tensor, FiLM rows, and two sets of images
(the launches of the second set start at offsets into x, y, the residual and the partials).  y and the partials are NaN before
the call, so a tile nobody wrote shows."""
import pytest
import torch
import torch.nn.functional as F

import helpers as H

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24   # one fp32 rounding, relative
WINO4_REL = 8e-6   # tests/test_kernels_gpu.py: F(4x4,3x3) re-association in fp32, per conv rel-L2 against fp64
G, EPS = 8, 1e-5

SHAPES = [  # (B, H, W, Cin, Cout): one set of images
    pytest.param(4, 32, 32, 128, 128, id="4x32x32-128-128"),
    pytest.param(16, 16, 16, 256, 128, id="16x16x16-256-128-all-edge-tiles"),
    pytest.param(1, 64, 64, 32, 128, id="1x64x64-32-128-narrow-channel-run"),
    pytest.param(2, 32, 64, 128, 256, id="2x32x64-128-256-non-square-two-n-tiles"),
]
MODES = [pytest.param(2, id="v-fp32"), pytest.param(1, id="v-planes")]


engine, dp, nan_dev = H.engine, H.dev_ptr, H.nan_dev   # (H is the image height in the functions below)


@pytest.fixture(scope="module")
def lib():
    return engine().load()


_cases = {}


def _case(B, H, W, Cin, Cout):
    """Inputs of two sets of B images and their fp64 references, built once per shape (a few MB each) and left unchanged.
    `full`: x = channels [0, Cin) of rows of ldx floats, the upper half an unscaled skip tensor that the layer sees times
    2^-1/2, FiLM, residual.  `plain`: the same first Cin channels dense and unscaled, no FiLM, no residual, first set only."""
    key = (B, H, W, Cin, Cout)
    if key in _cases:
        return _cases[key]
    gen = torch.Generator().manual_seed(97 + Cin + H)
    B2, ldx, c0, sscale = 2 * B, Cin + 32, Cin // 2, 2 ** -0.5
    xbuf = torch.randn(B2, H, W, ldx, generator=gen) * 0.8
    xbuf[..., :c0] += 1.5
    gamma, beta = 1.0 + 0.2 * torch.randn(Cin, generator=gen), 0.1 * torch.randn(Cin, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * (Cin * 9) ** -0.5
    b = torch.randn(Cout, generator=gen)   # ~ N(0, 1), as where WINO4_REL was set
    ld_ss = 2 * Cin + 32
    ss = torch.randn(B2, ld_ss, generator=gen) * 0.3
    ldres = Cout + 32
    resbuf = torch.randn(B2, H, W, ldres, generator=gen)

    def ref(x64, film, res):
        xn = F.group_norm(x64.permute(0, 3, 1, 2), G, gamma.double(), beta.double(), eps=EPS)
        if film is not None:
            xn = xn * (film[:, :Cin].double() + 1.0)[:, :, None, None] + film[:, Cin:2 * Cin].double()[:, :, None, None]
        y = F.conv2d(F.silu(xn), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
        return y + res.double() if res is not None else y

    def stats(x64):   # (mean, rstd) per image and group, as the GroupNorm fold hands them to the transform
        xg = x64.reshape(x64.shape[0], H * W, G, Cin // G)
        mean = xg.mean(dim=(1, 3))
        var = (xg * xg).mean(dim=(1, 3)) - mean * mean
        return torch.stack([mean, (var + EPS).rsqrt()], dim=-1).float()

    x_full = torch.cat([xbuf[..., :c0].double(), xbuf[..., c0:Cin].double() * sscale], dim=-1)
    x_plain = xbuf[:B, ..., :Cin].double()
    c = dict(xbuf=xbuf, gamma=gamma, beta=beta, w=w, b=b, ss=ss, ld_ss=ld_ss, resbuf=resbuf, ldres=ldres, ldx=ldx, c0=c0,
             sscale=sscale, x_plain=xbuf[:B, ..., :Cin].contiguous(),
             stats_full=stats(x_full), ref_full=ref(x_full, ss, resbuf[..., :Cout]),
             stats_plain=stats(x_plain), ref_plain=ref(x_plain, None, None))
    _cases[key] = c
    return c


def _check(tag, y, seg, ref):
    got = y.cpu().double()
    assert torch.isfinite(got).all(), (tag, "y not written everywhere")
    err = float((got - ref).norm() / ref.norm())
    mx = float((got - ref).abs().max() / ref.abs().max())
    # per tile too: a few wrong tiles of a large map would pass the whole-map norm only if they were nearly right
    Bn, H, W, C = got.shape
    dt = (got - ref).reshape(Bn, H // 4, 4, W // 4, 4, C).pow(2).sum(dim=(2, 4, 5)).sqrt()
    rt = ref.reshape(Bn, H // 4, 4, W // 4, 4, C).pow(2).sum(dim=(2, 4, 5)).sqrt()
    worst = float((dt / rt).max())
    print(f"{tag}: rel-L2 {err:.2e}, max {mx:.2e}, worst tile rel-L2 {worst:.2e}")
    assert err <= WINO4_REL, (tag, err)
    assert mx <= 5e-5, (tag, "element-wise outlier", mx)   # (5e-5 max|ref|: test_conv3x3_winograd4_matches_direct)
    # the partials [B][C/16][(H/4)(W/4)][2] against fp64 sums of the returned y: each thread sums its 32 values in fp32 (then
    # fp64), 32 fp32 roundings of sum |y| at most
    yt = got.reshape(Bn, H // 4, 4, W // 4, 4, C // 16, 16)
    red = lambda t: t.sum(dim=(2, 4, 6)).permute(0, 3, 1, 2).reshape(Bn, C // 16, -1)
    s1, s2, a1 = red(yt), red(yt * yt), red(yt.abs())
    sg = seg.cpu()
    assert torch.isfinite(sg).all(), (tag, "partials not written everywhere")
    e1 = float(((sg[..., 0] - s1).abs() / a1).max())
    e2 = float(((sg[..., 1] - s2).abs() / s2).max())
    print(f"{tag}: partials rel err {e1:.1e} / {e2:.1e}")
    assert e1 <= 32 * U24 and e2 <= 32 * U24, (tag, e1, e2)


def _run_full(lib, device, c, B, H, W, Cin, Cout, mode, nsets=2):
    E = engine()
    dv = lambda t: t.contiguous().to(device)
    Bn = nsets * B
    xd, resd, ssd, st = dv(c["xbuf"][:Bn]), dv(c["resbuf"][:Bn]), dv(c["ss"][:Bn]), dv(c["stats_full"][:Bn])
    gd, bed, wd, bd = map(dv, (c["gamma"], c["beta"], c["w"], c["b"]))
    y = nan_dev(Bn, H, W, Cout)
    seg = nan_dev(Bn, Cout // 16, (H // 4) * (W // 4), 2, dtype=torch.float64)
    E.check(lib.kd_gn_conv3x3_winograd4_nhwc(dp(xd), c["ldx"], dp(st), dp(gd), dp(bed), dp(ssd), c["ld_ss"], c["c0"], c["sscale"],
                                             dp(wd), dp(bd), dp(resd), c["ldres"], dp(y), dp(seg), Bn, H, W, Cin, Cout, G, mode,
                                             B if nsets > 1 else 0, E.current_stream()))
    return y, seg


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_wino4_plain(lib, device, B, H, W, Cin, Cout, mode):
    """dense x, no FiLM, no residual (the output transform's form without one), one set"""
    E = engine()
    c = _case(B, H, W, Cin, Cout)
    dv = lambda t: t.contiguous().to(device)
    xd, st = dv(c["x_plain"]), dv(c["stats_plain"])
    gd, bed, wd, bd = map(dv, (c["gamma"], c["beta"], c["w"], c["b"]))
    y = nan_dev(B, H, W, Cout)
    seg = nan_dev(B, Cout // 16, (H // 4) * (W // 4), 2, dtype=torch.float64)
    E.check(lib.kd_gn_conv3x3_winograd4_nhwc(dp(xd), 0, dp(st), dp(gd), dp(bed), None, 0, -1, 1.0, dp(wd), dp(bd), None, 0, dp(y),
                                             dp(seg), B, H, W, Cin, Cout, G, mode, 0, E.current_stream()))
    _check(f"plain B{B} {H}x{W} {Cin}->{Cout} mode {mode}", y, seg, c["ref_plain"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,Cin,Cout", SHAPES)
def test_wino4_residual_strided_skip_scale_two_sets(lib, device, B, H, W, Cin, Cout, mode):
    """residual, ldx > Cin with skip_c0 / skip_scale, FiLM, images_per_set = B of 2 B images"""
    c = _case(B, H, W, Cin, Cout)
    y, seg = _run_full(lib, device, c, B, H, W, Cin, Cout, mode)
    _check(f"full 2x B{B} {H}x{W} {Cin}->{Cout} mode {mode}", y, seg, c["ref_full"])


@pytest.mark.parametrize("mode", MODES)
def test_wino4_leaves_no_tile_unwritten(lib, device, mode):
    """V and D are the entry's own allocations, so what can be made NaN from here is y, the partials and the memory V and D are
    about to be given: a NaN-filled block of more than their size goes back to the driver right before the call.  Every value
    of y and of the partials must then be finite and right - a tile of V or D that no workgroup wrote would carry what lay
    there before."""
    B, H, W, Cin, Cout = 4, 32, 32, 128, 128
    c = _case(B, H, W, Cin, Cout)
    Mt = B * (H // 4) * (W // 4)
    poison = nan_dev(36 * Mt * (2 * Cin + Cout) + (1 << 20))
    torch.cuda.synchronize()
    del poison
    torch.cuda.empty_cache()
    y, seg = _run_full(lib, device, c, B, H, W, Cin, Cout, mode, nsets=1)
    _check(f"poisoned B{B} {H}x{W} {Cin}->{Cout} mode {mode}", y, seg, c["ref_full"][:B])
