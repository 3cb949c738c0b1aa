"""kd_sample_start on the MI355X: x = scale * z + (2 * nearest(init) - 1) in one launch, bit for bit the torch composition
of the same parts - z from kd_philox_normal (int seed: one stream over the batch tensor) or kd_philox_normal_rows (a key per
image) or an injected tensor, F.interpolate(mode="nearest") for the source pixel, then torch's multiply, subtract, multiply
and add as separate ops.  Neither side is approximated, so every comparison is torch.equal.

Shapes: B = 1, 3 and 33 (33 passes the 32 keys one launch carries), C = 1, 3, 4, S = 16, 32 - rows of 64 to 1024 float4, so
image boundaries fall inside a block and a float4 never leaves its image; sources 16 x 16 (x 2), 64 x 64 (/ 2), 24 x 24 and
37 x 50 (non-integer ratios, non-square, a width that is no multiple of 4) and 32 x 32 (the identity) into 32."""
import pytest
import torch
import torch.nn.functional as F

import helpers as H

pytestmark = pytest.mark.gpu

SID = (16 << 32) | 2
INT_SEED = 0xD1B54A32D192ED03
SEEDS = [0x9E3779B97F4A7C15, 7, 0x1_0000_0001, 2 ** 64 - 1, 12345]


def _seeds(B):
    return [(SEEDS[b % len(SEEDS)] + b // len(SEEDS)) % 2 ** 64 for b in range(B)]


def _z(device, B, n, source):
    """(z [B, n] as the composition draws it, (seed, seeds, d_noise) for kd_sample_start)."""
    E = H.engine()
    lib = E.load()
    z = torch.full((B, n), 7.0, device=device)
    if source == "int":
        E.check(lib.kd_philox_normal(E.ptr(z), B * n, INT_SEED, SID, E.current_stream()))
        return z, (INT_SEED, None, None)
    if source == "list":
        seeds = _seeds(B)
        E.check(lib.kd_philox_normal_rows(E.ptr(z), B, n, E.seed_array(seeds), SID, E.current_stream()))
        return z, (99, E.seed_array(seeds), None)   # (seed is not read)
    z = torch.randn(B, n, generator=torch.Generator().manual_seed(B * 1000 + n)).to(device)
    return z, (99, E.seed_array(_seeds(B)), z)      # (neither seed nor seeds is read)


def _start(device, B, C, S, scale, keys, init):
    E = H.engine()
    seed, seeds, noise = keys
    out = torch.full((B, C, S, S), float("nan"), device=device)
    hs, ws = init.shape[2:] if init is not None else (0, 0)
    E.check(E.load().kd_sample_start(E.ptr(out), B, C, S, scale, seed, seeds, E.ptr(noise), E.ptr(init), hs, ws,
                                     E.current_stream()))
    return out


def _init(B, C, hs, ws, seed=0):
    return torch.rand(B, C, hs, ws, generator=torch.Generator().manual_seed(seed + 7 * hs + ws))


def _compose(z, scale, init, S, device):
    """torch, op by op: z * scale, then + (resize(init) * 2 - 1); the resize on the CPU (a gather: exact anywhere)."""
    x = z * scale
    if init is None:
        return x
    src = init if tuple(init.shape[2:]) == (S, S) else F.interpolate(init, (S, S), mode="nearest")
    src = src.to(device)
    return x + (src * 2 - 1)


@pytest.mark.parametrize("source", ["int", "list", "noise"])
@pytest.mark.parametrize("scale", [1.0, 80.0])
def test_start_without_an_image_is_the_scaled_draw(device, source, scale):
    """init == NULL: scale = 1 gives z's bits, scale = 80 (the EDM product) what z.mul_(80.) gives."""
    for B in (1, 3, 33):
        for C in (1, 3, 4):
            for S in (16, 32):
                z, keys = _z(device, B, C * S * S, source)
                got = _start(device, B, C, S, scale, keys, None)
                want = z.clone().mul_(scale).reshape(B, C, S, S)
                assert bool(torch.isfinite(got).all())
                assert torch.equal(got, want), (B, C, S)
                if scale == 1.0:
                    assert torch.equal(got.reshape(B, -1), z)


SOURCES_32 = [(16, 16), (64, 64), (24, 24), (37, 50), (32, 32)]


@pytest.mark.parametrize("source", ["int", "list", "noise"])
@pytest.mark.parametrize("hs,ws", SOURCES_32)
def test_start_from_an_image_is_the_torch_composition(device, source, hs, ws):
    S = 32
    for B in (1, 3, 33):
        for C in (1, 3, 4):
            for scale in (1.0, 80.0):
                z, keys = _z(device, B, C * S * S, source)
                init = _init(B, C, hs, ws)
                got = _start(device, B, C, S, scale, keys, init.to(device))
                want = _compose(z.reshape(B, C, S, S), scale, init, S, device)
                assert torch.equal(got, want), (B, C, scale)
    # the image term is there and it is the image's: image 1 of another source changes image 1 alone
    other = init.clone()
    other[1] = 1 - other[1]
    got2 = _start(device, B, C, S, scale, keys, other.to(device))
    assert not torch.equal(got2[1], got[1]) and torch.equal(got2[0], got[0]) and torch.equal(got2[2:], got[2:])


@pytest.mark.parametrize("source", ["int", "list"])
def test_start_at_16_from_larger_smaller_and_odd_sources(device, source):
    S = 16
    for hs, ws in [(8, 8), (16, 16), (37, 50), (5, 3), (1, 1), (299, 17)]:
        for B, C in [(3, 3), (33, 1), (1, 4)]:
            z, keys = _z(device, B, C * S * S, source)
            init = _init(B, C, hs, ws, seed=1)
            got = _start(device, B, C, S, 1.0, keys, init.to(device))
            assert torch.equal(got, _compose(z.reshape(B, C, S, S), 1.0, init, S, device)), (hs, ws, B, C)


def test_a_row_length_that_is_no_multiple_of_4_is_refused_and_nothing_is_launched(device):
    E = H.engine()
    out = torch.full((2, 1, 3, 3), 7.0, device=device)
    with pytest.raises(E.EngineError, match="multiple of 4"):
        E.check(E.load().kd_sample_start(E.ptr(out), 2, 1, 3, 1.0, 5, None, None, None, 0, 0, E.current_stream()))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
