"""The library's other resampling layers (`Unet(cross_embed_downsample=True)`, `Unet(pixel_shuffle_upsample=False)`) without a
GPU: the state-dict layout against the restatement in tests/resample_ref.py, strict loading, the version-fork hook, the
config structs, the phase identity the upsample kernel's weight pack rests on, and the new kernel file's resource usage."""
import ctypes as C
import functools
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import helpers as H
import resample_ref as RR

ROOT = Path(__file__).resolve().parent.parent
KW = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
          layer_cross_attns=(False, False, True), cond_on_text=False, text_embed_dim=None)
SWITCHES = {"cross_embed": dict(cross_embed_downsample=True), "nearest": dict(pixel_shuffle_upsample=False),
            "both": dict(cross_embed_downsample=True, pixel_shuffle_upsample=False)}


_product = functools.partial(H.random_product_unet, **KW)   # _product(seed=0, **over)


def _ref(seed=0, **over):
    return H.randomize_(RR.Unet(**{**KW, **over}), seed)


@pytest.mark.parametrize("mem", [False, True])
@pytest.mark.parametrize("sw", list(SWITCHES))
def test_state_dict_layout_equals_the_restatement_and_round_trips(sw, mem):
    import imagen_pytorch as ip

    over = dict(SWITCHES[sw], memory_efficient=mem)
    p, r = _product(seed=1, **over), _ref(seed=2, **over)
    sp = p.state_dict()
    assert H.state_layout(sp) == H.state_layout(r.state_dict())
    if "cross_embed_downsample" in over:
        pre = "downs.0.0" if mem else "downs.0.4"
        assert tuple(sp[pre + ".convs.0.weight"].shape) == (16, 32, 2, 2) and tuple(sp[pre + ".convs.0.bias"].shape) == (16,)
        assert tuple(sp[pre + ".convs.1.weight"].shape) == (16, 32, 4, 4)
        assert (("downs.2.0.convs.0.weight" in sp) if mem else ("downs.2.4.fns.0.weight" in sp))   # the last level's Parallel stays
        assert not any(re.fullmatch(r"downs\.\d+\.[04]\.1\.weight", k) for k in sp)
    if "pixel_shuffle_upsample" in over:
        assert tuple(sp["ups.0.3.1.weight"].shape) == (64, 128, 3, 3) and tuple(sp["ups.0.3.1.bias"].shape) == (64,)
        assert ("ups.2.3.1.weight" in sp) == mem   # Identity on the last up level unless memory_efficient
        assert not any(".3.net.0." in k for k in sp)
    p.load_state_dict(r.state_dict(), strict=True)
    got, want = p.state_dict(), r.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    r.load_state_dict(_product(seed=3, **over).state_dict(), strict=True)
    # a default UNet refuses those keys on a strict load
    plain = ip.Unet(**{**KW, "memory_efficient": mem})
    with pytest.raises(RuntimeError):
        plain.load_state_dict(want, strict=True)


def test_cross_embed_keys_do_not_trigger_the_version_fork_hook(capsys):
    p, r = _product(seed=1, **SWITCHES["both"]), _ref(seed=2, **SWITCHES["both"])
    calls = []
    orig = p.set_version_forks
    p.set_version_forks = lambda *a, **k: (calls.append((a, k)), orig(*a, **k))[1]
    p.load_state_dict(r.state_dict(), strict=True)
    assert not calls and p.downsample_form == "unshuffle" and p._locals["downsample_form"] == "unshuffle"
    assert capsys.readouterr().out == ""
    # asked directly, the fork leaves a cross-embed UNet's downsample slots alone
    before = H.state_layout(p.state_dict())
    orig(downsample_form="conv4x4")
    assert H.state_layout(p.state_dict()) == before and p.downsample_form == "unshuffle"
    assert type(p.downs[0][4]).__name__ == "CrossEmbedLayer"


def test_conv4x4_fork_is_still_detected_on_a_default_unet(capsys):
    import imagen_pytorch as ip
    from oracle import imagen_ref as R

    old = H.randomize_(R.Unet(**KW, downsample_form="conv4x4"), 5)
    p = ip.Unet(**KW)
    p.load_state_dict(old.state_dict(), strict=True)
    assert p.downsample_form == "conv4x4" and "downsample=conv4x4" in capsys.readouterr().out
    # ... and on a nearest-upsample UNet, whose Downsample slots are the ordinary ones
    sd = {k: v for k, v in _product(seed=6, pixel_shuffle_upsample=False).state_dict().items()}
    for k, v in old.state_dict().items():
        if re.fullmatch(r"downs\.\d+\.4\.(weight|bias)", k):
            sd[k] = v
    sd = {k: v for k, v in sd.items() if not re.fullmatch(r"downs\.\d+\.4\.1\.(weight|bias)", k)}
    q = ip.Unet(**KW, pixel_shuffle_upsample=False)
    q.load_state_dict(sd, strict=True)
    assert q.downsample_form == "conv4x4" and "ups.0.3.1.weight" in q.state_dict()


def test_kernel_sizes_other_than_the_default_are_refused():
    import imagen_pytorch as ip

    with pytest.raises(NotImplementedError):
        ip.Unet(**KW, cross_embed_downsample=True, cross_embed_downsample_kernel_sizes=(2, 4, 8))
    ip.Unet(**KW, cross_embed_downsample=True, cross_embed_downsample_kernel_sizes=[2, 4])


def test_cast_model_parameters_clones_keep_both_switches():
    u = _product(**SWITCHES["both"])
    clone = u.cast_model_parameters(lowres_cond=True, text_embed_dim=None, channels=3, channels_out=3, cond_on_text=False)
    assert clone is not u and clone.lowres_cond
    assert clone.cross_embed_downsample and not clone.pixel_shuffle_upsample
    assert clone._plan["cross_embed_downsample"] is True and clone._plan["upsample_nearest"] is True
    assert "downs.0.4.convs.1.weight" in clone.state_dict() and "ups.0.3.1.weight" in clone.state_dict()
    d = _product()
    assert d._plan["cross_embed_downsample"] is False and d._plan["upsample_nearest"] is False


def test_ext_struct_mirrors_the_header_and_the_config_keeps_its_size():
    from imagen_pytorch import _engine as E

    header = (ROOT / "include" / "kd_engine.h").read_text()
    body = re.search(r"typedef struct kd_unet_ext \{(.*?)\} kd_unet_ext_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\bint\s+(\w+)(\[KD_MAX_LEVELS\])?;", body)
    assert [f[0] for f in fields] == [n for n, _ in E.kd_unet_ext_t._fields_]
    assert [f[0] for f in fields][-2:] == ["cross_embed_downsample", "upsample_nearest"]   # appended: the old fields keep their offsets
    ints = sum(E.KD_MAX_LEVELS if arr else 1 for _, arr in fields)
    assert C.sizeof(E.kd_unet_ext_t) == 4 * ints == 4 * (3 + 2 * E.KD_MAX_LEVELS)
    assert C.sizeof(E.kd_unet_config_t) == 4 * (2 + 4 * E.KD_MAX_LEVELS + 27)
    ext = E.kd_unet_ext_t()
    assert ext.cross_embed_downsample == 0 and ext.upsample_nearest == 0


def phase_weights(w):
    """The sixteen summed tap matrices of the upsample kernel's weight pack (kernels_resample.hip), [p][q][a][b][O][I]: phase
    (p, q) of the output reads input pixel (y - 1 + p + a, x - 1 + q + b) with the 3x3 taps that land on it summed -
    rows p = 0: {w[0]}, {w[1] + w[2]}; p = 1: {w[0] + w[1]}, {w[2]}; columns the same with q."""
    sets = [[[0], [1, 2]], [[0, 1], [2]]]
    out = w.new_zeros(2, 2, 2, 2, *w.shape[:2])
    for p in range(2):
        for q in range(2):
            for a in range(2):
                for b in range(2):
                    out[p, q, a, b] = sum(w[:, :, kh, kw] for kh in sets[p][a] for kw in sets[q][b])
    return out


def test_phase_decomposition_equals_the_conv_over_the_upsampled_map():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64)
    w = torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    wp = phase_weights(w)
    xp = F.pad(x, (1, 1, 1, 1))   # taps off the low-res map are zero
    out = torch.zeros_like(ref)
    for p in range(2):
        for q in range(2):
            k = wp[p, q].permute(2, 3, 0, 1)   # [O][I][a][b]: a 2 x 2 conv over rows y - 1 + p + a, columns x - 1 + q + b
            out[:, :, p::2, q::2] = F.conv2d(xp[:, :, p:p + 6, q:q + 8], k)
    assert float((out - ref).abs().max()) < 1e-12


def test_resample_kernels_compile_without_scratch_or_spills(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "kidney-diffusion_amd" / "csrc"
    assert "kernels_resample.hip" in (csrc / "Makefile").read_text()
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", str(csrc / "kernels_resample.hip"),
                          f"-I{csrc}", f"-I{ROOT / 'include'}", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "kernels_resample.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", out.stderr)]
    assert len(names) == 2 and len(scratch) == len(spills) == 2, names   # weight pack, phase GEMMs
    assert not any(scratch) and not any(spills), f"scratch {scratch}, spills {spills}"
