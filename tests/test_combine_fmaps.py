"""`Unet(combine_upsample_fmaps=True)` (the library's UpsampleCombiner) without a GPU: the state-dict layout and constructor
against the restatement in tests/combine_fmaps_ref.py, strict loading both ways, the new config struct and symbols, the
class decomposition the kernel's weight pack rests on, and the new kernel file's resource usage."""
import ctypes as C
import functools
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import combine_fmaps_ref as CR
import helpers as H

ROOT = Path(__file__).resolve().parent.parent
KW = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
          layer_cross_attns=(False, False, True), cond_on_text=False, text_embed_dim=None)


_product = functools.partial(H.random_product_unet, **KW)   # _product(seed=0, **over)


def _ref(seed=0, **over):
    return H.randomize_(CR.Unet(**{**KW, **over}), seed)


# ------------------------------------------------------------------------------- state dict and constructor
@pytest.mark.parametrize("init_res", [False, True])
@pytest.mark.parametrize("mem", [False, True])
def test_state_dict_layout_equals_the_restatement_and_round_trips(mem, init_res):
    over = dict(combine_upsample_fmaps=True, memory_efficient=mem, init_conv_to_final_conv_residual=init_res)
    p, r = _product(seed=1, **over), _ref(seed=2, **over)
    sp = p.state_dict()
    assert H.state_layout(sp) == H.state_layout(r.state_dict())
    # up level i (deepest first) works at dims[L - i] = 128, 64, 32 channels; Block's own 8 groups
    for i, cin in enumerate((128, 64, 32)):
        pre = f"upsample_combiner.fmap_convs.{i}"
        assert tuple(sp[pre + ".groupnorm.weight"].shape) == tuple(sp[pre + ".groupnorm.bias"].shape) == (cin,)
        assert tuple(sp[pre + ".project.weight"].shape) == (32, cin, 3, 3) and tuple(sp[pre + ".project.bias"].shape) == (32,)
        assert p.upsample_combiner.fmap_convs[i].groupnorm.num_groups == 8
    fin = 32 * 4 + (32 if init_res else 0)
    assert tuple(sp["final_res_block.block1.project.weight"].shape) == (32, fin, 3, 3)
    assert tuple(sp["final_res_block.res_conv.weight"].shape) == (32, fin, 1, 1)
    p.load_state_dict(r.state_dict(), strict=True)
    got, want = p.state_dict(), r.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)
    r.load_state_dict(_product(seed=3, **over).state_dict(), strict=True)


def test_combiner_groups_are_not_resnet_groups():
    p = _product(combine_upsample_fmaps=True, resnet_groups=4)
    assert p.upsample_combiner.fmap_convs[0].groupnorm.num_groups == 8
    assert p.final_res_block.block1.groupnorm.num_groups == 4


def test_default_unet_is_unchanged():
    from oracle import imagen_ref as R

    for mem in (False, True):
        over = dict(memory_efficient=mem, init_conv_to_final_conv_residual=mem)
        d = _product(**over)
        assert H.state_layout(d.state_dict()) == H.state_layout(R.Unet(**{**KW, **over}).state_dict())
        assert H.state_layout(d.state_dict()) == H.state_layout(_product(combine_upsample_fmaps=False, **over).state_dict())
        assert not any(k.startswith("upsample_combiner") for k in d.state_dict())
        assert d._plan["combine_upsample_fmaps"] is False and not hasattr(d, "upsample_combiner")
    assert _product(combine_upsample_fmaps=True)._plan["combine_upsample_fmaps"] is True


def test_cast_model_parameters_clones_keep_the_switch():
    u = _product(combine_upsample_fmaps=True)
    clone = u.cast_model_parameters(lowres_cond=True, text_embed_dim=None, channels=3, channels_out=3, cond_on_text=False)
    assert clone is not u and clone.lowres_cond and clone.combine_upsample_fmaps
    assert clone._plan["combine_upsample_fmaps"] is True
    assert "upsample_combiner.fmap_convs.2.project.weight" in clone.state_dict()
    assert tuple(clone.state_dict()["final_res_block.block1.project.weight"].shape) == (32, 128, 3, 3)


# ------------------------------------------------------------------------------- loading
def test_strict_load_needs_the_combiner_keys_on_both_sides():
    import imagen_pytorch as ip

    comb, plain = _ref(seed=4, combine_upsample_fmaps=True).state_dict(), _ref(seed=5).state_dict()
    ip.Unet(**KW, combine_upsample_fmaps=True).load_state_dict(comb, strict=True)
    with pytest.raises(RuntimeError):
        ip.Unet(**KW, combine_upsample_fmaps=True).load_state_dict(plain, strict=True)
    with pytest.raises(RuntimeError):
        ip.Unet(**KW).load_state_dict(comb, strict=True)


def test_trainer_load_is_strict_about_the_combiner_keys(tmp_path, capsys):
    """ImagenTrainer.load(strict=True) of a combine checkpoint succeeds on a combine UNet without the partial-load fallback;
    a default UNet does not take it silently."""
    import imagen_pytorch as ip
    from oracle import sampler_ref as RS

    kw = dict(image_sizes=(32,), timesteps=(4,), condition_on_text=False)
    online = _ref(seed=6, combine_upsample_fmaps=True)
    oim = RS.Imagen([online], **kw)
    ema = {f"0.ema_model.{k}": v for k, v in online.state_dict().items()}
    path = tmp_path / "ckpt.pt"
    torch.save({"model": oim.state_dict(), "ema": ema, "version": ip.__version__, "steps": torch.tensor([3])}, path)
    trainer = ip.ImagenTrainer(imagen=ip.Imagen([ip.Unet(**online._locals)], **kw))
    capsys.readouterr()
    trainer.load(str(path), strict=True)
    assert "Trying partial load" not in capsys.readouterr().out
    got = trainer.imagen.unets[0].state_dict()
    assert all(torch.equal(got[k], v) for k, v in online.state_dict().items())
    plain = ip.ImagenTrainer(imagen=ip.Imagen([ip.Unet(**{**online._locals, "combine_upsample_fmaps": False})], **kw))
    capsys.readouterr()
    try:
        plain.load(str(path), strict=True)
    except RuntimeError:
        return
    assert "Trying partial load" in capsys.readouterr().out


# ------------------------------------------------------------------------------- ABI
def test_ext2_struct_mirrors_the_header_and_the_older_structs_keep_their_size():
    from imagen_pytorch import _engine as E

    header = (ROOT / "include" / "kd_engine.h").read_text()
    body = re.search(r"typedef struct kd_unet_ext2 \{(.*?)\} kd_unet_ext2_t;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\bint\s+(\w+);", body)
    assert fields == [n for n, _ in E.kd_unet_ext2_t._fields_]
    assert fields[0] == "combine_upsample_fmaps"
    assert E.kd_unet_ext2_t().combine_upsample_fmaps == 0
    assert C.sizeof(E.kd_unet_ext_t) == 4 * (3 + 2 * E.KD_MAX_LEVELS)
    assert C.sizeof(E.kd_unet_config_t) == 4 * (2 + 4 * E.KD_MAX_LEVELS + 27)
    assert "int kd_unet_create_ext2(" in header and "int kd_upsample_nearest_gn_conv3x3_nhwc(" in header
    assert "#define KD_ENGINE_ABI_VERSION 2" in header


def test_library_exports_the_new_symbols():
    from imagen_pytorch import _engine as E

    lib = E.load()
    for name in ("kd_unet_create_ext2", "kd_upsample_nearest_gn_conv3x3_nhwc", "kd_unet_create_ext"):
        assert hasattr(lib, name), name
        assert name in E.SIGNATURES
    assert lib.kd_version() == 2


# ------------------------------------------------------------------------------- the class decomposition
TAPS = [[0], [1, 2], [0, 1, 2], [0, 1], [2]]   # kernel rows (columns) summed into tap 0 .. 4 (kernels_upcombine.hip)
CLASS_TAPS = [[(-1, 0), (0, 1)], [(0, 2)], [(0, 3), (1, 4)]]   # class first / interior / last: (source offset, tap)


def class_weights(w):
    """The 25 summed tap matrices of the kernel's weight pack, [rt][ct][O][I]."""
    out = w.new_zeros(5, 5, *w.shape[:2])
    for rt in range(5):
        for ct in range(5):
            out[rt, ct] = sum(w[:, :, kh, kw] for kh in TAPS[rt] for kw in TAPS[ct])
    return out


def class_decomposition(a, w, s):
    """conv3x3(pad 1) over nearest(a, s) from the LOW-RES map a [B,C,H,W] (already activated; taps off it are zero): nine
    class values per low-res pixel, each replicated to its pixels of the s x s block."""
    B, _, Hh, Ww = a.shape
    wp = class_weights(w)
    ap = F.pad(a, (1, 1, 1, 1))
    out = a.new_zeros(B, w.shape[0], s * Hh, s * Ww)
    rng = [range(0, 1), range(1, s - 1), range(s - 1, s)]
    for r in range(3):
        for c in range(3):
            if not len(rng[r]) or not len(rng[c]):   # s = 2: no interior row or column
                continue
            v = 0
            for dy, rt in CLASS_TAPS[r]:
                for dx, ct in CLASS_TAPS[c]:
                    v = v + torch.einsum("oi,bihw->bohw", wp[rt, ct], ap[:, :, 1 + dy:1 + dy + Hh, 1 + dx:1 + dx + Ww])
            for dy in rng[r]:
                for dx in rng[c]:
                    out[:, :, dy::s, dx::s] = v
    return out


@pytest.mark.parametrize("s,Hh,Ww", [(2, 5, 7), (3, 5, 7), (4, 5, 7), (16, 2, 3), (4, 1, 1), (2, 1, 1)])
def test_class_decomposition_equals_the_conv_over_the_upsampled_map(s, Hh, Ww):
    g = torch.Generator().manual_seed(s)
    x = torch.randn(2, 16, Hh, Ww, generator=g, dtype=torch.float64)
    w = torch.randn(3, 16, 3, 3, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(16, generator=g, dtype=torch.float64), torch.randn(16, generator=g, dtype=torch.float64)
    up = F.interpolate(x, scale_factor=s, mode="nearest")
    ref = F.conv2d(F.silu(F.group_norm(up, 8, gamma, beta)), w, padding=1)
    # statistics from the LOW-RES map: every pixel is replicated s^2 times
    a = F.silu(F.group_norm(x, 8, gamma, beta))
    out = class_decomposition(a, w, s)
    assert float((out - ref).abs().max()) < 1e-11
    if s == 2:   # the sixteen matrices of the x2 kernel are among the 25
        from test_resample import phase_weights

        wp, p16 = class_weights(w), phase_weights(w)
        idx = [0, 1, 3, 4]
        for p in range(2):
            for q in range(2):
                for a_ in range(2):
                    for b_ in range(2):
                        assert torch.equal(p16[p, q, a_, b_], wp[idx[2 * p + a_], idx[2 * q + b_]])


def test_upcombine_kernels_compile_without_scratch_or_spills(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "kidney-diffusion_amd" / "csrc"
    assert "kernels_upcombine.hip" in (csrc / "Makefile").read_text()
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", str(csrc / "kernels_upcombine.hip"),
                          f"-I{csrc}", f"-I{ROOT / 'include'}", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "kernels_upcombine.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", out.stderr)]
    assert len(names) == 3 and len(scratch) == len(spills) == 3, names   # weight pack, s = 2, s > 2
    assert not any(scratch) and not any(spills), f"scratch {scratch}, spills {spills}"
