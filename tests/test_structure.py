"""The structural switches of the UNet's first and last layer (library `Unet(init_cross_embed=False, init_conv_kernel_size=k,
init_cross_embed_kernel_sizes=..., final_conv_kernel_size=k, final_resnet_block=False, scale_skip_connection=False)`) without
a GPU: construction, the state-dict layout against the restatement in tests/structure_ref.py, strict loading (also through
ImagenTrainer), the clones of cast_model_parameters, the refusals by name, the ABI struct and the resource usage of
kernels_final.hip."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import helpers as H
import structure_ref as SR

ROOT = Path(__file__).resolve().parent.parent
KW = dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True), layer_cross_attns=(False, True),
          cond_on_text=False, text_embed_dim=None)
SWITCHES = {
    "plain_init": dict(init_cross_embed=False),
    "plain_init_k3": dict(init_cross_embed=False, init_conv_kernel_size=3),
    "sizes_3_5": dict(init_cross_embed_kernel_sizes=(3, 5)),
    "sizes_4": dict(init_cross_embed_kernel_sizes=(15, 3, 7, 5)),
    "final_k1": dict(final_conv_kernel_size=1),
    "final_k7": dict(final_conv_kernel_size=7),
    "no_final_block": dict(final_resnet_block=False),
    "no_skip_scale": dict(scale_skip_connection=False),
}
ALL = dict(SR.FIVE, init_cross_embed_kernel_sizes=(3, 5), lowres_cond=True, cond_images_channels=3, memory_efficient=True,
           init_conv_to_final_conv_residual=True, self_cond=True)


def _product(seed=0, **over):
    return H.random_product_unet(seed, **{**KW, **over})


def _ref(seed=0, **over):
    return H.randomize_(SR.Unet(**{**KW, **over}), seed)


def test_the_five_switches_construct_the_library_modules():
    u = _product(**SR.FIVE)
    assert isinstance(u.init_conv, torch.nn.Conv2d) and u.init_conv.kernel_size == (5, 5) and u.init_conv.padding == (2, 2)
    assert u.final_res_block is None
    assert u.final_conv.kernel_size == (5, 5) and u.final_conv.padding == (2, 2) and u.final_conv.in_channels == 32
    p = u._plan
    assert (p["init_cross_embed"], p["init_conv_kernel_size"], p["final_conv_kernel_size"], p["final_resnet_block"],
            p["scale_skip_connection"]) == (False, 5, 5, False, False)
    d = _product()._plan
    assert (d["init_cross_embed"], d["init_cross_embed_kernel_sizes"], d["final_conv_kernel_size"], d["final_resnet_block"],
            d["scale_skip_connection"]) == (True, (3, 7, 15), 3, True, True)
    assert _product(init_cross_embed_kernel_sizes=(15, 3, 7, 5))._plan["init_cross_embed_kernel_sizes"] == (3, 5, 7, 15)
    assert _product()._locals["init_conv_kernel_size"] == 7   # the library's default, in the signature


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_state_dict_layout_of_each_switch_equals_the_restatement(name):
    over = SWITCHES[name]
    sp = _product(**over).state_dict()
    assert H.state_layout(sp) == H.state_layout(_ref(**over).state_dict())
    if "init_cross_embed" in over:
        k = over.get("init_conv_kernel_size", 7)
        assert tuple(sp["init_conv.weight"].shape) == (32, 3, k, k) and tuple(sp["init_conv.bias"].shape) == (32,)
        assert not any(key.startswith("init_conv.convs") for key in sp)
    if name == "sizes_4":
        assert [tuple(sp[f"init_conv.convs.{i}.weight"].shape) for i in range(4)] == \
            [(16, 3, 3, 3), (8, 3, 5, 5), (4, 3, 7, 7), (4, 3, 15, 15)]
    if name == "no_final_block":
        assert not any(key.startswith("final_res_block") for key in sp)
    if "final_conv_kernel_size" in over:
        k = over["final_conv_kernel_size"]
        assert tuple(sp["final_conv.weight"].shape) == (3, 32, k, k)


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("combine", [False, True])
def test_state_dict_layout_of_all_five_at_once_equals_the_restatement(channels, combine):
    over = dict(ALL, channels=channels, combine_upsample_fmaps=combine)
    sp = _product(**over).state_dict()
    assert H.state_layout(sp) == H.state_layout(_ref(**over).state_dict())
    # fin = dim + dim L (combiner) + dim (init residual) + channels (lowres)
    fin = 32 + (64 if combine else 0) + 32 + channels
    assert tuple(sp["final_conv.weight"].shape) == (channels, fin, 5, 5)
    assert tuple(sp["init_conv.weight"].shape) == (32, 3 * channels + 3, 5, 5)   # cond_images | x | self_cond | lowres
    assert not any(key.startswith("final_res_block") for key in sp)


def test_strict_load_both_ways():
    over = dict(ALL, combine_upsample_fmaps=True)
    p, r = _product(seed=1, **over), _ref(seed=2, **over)
    p.load_state_dict(r.state_dict(), strict=True)
    sp, sr = p.state_dict(), r.state_dict()
    assert sorted(sp) == sorted(sr) and all(torch.equal(sp[k], sr[k]) for k in sr)   # (module order differs: final_conv rebuilt)
    p2 = _product(seed=3, **over)
    r.load_state_dict(p2.state_dict(), strict=True)
    sr, s2 = r.state_dict(), p2.state_dict()
    assert all(torch.equal(sr[k], s2[k]) for k in s2)


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_the_constructor_decides_the_form_and_a_mismatch_is_a_strict_load_error(name):
    """load_state_dict does not follow a checkpoint's keys for these switches: a default UNet refuses the checkpoint of
    every structural switch (and the other way round); scale_skip_connection has no parameters and loads either way."""
    over = SWITCHES[name]
    ckpt = _product(seed=4, **over).state_dict()
    default = _product(seed=5)
    if name == "no_skip_scale":
        default.load_state_dict(ckpt, strict=True)
        return
    with pytest.raises(RuntimeError):
        default.load_state_dict(ckpt, strict=True)
    with pytest.raises(RuntimeError):
        _product(seed=6, **over).load_state_dict(default.state_dict(), strict=True)
    assert isinstance(default.init_conv.convs[1], torch.nn.Conv2d) and default.final_res_block is not None   # nothing followed


def test_checkpoint_of_all_five_loads_strictly_through_the_trainer(tmp_path, monkeypatch):
    import imagen_pytorch as ip
    import imagen_pytorch.trainer as T

    kw = dict(image_sizes=(32,), timesteps=(2,), condition_on_text=False)
    over = dict(SR.FIVE, init_conv_to_final_conv_residual=True, combine_upsample_fmaps=True)
    src = ip.Imagen([_product(seed=4, **over)], **kw)
    dst = ip.Imagen([_product(seed=5, **over)], **kw)
    ema = {f"0.ema_model.{k}": v + 1.0 for k, v in src.unets[0].state_dict().items()}
    path = tmp_path / "ckpt.pt"
    torch.save({"model": src.state_dict(), "ema": ema, "version": ip.__version__, "steps": torch.tensor([3])}, path)

    def no_partial(*a, **k):
        raise AssertionError("the partial-load fallback ran")

    monkeypatch.setattr(T, "restore_parts", no_partial)
    trainer = ip.ImagenTrainer(imagen=dst)
    trainer.load(str(path))
    got, want = dst.state_dict(), src.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    for k, v in trainer.ema_unets[0].state_dict().items():
        assert torch.equal(v, ema[f"0.ema_model.{k}"]), k


def test_imagen_recasts_a_unet_and_keeps_the_five_options():
    import imagen_pytorch as ip

    u = ip.Unet(**{**KW, **SR.FIVE, "init_cross_embed_kernel_sizes": (3, 5)})
    im = ip.Imagen([u], image_sizes=(32,), timesteps=(2,), condition_on_text=False, channels=1)
    c = im.unets[0]
    assert c is not u and c.channels == 1
    for k in ("init_cross_embed", "init_conv_kernel_size", "final_conv_kernel_size", "final_resnet_block",
              "scale_skip_connection"):
        assert c._plan[k] == u._plan[k], k
        assert c._locals[k] == u._locals[k], k
    assert tuple(c.init_conv.weight.shape) == (32, 1, 5, 5) and tuple(c.final_conv.weight.shape) == (1, 32, 5, 5)
    assert c.final_res_block is None
    clone = u.cast_model_parameters(lowres_cond=True, text_embed_dim=None, channels=3, channels_out=3, cond_on_text=False)
    assert clone._plan["scale_skip_connection"] is False and tuple(clone.final_conv.weight.shape) == (3, 35, 5, 5)


REFUSED = [("init_conv_kernel_size", dict(init_cross_embed=False, init_conv_kernel_size=4)),
           ("init_conv_kernel_size", dict(init_cross_embed=False, init_conv_kernel_size=17)),
           ("init_conv_kernel_size", dict(init_cross_embed=False, init_conv_kernel_size=0)),
           ("init_cross_embed_kernel_sizes", dict(init_cross_embed_kernel_sizes=(3, 6))),
           ("init_cross_embed_kernel_sizes", dict(init_cross_embed_kernel_sizes=(3, 7, 17))),
           ("init_cross_embed_kernel_sizes", dict(init_cross_embed_kernel_sizes=())),
           ("init_cross_embed_kernel_sizes", dict(init_cross_embed_kernel_sizes=(1, 3, 5, 7, 9))),
           ("final_conv_kernel_size", dict(final_conv_kernel_size=2)),
           ("final_conv_kernel_size", dict(final_conv_kernel_size=9)),
           ("final_conv_kernel_size", dict(final_conv_kernel_size=0))]


@pytest.mark.parametrize("kwarg,over", REFUSED)
def test_values_the_engine_does_not_plan_are_refused_by_name(kwarg, over):
    import imagen_pytorch as ip

    with pytest.raises(NotImplementedError) as ei:
        ip.Unet(**{**KW, **over})
    msg = str(ei.value)
    assert kwarg in msg and str(over[kwarg]) in msg, msg


@pytest.mark.parametrize("over", [dict(init_cross_embed=False, init_conv_kernel_size=1),
                                  dict(init_cross_embed=False, init_conv_kernel_size=15),
                                  dict(init_cross_embed=False, init_conv_kernel_size=9),
                                  dict(init_cross_embed_kernel_sizes=(1,)), dict(init_cross_embed_kernel_sizes=(15,)),
                                  dict(init_cross_embed_kernel_sizes=(1, 3, 13, 15)),
                                  dict(final_conv_kernel_size=1), dict(final_conv_kernel_size=5),
                                  dict(final_conv_kernel_size=7)])
def test_the_neighbouring_planned_values_construct(over):
    import imagen_pytorch as ip

    ip.Unet(**{**KW, **over})


def test_gn_widths_do_not_demand_the_widths_of_an_absent_final_res_block():
    """The widths the GroupNorm check lists: without final_res_block the concat in front of final_conv (dim (2 + L) with the
    UpsampleCombiner and the init residual) is read by no GroupNorm and is not among them."""
    import imagen_pytorch as ip

    kw = dict(KW, dim=96, resnet_groups=12, combine_upsample_fmaps=True, init_conv_to_final_conv_residual=True)
    with_block = ip.Unet(**kw)
    without = ip.Unet(**kw, final_resnet_block=False)
    assert 96 * 4 in with_block._gn_widths
    assert set(without._gn_widths) == set(with_block._gn_widths) - {96 * 4}


def test_ext4_struct_mirrors_the_header_and_the_older_structs_keep_their_size():
    E = H.engine()
    header = (ROOT / "include" / "kd_engine.h").read_text()
    body = re.search(r"typedef struct kd_unet_ext4 \{(.*?)\} kd_unet_ext4_t;", header, re.S).group(1)
    fields = re.findall(r"\bint\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [n for n, _ in fields] == [n for n, _ in E.kd_unet_ext4_t._fields_]
    assert [int(k) if k else 1 for _, k in fields] == [C.sizeof(t) // 4 for _, t in E.kd_unet_ext4_t._fields_]
    assert C.sizeof(E.kd_unet_ext4_t) == 4 * 11 and not any(bytes(E.kd_unet_ext4_t()))
    assert C.sizeof(E.kd_unet_ext3_t) == 4 * E.KD_MAX_LEVELS and C.sizeof(E.kd_unet_ext2_t) == 4
    assert C.sizeof(E.kd_unet_ext_t) == 4 * (3 + 2 * E.KD_MAX_LEVELS)
    assert "#define KD_ENGINE_ABI_VERSION 2" in header and E.ABI_VERSION == 2
    for name in ("kd_unet_create_ext4", "kd_final_conv_k_nchw", "kd_init_conv_plain_nchw"):
        assert name in E.SIGNATURES and re.search(rf"\b{name}\(", header), name


def test_final_conv_kernels_compile_without_scratch_or_spills(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "kidney-diffusion_amd" / "csrc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", str(csrc / "kernels_final.hip"),
                          f"-I{csrc}", f"-I{ROOT / 'include'}", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "kernels_final.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", out.stderr)]
    # pack, static, gather x 4 channel counts (k = 3), the k = 1 columns kernel, gather k = 5 and k = 7
    assert len(names) == 9 and len(scratch) == len(spills) == 9, names
    assert sum("pack_final" in n for n in names) == 1, names
    assert any("final_gather_k_kernel" in n for n in names) and any("final_cols_kernel" in n for n in names), names
    assert not any(scratch) and not any(spills), f"scratch {scratch}, spills {spills}"
