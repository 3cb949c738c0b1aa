"""Linear-attention UNets (library `Unet(use_linear_attn=..., use_linear_cross_attn=...)`) without a GPU: construction,
the state-dict layout against the restatement in tests/linear_attn_ref.py, strict loading (also through ImagenTrainer),
the per-level rules, and the resource usage of the new kernel file."""
import functools
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

import helpers as H
import linear_attn_ref as LR

ROOT = Path(__file__).resolve().parent.parent
KW = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, False, True),
          layer_cross_attns=(False, False, True), use_linear_attn=True, use_linear_cross_attn=(False, True, False),
          cond_on_text=False, text_embed_dim=None)


_product = functools.partial(H.random_product_unet, **KW)   # _product(seed=0, **over)


def _ref(seed=0, **over):
    return H.randomize_(LR.Unet(**{**KW, **over}), seed)


def test_linear_attention_unet_constructs():
    u = _product()
    assert type(u.downs[0][3]).__name__ == "LinearAttentionTransformerBlock"
    assert type(u.downs[1][3]).__name__ == "LinearAttentionTransformerBlock"
    assert type(u.downs[2][3]).__name__ == "TransformerBlock"   # full attention wins
    assert type(u.downs[1][1].cross_attn).__name__ == "LinearCrossAttention"
    assert not hasattr(u.downs[0][1], "cross_attn")
    assert type(u.downs[2][1].cross_attn).__name__ == "CrossAttention"


def test_state_dict_layout_equals_the_restatement():
    sp = _product().state_dict()
    assert H.state_layout(sp) == H.state_layout(_ref().state_dict())
    assert tuple(sp["downs.0.3.layers.0.0.to_q.2.weight"].shape) == (512, 1, 3, 3)
    assert tuple(sp["downs.0.3.layers.0.0.to_k.1.weight"].shape) == (512, 32, 1, 1)
    assert tuple(sp["downs.0.3.layers.0.0.norm.g"].shape) == (1, 32, 1, 1)
    assert tuple(sp["downs.0.3.layers.0.0.to_context.1.weight"].shape) == (1024, 32)
    assert "downs.0.3.layers.0.0.to_context.1.bias" not in sp
    assert tuple(sp["downs.0.3.layers.0.0.to_context.0.bias"].shape) == (32,)
    assert tuple(sp["downs.0.3.layers.0.1.4.weight"].shape) == (32, 64, 1, 1)
    assert tuple(sp["downs.0.3.layers.0.1.3.g"].shape) == (1, 64, 1, 1)
    assert "downs.2.3.layers.0.0.to_kv.weight" in sp and "downs.2.3.layers.0.0.to_k.1.weight" not in sp
    assert tuple(sp["downs.1.1.cross_attn.null_kv"].shape) == (2, 64)
    assert tuple(sp["ups.1.0.cross_attn.to_kv.weight"].shape) == (1024, 32)
    assert "ups.2.2.layers.0.0.to_v.2.weight" in sp and "ups.0.2.layers.0.0.to_kv.weight" in sp
    assert "downs.0.1.cross_attn.null_kv" not in sp


def test_strict_load_both_ways():
    p, r = _product(seed=1), _ref(seed=2)
    p.load_state_dict(r.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(p.state_dict().values(), [r.state_dict()[k] for k in p.state_dict()]))
    p2 = _product(seed=3)
    r.load_state_dict(p2.state_dict(), strict=True)
    sr, s2 = r.state_dict(), p2.state_dict()
    assert all(torch.equal(sr[k], s2[k]) for k in s2)
    # a plain UNet refuses a linear-attention checkpoint on a strict load
    import imagen_pytorch as ip

    plain = ip.Unet(**{**KW, "use_linear_attn": False, "use_linear_cross_attn": False})
    with pytest.raises(RuntimeError):
        plain.load_state_dict(p2.state_dict(), strict=True)


def test_linear_attention_checkpoint_loads_strictly_through_the_trainer(tmp_path, monkeypatch):
    import imagen_pytorch as ip
    import imagen_pytorch.trainer as T

    kw = dict(image_sizes=(32,), timesteps=(2,), condition_on_text=False)
    src = ip.Imagen([_product(seed=4)], **kw)
    dst = ip.Imagen([_product(seed=5)], **kw)
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


def test_per_level_tuples_and_the_full_attention_precedence():
    over = dict(use_linear_attn=(True, False, True), use_linear_cross_attn=True)
    u = _product(**over)
    kinds = [type(u.downs[l][3]).__name__ for l in range(3)]
    assert kinds == ["LinearAttentionTransformerBlock", "_Stateless", "TransformerBlock"]
    assert [type(u.ups[j][2]).__name__ for j in range(3)] == ["TransformerBlock", "_Stateless",
                                                              "LinearAttentionTransformerBlock"]
    for l in range(3):   # every level, the one with layer_cross_attns included, gets the linear form
        assert type(u.downs[l][1].cross_attn).__name__ == "LinearCrossAttention"
        assert type(u.ups[2 - l][0].cross_attn).__name__ == "LinearCrossAttention"
    assert type(u.mid_block1.cross_attn).__name__ == "CrossAttention"   # the middle is unchanged
    assert H.state_layout(u.state_dict()) == H.state_layout(_ref(**over).state_dict())
    assert u._plan["use_linear_attn"] == (True, False, True) and u._plan["use_linear_cross_attn"] == (True,) * 3


def test_memory_efficient_self_cond_and_qk_norm_layouts_equal_the_restatement():
    import imagen_pytorch as ip

    kw = dict(H.UNET_KW["ultra2"], use_linear_attn=True, use_linear_cross_attn=True, lowres_cond=True,
              cond_on_text=False, text_embed_dim=None)
    assert H.state_layout(ip.Unet(**kw).state_dict()) == H.state_layout(LR.Unet(**kw).state_dict())
    kw.update(self_cond=True, attn_qk_norm=2)
    sp = ip.Unet(**kw).state_dict()
    assert H.state_layout(sp) == H.state_layout(LR.SelfCondUnet(**kw).state_dict())
    assert "downs.0.1.cross_attn.q_scale" in sp   # (loads with the module; the linear form does not use it)


def test_restated_linear_cross_attention_with_one_token_keys_equals_its_value_map():
    """Sanity of the restatement: with every key equal the k-softmax is uniform, so the output is mean(v) mapped by
    to_out; checked on a LinearCrossAttention whose null key and context keys are all zero."""
    torch.manual_seed(0)
    ca = LR.LinearCrossAttention(32, context_dim=16, heads=2, dim_head=64)
    with torch.no_grad():
        ca.to_kv.weight[:128].zero_()
        ca.null_kv[0].zero_()
    x, c = torch.randn(2, 5, 32), torch.randn(2, 3, 16)
    v = torch.cat((ca.null_kv[1].expand(2, 2, 1, 64), ca.to_kv(c)[..., 128:].reshape(2, 3, 2, 64).transpose(1, 2)), 2)
    q = ca.to_q(ca.norm(x)).reshape(2, 5, 2, 64).transpose(1, 2).softmax(-1) * ca.scale
    want = ca.to_out((q.sum(-1, keepdim=True) * v.mean(2, keepdim=True)).transpose(1, 2).reshape(2, 5, -1))
    assert torch.allclose(ca(x, c), want, atol=1e-6)


def test_linattn_kernels_compile_without_scratch_or_spills(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "kidney-diffusion_amd" / "csrc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", str(csrc / "kernels_linattn.hip"),
                          f"-I{csrc}", f"-I{ROOT / 'include'}", "-Rpass-analysis=kernel-resource-usage",
                          "-o", str(tmp_path / "kernels_linattn.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", out.stderr)]
    assert len(names) == 5 and len(scratch) == len(spills) == 5, names   # pack, dwconv, reduce, combine, apply
    assert not any(scratch) and not any(spills), f"scratch {scratch}, spills {spills}"
