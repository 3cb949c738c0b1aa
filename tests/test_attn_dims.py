"""`Unet(attn_dim_head=32 | 128, layer_attns_depth=...)` without a GPU: the constructor and state-dict layout against
oracle.imagen_ref.Unet, strict loading both ways, the refusals, the plan's depths, the new ABI struct and entries, and the
resource usage of the attention and qk-norm kernels' instantiations."""
import ctypes as C
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest
import torch

import helpers as H
from oracle import imagen_ref as R

ROOT = Path(__file__).resolve().parent.parent
KW = dict(dim=32, dim_mults=(1, 2, 4), num_resnet_blocks=1, layer_attns=(False, True, True),
          layer_cross_attns=(False, True, True), attn_heads=4, cond_on_text=False, text_embed_dim=None)
TEXT = dict(KW, cond_dim=64, cond_on_text=True, text_embed_dim=3)


# ------------------------------------------------------------------------------- construction and state dict
@pytest.mark.parametrize("d", [32, 128])
@pytest.mark.parametrize("dep", [2, (1, 2, 3)])
@pytest.mark.parametrize("base", ["plain", "text"])
def test_state_dict_layout_equals_the_oracle_and_round_trips(d, dep, base):
    kw = dict(TEXT if base == "text" else KW, attn_dim_head=d, layer_attns_depth=dep)
    p, r = H.random_product_unet(1, **kw), H.randomize_(R.Unet(**kw), 2)
    sp, sr = p.state_dict(), r.state_dict()
    assert H.state_layout(sp) == H.state_layout(sr)
    depths = (dep,) * 3 if isinstance(dep, int) else dep
    assert p._plan["layer_attns_depth"] == depths and p._plan["attn_dim_head"] == d
    for l in (1, 2):   # the attention levels: downs.l.3 and ups.(2 - l).2
        for pre in (f"downs.{l}.3", f"ups.{2 - l}.2"):
            for i in range(depths[l]):
                a = f"{pre}.layers.{i}.0"
                assert tuple(sp[a + ".null_kv"].shape) == (2, d)
                assert tuple(sp[a + ".to_q.weight"].shape)[0] == 4 * d and tuple(sp[a + ".to_kv.weight"].shape)[0] == 2 * d
                assert tuple(sp[a + ".to_context.1.weight"].shape)[0] == 2 * d
                assert f"{pre}.layers.{i}.1.4.weight" in sp
            assert f"{pre}.layers.{depths[l]}.0.to_q.weight" not in sp
    assert "downs.0.3.layers.0.0.to_q.weight" not in sp            # no attention at level 0, whatever its depth
    assert "mid_attn.layers.0.0.to_q.weight" in sp and "mid_attn.layers.1.0.to_q.weight" not in sp   # mid_attn: depth 1
    assert tuple(sp["mid_attn.layers.0.0.null_kv"].shape) == (2, d)
    assert tuple(sp["downs.1.1.cross_attn.null_kv"].shape) == (2, d)
    # the library builds the two middle ResnetBlocks without the attention kwargs: 8 heads of 64 whatever the UNet's are
    cd = kw.get("cond_dim", 32)
    for mb in ("mid_block1", "mid_block2"):
        assert tuple(sp[mb + ".cross_attn.null_kv"].shape) == (2, 64)
        assert tuple(sp[mb + ".cross_attn.to_kv.weight"].shape) == (2 * 8 * 64, cd)
    if base == "text":
        assert tuple(sp["attn_pool.layers.1.0.to_q.weight"].shape) == (4 * d, 64)
        assert tuple(sp["attn_pool.layers.0.0.to_kv.weight"].shape) == (8 * d, 64)
    p.load_state_dict(sr, strict=True)
    got = p.state_dict()
    assert all(torch.equal(got[k], sr[k]) for k in sr)
    r.load_state_dict(H.random_product_unet(3, **kw).state_dict(), strict=True)


@pytest.mark.parametrize("d", [32, 128])
def test_learned_scale_fork_sizes_q_scale_and_k_scale_by_dim_head(d):
    kw = dict(TEXT, attn_dim_head=d, layer_attns_depth=2)
    p, r = H.random_product_unet(4, **kw, attn_qk_norm=2), H.randomize_(R.Unet(**kw, attn_qk_norm=2), 5)
    sp, sr = p.state_dict(), r.state_dict()
    assert H.state_layout(sp) == H.state_layout(sr)
    scales = [k for k in sp if k.endswith(".q_scale") or k.endswith(".k_scale")]
    assert any(k.startswith("downs.1.3.layers.1.0.") for k in scales) and any(k.startswith("attn_pool.layers.") for k in scales)
    assert any(k.startswith("downs.1.1.cross_attn.") for k in scales) and any(k.startswith("mid_block1.cross_attn.") for k in scales)
    assert all(tuple(sp[k].shape) == ((64,) if k.startswith("mid_block") else (d,)) for k in scales)   # (mid blocks: 8 x 64)
    p.load_state_dict(sr, strict=True)
    # a Unet built without the fork follows a checkpoint that carries it
    q = H.random_product_unet(6, **kw)
    assert not any(k.endswith(".q_scale") for k in q.state_dict())
    q.load_state_dict(sr, strict=True)
    assert q.attn_qk_norm == 2 and H.state_layout(q.state_dict()) == H.state_layout(sr)


def test_default_unet_is_unchanged():
    d = H.random_product_unet(**KW)
    assert H.state_layout(d.state_dict()) == H.state_layout(R.Unet(**KW).state_dict())
    same = H.random_product_unet(**KW, attn_dim_head=64, layer_attns_depth=1)
    assert H.state_layout(d.state_dict()) == H.state_layout(same.state_dict())
    assert d._plan["layer_attns_depth"] == (1, 1, 1) and d._plan["attn_dim_head"] == 64


def test_cast_model_parameters_clones_keep_both_options():
    u = H.random_product_unet(**KW, attn_dim_head=32, layer_attns_depth=(1, 2, 3))
    clone = u.cast_model_parameters(lowres_cond=True, text_embed_dim=None, channels=3, channels_out=3, cond_on_text=False)
    assert clone._plan["layer_attns_depth"] == (1, 2, 3) and clone._plan["attn_dim_head"] == 32
    assert "ups.0.2.layers.2.0.to_q.weight" in clone.state_dict()


# ------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("d", [48, 256])
def test_other_dim_heads_are_refused(d):
    import imagen_pytorch as ip

    with pytest.raises(NotImplementedError, match="32, 64 and 128"):
        ip.Unet(**KW, attn_dim_head=d)


def test_linear_attention_keeps_dim_head_64_and_depth_1():
    import imagen_pytorch as ip

    lin = dict(KW, layer_attns=(False, False, True))
    with pytest.raises(NotImplementedError, match="linear-attention kernels are built for dim_head 64"):
        ip.Unet(**lin, use_linear_attn=True, attn_dim_head=32)
    with pytest.raises(NotImplementedError, match="dim_head 64"):
        ip.Unet(**lin, use_linear_cross_attn=True, attn_dim_head=128)
    with pytest.raises(NotImplementedError, match="linear-attention level"):
        ip.Unet(**lin, use_linear_attn=True, layer_attns_depth=2)
    with pytest.raises(NotImplementedError, match="linear-attention level"):
        ip.Unet(**lin, use_linear_attn=True, layer_attns_depth=(1, 2, 1))
    # depth > 1 only where full attention wins the slot: planned
    u = ip.Unet(**lin, use_linear_attn=True, layer_attns_depth=(1, 1, 2))
    assert "downs.2.3.layers.1.0.to_q.weight" in u.state_dict()
    assert "downs.1.3.layers.0.0.to_q.1.weight" in u.state_dict() and "downs.1.3.layers.1.0.to_q.1.weight" not in u.state_dict()


def test_strict_load_tells_depths_apart():
    import imagen_pytorch as ip

    two = R.Unet(**KW, layer_attns_depth=2).state_dict()
    ip.Unet(**KW, layer_attns_depth=2).load_state_dict(two, strict=True)
    with pytest.raises(RuntimeError):
        ip.Unet(**KW).load_state_dict(two, strict=True)
    with pytest.raises(RuntimeError):
        ip.Unet(**KW, layer_attns_depth=2).load_state_dict(R.Unet(**KW).state_dict(), strict=True)
    with pytest.raises(RuntimeError):
        ip.Unet(**KW, attn_dim_head=32).load_state_dict(R.Unet(**KW).state_dict(), strict=True)


# ------------------------------------------------------------------------------- ABI
def test_ext3_struct_mirrors_the_header_and_the_older_structs_keep_their_size():
    from imagen_pytorch import _engine as E

    header = (ROOT / "include" / "kd_engine.h").read_text()
    body = re.search(r"typedef struct kd_unet_ext3 \{(.*?)\} kd_unet_ext3_t;", header, re.S).group(1)
    assert re.findall(r"\bint\s+(\w+)\[KD_MAX_LEVELS\];", body) == [n for n, _ in E.kd_unet_ext3_t._fields_] == ["layer_attns_depth"]
    assert C.sizeof(E.kd_unet_ext3_t) == 4 * E.KD_MAX_LEVELS and list(E.kd_unet_ext3_t().layer_attns_depth) == [0] * E.KD_MAX_LEVELS
    assert C.sizeof(E.kd_unet_ext2_t) == 4
    assert C.sizeof(E.kd_unet_ext_t) == 4 * (3 + 2 * E.KD_MAX_LEVELS)
    assert C.sizeof(E.kd_unet_config_t) == 4 * (2 + 4 * E.KD_MAX_LEVELS + 27)
    assert "#define KD_ENGINE_ABI_VERSION 2" in header
    lib = E.load()
    for name in ("kd_unet_create_ext3", "kd_attention_ex_d", "kd_l2norm_heads_d", "kd_attention_key_tile"):
        assert f" {name}(" in header and name in E.SIGNATURES and hasattr(lib, name), name
    assert lib.kd_version() == 2
    assert [lib.kd_attention_key_tile(d) for d in (32, 64, 128, 48, 256)] == [64, 64, 32, 0, 0]


# ------------------------------------------------------------------------------- compile check
def test_attention_and_qk_norm_kernels_compile_without_scratch_or_spills(tmp_path):
    """Every kernel of kernels_attn.hip and kernels_text.hip (l2norm_heads_kernel): ScratchSize 0 and no spilled VGPRs.  The
    guard for the D = 128 instantiations, which hold 64 + 64 registers of q / o per lane."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = ROOT / "kidney-diffusion_amd" / "csrc"
    srcs = ("kernels_attn.hip", "kernels_text.hip")

    def compile_one(src):
        return subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", str(csrc / src),
                               f"-I{csrc}", f"-I{ROOT / 'include'}", "-Rpass-analysis=kernel-resource-usage",
                               "-o", str(tmp_path / (src + ".o"))], capture_output=True, text=True, timeout=900)

    with ThreadPoolExecutor(max_workers=2) as pool:
        outs = dict(zip(srcs, pool.map(compile_one, srcs)))
    names = []
    for src, out in outs.items():
        assert out.returncode == 0, out.stderr[-2000:]
        fn = re.findall(r"Function Name: (\S+)", out.stderr)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
        spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", out.stderr)]
        assert fn and len(fn) == len(scratch) == len(spills), f"{src}: no resource-usage remarks"
        bad = [(n, s, v) for n, s, v in zip(fn, scratch, spills) if s or v]
        assert not bad, f"{src}: (kernel, scratch, spilled VGPRs) {bad}"
        names += fn
    for d in (32, 64, 128):   # the three instantiations of each kernel are there
        assert any(re.search(rf"attention_mfma_kernelILi{d}E", n) for n in names), d
        assert any(re.search(rf"attention_kernelILi4ELi{d}E", n) for n in names), d
        assert any(re.search(rf"l2norm_heads_kernelILi{d}E", n) for n in names), d
