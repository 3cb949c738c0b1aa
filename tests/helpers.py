"""Shared builders for the tests: matched (oracle, product) models with identical weights.

Reference kwargs being mirrored (at reduced `dim`, so the oracle finishes in seconds):
  ultra-res unet1/2/3   train_ultra_res.py:29-60
  uncond unet1          train_uncond.py:30-36
"""
import torch

from oracle import imagen_ref as R
from oracle import sampler_ref as RS

# name -> (Unet kwargs, lowres_cond)
UNET_KW = {
    "ultra1": dict(dim=32, dim_mults=(1, 2, 4, 8), num_resnet_blocks=3, layer_attns=(False, True, True, True),
                   layer_cross_attns=(False, True, True, True), cond_images_channels=3),
    "ultra2": dict(dim=32, dim_mults=(1, 2, 4, 8), num_resnet_blocks=2, memory_efficient=True,
                   layer_attns=(False, False, False, True), layer_cross_attns=(False, False, True, True),
                   init_conv_to_final_conv_residual=True, cond_images_channels=3),
    "ultra3": dict(dim=32, dim_mults=(1, 2, 4, 8), num_resnet_blocks=(2, 4, 6, 8), memory_efficient=True,
                   layer_attns=False, layer_cross_attns=(False, False, False, True),
                   init_conv_to_final_conv_residual=True, cond_images_channels=3),
    "uncond1": dict(dim=32, dim_mults=(1, 2, 4, 8), cond_dim=64, num_resnet_blocks=3,
                    layer_attns=(False, True, True, True), layer_cross_attns=(False, True, True, True)),
    "small1": dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, layer_attns=(False, True),
                   layer_cross_attns=(False, True)),
    "small2": dict(dim=32, dim_mults=(1, 2), num_resnet_blocks=1, memory_efficient=True, layer_attns=(False, True),
                   layer_cross_attns=(False, True), init_conv_to_final_conv_residual=True, cond_images_channels=3),
}


NOTEXT = dict(cond_on_text=False, text_embed_dim=None)


def randomize_(module, seed, std=0.05):
    """Deterministic non-trivial weights: defaults under the seed, then every zero-/one-initialised
    tensor (final conv, norm gains/biases, pixel-shuffle biases) gets noise so no term is hidden."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            if p.numel() == 1 and name.endswith("dummy_parameter"):
                continue
            if name.endswith(".g") or name.endswith("groupnorm.weight") or name.endswith("norm.weight") \
                    or name.endswith("norm_cond.weight") or name.endswith("norm_latents.weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "final_conv" in name:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            else:
                fan_in = p[0].numel() if p.dim() > 1 else p.numel()
                p.copy_(torch.randn(p.shape, generator=g) * (fan_in ** -0.5))
    return module


def oracle_unet(name, lowres_cond=False, seed=0):
    kw = dict(UNET_KW[name])
    u = R.Unet(**kw, lowres_cond=lowres_cond, **NOTEXT)
    return randomize_(u, seed)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def engine():
    """imagen_pytorch._engine (the ctypes binding of the C ABI), imported on first use."""
    from imagen_pytorch import _engine

    return _engine


def ref_unet(cls, kw, *, seed, text=False, **extra):
    """A randomised oracle UNet in eval mode.  `cls` is the restatement under test (oracle.imagen_ref.Unet or a tests/*_ref.py
    subclass of it); lowres_cond=..., self_cond=... and the option under test go through `extra`."""
    return randomize_(cls(**{**kw, **(dict(cond_on_text=True) if text else NOTEXT), **extra}), seed).eval()


def product_like(ou, device=None, **plan):
    """The product UNet over the oracle UNet's constructor arguments and weights.  `plan`: engine extensions (conv_algo,
    gemm_bf16x3, ...), set as attributes before any plan is built."""
    import imagen_pytorch as ip

    u = ip.Unet(**ou._locals)
    missing, unexpected = u.load_state_dict(ou.state_dict(), strict=True)
    assert not missing and not unexpected
    for k, v in plan.items():
        setattr(u, k, v)
    return u if device is None else u.to(device)


product_unet_like = product_like


def random_product_unet(seed=0, **kw):
    """A product UNet with randomize_'d weights of its own (the CPU tests of constructors and state-dict layouts)."""
    import imagen_pytorch as ip

    return randomize_(ip.Unet(**kw), seed)


def unet_inputs(ou, B, S, seed, text_len=2):
    """(x, t, kw) of one forward of `ou` on the CPU, drawn in this order from one generator: x, t, the low-res image, the
    cond images, self_cond, the text embeddings - each only where the UNet takes it."""
    g, C = gen(seed), ou.channels
    x = torch.randn(B, C, S, S, generator=g)
    t = torch.randn(B, generator=g) * 3
    kw = {}
    if ou.lowres_cond:
        kw.update(lowres_cond_img=torch.randn(B, C, S, S, generator=g), lowres_noise_times=torch.full((B,), 1.5))
    if ou.has_cond_image:
        kw["cond_images"] = torch.rand(B, ou.cond_images_channels, S, S, generator=g)
    if getattr(ou, "self_cond", False):
        kw["self_cond"] = torch.rand(B, C, S, S, generator=g) * 2 - 1
    if ou.cond_on_text:
        kw["text_embeds"] = torch.randn(B, text_len, 3, generator=g)
    return x, t, kw


def forward_err(ou, device, x, t, kw, ref=None, **plan):
    """(rel-L2 of the product's forward against the oracle's, the product UNet).  The product runs twice: the engine has no
    atomics, so the two results must be bit-identical.  `ref`: the oracle's output where the caller has it already."""
    pu = product_like(ou, device, **plan)
    if ref is None:
        with torch.no_grad():
            ref = ou(x, t, **kw)
    dv = {k: v.to(device) for k, v in kw.items()}
    got = pu(x.to(device), t.to(device), **dv).cpu()
    assert torch.equal(got, pu(x.to(device), t.to(device), **dv).cpu())   # no atomics: run-to-run bit-identical
    return rel_l2(got, ref), pu


def plan_csv(pu, B=None, S=None, device=None, with_text=False):
    """The CSV of kd_unet_profile (one iteration, current stream) for a plan handle, or for the plan
    `pu.engine(B, S, device, with_text=with_text)` of a product UNet.  The profile replays the inputs of the last forward."""
    import ctypes

    E = engine()
    h = pu.engine(B, S, device, with_text=with_text) if hasattr(pu, "engine") else pu
    buf = ctypes.create_string_buffer(1 << 20)
    E.check(E.load().kd_unet_profile(h, 1, buf, len(buf), E.current_stream()))
    return buf.value.decode()


def plan_labels(pu, *args, **kw):
    """The label column of plan_csv (the strings of Builder's emit() calls, engine.hip), one per launch."""
    return [row.split(",")[1] for row in plan_csv(pu, *args, **kw).strip().split("\n")[1:]]


def count_labels(labels, *prefixes):
    return sum(l.startswith(prefixes) for l in labels)


def product_imagen(oim, cls_p, device, **imagen_kw):
    """The product sampler `cls_p` ("Imagen" | "ElucidatedImagen") over the UNets and weights of the oracle sampler `oim`."""
    import imagen_pytorch as ip

    pus = [ip.NullUnet() if isinstance(u, R.NullUnet) else ip.Unet(**u._locals) for u in oim.unets]
    pim = getattr(ip, cls_p)(pus, **imagen_kw)
    pim.load_state_dict(oim.state_dict(), strict=True)
    return pim.to(device)


def imagen_pair(device, cls_o, cls_p, unets, **imagen_kw):
    """(oracle sampler on the CPU, product sampler on `device`) over the same UNets, weights and keyword arguments."""
    oim = cls_o(unets, **imagen_kw)
    return oim, product_imagen(oim, cls_p, device, **imagen_kw)


def sample_last(h, which, shape, device):
    """kd_sample_last of a sampling plan (0 the UNet output, 1 the x0 estimate, 2 the thresholds), fp64 on the CPU."""
    E = engine()
    out = torch.empty(shape, device=device)
    E.check(E.load().kd_sample_last(h, which, E.ptr(out), E.current_stream()))
    return out.double().cpu()


def dev_ptr(t):
    """Device address of a (possibly strided, possibly fp64) tensor view: the entries take the strides as arguments."""
    assert t is None or t.is_cuda
    return None if t is None else t.data_ptr()


def nan_dev(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda:0")


def state_layout(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def fast_oracle(u):
    """The oracle UNet `u` with its convolutions in channels_last (oneDNN's NHWC kernels: about a third less host time at full
    size; same arithmetic, another fp32 summation order - 1e-6 rel-L2, the oracle's own resolution).  Used by the full-size
    GPU tests only; the golden fixtures and the CPU tests run the default layout."""
    import torch

    u = u.to(memory_format=torch.channels_last)
    u.channels_last = True
    return u
