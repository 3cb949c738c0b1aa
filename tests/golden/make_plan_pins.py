"""Records tests/golden/plan_pins.json: what the plan builder gives for the cases of tests/test_plan_pins_gpu.py.  Needs the
GPU.  The committed file was recorded on an MI355X with the library of the last commit that had Builder::build() as one
body (before it became the list of its stages); recording it again from a later build only pins that build to itself.
It uses nothing but Unet.engine, helpers.plan_csv, kd_unet_num_launches, kd_unet_num_cond_launches and kd_unet_hbm_bytes.

    python tests/golden/make_plan_pins.py [OUT]

Recipe of the recording: check out the last commit with the one-body build() (the parent of the commit that added this
file), build its library, copy this file and tests/test_plan_pins_gpu.py (the case table and record(); neither exists
there) into that checkout, and run the line above in it; the JSON it writes is the committed one.

Which case takes which branch of build() (every case also walks the common path):

  batch 1 / 2 / 3                          narrow_b1, narrow_b2, narrow_b3
  the default fast plan (F(4x4,3x3) and fused F(2x2,3x3) layers; the popped skip's scale folded by its consumer)
                                           fast, fast_no_gca, fast_mem_eff_residual_lowres, fast_combine; fast_no_skip_scale
                                           (nothing to fold)
  memory_efficient off / on                narrow_b2 / mem_eff, mem_eff_residual, blocks_3_mem_eff
  use_gca on / off (hiddens without a slot, the offered concat allocated for the offer, concat_skip)
                                           narrow_b2 / no_gca, no_gca_residual, no_gca_mem_eff_residual, combine_no_gca,
                                           blocks_0_no_gca_mem_eff
  full attention, linear attention, neither (the copied second skip) in one model
                                           linear_attn, linear_attn_mem_eff (levels 2, 1, 0); neither + full: narrow_b2
  use_linear_cross_attn                    linear_attn
  layer_attns_depth > 1                    attn_depth_2_3
  num_resnet_blocks 1 / 3 / 0 (the up path's nb == 0 branch)
                                           narrow_b2 / blocks_132, blocks_3_mem_eff / blocks_011, blocks_0_no_gca_mem_eff,
                                           no_final_block_blocks_0
  init_conv_to_final_conv_residual off / on (written in place by the last upsample; behind a copied head)
                                           narrow_b2 / mem_eff_residual, nearest_up_mem_eff_residual; residual, no_gca_residual
  combine_upsample_fmaps x memory_efficient x the init residual
                                           combine, combine_mem_eff, combine_residual, combine_mem_eff_residual
  ... the head written by a ResnetBlock / a TransformerBlock / a linear block / copied
                                           combine / combine_attn_outer / combine_linear_outer / combine_no_gca
  lowres_cond (both hoisted static shares) lowres, text_lowres, plain_init_k7_lowres, final_k5_lowres, channels_4_lowres
  cond_images_channels > 0                 cond_images, self_cond_lowres_cond_images
  self_cond                                self_cond, self_cond_lowres_cond_images, channels_4_final_k7_self_cond
  text conditioning                        text, text_lowres
  init_cross_embed=False at k = 3, 7 (one kernel), 9 (generic)
                                           plain_init_k3, plain_init_k7_lowres, plain_init_k9
  init_cross_embed_kernel_sizes            init_sizes_3_5, init_sizes_3_7_15_5_lowres (a slice of 4 channels: no partials)
  init_conv_generic                        init_generic, init_generic_self_cond_lowres_residual, plain_init_k7_generic
  final_conv_kernel_size 1 / 3 / 5 / 7     final_k1 / narrow_b2 / final_k5_lowres / final_k7, channels_4_final_k7_self_cond
  final_resnet_block=False, a ResnetBlock last / an upsample last
                                           no_final_block, no_final_block_blocks_0, no_final_block_residual /
                                           no_final_block_mem_eff, no_final_block_mem_eff_residual_lowres
  ... over the combiner's concat           no_final_block_combine_residual
  scale_skip_connection=False              no_skip_scale, fast_no_skip_scale
  cross_embed_downsample                   cross_embed_down, cross_embed_down_mem_eff
  pixel_shuffle_upsample=False             nearest_up, nearest_up_mem_eff_residual
  channels 1 / 4                           channels_1 / channels_4_lowres, channels_4_final_k7_self_cond
  the conv4x4 downsample fork              conv4x4_down, conv4x4_down_mem_eff
  the residual_attention mid fork; no middle attention
                                           residual_attention_mid; no_mid_attn
"""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "kidney-diffusion_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_plan_pins_gpu as T  # noqa: E402

MAX_BYTES = 115 * 1000   # what the last fixture kept to


def main():
    device = torch.device("cuda:0")
    out = {}
    for name in sorted(T.CASES):
        t0 = time.time()
        out[name] = T.record(name, device)
        print(f"{name}: {out[name]['launches']} launches, {out[name]['hbm_bytes']} bytes, {time.time() - t0:.1f} s", flush=True)
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else T.GOLDEN
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
    size = path.stat().st_size
    assert size < MAX_BYTES, f"{path}: {size} bytes"
    print(f"{path}: {size} bytes, {len(out)} cases")


if __name__ == "__main__":
    main()
