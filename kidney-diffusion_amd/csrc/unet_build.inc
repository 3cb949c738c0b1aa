// Builder::build(): emits the launch list of one UNet forward.  Mirrors Unet.forward of
// imagen-pytorch 1.18.5 as restated in SURVEY.md Appendix A.1 (the reference selects the
// variants at train_ultra_res.py:29-60, train.py:30-65, train_uncond.py:30-61).
// build() is the list of its stages; the order of every alloc / free / retain / emit across them fixes the arena's offsets.
namespace kd {

void Builder::build() {
  const Model m = model();
  collect_time_mlps();
  gn_scratch(m);
  const FinalConv fin = final_conv_setup(m);
  const T c = conditioning(m);
  const InitConv init = init_conv(m);
  T x = init.x;
  if (m.keep_init) retain(init.x);   // it lives on to the tail as the residual
  SkipStack skips(*this);
  Combiner comb(*this, m);
  down_path(m, x, c, skips);
  middle(m, x, c);
  up_path(m, x, c, skips, comb, init.x);
  skips.finish();
  tail(m, x, c, comb, init.x);
  final_conv(m, fin, x);
  release(x, fin, init);
}

// ---- argument checks; the per-model constants every stage reads
Builder::Model Builder::model() {
  Model m;
  const int dim = m.dim = cfg.dim, L = m.L = cfg.num_levels, S = m.S = cfg.image_size;
  u->time_cond_dim = m.tcd = dim * 4 * (cfg.lowres_cond ? 2 : 1);
  if (L < 1 || L > KD_MAX_LEVELS) throw std::runtime_error("num_levels out of range");
  if (cfg.channels < 1 || cfg.channels > 4) throw std::runtime_error("images of 1 to 4 channels are supported");
  m.Ci = cfg.channels;
  if (cfg.attn_dim_head != 32 && cfg.attn_dim_head != 64 && cfg.attn_dim_head != 128)
    throw std::runtime_error("the attention kernels are built for attn_dim_head 32, 64 and 128");
  for (int l = 0; l < L; ++l)
    if (u->lin_attn[l] || u->lin_cross[l]) {
      if (cfg.attn_dim_head != 64) throw std::runtime_error("the linear-attention kernels are built for attn_dim_head = 64");
      if (u->lin_attn[l] && !cfg.layer_attns[l] && u->attn_depth[l] != 1)
        throw std::runtime_error("layer_attns_depth > 1 on a linear-attention level is not supported");
      if (u->lin_cross[l]) {   // use_linear_cross_attn: the level's first ResnetBlock on each path gets (linear) cross-attention
        lin_cross_pre.insert("downs." + std::to_string(l) + ".1");
        lin_cross_pre.insert("ups." + std::to_string(L - 1 - l) + ".0");
      }
    }
  if (B < 1 || S < 1) throw std::runtime_error("batch and image_size must be positive");
  const int n_down = cfg.memory_efficient ? L : L - 1;
  if (S % (1 << n_down)) throw std::runtime_error("image_size must be divisible by the total downsampling factor");
  if (dim % 32) throw std::runtime_error("dim must be a multiple of 32 (GroupNorm(8) over dim/8 channels, 16-B loads)");
  m.dims.push_back(dim);
  for (int l = 0; l < L; ++l) m.dims.push_back(dim * cfg.dim_mults[l]);
  m.keep_init = cfg.init_conv_to_final_conv_residual != 0;
  m.combine = u->combine_upsample_fmaps != 0;
  m.cat_w = dim * (1 + L) + (m.keep_init ? dim : 0);
  m.final_res = u->no_final_res == 0;
  m.fin_w = m.final_res ? dim : m.combine ? m.cat_w : dim + (m.keep_init ? dim : 0);
  m.skip_scale = u->skip_scale;
  return m;
}

// scratch shared by every GroupNorm, sized for the largest (rows x channels) it will see
void Builder::gn_scratch(const Model& m) {
  size_t mx = gn_partial_bytes(B, m.S * m.S, 2 * m.dim, cfg.resnet_groups);
  int res = m.S;
  for (int l = 0; l < m.L; ++l) {
    if (cfg.memory_efficient) res /= 2;
    int widest = 2 * std::max(m.dims[l], m.dims[l + 1]) + m.dims[l + 1];
    mx = std::max(mx, gn_partial_bytes(B, res * res, widest, cfg.resnet_groups));
    if (!cfg.memory_efficient && l < m.L - 1) res /= 2;
  }
  gn_partial_max = mx;
  gn_partial_t = alloc_bytes(mx);
  gn_stats_t = alloc_bytes((size_t)B * cfg.resnet_groups * 2 * sizeof(float));
}

// ---- final conv over cat(x, lowres_cond_img) to the image's channels (kernels_final.hip): a 1x1 GEMM to the ks^2 Ci
// (output, tap) columns on the matrix cores + a ks^2-tap gather; the low-res planes' share is step-invariant and computed
// once per sampling call.  A buffer that is written once per sampling call (static_ops) and read by every step is allocated
// FIRST and stays live to the end of the build, so the arena can never hand its space to a per-step tensor: the set-up runs
// at the top of build(), the launches are emitted at the bottom.
// (final_resnet_block=False: final_conv reads the concat in front of it, fin_w channels)
Builder::FinalConv Builder::final_conv_setup(const Model& m) {
  FinalConv f;
  const int Ci = m.Ci, S = m.S, Bx = B, fks = f.ks = u->final_ks, fin_w = f.w = m.fin_w;
  const int fin_c = f.cin = fin_w + (cfg.lowres_cond ? Ci : 0);
  f.n = final_gemm_cols_k(Ci, fks);
  const float* wfin = P("final_conv.weight", (int64_t)Ci * fin_c * fks * fks);
  const float* bfin = f.bias = P("final_conv.bias", Ci);
  f.w_packed = cached("final_conv_gemm", (size_t)f.n * fin_w,
                      [&](float* dst) { KD_THROW_IF(launch_pack_final_k(wfin, dst, fin_c, fin_w, Ci, fks, 0)); });
  f.has_static = cfg.lowres_cond != 0;
  if (f.has_static) {
    auto ph = scope(Phase::Static);
    f.stat = alloc(B, Ci, S, S);
    const Ref fr = at(f.stat);
    const kd_unet* io = u;   // the per-call inputs and the output buffer are read through it when an op runs
    emit([=](hipStream_t s) {
      if (!io->in_lowres) {
        set_error("lowres_cond_img must be given iff the UNet has lowres_cond");
        return 1;
      }
      return launch_final_static(io->in_lowres, wfin, bfin, fr.f(), fin_c, fin_w, Ci, Bx, S, S, s, fks);
    });
  }
  return f;
}

void Builder::final_conv(const Model& m, const FinalConv& f, const T& x) {
  if (x.C != f.w) throw std::runtime_error("plan: final conv input of the wrong width");
  const int Ci = m.Ci, S = m.S, Bx = B, fks = f.ks;
  const float* bfin = f.bias;
  const kd_unet* io = u;
  ConvOpt o;
  o.macs_override = (int64_t)B * S * S * Ci * f.cin * fks * fks;
  T pm = conv(x, f.w_packed, nullptr, f.n, 1, 1, 0, o);
  const Ref pr = at(pm), fr = f.has_static ? at(f.stat) : Ref();
  emit([=](hipStream_t s) {
    return launch_final_gather_k(pr.f(), fr.f(), bfin, io->out, Ci, fks, Bx, S, S, s);
  }, fks == 3 ? std::string("final gather") : "final gather k" + std::to_string(fks));
  free(pm);
}

// ---- conditioning: time (+ low-res time) embeddings, tokens, batched FiLM scale/shift (t_ss).  Returns the normalised
// conditioning tokens; everything here is a function of (log_snr, lowres_log_snr, text) only
T Builder::conditioning(const Model& m) {
  const int cd = cfg.cond_dim, tcd = m.tcd, Bx = B;
  const kd_unet* io = u;
  const int n_time_tok = cfg.num_time_tokens * (cfg.lowres_cond ? 2 : 1);
  const int ntok = n_time_tok + cfg.text_tokens;
  auto cond_ph = scope(Phase::Cond);
  T c_raw = alloc(B, 1, ntok, cd);
  T t_emb = alloc(B, 1, 1, tcd);
  {
    T emb = alloc(B, 1, 1, cfg.sinu_dim + 1), hidden = alloc(B, 1, 1, tcd);
    time_trio("to_time_hiddens", "to_time_cond", "to_time_tokens", false, t_emb, c_raw, 0, emb, hidden);
    if (cfg.lowres_cond) {
      T t2 = alloc(B, 1, 1, tcd);
      time_trio("to_lowres_time_hiddens", "to_lowres_time_cond", "to_lowres_time_tokens", true, t2, c_raw,
                cfg.num_time_tokens, emb, hidden);
      const Ref ar = at(t_emb), br = at(t2);
      int64_t n = (int64_t)B * tcd;
      emit([=](hipStream_t s) { return launch_add(ar.f(), br.f(), ar.f(), n, s); });
      free(t2);
    }
    free(emb);
    free(hidden);
  }
  if (cfg.text_tokens > 0) {
    int nt = cfg.text_tokens;
    const Ref cr = at(c_raw).floats((int64_t)n_time_tok * cd), tr = at(t_emb);
    int64_t n = (int64_t)B * tcd;
    emit([=](hipStream_t s) {
      if (!io->in_text_tokens || !io->in_text_hiddens) {
        set_error("this UNet was planned with text conditioning: text_tokens/text_hiddens are required");
        return 1;
      }
      if (launch_copy_rows(io->in_text_tokens, (int64_t)nt * cd, cd, cr.f(), (int64_t)ntok * cd, cd, nt, cd, Bx, s)) return 1;
      return launch_add(tr.f(), io->in_text_hiddens, tr.f(), n, s);
    });
  }
  T c = layernorm(c_raw, P("norm_cond.weight", cd), P("norm_cond.bias", cd));
  free(c_raw);
  if (tmlp_total > 0) {
    t_ss = alloc(B, 1, 1, tmlp_total);
    skinny(at(t_emb), tcd, tmlp_w, tmlp_b, at(t_ss), tmlp_total, B, tcd, tmlp_total, ACT_SILU, ACT_NONE);
  }
  free(t_emb);
  return c;
}

// ---- initial cross-embed convolution (k = 3, 7, 15) over cond | x | lowres.
// The cond / low-res planes do not change during a sampling loop: their share of the convolution
// (2/3 of its K for the SR UNets) is computed ONCE per sampling call into `stat` (static_ops)
// and enters the per-step convolution over x's planes through the residual epilogue.  The sum is
// the same convolution, only associated differently.
// A self-conditioned UNet (u->self_cond) reads x AND the previous step's x0 estimate every step: its per-step planes
// are the 2 C of cat(x, self_cond), input channels Cc .. Cc + 2 C - 1 (library order: cond_images | x | self_cond | lowres)
// The per-step share: one kernel (the k = 3 / 7 / 15 CrossEmbedLayer; a plain conv of k = 3 | 5 | 7 whose weights fit LDS), else
// (and under u->init_generic) one launch of the generic conv per kernel size.  Returns the output map and the static buffer.
Builder::InitConv Builder::init_conv(const Model& m) {
  const int dim = m.dim, S = m.S, Ci = m.Ci, Bx = B;
  const kd_unet* io = u;
  const int Cc = cfg.cond_images_channels, Cl = cfg.lowres_cond ? Ci : 0;
  const int NPs = u->self_cond ? 2 * Ci : Ci;
  const int init_ch = Cc + NPs + Cl, Cs = Cc + Cl;
  InitConv r;
  const bool hoist = r.hoist = Cs > 0;
  // init_cross_embed_kernel_sizes: n_ic convs of the sizes ks, widths dim / 2, dim / 4, .., the rest (the library's rule);
  // init_cross_embed=False: ONE conv of size ks[0] to all dim channels, parameters init_conv.{weight,bias}
  const bool init_plain = u->init_plain != 0;
  const int n_ic = init_plain ? 1 : u->n_init_ks;
  int ks[4] = {0, 0, 0, 0}, ds[4] = {0, 0, 0, 0};
  bool ds16 = true;   // every conv's slice is whole 16-channel segments: the convs can leave the GroupNorm partials
  for (int i = 0, left = dim; i < n_ic; ++i) {
    ks[i] = u->init_ks[i];
    ds[i] = i + 1 < n_ic ? dim >> (i + 1) : left;
    left -= ds[i];
    if (ds[i] < 4 || ds[i] % 4) throw std::runtime_error("init conv: every conv's width must be a multiple of 4");
    ds16 = ds16 && ds[i] % 16 == 0;
  }
  const bool ks_default = !init_plain && n_ic == 3 && ks[0] == 3 && ks[1] == 7 && ks[2] == 15;
  auto init_pre = [&](int i) { return init_plain ? std::string("init_conv") : "init_conv.convs." + std::to_string(i); };
  auto check_inputs = [=]() {
    if ((Cc > 0) != (io->in_cond != nullptr)) {
      set_error("cond_images must be given iff the UNet has cond_images_channels > 0");
      return 1;
    }
    if ((Cl > 0) != (io->in_lowres != nullptr)) {
      set_error("lowres_cond_img must be given iff the UNet has lowres_cond");
      return 1;
    }
    return 0;
  };
  if (hoist) {
    const int spad = (Cs + 3) & ~3;
    auto ph = scope(Phase::Static);
    T simg = alloc(B, S, S, spad);
    const Ref sr = at(simg);
    const int HW = S * S;
    emit([=](hipStream_t s) {
      if (check_inputs()) return 1;
      return launch_pack_init(io->in_cond, Cc, nullptr, 0, io->in_lowres, Cl, sr.f(), spad, Bx, HW, s);
    });
    r.stat = alloc(B, S, S, dim);
    int off = 0;
    for (int i = 0; i < n_ic; ++i) {
      std::string pre = init_pre(i);
      ConvOpt o;
      o.dst = &r.stat;
      o.yoff = off;
      o.cin_logical = Cs;
      o.rowrun = true;
      conv(simg, pack_conv_rowrun_sub(pre + ".weight", ds[i], init_ch, 0, Cc, Cc + NPs, Cl, spad, ks[i]),
           P(pre + ".bias", ds[i]), ds[i], ks[i], 1, ks[i] / 2, o);
      off += ds[i];
    }
    free(simg);
  }
  // init_conv_to_final_conv_residual: the init conv's output is the last dim channels of the concat in front of
  // final_res_block (x | the residual; combine_upsample_fmaps: x | the L combiner maps | the residual), so it is written
  // there from the start (a channel slice of that buffer): no copy later
  T& xt = r.x;
  const int before = !m.keep_init ? 0 : m.combine ? m.cat_w - dim : dim;
  xt = m.keep_init ? alloc(B, S, S, before + dim).slice(before, dim) : alloc(B, S, S, dim);
  const bool fused_init = ks_default && !u->init_generic && init_conv_fused_ok(S, ds[0], ds[1], ds[2], NPs);
  const bool fused_plain = init_plain && !u->init_generic && init_plain_ok(S, dim, ks[0], NPs);
  if (fused_plain) {
    const int k = ks[0], np = NPs, Itot = init_ch, c0 = Cc;
    const float* w = raw("init_conv.weight", (int64_t)dim * init_ch * k * k);
    float* wp = cached("init_conv_plain" + std::to_string(np), init_plain_weight_floats(dim, k, np),
                       [&](float* dst) { KD_THROW_IF(launch_init_plain_pack(w, dst, dim, Itot, c0, np, k, 0)); });
    const float* biasp = hoist ? nullptr : P("init_conv.bias", dim);   // (hoisted: the step-invariant share carries the bias)
    const Ref seg = dim % 16 == 0 ? seg_at(add_seg(xt, 0, dim / 16, S * S / 32)) : Ref();
    const Ref yr = at(xt), rr = hoist ? at(r.stat) : Ref();
    const int ldy = xt.LD();
    const int64_t mc = (int64_t)B * S * S * np * k * k * dim;
    emit([=](hipStream_t s) {
      if (check_inputs()) return 1;
      return launch_init_plain(io->in_x, io->in_self_cond, Ci, np, wp, biasp, rr.f(), yr.f(), ldy, seg.d(), Bx, S, dim, k, io->cus, s);
    }, "init conv plain fused k" + std::to_string(k) + " S" + std::to_string(S) + " C" + std::to_string(dim) + (u->self_cond ? " self-cond" : ""), mc);
    count_macs(mc, (int64_t)B * S * S * k * (((k * np + 1) / 2) * 2) * ((dim + 31) / 32 * 32));
  } else if (fused_init) {
    // x's (| self_cond's) share of the three convs in ONE persistent kernel straight from the NCHW planes (kernels_init.hip)
    const float* w3 = raw("init_conv.convs.0.weight", (int64_t)ds[0] * init_ch * 9);
    const float* w7 = raw("init_conv.convs.1.weight", (int64_t)ds[1] * init_ch * 49);
    const float* w15 = raw("init_conv.convs.2.weight", (int64_t)ds[2] * init_ch * 225);
    const int n3 = ds[0], n7 = ds[1], n15 = ds[2], Itot = init_ch, c0 = Cc;
    const int np = NPs;
    float* wp = cached(u->self_cond ? "init_conv_fused6" : "init_conv_fused", init_conv_weight_floats(n3, n7, n15, np), [&](float* dst) {
      KD_THROW_IF(launch_init_conv_pack(w3, w7, w15, dst, n3, n7, n15, Itot, c0, np, 0));
    });
    float* biasp = nullptr;
    if (!hoist) {   // no step-invariant share to carry the biases: one contiguous bias vector
      biasp = cached("init_conv_bias", (size_t)dim, [&](float* dst) {
        int o = 0;
        for (int i = 0; i < 3; ++i) {
          const std::string bn = "init_conv.convs." + std::to_string(i) + ".bias";
          KD_HIP_THROW(hipMemcpyAsync(dst + o, raw(bn, ds[i]), (size_t)ds[i] * 4, hipMemcpyDeviceToDevice, 0));
          o += ds[i];
        }
      });
    }
    const bool sg = dim % 16 == 0 && ds[0] % 16 == 0 && ds[1] % 16 == 0 && ds[2] % 16 == 0;
    const Ref seg = sg ? seg_at(add_seg(xt, 0, dim / 16, S * S / 32)) : Ref();
    const Ref yr = at(xt), rr = hoist ? at(r.stat) : Ref();
    const int ldy = xt.LD();
    const int64_t mc = (int64_t)B * S * S * np * (9 * n3 + 49 * n7 + 225 * n15);
    emit([=](hipStream_t s) {
      if (check_inputs()) return 1;
      return launch_init_conv(io->in_x, io->in_self_cond, Ci, np, wp, biasp, rr.f(), yr.f(), ldy, seg.d(), Bx, S, n3, n7, n15, io->cus, s);
    }, "init conv fused S" + std::to_string(S) + " C" + std::to_string(dim) + (u->self_cond ? " self-cond" : ""), mc);
    // K runs (3 / 7 / 15 kernel rows of np k values, padded to even) x 32-row tiles
    const int r3 = 3 * (((3 * np + 1) / 2) * 2), r7 = 7 * (((7 * np + 1) / 2) * 2), r15 = 15 * (((15 * np + 1) / 2) * 2);
    count_macs(mc, (int64_t)B * S * S * (r3 * ((n3 + 31) / 32 * 32) + r7 * 32 + r15 * 32));
  } else {
    const int np = NPs, ipad = (np + 3) & ~3;
    T img = alloc(B, S, S, ipad);  // x's planes (| self_cond's: zeros when it is not given) + zero channels
    const Ref ir = at(img);
    const int HW = S * S;
    emit([=](hipStream_t s) {
      if (check_inputs()) return 1;
      const float* sc = io->self_cond ? io->in_self_cond : nullptr;
      return launch_pack_init(nullptr, 0, io->in_x, Ci, sc, sc ? Ci : 0, ir.f(), ipad, Bx, HW, s);
    });
    int off = 0;
    for (int i = 0; i < n_ic; ++i) {
      std::string pre = init_pre(i);
      ConvOpt o;
      o.dst = &xt;
      o.yoff = off;
      o.cin_logical = np;
      o.rowrun = true;  // K runs over whole kernel rows (ks*ipad contiguous floats)
      o.want_seg = ds16;  // the slices fill one partial buffer: GroupNorm of init_resnet_block / the tail
      o.seg_c0 = 0;
      o.seg_cn = dim;
      if (hoist) {
        o.res = &r.stat;
        o.res_coff = off;
      }
      conv(img, pack_conv_rowrun_sub(pre + ".weight", ds[i], init_ch, Cc, np, 0, 0, ipad, ks[i]),
           hoist ? nullptr : P(pre + ".bias", ds[i]), ds[i], ks[i], 1, ks[i] / 2, o);
      off += ds[i];
    }
    free(img);
  }
  return r;
}

// ---- the skip stack and the concat offered to the producer in front of a pop
void Builder::SkipStack::push(T& x, const T& y, const T* slot) {
  if (slot && y.off != slot->off) b.free(*slot);   // an offered slot that was not taken is released
  b.step(x, y);
  push(x);
}
// A slice can serve ONE concat (its buffer's first half is written by that concat's producer), so a second entry of x
// is a copy in a slot of its own; it is popped - and dies - before the original, whose partials it shares.
void Builder::SkipStack::push_copy(const T& x, int dim_out) {
  T slot = make_slot(x, dim_out);
  const Ref sr = b.at(x), dr = b.at(slot);
  int lds_ = x.LD(), ldd = slot.LD(), Cc = x.C;
  int64_t rows = x.rows();
  b.emit([=](hipStream_t s) { return launch_copy_scale_rows(sr.f(), lds_, dr.f(), ldd, Cc, 1.0f, rows, s); },
         "skip copy rows" + std::to_string(rows) + " C" + std::to_string(Cc));
  b.share_seg(x, slot);
  hiddens.push_back(slot);   // the stack owns the slot's reference
}
// A producer that is directly followed by a skip concat (a ResnetBlock ending in its 1x1 skip conv, an upsample conv)
// writes its Ca channels straight into the concat buffer offered here, and pop() then only adds the skip half
const T* Builder::SkipStack::offer(int Bc, int Hc, int Wc, int Ca) {
  if (hiddens.empty()) return nullptr;
  const T& skip = hiddens.back();
  if (skip.B != Bc || skip.H != Hc || skip.W != Wc) return nullptr;
  if (skip.ld != 0 && skip.coff != Ca) return nullptr;
  ct_owned = skip.ld == 0;   // else the skip already sits behind Ca channels of its concat buffer
  ct = ct_owned ? b.alloc(Bc, Hc, Wc, Ca + skip.C) : whole(skip);
  have_ct = true;
  ct_ca = Ca;
  return &ct;
}
// x <- cat(x, skip * skip_scale) for the ResnetBlock that follows (dim_out output channels).  Returns the first
// skip channel when that block has to apply the scale itself (skip half left unscaled in memory), else -1.
int Builder::SkipStack::pop(T& x, int dim_out, float skip_scale) {
  if (hiddens.empty()) throw std::runtime_error("plan: skip stack underflow");
  T skip = hiddens.back();
  hiddens.pop_back();
  if (skip.ld != 0) {
    T full = whole(skip);
    const int Ca = skip.coff;
    if (x.off != skip.off) {   // the producer of x did not write in place (or no offer was made)
      if (x.C != Ca) throw std::runtime_error("plan: skip slot behind the wrong number of channels");
      b.concat_head(full, x);
      b.free(x);
    }
    drop_offer();
    x = full;   // the reference the skip stack held is x's now
    // scale 2^-1/2 of the skip half: folded into the consumer where it reads statistics and weights that can
    // carry it (block1's 3x3 conv on the F(4x4,3x3) paths conv3x3_choice names, whose input transform takes the factor
    // into its affine, + the 1x1 skip conv), else applied in place
    b.move_seg(skip, full, Ca, skip_scale, skip_scale);
    if (skip_scale == 1.0f) return -1;   // scale_skip_connection=False: nothing to fold, nothing to scale
    SegPart sp[2];
    int nsp = 0;
    const Conv3x3 algo = b.conv3x3_choice(full, dim_out).algo;
    if ((algo == Conv3x3::Wino4 || algo == Conv3x3::WinoFused) && b.seg_sources(full, sp, nsp)) return Ca;
    b.scale_slice(full, Ca, skip.C, skip_scale);
    auto it = b.seg_of.find(full.at());
    if (it != b.seg_of.end())
      for (auto& p : it->second.parts)
        if (p.c0 >= Ca) p.ab_mul = 1.0f;
    return -1;
  }
  if (have_ct && x.off == ct.off) {        // the producer took the offer: x IS the concat buffer
    b.concat_skip_tail(x, ct_ca, skip, skip_scale);
    b.free(skip);
    have_ct = false;
    return -1;
  }
  drop_offer();                            // offer not taken (the block ended without a skip conv)
  T y = b.concat_skip(x, skip, skip_scale);
  b.free(skip);
  b.step(x, y);
  return -1;
}
void Builder::SkipStack::finish() const {
  if (have_ct) throw std::runtime_error("plan: concat buffer offered but never consumed");
  if (!hiddens.empty()) throw std::runtime_error("plan: skip stack not empty after the up path");
}

// ---- combine_upsample_fmaps: each up level's map after its attention slot lives on to the tail, and whichever launch
// produces the final x writes channels [0, dim) of the combiner's concat in place - the last upsample (memory_efficient),
// else the last level's attention block or the skip conv of its last ResnetBlock
void Builder::Combiner::open(const T& x, const T& init_residual, int dim_out, bool ups, bool attn) {
  if (!m.combine) return;
  cat = m.keep_init ? SkipStack::whole(init_residual) : b.alloc(x.B, m.S, m.S, m.cat_w);
  head = cat.slice(0, m.dim);
  head_here = !ups && dim_out == m.dim && x.H == m.S && x.W == m.S;
  head_resnet = head_here && !attn;
}
// x <- cat(x, fmap_convs.i(nearest(up level i's map)) ..[, init conv residual]): x's channels are there already where its
// producer wrote them in place (else copied, row "combine head"); every combiner launch writes its slice
void Builder::Combiner::close(T& x) {
  const int S = m.S, dim = m.dim;
  const T full = cat;
  if (full.C != m.cat_w || full.H != S || full.W != S || x.H != S || x.W != S || x.C != (x.off == full.off && x.ld == 0 ? m.cat_w : dim))
    throw std::runtime_error("plan: combiner concat of the wrong shape");
  if (x.off != full.off) b.concat_head(full, x, "combine head");
  for (int i = 0; i < m.L; ++i) {
    const T& f = maps[i];
    if (f.H < 1 || S % f.H || f.W != f.H) throw std::runtime_error("plan: up level map is no integer fraction of the image");
    b.combine_fmap(f, i, S / f.H, full, dim * (1 + i));
    b.free(f);
  }
  if (x.off != full.off) b.free(x);
  x = full;   // (keep_init: init_residual's reference is x's now; more than two sources: final_res_block takes its statistics itself)
}

// ---- down path
void Builder::down_path(const Model& m, T& x, const T& c, SkipStack& skips) {
  const int L = m.L;
  const bool gca = cfg.use_gca != 0;
  if (cfg.memory_efficient) step(x, resnet(x, "init_resnet_block", m.dim, nullptr, gca, ResnetOpt()));
  for (int l = 0; l < L; ++l) {
    const std::string pre = "downs." + std::to_string(l);
    const int dim_in = m.dims[l], dim_out = m.dims[l + 1];
    const bool is_last = l == L - 1;
    int cur = dim_in;
    if (cfg.memory_efficient) {
      step(x, downsample(x, pre + ".0", dim_out));
      cur = dim_out;
    }
    step(x, resnet(x, pre + ".1", cur, cfg.layer_cross_attns[l] || u->lin_cross[l] ? &c : nullptr, false, ResnetOpt()));
    // a block ending in gate_add or an attention block is offered the hidden's slot; without use_gca it is a tensor of its own
    for (int n = 0; n < cfg.num_resnet_blocks[l]; ++n) {
      T slot = gca ? skips.make_slot(x, dim_out) : T();
      ResnetOpt ro;
      ro.out_slot = gca ? &slot : nullptr;
      skips.push(x, resnet(x, pre + ".2." + std::to_string(n), cur, nullptr, gca, ro), ro.out_slot);
    }
    if (cfg.layer_attns[l]) {
      T slot = skips.make_slot(x, dim_out);
      skips.push(x, transformer(x, pre + ".3", &c, &slot, false, u->attn_depth[l]), &slot);
    } else if (u->lin_attn[l]) {   // LinearAttentionTransformerBlock: where full attention is off
      T slot = skips.make_slot(x, dim_out);
      skips.push(x, linear_attn_block(x, pre + ".3", &c, &slot), &slot);
    } else if (x.ld != 0) {   // no attention at this level: the library pushes the last block's output a second time
      skips.push_copy(x, dim_out);
    } else {
      skips.push(x);
    }
    if (!cfg.memory_efficient) {
      if (!is_last) {
        step(x, downsample(x, pre + ".4", dim_out));
      } else {  // Parallel(conv3x3, conv1x1), summed
        T y1 = conv(x, P(pre + ".4.fns.1.weight", (int64_t)dim_out * dim_in), P(pre + ".4.fns.1.bias", dim_out),
                    dim_out, 1, 1, 0, ConvOpt());
        ConvOpt o3;
        o3.res = &y1;
        T y = conv(x, pack_conv(pre + ".4.fns.0.weight", dim_out, dim_in, dim_in, 3),
                   P(pre + ".4.fns.0.bias", dim_out), dim_out, 3, 1, 1, o3);
        free(y1);
        step(x, y);
      }
    }
  }
}

void Builder::middle(const Model& m, T& x, const T& c) {
  const int mid = m.dims[m.L];
  step(x, resnet(x, "mid_block1", mid, &c, false, ResnetOpt()));
  if (cfg.attend_at_middle) step(x, transformer(x, "mid_attn", nullptr, nullptr, cfg.mid_attn_plain != 0));
  step(x, resnet(x, "mid_block2", mid, &c, false, ResnetOpt()));
}

// ---- up path.  skip_scale: scale_skip_connection's 2^-0.5; 1 without it, and then no scale pass is emitted
void Builder::up_path(const Model& m, T& x, const T& c, SkipStack& skips, Combiner& comb, const T& init_residual) {
  const int L = m.L;
  for (int i = 0; i < L; ++i) {
    const int l = L - 1 - i;
    const std::string pre = "ups." + std::to_string(i);
    const int dim_in = m.dims[l], dim_out = m.dims[l + 1];
    const bool is_last = i == L - 1;
    const int nb = cfg.num_resnet_blocks[l];
    const bool attn = cfg.layer_attns[l] != 0;
    const bool lin = !attn && u->lin_attn[l] != 0;
    const bool ups = !is_last || cfg.memory_efficient;
    if (is_last) comb.open(x, init_residual, dim_out, ups, attn || lin);
    // final_resnet_block=False: the final conv reads the last producer's output itself - a ResnetBlock (no attention behind it, no
    // upsample, and not an UpsampleCombiner map, whose Block normalises it) or the last upsample: no GroupNorm partials asked for
    const bool last_is_resnet = is_last && !m.final_res && !ups && !attn && !lin && !m.combine;
    ResnetOpt ro;
    ro.skip_scale = m.skip_scale;
    ro.skip_c0 = skips.pop(x, dim_out, m.skip_scale);
    ro.out_seg = !(last_is_resnet && nb == 0);
    ro.ct = nb > 0 ? skips.offer(x.B, x.H, x.W, dim_out) : comb.resnet_target();
    step(x, resnet(x, pre + ".0", dim_out, cfg.layer_cross_attns[l] || u->lin_cross[l] ? &c : nullptr, false, ro));
    if (nb == 0) comb.took_head(x);
    for (int n = 0; n < nb; ++n) {
      ro.skip_c0 = skips.pop(x, dim_out, m.skip_scale);
      const bool next_is_skip = n + 1 < nb || (!attn && !lin && !ups && !is_last);
      ro.out_seg = !(last_is_resnet && n == nb - 1);
      ro.ct = next_is_skip ? skips.offer(x.B, x.H, x.W, dim_out) : n == nb - 1 ? comb.resnet_target() : nullptr;
      step(x, resnet(x, pre + ".1." + std::to_string(n), dim_out, nullptr, cfg.use_gca != 0, ro));
      if (n == nb - 1) comb.took_head(x);
    }
    if (attn) step(x, transformer(x, pre + ".2", &c, comb.attn_target(), false, u->attn_depth[l]));
    if (lin) step(x, linear_attn_block(x, pre + ".2", &c, comb.attn_target()));
    comb.keep(x);
    if (ups) {
      const T* target = nullptr;
      T fin;
      if (!is_last) {
        target = skips.offer(x.B, 2 * x.H, 2 * x.W, dim_in);
      } else if (m.combine) {
        target = &comb.cat;
      } else if (m.keep_init) {
        fin = SkipStack::whole(init_residual);   // the last upsample writes the first half of the concat in front of final_res_block
        target = &fin;
      }
      step(x, upsample(x, pre + ".3", dim_in, target, !(is_last && !m.final_res)));
    }
  }
}

// ---- tail: the combiner / the init conv residual behind x, final_res_block; the conditioning is released
void Builder::tail(const Model& m, T& x, const T& c, Combiner& comb, const T& init_residual) {
  if (m.combine) {
    comb.close(x);
  } else if (m.keep_init) {   // the init conv wrote its half of this concat at the start of the forward
    T full = SkipStack::whole(init_residual);
    if (x.off != full.off) {
      concat_head(full, x);
      free(x);
    }
    move_seg(init_residual, full, init_residual.coff, 1.0f, 1.0f);
    x = full;   // init_residual's reference is x's now
  }
  if (m.final_res) step(x, resnet(x, "final_res_block", m.dim, nullptr, true, ResnetOpt()));
  free(c);
  if (tmlp_total > 0) free(t_ss);
}

void Builder::release(const T& x, const FinalConv& fin, const InitConv& init) {
  free(x);
  if (fin.has_static) free(fin.stat);
  if (init.hoist) free(init.stat);
  free(gn_partial_t);
  free(gn_stats_t);
  if (!refs.empty()) throw std::runtime_error("plan: " + std::to_string(refs.size()) + " tensors leaked");
  u->cond_bytes = cond_end;
}

}  // namespace kd
