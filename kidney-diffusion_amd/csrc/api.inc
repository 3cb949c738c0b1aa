// The extern "C" entry points declared in include/kd_engine.h.
// =============================================================================== C ABI
extern "C" {

const char* kd_last_error(void) { return kd::g_err.c_str(); }
int kd_version(void) { return KD_ENGINE_ABI_VERSION; }

int kd_unet_create(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, kd_unet_t** out) {
  return kd_unet_create_shared(cfg, params, n_params, nullptr, out);
}

int kd_unet_create_shared(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params,
                          const kd_unet_t* share_with, kd_unet_t** out) {
  return kd_unet_create_self_cond(cfg, params, n_params, share_with, 0, out);
}

int kd_unet_create_self_cond(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params,
                             const kd_unet_t* share_with, int self_cond, kd_unet_t** out) {
  kd_unet_ext_t ext;
  memset(&ext, 0, sizeof ext);
  ext.self_cond = self_cond;
  return kd_unet_create_ext(cfg, params, n_params, share_with, &ext, out);
}

int kd_unet_create_ext(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                       const kd_unet_ext_t* ext, kd_unet_t** out) {
  return kd_unet_create_ext2(cfg, params, n_params, share_with, ext, nullptr, out);
}

int kd_unet_create_ext2(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                        const kd_unet_ext_t* ext, const kd_unet_ext2_t* ext2, kd_unet_t** out) {
  return kd_unet_create_ext3(cfg, params, n_params, share_with, ext, ext2, nullptr, out);
}

int kd_unet_create_ext3(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                        const kd_unet_ext_t* ext, const kd_unet_ext2_t* ext2, const kd_unet_ext3_t* ext3, kd_unet_t** out) {
  return kd_unet_create_ext4(cfg, params, n_params, share_with, ext, ext2, ext3, nullptr, out);
}

int kd_unet_create_ext4(const kd_unet_config_t* cfg, const kd_param_t* params, int n_params, const kd_unet_t* share_with,
                        const kd_unet_ext_t* ext, const kd_unet_ext2_t* ext2, const kd_unet_ext3_t* ext3,
                        const kd_unet_ext4_t* ext4, kd_unet_t** out) {
  const int self_cond = ext ? ext->self_cond : 0;
  if (!cfg || !params || !out) {
    set_error("kd_unet_create: null argument");
    return 1;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("kd_unet_create: no HIP device visible — the engine has no CPU path");
    return 1;
  }
  if (share_with && (share_with->self_cond != 0) != (self_cond != 0)) {
    set_error("kd_unet_create: a shared plan must have the same self_cond");
    return 1;
  }
  kd_unet* u = new kd_unet();
  u->cfg = *cfg;
  u->self_cond = self_cond != 0;
  if (ext)
    for (int l = 0; l < KD_MAX_LEVELS; ++l) {
      u->lin_attn[l] = l < cfg->num_levels && ext->use_linear_attn[l] != 0;
      u->lin_cross[l] = l < cfg->num_levels && ext->use_linear_cross_attn[l] != 0;
    }
  if (ext) {
    u->cross_embed_downsample = ext->cross_embed_downsample != 0;
    u->upsample_nearest = ext->upsample_nearest != 0;
  }
  u->combine_upsample_fmaps = ext2 && ext2->combine_upsample_fmaps != 0;
  if (ext3)
    for (int l = 0; l < KD_MAX_LEVELS && l < cfg->num_levels; ++l) {
      if (ext3->layer_attns_depth[l] < 0) {
        set_error("kd_unet_create: layer_attns_depth must not be negative (0 means 1)");
        delete u;
        return 1;
      }
      u->attn_depth[l] = ext3->layer_attns_depth[l] ? ext3->layer_attns_depth[l] : 1;
    }
  if (ext4) {
    const char* bad = nullptr;
    auto odd15 = [](int k) { return k >= 1 && k <= 15 && (k & 1); };
    if (ext4->init_plain) {
      u->init_plain = 1;
      u->n_init_ks = 1;
      u->init_ks[0] = ext4->init_kernel_size ? ext4->init_kernel_size : 7;
      if (!odd15(u->init_ks[0])) bad = "kd_unet_create: init_kernel_size must be odd, 1 .. 15 (0 means 7)";
    } else if (ext4->n_init_kernel_sizes) {
      const int n = ext4->n_init_kernel_sizes;
      if (n < 1 || n > 4) {
        bad = "kd_unet_create: n_init_kernel_sizes must be 1 .. 4 (0 means the sizes 3, 7, 15)";
      } else {
        u->n_init_ks = n;
        for (int i = 0; i < n; ++i) {
          u->init_ks[i] = ext4->init_kernel_sizes[i];
          if (!odd15(u->init_ks[i]) || (i && u->init_ks[i] < u->init_ks[i - 1]))
            bad = "kd_unet_create: init_kernel_sizes must be odd, 1 .. 15, in ascending order";
        }
      }
    }
    u->final_ks = ext4->final_kernel_size ? ext4->final_kernel_size : 3;
    if (u->final_ks != 1 && u->final_ks != 3 && u->final_ks != 5 && u->final_ks != 7)
      bad = "kd_unet_create: final_kernel_size must be 1, 3, 5 or 7 (0 means 3)";
    u->no_final_res = ext4->no_final_resnet_block != 0;
    if (ext4->no_skip_scale) u->skip_scale = 1.0f;
    u->init_generic = ext4->init_generic != 0;
    if (bad) {
      set_error(bad);
      delete u;
      return 1;
    }
  }
  // plans of one UNet (other batch / image size) share its packed weights
  u->wstore = share_with ? share_with->wstore : std::make_shared<WeightStore>();
  u->cus = gemm_bf16x3_device_cus();   // read once: every plan-time question and every launch shape of this plan uses it
  try {
    Builder b(u);
    for (int i = 0; i < n_params; ++i) {
      if (!params[i].name || !params[i].d_data) throw std::runtime_error("parameter table has a null entry");
      b.params[params[i].name] = {params[i].d_data, params[i].numel};
    }
    b.build();
    u->ws_bytes = b.arena.peak;
    if (cfg->cond_on_text && cfg->text_tokens > 0) {  // step-invariant text conditioning, same workspace
      Builder bt(u);
      bt.params = b.params;
      bt.phase = Builder::Phase::Text;
      bt.build_text();
      u->ws_bytes = std::max(u->ws_bytes, bt.arena.peak);
    }
    KD_HIP_THROW(hipMalloc((void**)&u->ws, u->ws_bytes ? u->ws_bytes : 256));
    u->cond_bytes = (u->cond_bytes + 255) & ~size_t(255);
    KD_HIP_THROW(hipMalloc((void**)&u->cond_ws, u->cond_bytes ? u->cond_bytes : 256));
    if (u->cond_rows_ok && !u->cond_segs.empty()) {   // row layout of the cond region, for the batched table build
      uint64_t run = 0;
      for (auto& sg : u->cond_segs) {
        sg.start = (uint32_t)run;
        run += sg.row4;
      }
      if (run < (uint64_t(1) << 31)) {
        u->cond_row_total = (uint32_t)run;
        KD_HIP_THROW(hipMalloc((void**)&u->d_cond_segs, u->cond_segs.size() * sizeof(CondSeg)));
        KD_HIP_THROW(hipMemcpy(u->d_cond_segs, u->cond_segs.data(), u->cond_segs.size() * sizeof(CondSeg), hipMemcpyHostToDevice));
      }
    }
    KD_HIP_THROW(hipDeviceSynchronize());  // weight packing done; caller may free its tensors
  } catch (const std::exception& e) {
    set_error(std::string("kd_unet_create: ") + e.what());
    delete u;
    return 1;
  }
  *out = u;
  return 0;
}

void kd_unet_destroy(kd_unet_t* u) { delete u; }
int64_t kd_unet_hbm_bytes(const kd_unet_t* u) {
  return u ? (int64_t)(u->ws_bytes + u->cond_bytes + u->smp.cond.bytes + u->wstore->pool.total) : 0;
}
int64_t kd_unet_weight_bytes(const kd_unet_t* u) { return u ? (int64_t)u->wstore->pool.total : 0; }
int64_t kd_unet_macs(const kd_unet_t* u) { return u ? u->macs : 0; }
int64_t kd_unet_mfma_macs(const kd_unet_t* u) { return u ? u->mfma_macs : 0; }
int64_t kd_unet_mfma_bf16_macs(const kd_unet_t* u) { return u ? u->mfma_bf16_macs : 0; }
int kd_unet_num_launches(const kd_unet_t* u) { return u ? (int)u->ops.size() : 0; }
float kd_unet_cond_table_build_ms(kd_unet_t* u, int* rows, int* runs) {
  if (rows) *rows = u ? u->smp.cond.build_rows : 0;
  if (runs) *runs = u ? u->smp.cond.build_runs : 0;
  if (!u) return -1.f;
  CondTable& c = u->smp.cond;
  if (c.ev_pending) {   // the events of the last build: read here, never on the sampling path
    c.ev_pending = false;
    float ms = -1.f;
    if (hipEventSynchronize(c.ev1) == hipSuccess && hipEventElapsedTime(&ms, c.ev0, c.ev1) == hipSuccess)
      c.build_ms = ms;
    else
      (void)hipGetLastError();
  }
  return c.build_ms;
}
int64_t kd_unet_cond_table_refused_bytes(const kd_unet_t* u) { return u ? u->smp.cond.refused_bytes : 0; }
int kd_unet_num_cond_launches(const kd_unet_t* u) {
  int n = 0;
  if (u)
    for (char c : u->op_is_cond) n += c != 0;
  return n;
}

int kd_unet_forward(kd_unet_t* u, const float* d_x, const float* d_lowres, const float* d_cond_images,
                    const float* d_log_snr, const float* d_lowres_log_snr, const float* d_text_tokens,
                    const float* d_text_hiddens, float* d_out, void* stream) {
  return kd_unet_forward_self_cond(u, d_x, nullptr, d_lowres, d_cond_images, d_log_snr, d_lowres_log_snr, d_text_tokens,
                                   d_text_hiddens, d_out, stream);
}

int kd_unet_forward_self_cond(kd_unet_t* u, const float* d_x, const float* d_self_cond, const float* d_lowres,
                              const float* d_cond_images, const float* d_log_snr, const float* d_lowres_log_snr,
                              const float* d_text_tokens, const float* d_text_hiddens, float* d_out, void* stream) {
  if (!u || !d_x || !d_out || !d_log_snr) {
    set_error("kd_unet_forward: null argument");
    return 1;
  }
  kd_sample_args_t a{};
  a.d_lowres = d_lowres;
  a.d_cond_images = d_cond_images;
  a.d_lowres_log_snr = d_lowres_log_snr;
  a.d_text_tokens = d_text_tokens;
  a.d_text_hiddens = d_text_hiddens;
  set_inputs(u, d_x, &a, d_log_snr, d_self_cond, d_out);
  if (run_static(u, (hipStream_t)stream)) return 1;
  return run_forward(u, (hipStream_t)stream);
}

int kd_unet_text_cond(kd_unet_t* u, const float* d_text_embeds, const float* d_text_mask, int L, int drop,
                      float* d_text_tokens, float* d_text_hiddens, void* stream) {
  if (!u || !d_text_tokens || !d_text_hiddens) {
    set_error("kd_unet_text_cond: null argument");
    return 1;
  }
  KD_REQUIRE(!u->text_ops.empty(), "this UNet was planned without text conditioning");
  u->in_text_embeds = d_text_embeds;
  u->in_text_mask = d_text_mask;
  u->in_text_len = L;
  u->in_text_drop = drop;
  u->out_text_tokens = d_text_tokens;
  u->out_text_hiddens = d_text_hiddens;
  for (auto& op : u->text_ops)
    if (op((hipStream_t)stream)) return 1;
  return 0;
}

// Per-op device times of one forward (inputs as last set by kd_unet_forward / the sampler):
// CSV "index,label,macs,avg_us" into buf.  Diagnostic; synchronises.
int kd_unet_profile(kd_unet_t* u, int iters, char* buf, size_t buflen, void* stream) {
  if (!u || !buf || buflen == 0 || iters < 1) {
    set_error("kd_unet_profile: bad argument");
    return 1;
  }
  KD_REQUIRE(u->in_x && u->out, "kd_unet_profile: run kd_unet_forward once first");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = u->ops.size();
  struct Events {  // destroyed on every return path
    std::vector<hipEvent_t> ev;
    ~Events() {
      for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
    }
  } evs;
  evs.ev.assign(n + 1, nullptr);
  auto& ev = evs.ev;
  for (auto& e : ev) KD_HIP_CHECK(hipEventCreate(&e));
  std::vector<double> acc(n, 0.0);
  for (int it = 0; it < iters; ++it) {
    KD_HIP_CHECK(hipEventRecord(ev[0], s));
    for (size_t i = 0; i < n; ++i) {
      if (u->ops[i](s)) return 1;
      KD_HIP_CHECK(hipEventRecord(ev[i + 1], s));
    }
    KD_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
      float ms = 0.f;
      KD_HIP_CHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      acc[i] += ms;
    }
  }
  std::string out = "index,label,macs,avg_us,mfma_macs\n";
  for (size_t i = 0; i < n; ++i)
    out += std::to_string(i) + "," + u->op_label[i] + "," + std::to_string(u->op_macs[i]) + "," +
           std::to_string(acc[i] * 1e3 / iters) + "," + std::to_string(u->op_mfma[i]) + "\n";
  KD_REQUIRE(out.size() + 1 <= buflen, "kd_unet_profile: buffer too small");
  memcpy(buf, out.c_str(), out.size() + 1);
  return 0;
}

// Test infrastructure (tests/test_poisoned_scratch_gpu.py): every 32-bit word of what is scratch by contract at the start
// of a forward or of a sampling call becomes `word`.  None of it was initialised when it was allocated, so a plan whose
// results change under this call reads memory that no op of the same call has written.
//   filled - every op that reads it has a writer earlier in the same call:
//     ws        the arena: every tensor is written by the op that produces it; what static_ops leave there lives from
//               them to the last step of the same call, never across calls (so: not between kd_unet_forward's static part and
//               its steps - there is no entry that separates them - and not between the steps of one sampling call)
//     cond_ws   written by the conditioning ops of every forward, or restored whole from the table by the step's gather
//     x3_ws     the k-cut slabs of a bf16x3 GEMM: its parts store them, the summing launch behind it reads them
//     sampler   pred, pred_null, x0, thresh, time, xhat, d, net_in: written by the kernels of an iteration before they
//               are read (kd_sample_last reports the last call's: read it before poisoning); self_cond: zeroed at step 0
//               of a call (a caller that continues with k_begin > 0 seeds it after this call, kd_sample_set_self_cond);
//               hist (few-step solvers): the first step a call walks is first order and does not read it, and its
//               last resample slot writes it (a caller that continues with k_begin > 0 poisons before the first call);
//               hist2 (third-order solvers): with hist a ring - the first two steps a call walks read neither slot
//               through a non-zero coefficient, and each writes the slot the step behind it reads;
//               qws: the quantile's QState and histograms are integers - q_init_kernel sets every one of them at the
//               start of each launch_quantile_abs, before q_hist / q_scan / q_next / q_final index or count with them
//   left alone - state that outlives a call:
//     the packed weights and every table cached with them (the fused Winograd kernel's item lists are indices);
//     iter and the seed block (set by launch_iter_set / launch_seed_set per call, read as a table index and Philox keys);
//     ddpm_tab / edm_tab (keyed on their content: an unchanged schedule uploads nothing); the conditioning table
//     smp.cond.tab (rows built once per schedule); d_cond_segs (row layout, read as offsets); captured graphs; the text
//     conditioning's outputs, which live in the caller's buffers.
// Apart from those integers of qws, no word of the filled buffers is ever used as an index, a count or an address.
int kd_unet_poison_scratch(kd_unet_t* u, uint32_t word, int64_t* bytes_filled, void* stream) {
  if (!u) {
    set_error("kd_unet_poison_scratch: null argument");
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  const Sampler& m = u->smp;
  const size_t img = image_bytes(u), per_b = (size_t)u->cfg.batch * sizeof(float);
  const std::pair<void*, size_t> bufs[] = {
      {u->ws, u->ws_bytes},   {u->cond_ws, u->cond_bytes}, {u->x3_ws, gemm_bf16x3_workspace_bytes()},
      {m.pred, img},          {m.pred_null, img},          {m.x0, img},
      {m.thresh, per_b},      {m.time, per_b},             {m.xhat, img},
      {m.d, img},             {m.net_in, img},             {m.self_cond, img},
      {m.hist, img},          {m.hist2, img},
      {m.qws, quantile_ws_bytes(u->cfg.batch)}};
  int64_t total = 0;
  for (const auto& b : bufs) {
    if (!b.first || !b.second) continue;   // (the sampler's come with the first sampling call, x3_ws with the first bf16x3 layer)
    KD_REQUIRE(b.second % 4 == 0, "kd_unet_poison_scratch: a scratch buffer is not a whole number of words");
    KD_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)b.first, (int)word, b.second / 4, s));
    total += (int64_t)b.second;
  }
  if (bytes_filled) *bytes_filled = total;
  return 0;
}

int kd_sample_steps(kd_unet_t* u, const kd_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                    int k_begin, int k_end, void* stream) {
  return sample_steps(u, sched, args, d_img, k_begin, k_end, (hipStream_t)stream);
}

// Builds (force != 0: rebuilds) the conditioning-table rows of schedule steps [k_begin, k_end) without sampling: a
// caller that wants the first sample() call of a schedule to start at full speed, and bench.py's cond_table_build_ms.
// Returns 0 also when the plan runs without a table (text conditioning, per-sample low-res levels, table switched
// off or over its size cap): *built = 0 then.
int kd_sample_build_cond_table(kd_unet_t* u, const kd_schedule_t* sched, const kd_sample_args_t* args, int k_begin, int k_end,
                               int force, int* built, void* stream) {
  if (built) *built = 0;
  hipStream_t s = (hipStream_t)stream;
  SamplerCtx ctx;
  if (begin_call(u, sched, args, nullptr, false, ctx, s)) return 1;
  if (ddpm_prepare(u, sched, ctx, s)) return 1;
  KD_REQUIRE(0 <= k_begin && k_begin <= k_end && k_end <= ctx.T, "step range out of bounds");
  u->smp.cond.build_rows = 0;
  if (sampler_cond_table(u, u->smp.ddpm_tab.host, args, ctx, k_begin, k_end, s, force != 0)) return 1;
  if (built) *built = ctx.cond_tab ? u->smp.cond.build_rows : 0;
  return 0;
}

int kd_edm_sample_steps(kd_unet_t* u, const kd_edm_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                        int k_begin, int k_end, void* stream) {
  return edm_sample_steps(u, sched, args, d_img, k_begin, k_end, (hipStream_t)stream);
}

int kd_edm_sample_loop(kd_unet_t* u, const kd_edm_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                       void* stream) {
  if (!sched) {
    set_error("kd_edm_sample_loop: null schedule");
    return 1;
  }
  if (edm_sample_steps(u, sched, args, d_img, 0, sched->N, (hipStream_t)stream)) return 1;
  return kd_sample_finalize(u, args, d_img, stream);
}

int kd_solver_sample_steps(kd_unet_t* u, const kd_solver_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                           int k_begin, int k_end, void* stream) {
  return solver_sample_steps(u, sched, nullptr, args, d_img, k_begin, k_end, (hipStream_t)stream);
}

int kd_solver_sample_loop(kd_unet_t* u, const kd_solver_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                          void* stream) {
  if (!sched) {
    set_error("kd_solver_sample_loop: null schedule");
    return 1;
  }
  if (solver_sample_steps(u, sched, nullptr, args, d_img, 0, sched->T, (hipStream_t)stream)) return 1;
  return kd_sample_finalize(u, args, d_img, stream);
}

// kd_solver3_schedule_t: kd_solver_schedule_t's fields, then coef_prev2
static kd_solver_schedule_t solver3_head(const kd_solver3_schedule_t* q) {
  kd_solver_schedule_t sc{};
  sc.T = q->T;
  sc.log_snr = q->log_snr;
  sc.alpha = q->alpha;
  sc.sigma = q->sigma;
  sc.rn_a = q->rn_a;
  sc.rn_b = q->rn_b;
  sc.coef_x = q->coef_x;
  sc.coef_x0 = q->coef_x0;
  sc.coef_prev = q->coef_prev;
  sc.coef_noise = q->coef_noise;
  return sc;
}

int kd_solver3_sample_steps(kd_unet_t* u, const kd_solver3_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                            int k_begin, int k_end, void* stream) {
  if (!sched) {
    set_error("kd_solver3_sample_steps: null schedule");
    return 1;
  }
  const kd_solver_schedule_t sc = solver3_head(sched);
  return solver_sample_steps(u, &sc, sched->coef_prev2, args, d_img, k_begin, k_end, (hipStream_t)stream);
}

int kd_solver3_sample_loop(kd_unet_t* u, const kd_solver3_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                           void* stream) {
  if (!sched) {
    set_error("kd_solver3_sample_loop: null schedule");
    return 1;
  }
  if (kd_solver3_sample_steps(u, sched, args, d_img, 0, sched->T, stream)) return 1;
  return kd_sample_finalize(u, args, d_img, stream);
}

int kd_sample_loop(kd_unet_t* u, const kd_schedule_t* sched, const kd_sample_args_t* args, float* d_img,
                   void* stream) {
  if (!sched) {
    set_error("kd_sample_loop: null schedule");
    return 1;
  }
  if (sample_steps(u, sched, args, d_img, 0, sched->T, (hipStream_t)stream)) return 1;
  return kd_sample_finalize(u, args, d_img, stream);
}

// What the last executed denoising iteration left in the sampler's scratch: which = 0 the UNet output (eps-hat /
// v-hat, after guidance) [B,C,S,S]; 1 the x0 estimate BEFORE the threshold clamp [B,C,S,S]; 2 the per-sample
// dynamic thresholds max(1, quantile) [B].  Stream-ordered device-to-device copy (parity checks: bench.py, tests).
int kd_sample_last(kd_unet_t* u, int which, float* d_out, void* stream) {
  if (!u || !d_out) {
    set_error("kd_sample_last: null argument");
    return 1;
  }
  const Sampler& m = u->smp;
  KD_REQUIRE(m.pred, "kd_sample_last: no sampling step has run on this plan");
  KD_REQUIRE(which >= 0 && which <= 5,
             "kd_sample_last: which must be 0 (pred), 1 (x0), 2 (thresholds), 3 / 4 (EDM x_hat / d), 5 (self-cond planes)");
  KD_REQUIRE(which <= 2 || which == 5 || m.xhat, "kd_sample_last: no EDM step has run on this plan");
  KD_REQUIRE(which != 5 || m.self_cond, "kd_sample_last: which = 5 needs a plan with self_cond");
  const int B = u->cfg.batch, S = u->cfg.image_size;
  const float* src = which == 0 ? m.pred : which == 1 ? m.x0 : which == 2 ? m.thresh : which == 3 ? m.xhat
                   : which == 4 ? m.d : m.self_cond;
  const size_t bytes = (which == 2 ? (size_t)B : (size_t)B * u->cfg.channels * S * S) * sizeof(float);
  KD_HIP_CHECK(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// Seeds the self-conditioning estimate a self_cond plan carries (d_x_start [B,C,S,S], NULL = zeros), so that
// kd_sample_steps / kd_edm_sample_steps with k_begin > 0 continue from a chosen state.  Stream-ordered.
int kd_sample_set_self_cond(kd_unet_t* u, const float* d_x_start, void* stream) {
  if (!u) {
    set_error("kd_sample_set_self_cond: null argument");
    return 1;
  }
  KD_REQUIRE(u->self_cond, "kd_sample_set_self_cond: the plan was created without self_cond");
  if (sampler_scratch(u)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (d_x_start)
    KD_HIP_CHECK(hipMemcpyAsync(u->smp.self_cond, d_x_start, image_bytes(u), hipMemcpyDeviceToDevice, s));
  else
    KD_HIP_CHECK(hipMemsetAsync(u->smp.self_cond, 0, image_bytes(u), s));
  return 0;
}

int kd_sample_finalize(kd_unet_t* u, const kd_sample_args_t* args, float* d_img, void* stream) {
  if (!u || !args || !d_img) {
    set_error("kd_sample_finalize: null argument");
    return 1;
  }
  return launch_finalize(d_img, args->d_inpaint_images, args->d_inpaint_masks, u->cfg.batch, u->cfg.channels,
                         (int64_t)u->cfg.image_size * u->cfg.image_size, (hipStream_t)stream);
}

// ---- single-kernel entry points (tests).  Every shape is checked before the first allocation; the temporaries live in
// one holder (kd::DevBufs) that frees them on every path, after entry_finish has waited for the launches that use them.
namespace {
using EntryBufs = kd::DevBufs;
int entry_finish(int rc, hipStream_t s) {
  hipError_t e = hipStreamSynchronize(s);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
}
// the slab workspace of a test entry's bf16x3 GEMMs, every byte 0xFF (NaN as float): the launch must not depend on what
// the slabs held (kd_unet_poison_scratch holds the plans to the same)
int entry_x3_ws(EntryBufs& bufs, void** ws, hipStream_t s) {
  if (bufs.get(ws, gemm_bf16x3_workspace_bytes())) return 1;
  KD_HIP_CHECK(hipMemsetAsync(*ws, 0xFF, gemm_bf16x3_workspace_bytes(), s));
  return 0;
}
// the launch shape of a bf16x3 GEMM of a test entry point: one per call, for the device that is current
X3Shape entry_x3_shape(int G, int64_t M, int N, int K) { return gemm_bf16x3_shape(G, (int)M, N, K, gemm_bf16x3_device_cus()); }
// a conv of a test entry point: its launch shape from the pointers it holds, one per call, for the device that is current
int entry_conv(const ConvParams& p, hipStream_t s) {
  return launch_conv_igemm(p, conv_shape(p, conv_ptrs_of(p), gemm_bf16x3_device_cus()), s);
}
}  // namespace

// act bit 8 (0x100) selects the row-run K layout used for the small-Cin init convs
int kd_conv2d_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, float* d_y, int B, int Hi, int Wi,
                   int Cin, int Cout, int KH, int KW, int stride, int pad, int act, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool rowrun = (act & 0x100) != 0;
  const bool pixshuf = (act & 0x200) != 0;   // 1x1 conv + PixelShuffle(2): d_y is [B, 2 Ho, 2 Wo, Cout / 4]
  act &= 0xff;
  KD_REQUIRE(!pixshuf || (KH == 1 && KW == 1 && Cout % 4 == 0 && !rowrun), "pixel-shuffle test path: 1x1 conv, Cout % 4 == 0");
  EntryBufs bufs;
  float *wp = nullptr, *part = nullptr, *bp = nullptr;
  if (bufs.get(&wp, (size_t)Cout * Cin * KH * KW * sizeof(float))) return 1;
  if (pixshuf && bufs.get(&bp, (size_t)Cout * sizeof(float))) return 1;
  int rc = pixshuf  ? launch_pack_shuffle(d_w_oihw, d_bias, wp, bp, Cout / 4, Cin, s)
           : rowrun ? launch_pack_oihw_rowrun(d_w_oihw, wp, Cout, Cin, Cin, KH, KW, s)
                    : launch_pack_oihw(d_w_oihw, wp, Cout, Cin, Cin, KH, KW, s);
  if (!rc) {
    ConvParams p{};
    p.x = d_x; p.w = wp; p.bias = d_bias; p.y = d_y;
    p.B = B; p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.ldx = Cin;
    p.Ho = (Hi + 2 * pad - KH) / stride + 1;
    p.Wo = (Wi + 2 * pad - KW) / stride + 1;
    p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
    if (rowrun) {
      p.KW = 1;
      p.Cin = KW * Cin;
      p.rr_cin = Cin;
    }
    p.act = act; p.out_mode = OUT_NHWC; p.ldy = Cout;
    if (pixshuf) {
      p.bias = bp;
      p.out_mode = OUT_PIXSHUF;
      p.ldy = Cout / 4;
    }
    ConvPtrs ptrs = conv_ptrs_of(p);   // small-M shapes take the split-K path, as in the plan: a scratch (hipMalloc) is on offer
    ptrs.has |= CONV_PARTIAL;
    const ConvShape sh = conv_shape(p, ptrs, gemm_bf16x3_device_cus());
    if (sh.ksplit > 1) rc = bufs.get(&part, (size_t)sh.ksplit * B * p.Ho * p.Wo * Cout * sizeof(float));
    p.partial = part;
    if (!rc) rc = launch_conv_igemm(p, sh, s);
  }
  return entry_finish(rc, s);
}

// nn.Upsample(2, nearest) -> Conv2d(Cin, Cout, 3, padding 1) through the plan's launches (kernels_resample.hip): the pack of
// the sixteen summed tap matrices, then the four phase GEMMs
int kd_upsample_nearest_conv3x3_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, float* d_y, int ldy, int yoff,
                                     int B, int H, int W, int Cin, int Cout, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ldy == 0) ldy = Cout;
  if (const char* why = upsample_nearest_refusal(Cin, ldy, yoff, B, H, W, Cin, Cout)) {
    set_error(why);
    return 1;
  }
  EntryBufs bufs;
  float* wp = nullptr;
  if (bufs.get(&wp, upsample_nearest_weight_floats(Cin, Cout) * sizeof(float))) return 1;
  int rc = launch_upsample_nearest_pack(d_w_oihw, wp, Cout, Cin, s);
  if (!rc) rc = launch_upsample_nearest_conv3x3(d_x, Cin, wp, d_bias, d_y, ldy, yoff, B, H, W, Cin, Cout, s);
  return entry_finish(rc, s);
}

// nn.Upsample(s, nearest) -> [SiLU(A x + B)] -> Conv2d(Cin, Cout, 3, padding 1) through the plan's launches
// (kernels_upcombine.hip): the pack of the 25 summed tap matrices, then the class GEMMs with the replicating stores
int kd_upsample_nearest_gn_conv3x3_nhwc(const float* d_x, int ldx, const float* d_ab, const float* d_w_oihw, const float* d_bias,
                                        float* d_y, int ldy, int yoff, int B, int H, int W, int Cin, int Cout, int scale,
                                        void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ldx == 0) ldx = Cin;
  if (ldy == 0) ldy = Cout;
  KD_REQUIRE(d_x && d_w_oihw && d_y, "kd_upsample_nearest_gn_conv3x3_nhwc: null argument");
  if (const char* why = upsample_scale_refusal(ldx, ldy, yoff, B, H, W, Cin, Cout, scale)) {
    set_error(why);
    return 1;
  }
  EntryBufs bufs;
  float* wp = nullptr;
  if (bufs.get(&wp, upsample_scale_weight_floats(Cin, Cout) * sizeof(float))) return 1;
  int rc = launch_upsample_scale_pack(d_w_oihw, wp, Cout, Cin, s);
  if (!rc) rc = launch_upsample_scale_conv3x3(d_x, ldx, d_ab, wp, d_bias, d_y, ldy, yoff, B, H, W, Cin, Cout, scale, s);
  return entry_finish(rc, s);
}

// 3x3 / stride 1 / pad 1 conv through the Winograd F(2x2,3x3) path of the plan: weight transform,
// input transform, 16 batched GEMMs on the fast implicit-GEMM kernel, output transform (+ bias).
int kd_conv3x3_winograd_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, float* d_y, int B, int H,
                             int W, int Cin, int Cout, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(H % 2 == 0 && W % 2 == 0, "Winograd path needs even H and W");
  const int64_t Mt = (int64_t)B * (H / 2) * (W / 2);
  KD_REQUIRE(Mt % 256 == 0 && Cin % 32 == 0 && Cout > 32 && Cout % 4 == 0,
             "Winograd path needs B*H*W/4 % 256 == 0, Cin % 32 == 0, Cout > 32");
  EntryBufs bufs;
  float *U = nullptr, *V = nullptr, *D = nullptr;
  if (bufs.get(&U, (size_t)16 * Cout * Cin * sizeof(float))) return 1;
  if (bufs.get(&V, (size_t)16 * Mt * Cin * sizeof(float))) return 1;
  if (bufs.get(&D, (size_t)16 * Mt * Cout * sizeof(float))) return 1;
  int rc = launch_wino_pack(d_w_oihw, U, Cout, Cin, s);
  if (!rc) rc = launch_wino_in(d_x, Cin, nullptr, nullptr, nullptr, nullptr, 0, V, B, H, W, Cin, 1, 0, Mt, s);
  if (!rc) {
    ConvParams p{};
    p.x = V; p.w = U; p.y = D;
    p.B = 1; p.Hi = 1; p.Wi = (int)(16 * Mt); p.Cin = Cin; p.ldx = Cin;
    p.Ho = 1; p.Wo = (int)(16 * Mt); p.Cout = Cout;
    p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0;
    p.out_mode = OUT_NHWC; p.ldy = Cout;
    p.wz_rows = (int)Mt; p.wz_count = 16;
    rc = entry_conv(p, s);
  }
  if (!rc) rc = launch_wino_out(D, d_bias, nullptr, 0, d_y, B, H, W, Cout, 0, Mt, s);
  return entry_finish(rc, s);
}

int kd_conv3x3_winograd4_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, const float* d_res, float* d_y,
                              int B, int H, int W, int Cin, int Cout, int G, float eps, float* d_out_stats, int gemm_bf16x3,
                              void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(H % 4 == 0 && W % 4 == 0, "Winograd F(4x4,3x3) path needs H % 4 == 0 and W % 4 == 0");
  const int64_t Mt = (int64_t)B * (H / 4) * (W / 4);
  KD_REQUIRE(!gemm_bf16x3 || gemm_bf16x3_ok(36, Mt, Cout, Cin),
             "bf16x3 position GEMMs need B*H*W/16 % 256 == 0, Cout % 128 == 0, Cin % 32 == 0");
  KD_REQUIRE(Mt % 128 == 0 && Cin % 32 == 0 && Cout % 64 == 0,
             "Winograd F(4x4,3x3) path needs B*H*W/16 % 128 == 0, Cin % 32 == 0, Cout % 64 == 0");
  KD_REQUIRE(!d_out_stats || (G > 0 && Cout % G == 0 && (Cout / G) % 16 == 0), "output statistics need (Cout / G) % 16 == 0");
  EntryBufs bufs;
  float *U = nullptr, *V = nullptr, *D = nullptr;
  double* seg = nullptr;
  void *U3 = nullptr, *x3ws = nullptr;
  const int nchunk = (H / 4) * (W / 4);
  if (bufs.get(&U, (size_t)36 * Cout * Cin * sizeof(float))) return 1;
  if (bufs.get(&V, (size_t)36 * Mt * Cin * (gemm_bf16x3 == 1 ? 6 : sizeof(float)))) return 1;
  if (bufs.get(&D, (size_t)36 * Mt * Cout * sizeof(float))) return 1;
  if (gemm_bf16x3 && bufs.get(&U3, (size_t)36 * Cout * Cin * 6)) return 1;
  if (gemm_bf16x3 && entry_x3_ws(bufs, &x3ws, s)) return 1;
  if (d_out_stats && bufs.get(&seg, (size_t)B * (Cout / 16) * nchunk * 2 * sizeof(double))) return 1;
  int rc = launch_wino4_pack(d_w_oihw, U, Cout, Cin, s);
  if (!rc && gemm_bf16x3) {
    rc = launch_split3(U, U3, 36, Cout, Cin, s);
    if (!rc && gemm_bf16x3 == 1) rc = launch_wino4_in3(d_x, Cin, nullptr, nullptr, nullptr, nullptr, 0, V, B, H, W, Cin, 1, s);
    if (!rc && gemm_bf16x3 != 1) rc = launch_wino4_in(d_x, Cin, nullptr, nullptr, nullptr, nullptr, 0, V, B, H, W, Cin, 1, s);
    if (!rc) rc = launch_gemm_bf16x3(V, U3, D, 36, (int)Mt, Cout, Cin, entry_x3_shape(36, Mt, Cout, Cin), x3ws, s, gemm_bf16x3 != 1);
  }
  if (!rc && !gemm_bf16x3) rc = launch_wino4_in(d_x, Cin, nullptr, nullptr, nullptr, nullptr, 0, V, B, H, W, Cin, 1, s);
  if (!rc && !gemm_bf16x3) {
    ConvParams p{};
    p.x = V; p.w = U; p.y = D;
    p.B = 1; p.Hi = 1; p.Wi = (int)(36 * Mt); p.Cin = Cin; p.ldx = Cin;
    p.Ho = 1; p.Wo = (int)(36 * Mt); p.Cout = Cout;
    p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0;
    p.out_mode = OUT_NHWC; p.ldy = Cout;
    p.wz_rows = (int)Mt; p.wz_count = 36;
    rc = entry_conv(p, s);
  }
  if (!rc) rc = launch_wino4_out(D, d_bias, d_res, Cout, d_y, Cout, seg, B, H, W, Cout, s);
  if (!rc && seg)   // the 16-channel segments of a group are adjacent: [B][G][(Cout / G / 16) nchunk][2]
    rc = launch_gn_finalize(seg, d_out_stats, (Cout / G / 16) * nchunk, B, G, (double)H * W * (Cout / G), eps, s);
  return entry_finish(rc, s);
}

int kd_gemm_bf16x3(const float* d_a, const float* d_b, float* d_c, int G, int M, int N, int K, int a_planes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(gemm_bf16x3_ok(G, M, N, K), "kd_gemm_bf16x3 needs M % 256 == 0, N % 128 == 0, K % 32 == 0, operand planes < 4 GB");
  EntryBufs bufs;
  void *A3 = nullptr, *B3 = nullptr, *ws = nullptr;
  if (bufs.get(&B3, (size_t)G * N * K * 6)) return 1;
  if (a_planes && bufs.get(&A3, (size_t)G * M * K * 6)) return 1;   // (a_planes == 0: the loader waves split A)
  if (entry_x3_ws(bufs, &ws, s)) return 1;   // slabs of the left-over tiles' k-parts
  int rc = a_planes ? launch_split3(d_a, A3, G, M, K, s) : 0;
  if (!rc) rc = launch_split3(d_b, B3, G, N, K, s);
  if (!rc) rc = launch_gemm_bf16x3(a_planes ? A3 : (const void*)d_a, B3, d_c, G, M, N, K, entry_x3_shape(G, M, N, K), ws, s, !a_planes);
  return entry_finish(rc, s);
}

int kd_downsample_bf16x3(const float* d_x, int ldx, const float* d_w, const float* d_bias, float* d_y, int B, int H, int W, int C,
                         int O, double* d_seg, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int K = 4 * C;
  const int64_t M = (int64_t)B * (H / 2) * (W / 2);
  X3Epi e;
  e.bias = d_bias;
  e.lda = ldx > 0 ? ldx : C;
  e.ldy = O;
  e.a_tap_c = C;
  e.a_wi = W;
  e.a_hi = H;
  e.hw = (H / 2) * (W / 2);
  e.seg = d_seg;
  e.seg_nseg = d_seg ? O / 16 : 0;
  const X3Shape sh = entry_x3_shape(1, M, O, K);
  KD_REQUIRE(H > 0 && W > 0 && !(H & 1) && !(W & 1) && M < 0x7fffffff && gemm_bf16x3_epi_ok(M, O, K, e, sh),
             "kd_downsample_bf16x3 needs even map sides, C % 16 == 0, B (H/2) (W/2) % 256 == 0, O % 128 == 0");
  // torch weight [O][4 C] with k = c 4 + tap  ->  [tap][O][C] (launch_pack_unshuffle)  ->  [O][tap C + c]  ->  planes
  EntryBufs bufs;
  float *wt = nullptr, *wk = nullptr;
  void *W3 = nullptr, *ws = nullptr;
  if (bufs.get(&wt, (size_t)O * K * 4) || bufs.get(&wk, (size_t)O * K * 4) || bufs.get(&W3, (size_t)O * K * 6) ||
      entry_x3_ws(bufs, &ws, s))
    return 1;
  int rc = launch_pack_unshuffle(d_w, wt, O, C, s);
  for (int t = 0; t < 4 && !rc; ++t) rc = launch_copy_scale_rows(wt + (size_t)t * O * C, C, wk + (size_t)t * C, K, C, 1.0f, O, s);
  if (!rc) rc = launch_split3(wk, W3, 1, O, K, s);
  if (!rc) rc = launch_gemm_bf16x3(d_x, W3, d_y, 1, (int)M, O, K, sh, ws, s, true, true, &e);
  return entry_finish(rc, s);
}

int kd_linear_bf16x3_seg_rows(int M, int N, int K) { return gemm_bf16x3_ok(1, M, N, K) ? entry_x3_shape(1, M, N, K).seg_rows() : 0; }

int kd_linear_bf16x3(const float* d_x, int ldx, const float* d_w, const float* d_bias, const float* d_res, int ldres,
                     const float* d_gate_src, int ldgs, const float* d_gate, int hw, float* d_y, int ldy, int M, int N, int K,
                     int act, int pixshuf_wo, double* d_seg, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  X3Epi e;
  e.seg = d_seg;
  e.seg_nseg = d_seg ? (pixshuf_wo ? N / 4 : N) / 16 : 0;
  e.act = act;
  e.pixshuf_wo = pixshuf_wo;
  e.bias = d_bias;
  e.res = d_res;
  e.ldres = ldres;
  e.gate_src = d_gate_src;
  e.ldgs = ldgs;
  e.gate = d_gate;
  e.hw = hw;
  e.ldy = ldy > 0 ? ldy : (pixshuf_wo ? N / 4 : N);
  e.lda = ldx > 0 ? ldx : K;
  const X3Shape sh = entry_x3_shape(1, M, N, K);
  KD_REQUIRE(gemm_bf16x3_epi_ok(M, N, K, e, sh), "kd_linear_bf16x3 needs M % 256 == 0, N % 128 == 0, K % 32 == 0, row strides >= the "
                                             "rows, hw % 256 == 0 under a gate");
  EntryBufs bufs;
  void *W3 = nullptr, *ws = nullptr;
  if (bufs.get(&W3, (size_t)N * K * 6) || entry_x3_ws(bufs, &ws, s)) return 1;
  int rc = launch_split3(d_w, W3, 1, N, K, s);
  if (!rc) rc = launch_gemm_bf16x3(d_x, W3, d_y, 1, M, N, K, sh, ws, s, true, true, &e);
  return entry_finish(rc, s);
}

int kd_gn_conv3x3_winograd_fused_nhwc(const float* d_x, const float* d_gamma, const float* d_beta,
                                      const float* d_scale_shift, const float* d_w_oihw, const float* d_bias,
                                      const float* d_res, float* d_y, int B, int H, int W, int Cin, int Cout, int G,
                                      float eps, float* d_out_stats, int ldx, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ldx <= 0) ldx = Cin;
  KD_REQUIRE(wino_fused128_ok(B, H, W, Cin, Cout) && G > 0 && Cin % G == 0,
             "GroupNorm-fused Winograd path needs H % 8 == 0, W % 16 == 0, Cin % 4 == 0, Cin <= 2048, Cout % 128 == 0");
  KD_REQUIRE(ldx >= Cin && ldx % 4 == 0, "GroupNorm-fused Winograd path: input row stride must be >= Cin and a multiple of 4");
  KD_REQUIRE(!d_out_stats || (Cout % G == 0 && (Cout / G) % 16 == 0), "output statistics need (Cout / G) % 16 == 0");
  EntryBufs bufs;
  float *U = nullptr, *stats = nullptr, *ab = nullptr;
  double *partial = nullptr, *opart = nullptr;
  void* items = nullptr;
  if (bufs.get(&U, (size_t)16 * Cout * Cin * sizeof(float))) return 1;
  if (bufs.get(&stats, (size_t)B * G * 2 * sizeof(float))) return 1;
  if (bufs.get(&ab, (size_t)B * Cin * 2 * sizeof(float))) return 1;
  if (bufs.get(&partial, gn_partial_bytes(B, H * W, Cin, G))) return 1;
  if (d_out_stats && bufs.get(&opart, (size_t)B * G * wino_fused_out_stats_chunks(H, W, Cout, G) * 2 * sizeof(double))) return 1;
  if (bufs.get(&items, wino_fused128_items_count(B, H, W, Cout) * 16)) return 1;
  int rc = launch_wino_fused128_pack(d_w_oihw, U, Cout, Cin, s, WF_U_SCALE);
  if (!rc) rc = launch_gn_stats(d_x, ldx, stats, partial, B, H * W, Cin, G, eps, s);
  if (!rc) rc = launch_gn_fold(stats, d_gamma, d_beta, d_scale_shift, 2 * Cin, ab, B, Cin, G, s);
  if (!rc) rc = launch_wino_fused128_items(items, B, H, W, Cout, s);
  if (!rc)
    rc = launch_wino_fused_gn128(d_x, ldx, ab, U, d_bias, d_res, Cout, d_y, B, H, W, Cin, Cout, opart, opart ? G : 0, items, gemm_bf16x3_device_cus(), s);
  if (!rc && opart)
    rc = launch_gn_finalize(opart, d_out_stats, (int)wino_fused_out_stats_chunks(H, W, Cout, G), B, G,
                            (double)H * W * (Cout / G), eps, s);
  return entry_finish(rc, s);
}

// ---- the pieces of a ResnetBlock the plan joins (engine.hip: skinny, gca, wino4_block, resnet; the gate_add after a
// GlobalContext gate), one host wrapper each around the plan's own launch_* calls with the plan's argument forms.

int kd_linear_skinny(const float* d_x, int ldx, const float* d_w, const float* d_bias, float* d_y, int ldy, int M, int K,
                     int N, int in_act, int act, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_x && d_w && d_y, "kd_linear_skinny: null argument");
  KD_REQUIRE(M > 0 && K > 0 && N > 0 && ldx >= K && ldy >= N, "kd_linear_skinny needs M, K, N > 0, ldx >= K, ldy >= N");
  KD_REQUIRE(in_act >= ACT_NONE && in_act <= ACT_SIGMOID && act >= ACT_NONE && act <= ACT_SIGMOID,
             "kd_linear_skinny: unknown activation");
  return entry_finish(launch_linear_skinny(d_x, ldx, d_w, d_bias, d_y, ldy, M, K, N, in_act, act, s), s);
}

int kd_linattn_chunk_tokens(void) { return LA_CHUNK; }

int kd_linattn_dwconv_nhwc(const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, float* d_y,
                           float* d_part, int B, int H, int W, int heads, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_x && d_wq && d_wk && d_wv && d_y && d_part, "kd_linattn_dwconv_nhwc: null argument");
  KD_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, "kd_linattn_dwconv_nhwc needs B, H, W, heads > 0");
  const int inner = heads * 64;
  EntryBufs bufs;
  float* w = nullptr;
  if (bufs.get((void**)&w, (size_t)27 * inner * sizeof(float))) return 1;
  int rc = launch_linattn_pack_dw(d_wq, d_wk, d_wv, w, inner, s);
  if (!rc) rc = launch_linattn_dwconv(d_x, w, d_y, d_part, B, H, W, inner, s);
  return entry_finish(rc, s);
}

int kd_linattn_context(const float* d_k, const float* d_v, int ld, const float* d_part, int HW, const float* d_ck,
                       const float* d_cv, int ldc, int m, const float* d_null_k, const float* d_null_v, float* d_ctx, int B,
                       int heads, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_ctx && B > 0 && heads > 0 && HW >= 0 && m >= 0, "kd_linattn_context: null output or bad sizes");
  EntryBufs bufs;
  float* ws = nullptr;
  if (HW > 0 && bufs.get((void**)&ws, linattn_ws_floats(B, heads, HW) * sizeof(float))) return 1;
  return entry_finish(launch_linattn_context(d_k, d_v, ld, d_part, HW, d_ck, d_cv, ldc, m, d_null_k, d_null_v, ws, d_ctx, B,
                                             heads, s), s);
}

int kd_linattn_apply(const float* d_q, int ldq, const float* d_ctx, float* d_out, int ldo, int B, int N, int heads,
                     float scale, int silu, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_q && d_ctx && d_out, "kd_linattn_apply: null argument");
  return entry_finish(launch_linattn_apply(d_q, ldq, d_ctx, d_out, ldo, B, N, heads, scale, silu, s), s);
}

int kd_global_context_gate(const float* d_x, int B, int HW, int C, const float* d_wk, const float* d_bk, const float* d_w0,
                           const float* d_b0, int hid, const float* d_w2, const float* d_b2, float* d_gate, float* d_pooled,
                           int path, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_x && d_wk && d_bk && d_w0 && d_b0 && d_w2 && d_b2 && d_gate, "kd_global_context_gate: null argument");
  KD_REQUIRE(B > 0 && HW > 0 && hid > 0 && C % 4 == 0 && C > 0 && C <= 2048,
             "kd_global_context_gate needs B, HW, hid > 0 and C % 4 == 0, C <= 2048");
  KD_REQUIRE(path >= 0 && path <= 2, "kd_global_context_gate: path 0 (the plan's choice), 1 (pool + two linears), 2 (fused)");
  const bool fused_ok = gca_gate_fused_ok(C, hid) && (((uintptr_t)d_w0 | (uintptr_t)d_w2) & 15) == 0;
  KD_REQUIRE(path != 2 || fused_ok, "kd_global_context_gate: the fused gate needs C <= 512, hid <= 256, 16-byte aligned weights");
  const bool fused = path == 2 || (path == 0 && gca_gate_fused_ok(C, hid) && B > 1);   // engine.hip gca()
  KD_REQUIRE(!(fused && d_pooled), "kd_global_context_gate: the fused gate does not leave the pooled vector");
  EntryBufs bufs;
  float *scratch = nullptr, *pooled = d_pooled, *hidden = nullptr;
  if (bufs.get((void**)&scratch, gca_scratch_floats(B, HW, C) * sizeof(float))) return 1;
  if (fused) return entry_finish(launch_gca_gate(d_x, d_wk, d_bk, scratch, d_w0, d_b0, hid, d_w2, d_b2, d_gate, B, HW, C, s), s);
  if (!pooled && bufs.get((void**)&pooled, (size_t)B * C * sizeof(float))) return 1;
  if (bufs.get((void**)&hidden, (size_t)B * hid * sizeof(float))) return 1;
  int rc = launch_gca_pool(d_x, d_wk, d_bk, nullptr, pooled, scratch, B, HW, C, s);
  if (!rc) rc = launch_linear_skinny(pooled, C, d_w0, d_b0, hidden, hid, B, C, hid, ACT_NONE, ACT_SILU, s);
  if (!rc) rc = launch_linear_skinny(hidden, hid, d_w2, d_b2, d_gate, C, B, hid, C, ACT_NONE, ACT_SIGMOID, s);
  return entry_finish(rc, s);
}

int kd_gate_add_chunks(int B, int HW) { return B > 0 && HW > 0 ? gate_add_chunks(B, HW) : 0; }
int kd_conv_launch_shape(const int* geom, unsigned has, unsigned al16, int cus, int* out) {
  KD_REQUIRE(geom && out && cus > 0, "kd_conv_launch_shape: null argument or no compute units");
  ConvParams p{};
  int* const field[22] = {&p.B,  &p.Hi,  &p.Wi,     &p.Cin, &p.ldx,   &p.Ho,    &p.Wo,       &p.Cout, &p.KH,   &p.KW,      &p.stride,
                          &p.pad, &p.rr_cin, &p.act, &p.ldres, &p.ldgs, &p.out_mode, &p.ldy, &p.yoff, &p.wz_rows, &p.wz_count, &p.seg_c0};
  for (int i = 0; i < 22; ++i) *field[i] = geom[i];
  KD_REQUIRE(p.B > 0 && p.Ho > 0 && p.Wo > 0 && p.Cout > 0 && p.Cin > 0 && p.KH > 0 && p.KW > 0, "kd_conv_launch_shape: empty conv");
  const ConvShape sh = conv_shape(p, ConvPtrs{has | CONV_Y, al16}, cus);
  KD_REQUIRE(sh.variant >= 0, "kd_conv_launch_shape: no kernel takes a batched GEMM off the buffer-load fast path");
  const ConvTile& t = conv_tile(sh.variant);
  const int rec[12] = {t.igemm, t.bm, t.bn, t.waves_m, t.waves_n, (int)sh.grid[0], (int)sh.grid[1], (int)sh.grid[2],
                       64 * t.waves_m * t.waves_n, sh.ksplit, sh.wide_epilogue, sh.seg_chunks};
  std::copy(rec, rec + 12, out);
  return 0;
}

int kd_gate_add_nhwc(const float* d_a, const float* d_gate, const float* d_r, int ldr, float* d_y, int ldy, double* d_seg,
                     int B, int HW, int C, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ldr <= 0) ldr = C;
  if (ldy <= 0) ldy = C;
  KD_REQUIRE(d_a && d_r && d_y, "kd_gate_add_nhwc: null argument");
  KD_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 4 == 0 && ldr >= C && ldy >= C && ldr % 4 == 0 && ldy % 4 == 0,
             "kd_gate_add_nhwc needs C % 4 == 0 and row strides >= C, multiples of 4");
  KD_REQUIRE((((uintptr_t)d_a | (uintptr_t)d_gate | (uintptr_t)d_r | (uintptr_t)d_y) & 15) == 0,
             "kd_gate_add_nhwc: 16-byte aligned maps and gate");
  KD_REQUIRE(!d_seg || C % 16 == 0, "kd_gate_add_nhwc: segment partials need C % 16 == 0");
  return entry_finish(launch_gate_add(d_a, d_gate, d_r, ldr, d_y, ldy, d_seg, B, HW, C, s), s);
}

float kd_wf_ab_scale(void) { return WF_AB_SCALE; }

int kd_gn_fold_seg(const double* d_seg0, int nseg0, int nchunk0, float scale0, float ab_mul0, const double* d_seg1, int nseg1,
                   int nchunk1, float scale1, float ab_mul1, const float* d_gamma, const float* d_beta,
                   const float* d_scale_shift, int ld_ss, float* d_ab, float* d_stats, int B, int HW, int C, int G, float eps,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_seg0 && (d_ab || d_stats), "kd_gn_fold_seg: null argument");
  KD_REQUIRE(B > 0 && HW > 0 && G > 0 && C % G == 0 && (C / G) % 16 == 0, "kd_gn_fold_seg needs groups of 16 n channels");
  KD_REQUIRE(nseg0 > 0 && nchunk0 > 0 && (!d_seg1 || (nseg1 > 0 && nchunk1 > 0)) &&
                 16 * (nseg0 + (d_seg1 ? nseg1 : 0)) == C,
             "kd_gn_fold_seg: the sources' 16-channel segments must tile the C channels");
  KD_REQUIRE(!d_ab || (d_gamma && d_beta), "kd_gn_fold_seg: the affine needs gamma and beta");
  KD_REQUIRE(!d_scale_shift || ld_ss >= 2 * C, "kd_gn_fold_seg: FiLM rows [scale | shift] need ld_ss >= 2 C");
  SegSrc s0{d_seg0, nseg0, nchunk0, 0, scale0, ab_mul0};
  SegSrc s1{d_seg1, d_seg1 ? nseg1 : 0, d_seg1 ? nchunk1 : 0, 16 * nseg0, scale1, ab_mul1};
  return entry_finish(launch_gn_fold_seg(s0, s1, d_gamma, d_beta, d_scale_shift, ld_ss, d_ab, d_stats, B, C, G,
                                         (double)HW * (C / G), eps, s),
                      s);
}

int kd_gn_conv3x3_winograd4_nhwc(const float* d_x, int ldx, const float* d_stats, const float* d_gamma, const float* d_beta,
                                 const float* d_scale_shift, int ld_ss, int skip_c0, float skip_scale, const float* d_w_oihw,
                                 const float* d_bias, const float* d_res, int ldres, float* d_y, double* d_out_seg, int B,
                                 int H, int W, int Cin, int Cout, int G, int gemm_mode, int images_per_set, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ldx <= 0) ldx = Cin;
  if (ldres <= 0) ldres = Cout;
  const int Bx = images_per_set > 0 ? images_per_set : B;
  KD_REQUIRE(d_x && d_stats && d_gamma && d_beta && d_w_oihw && d_bias && d_y, "kd_gn_conv3x3_winograd4_nhwc: null argument");
  KD_REQUIRE(B > 0 && Bx > 0 && B % Bx == 0, "kd_gn_conv3x3_winograd4_nhwc: images_per_set must divide B");
  KD_REQUIRE(H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, "Winograd F(4x4,3x3) path needs H % 4 == 0 and W % 4 == 0");
  const int64_t Mt = (int64_t)Bx * (H / 4) * (W / 4);
  KD_REQUIRE(Mt % 128 == 0 && Cin % 32 == 0 && Cout % 64 == 0 && 36 * Mt < 0x7fffffff &&
                 (int64_t)36 * Cout * Cin * 4 < 0x7fffffff,
             "Winograd F(4x4,3x3) path needs images_per_set*H*W/16 % 128 == 0, Cin % 32 == 0, Cout % 64 == 0");
  KD_REQUIRE(gemm_mode == -1 || gemm_mode == 1 || gemm_mode == 2, "kd_gn_conv3x3_winograd4_nhwc: gemm_mode -1, 1 or 2");
  KD_REQUIRE(gemm_mode < 0 || gemm_bf16x3_ok(36, Mt, Cout, Cin),
             "bf16x3 position GEMMs need images_per_set*H*W/16 % 256 == 0, Cout % 128 == 0, Cin % 32 == 0");
  KD_REQUIRE(G > 0 && Cin % G == 0, "kd_gn_conv3x3_winograd4_nhwc: Cin % G == 0");
  KD_REQUIRE(ldx >= Cin && ldx % 2 == 0 && ((uintptr_t)d_x & 7) == 0 && (int64_t)Bx * H * W * ldx * 4 < ((int64_t)1 << 32),
             "kd_gn_conv3x3_winograd4_nhwc: x rows of stride >= Cin, even, 8-byte aligned, one set's map below 4 GB");
  KD_REQUIRE(skip_c0 < 0 || (skip_c0 <= Cin && skip_c0 % 2 == 0), "kd_gn_conv3x3_winograd4_nhwc: skip_c0 in [0, Cin], even");
  KD_REQUIRE(!d_scale_shift || ld_ss >= 2 * Cin, "kd_gn_conv3x3_winograd4_nhwc: FiLM rows [scale | shift] need ld_ss >= 2 Cin");
  KD_REQUIRE(!d_res || (ldres >= Cout && ldres % 2 == 0), "kd_gn_conv3x3_winograd4_nhwc: residual row stride >= Cout, even");
  KD_REQUIRE((((uintptr_t)d_y | (uintptr_t)d_res | (uintptr_t)d_bias) & 7) == 0,
             "kd_gn_conv3x3_winograd4_nhwc: 8-byte aligned y, residual and bias");
  const bool planes = gemm_mode == 1, x3 = gemm_mode > 0;
  const X3Shape sh = entry_x3_shape(36, Mt, Cout, Cin);
  EntryBufs bufs;
  float *U = nullptr, *D = nullptr;
  void *V = nullptr, *U3 = nullptr, *ws = nullptr;
  if (bufs.get((void**)&U, (size_t)36 * Cout * Cin * sizeof(float))) return 1;
  if (bufs.get(&V, planes ? (size_t)36 * Mt * Cin * 6 : (size_t)36 * Mt * Cin * sizeof(float))) return 1;
  if (bufs.get((void**)&D, (size_t)36 * Mt * Cout * sizeof(float))) return 1;
  if (x3 && bufs.get(&U3, ((size_t)36 * Cout * Cin * 3 + 1) / 2 * sizeof(float))) return 1;
  if (x3 && entry_x3_ws(bufs, &ws, s)) return 1;
  int rc = launch_wino4_pack(d_w_oihw, U, Cout, Cin, s);
  if (!rc && x3) rc = launch_split3(U, U3, 36, Cout, Cin, s);
  const int64_t HW = (int64_t)H * W, nchunk = (H / 4) * (W / 4);
  // the launch sequence of wino4_block (engine.hip), set by set: input transform with the GroupNorm / FiLM / SiLU affine
  // folded, the 36 position GEMMs (+ the k-cut tiles' sum), output transform with bias, residual and the output partials
  for (int st = 0; st < B / Bx && !rc; ++st) {
    const int b0 = st * Bx;
    const float* xs = d_x + (size_t)b0 * HW * ldx;
    const float* ss = d_stats + (size_t)b0 * G * 2;
    const float* ssp = d_scale_shift ? d_scale_shift + (size_t)b0 * ld_ss : nullptr;
    if (planes)
      rc = launch_wino4_in3(xs, ldx, ss, d_gamma, d_beta, ssp, ld_ss, V, Bx, H, W, Cin, G, s, skip_c0, skip_scale);
    else
      rc = launch_wino4_in(xs, ldx, ss, d_gamma, d_beta, ssp, ld_ss, (float*)V, Bx, H, W, Cin, G, s, skip_c0, skip_scale);
    if (!rc && x3) {
      rc = launch_gemm_bf16x3(V, U3, D, 36, (int)Mt, Cout, Cin, sh, ws, s, !planes);
    } else if (!rc) {
      ConvParams p{};
      p.x = (const float*)V; p.w = U; p.y = D;
      p.B = 1; p.Hi = 1; p.Wi = (int)(36 * Mt); p.Cin = Cin; p.ldx = Cin;
      p.Ho = 1; p.Wo = (int)(36 * Mt); p.Cout = Cout;
      p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0;
      p.out_mode = OUT_NHWC; p.ldy = Cout;
      p.wz_rows = (int)Mt; p.wz_count = 36;
      rc = entry_conv(p, s);
    }
    if (!rc)
      rc = launch_wino4_out(D, d_bias, d_res ? d_res + (size_t)b0 * HW * ldres : nullptr, ldres, d_y + (size_t)b0 * HW * Cout,
                            Cout, d_out_seg ? d_out_seg + (size_t)b0 * (Cout / 16) * nchunk * 2 : nullptr, Bx, H, W, Cout, s);
  }
  return entry_finish(rc, s);
}

// The init cross-embed convs over a 3-plane NCHW image through the plan's fused kernel (kernels_init.hip):
// y NHWC [B][S][S][n3+n7+n15] = cat(conv3, conv7, conv15)(x) + bias.  d_w*: OIHW [n][3][k][k].
int kd_init_conv_nchw(const float* d_x, const float* d_w3, const float* d_w7, const float* d_w15, const float* d_bias,
                      float* d_y, int B, int S, int n3, int n7, int n15, void* stream) {
  return kd_init_conv_planes_nchw(d_x, nullptr, d_w3, d_w7, d_w15, 3, 0, d_bias, nullptr, d_y, B, S, n3, n7, n15, 1, nullptr,
                                  stream);
}

int kd_init_conv_planes_nchw(const float* d_x, const float* d_self_cond, const float* d_w3, const float* d_w7,
                             const float* d_w15, int Itot, int c0, const float* d_bias, const float* d_res, float* d_y, int B,
                             int S, int n3, int n7, int n15, int iters, float* ms, void* stream) {
  return kd_init_conv_planes_c_nchw(d_x, d_self_cond, d_w3, d_w7, d_w15, Itot, c0, d_bias, d_res, d_y, B, S, n3, n7, n15, iters,
                                    ms, 3, stream);
}

int kd_init_conv_planes_c_nchw(const float* d_x, const float* d_self_cond, const float* d_w3, const float* d_w7,
                               const float* d_w15, int Itot, int c0, const float* d_bias, const float* d_res, float* d_y, int B,
                               int S, int n3, int n7, int n15, int iters, float* ms, int channels, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(channels >= 1 && channels <= 4, "kd_init_conv_planes_c_nchw: 1 to 4 image channels");
  const int np = d_self_cond ? 2 * channels : channels;
  KD_REQUIRE(d_x && d_w3 && d_w7 && d_w15 && d_y && iters >= 1, "kd_init_conv_planes_nchw: null argument or iters < 1");
  KD_REQUIRE(B >= 1 && S >= 1, "kd_init_conv_planes_nchw: empty shape");
  KD_REQUIRE(c0 >= 0 && c0 + np <= Itot, "kd_init_conv_planes_nchw: input channels c0 .. c0 + planes - 1 out of range");
  KD_REQUIRE(init_conv_fused_ok(S, n3, n7, n15, np), "init conv kernel: S % 32 == 0 and the weights must fit LDS");
  EntryBufs bufs;
  float* wp = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (bufs.get(&wp, init_conv_weight_floats(n3, n7, n15, np) * sizeof(float))) return 1;
  int rc = launch_init_conv_pack(d_w3, d_w7, d_w15, wp, n3, n7, n15, Itot, c0, np, s);
  if (!rc && ms) {
    rc = hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, s) != hipSuccess;
    if (rc) set_error("kd_init_conv_planes_nchw: event setup failed");
  }
  const int cus = gemm_bf16x3_device_cus();
  for (int i = 0; i < iters && !rc; ++i)
    rc = launch_init_conv(d_x, d_self_cond, channels, np, wp, d_bias, d_res, d_y, n3 + n7 + n15, nullptr, B, S, n3, n7, n15, cus, s);
  if (!rc && ms && hipEventRecord(e1, s) != hipSuccess) {
    set_error("kd_init_conv_planes_nchw: event record failed");
    rc = 1;
  }
  hipError_t e = hipStreamSynchronize(s);
  if (!rc && ms && e == hipSuccess) {
    float t = 0.f;
    e = hipEventElapsedTime(&t, e0, e1);
    *ms = t / iters;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
}

// The per-step share of a plain init conv through the plan's one-kernel form (kernels_init.hip, init_plain_kernel)
int kd_init_conv_plain_nchw(const float* d_x, const float* d_self_cond, const float* d_w, int Itot, int c0, const float* d_bias,
                            const float* d_res, float* d_y, int ldy, double* d_seg, int B, int S, int n, int ksize, int channels,
                            int iters, float* ms, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(channels >= 1 && channels <= 4, "kd_init_conv_plain_nchw: 1 to 4 image channels");
  const int np = d_self_cond ? 2 * channels : channels;
  KD_REQUIRE(d_x && d_w && d_y && iters >= 1, "kd_init_conv_plain_nchw: null argument or iters < 1");
  KD_REQUIRE(B >= 1 && S >= 1, "kd_init_conv_plain_nchw: empty shape");
  KD_REQUIRE(c0 >= 0 && c0 + np <= Itot, "kd_init_conv_plain_nchw: input channels c0 .. c0 + planes - 1 out of range");
  KD_REQUIRE(init_plain_ok(S, n, ksize, np),
             "plain init conv kernel: kernel size 3, 5 or 7, S % 32 == 0, n % 4 == 0, n <= 128 and the weights must fit LDS");
  KD_REQUIRE(ldy >= n, "kd_init_conv_plain_nchw: ldy below the output's channels");
  EntryBufs bufs;
  float* wp = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (bufs.get(&wp, init_plain_weight_floats(n, ksize, np) * sizeof(float))) return 1;
  int rc = launch_init_plain_pack(d_w, wp, n, Itot, c0, np, ksize, s);
  if (!rc && ms) {
    rc = hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, s) != hipSuccess;
    if (rc) set_error("kd_init_conv_plain_nchw: event setup failed");
  }
  const int cus = gemm_bf16x3_device_cus();
  for (int i = 0; i < iters && !rc; ++i)
    rc = launch_init_plain(d_x, d_self_cond, channels, np, wp, d_bias, d_res, d_y, ldy, d_seg, B, S, n, ksize, cus, s);
  if (!rc && ms && hipEventRecord(e1, s) != hipSuccess) {
    set_error("kd_init_conv_plain_nchw: event record failed");
    rc = 1;
  }
  hipError_t e = hipStreamSynchronize(s);
  if (!rc && ms && e == hipSuccess) {
    float t = 0.f;
    e = hipEventElapsedTime(&t, e0, e1);
    *ms = t / iters;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
}

// The final k x k conv to the image's channels as the plan runs it (unet_build.inc, kernels_final.hip): weight pack, the 1x1
// GEMM to the (output, tap) columns, the low-res planes' step-invariant share when d_lowres is given, the gather
static int final_conv_nchw(const std::string& w, const float* d_feat, const float* d_w_oihw, const float* d_bias,
                           const float* d_lowres, float* d_out, int B, int H, int W, int Cfeat, int channels, int ksize,
                           void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_feat && d_w_oihw && d_bias && d_out, w + ": null argument");
  KD_REQUIRE(channels >= 1 && channels <= 4, w + ": 1 to 4 image channels");
  KD_REQUIRE(ksize == 1 || ksize == 3 || ksize == 5 || ksize == 7, w + ": kernel size 1, 3, 5 or 7");
  const int most = ksize == 3 ? 48 : 208;   // columns of P at 4 channels
  KD_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cfeat >= 4 && Cfeat % 4 == 0 && (int64_t)B * H * W < 0x7fffffff / most,
             w + " needs a non-empty map below 2^31 / " + std::to_string(most) + " pixels and Cfeat % 4 == 0");
  const int Ctot = Cfeat + (d_lowres ? channels : 0), nf = final_gemm_cols_k(channels, ksize);
  EntryBufs bufs;
  float *wp = nullptr, *pm = nullptr, *stat = nullptr;
  if (bufs.get(&wp, (size_t)nf * Cfeat * sizeof(float)) || bufs.get(&pm, (size_t)B * H * W * nf * sizeof(float))) return 1;
  if (d_lowres && bufs.get(&stat, (size_t)B * channels * H * W * sizeof(float))) return 1;
  int rc = launch_pack_final_k(d_w_oihw, wp, Ctot, Cfeat, channels, ksize, s);
  if (!rc && d_lowres) rc = launch_final_static(d_lowres, d_w_oihw, d_bias, stat, Ctot, Cfeat, channels, B, H, W, s, ksize);
  if (!rc) {
    ConvParams p{};
    p.x = d_feat; p.w = wp; p.y = pm;
    p.B = B; p.Hi = H; p.Wi = W; p.Cin = Cfeat; p.ldx = Cfeat;
    p.Ho = H; p.Wo = W; p.Cout = nf;
    p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0;
    p.out_mode = OUT_NHWC; p.ldy = nf;
    rc = entry_conv(p, s);
  }
  if (!rc) rc = launch_final_gather_k(pm, stat, d_bias, d_out, channels, ksize, B, H, W, s);
  return entry_finish(rc, s);
}
int kd_final_conv_nchw(const float* d_feat, const float* d_w_oihw, const float* d_bias, const float* d_lowres, float* d_out,
                       int B, int H, int W, int Cfeat, int channels, void* stream) {
  return final_conv_nchw("kd_final_conv_nchw", d_feat, d_w_oihw, d_bias, d_lowres, d_out, B, H, W, Cfeat, channels, 3, stream);
}
int kd_final_conv_k_nchw(const float* d_feat, const float* d_w_oihw, const float* d_bias, const float* d_lowres, float* d_out,
                         int B, int H, int W, int Cfeat, int channels, int ksize, void* stream) {
  return final_conv_nchw("kd_final_conv_k_nchw", d_feat, d_w_oihw, d_bias, d_lowres, d_out, B, H, W, Cfeat, channels, ksize,
                         stream);
}

int kd_groupnorm_silu_nhwc(const float* d_x, const float* d_gamma, const float* d_beta, const float* d_scale_shift,
                           float* d_y, int B, int HW, int C, int G, float eps, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  EntryBufs bufs;
  float* stats = nullptr;
  double* partial = nullptr;
  if (bufs.get(&stats, (size_t)B * G * 2 * sizeof(float)) || bufs.get(&partial, gn_partial_bytes(B, HW, C, G))) return 1;
  int rc = launch_gn_stats(d_x, C, stats, partial, B, HW, C, G, eps, s);
  if (!rc) rc = launch_gn_apply_silu(d_x, C, stats, d_gamma, d_beta, d_scale_shift, 2 * C, d_y, B, HW, C, G, s);
  return entry_finish(rc, s);
}

int kd_layernorm(const float* d_x, const float* d_g, const float* d_beta, float* d_y, int rows, int C, float eps,
                 void* stream) {
  return launch_layernorm(d_x, C, d_g, d_beta, nullptr, 0, d_y, rows, C, eps, (hipStream_t)stream);
}

int kd_layernorm_ex(const float* d_x, const float* d_g, const float* d_beta, const float* d_res, float* d_y, int rows, int C,
                    float eps, int in_act, const float* d_g2, float* d_y2, void* stream) {
  KD_REQUIRE(in_act >= ACT_NONE && in_act <= ACT_SIGMOID, "kd_layernorm_ex: unknown activation");
  return launch_layernorm(d_x, C, d_g, d_beta, d_res, C, d_y, rows, C, eps, (hipStream_t)stream, in_act, d_g2, d_y2);
}

int kd_layernorm_linear_bf16x3(const float* d_x, const float* d_g, const float* d_beta, int rows, int C, float eps, int in_act,
                               const float* d_w, const float* d_bias, const float* d_res, int ldres, float* d_y, int ldy,
                               int N, void* d_planes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(in_act >= ACT_NONE && in_act <= ACT_SIGMOID, "kd_layernorm_linear_bf16x3: unknown activation");
  KD_REQUIRE(d_planes && C % 16 == 0 && C <= 4096, "kd_layernorm_linear_bf16x3 needs C % 16 == 0, C <= 4096 and the plane buffer");
  X3Epi e;
  e.bias = d_bias;
  e.res = d_res;
  e.ldres = ldres;
  e.hw = rows;
  e.ldy = ldy > 0 ? ldy : N;
  e.lda = C;
  const X3Shape sh = entry_x3_shape(1, rows, N, C);
  KD_REQUIRE(gemm_bf16x3_epi_ok(rows, N, C, e, sh), "kd_layernorm_linear_bf16x3 needs rows % 256 == 0, N % 128 == 0, C % 32 == 0");
  EntryBufs bufs;
  void *W3 = nullptr, *ws = nullptr;
  if (bufs.get(&W3, (size_t)N * C * 6) || entry_x3_ws(bufs, &ws, s)) return 1;
  int rc = launch_split3(d_w, W3, 1, N, C, s);
  if (!rc) rc = launch_layernorm(d_x, C, d_g, d_beta, nullptr, 0, (float*)d_planes, rows, C, eps, s, in_act, nullptr, nullptr, nullptr, 0, 1);
  if (!rc) rc = launch_gemm_bf16x3(d_planes, W3, d_y, 1, rows, N, C, sh, ws, s, false, true, &e);
  return entry_finish(rc, s);
}

int kd_attention(const float* d_q, const float* d_k, const float* d_v, float* d_out, int B, int Nq, int Nk, int H,
                 int Hkv, int D, void* stream) {
  KD_REQUIRE(D == 32 || D == 64 || D == 128, "kd_attention is built for D = 32, 64 and 128");
  KVSeg s0{d_k, d_v, Hkv * D, Nk};
  KVSeg s1{nullptr, nullptr, 0, 0};
  return launch_attention(d_q, H * D, nullptr, nullptr, s0, s1, d_out, H * D, B, Nq, H, Hkv, D, 1.0f,
                          (hipStream_t)stream);
}

// launch_attention with every argument the plan passes it (engine.hip transformer() / cross_attn(), text_build.inc):
// learned null key / value, two K/V segments with their own row strides, q / out row strides, scale
int kd_attention_ex(const float* d_q, int ldq, const float* d_null_kv, const float* d_k0, const float* d_v0, int ld0, int n0,
                    const float* d_k1, const float* d_v1, int ld1, int n1, float* d_out, int ldo, int B, int Nq, int H, int Hkv,
                    float scale, void* stream) {
  return kd_attention_ex_d(d_q, ldq, d_null_kv, d_k0, d_v0, ld0, n0, d_k1, d_v1, ld1, n1, d_out, ldo, B, Nq, H, Hkv, 64, scale,
                           stream);
}

int kd_attention_ex_d(const float* d_q, int ldq, const float* d_null_kv, const float* d_k0, const float* d_v0, int ld0, int n0,
                      const float* d_k1, const float* d_v1, int ld1, int n1, float* d_out, int ldo, int B, int Nq, int H, int Hkv,
                      int D, float scale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_q && d_out && B > 0 && H > 0 && n0 >= 0 && n1 >= 0, "kd_attention_ex: null argument or bad sizes");
  KD_REQUIRE((n0 == 0 || (d_k0 && d_v0)) && (n1 == 0 || (d_k1 && d_v1)), "kd_attention_ex: a segment with keys needs k and v");
  KD_REQUIRE((((uintptr_t)d_q | (uintptr_t)d_null_kv | (uintptr_t)d_k0 | (uintptr_t)d_v0 | (uintptr_t)d_k1 | (uintptr_t)d_v1 |
               (uintptr_t)d_out) & 15) == 0, "kd_attention_ex: 16-byte aligned pointers");
  KD_REQUIRE(D == 32 || D == 64 || D == 128, "kd_attention_ex_d: D must be 32, 64 or 128");
  KD_REQUIRE(ldq >= H * D && ldo >= H * D && (n0 == 0 || ld0 >= Hkv * D) && (n1 == 0 || ld1 >= Hkv * D),
             "kd_attention_ex: a row stride is shorter than its heads");
  KVSeg s0{d_k0, d_v0, ld0, n0};
  KVSeg s1{d_k1, d_v1, ld1, n1};
  return entry_finish(launch_attention(d_q, ldq, d_null_kv, d_null_kv ? d_null_kv + D : nullptr, s0, s1, d_out, ldo, B,
                                       Nq, H, Hkv, D, scale, s), s);
}

int kd_attention_key_tile(int D) { return attention_key_tile(D); }

int kd_l2norm_heads(float* d_x, int ld, int64_t rows, int heads, const float* d_scale_vec, void* stream) {
  return kd_l2norm_heads_d(d_x, ld, rows, heads, 64, d_scale_vec, stream);
}

int kd_l2norm_heads_d(float* d_x, int ld, int64_t rows, int heads, int D, const float* d_scale_vec, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(D == 32 || D == 64 || D == 128, "kd_l2norm_heads_d: D must be 32, 64 or 128");
  KD_REQUIRE(d_x && rows >= 0 && heads > 0 && ld >= heads * D, "kd_l2norm_heads: null argument or ld < heads * D");
  return entry_finish(launch_l2norm_heads(d_x, ld, rows, heads, D, d_scale_vec, s), s);
}

// ---- the small kernels of the text-conditioning plan (text_build.inc), one pass-through each with the plan's argument forms
int kd_text_select(const float* d_tok, const float* d_mask, const float* d_null_embed, float* d_out, int B, int L, int P, int C,
                   int drop, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_tok && d_null_embed && d_out, "kd_text_select: null argument");
  KD_REQUIRE(B > 0 && C > 0 && L >= 1 && L <= P, "kd_text_select needs B, C > 0 and 1 <= L <= P");
  return entry_finish(launch_text_select(d_tok, d_mask, d_null_embed, d_out, B, L, P, C, drop != 0, s), s);
}

int kd_add_rows_bcast(const float* d_x, const float* d_add, float* d_y, int B, int R, int C, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_x && d_add && d_y && B > 0 && R > 0 && C > 0, "kd_add_rows_bcast: null argument or empty shape");
  return entry_finish(launch_add_rows_bcast(d_x, d_add, d_y, B, R, C, s), s);
}

int kd_mean_rows(const float* d_x, float* d_y, int B, int R, int C, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_x && d_y && B > 0 && R > 0 && C > 0, "kd_mean_rows: null argument or empty shape");
  KD_REQUIRE((int64_t)B * C < 0x7fffffff, "kd_mean_rows: B * C must stay below 2^31 (one thread per output, int index)");
  return entry_finish(launch_mean_rows(d_x, d_y, B, R, C, s), s);
}

int kd_copy_rows(const float* d_src, int64_t src_bstride, int ld_src, float* d_dst, int64_t dst_bstride, int ld_dst, int rows,
                 int C, int B, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_src && d_dst && rows >= 0 && C >= 0 && B >= 0, "kd_copy_rows: null argument or negative size");
  KD_REQUIRE(ld_src >= C && ld_dst >= C && src_bstride >= 0 && dst_bstride >= 0, "kd_copy_rows needs row strides >= C, batch strides >= 0");
  return entry_finish(launch_copy_rows(d_src, src_bstride, ld_src, d_dst, dst_bstride, ld_dst, rows, C, B, s), s);
}

size_t kd_quantile_workspace_bytes(int B) { return quantile_ws_bytes(B); }
int kd_quantile_abs(const float* d_x, float* d_out, int B, int64_t n, float q, void* d_workspace,
                    size_t workspace_bytes, void* stream) {
  KD_REQUIRE(workspace_bytes >= quantile_ws_bytes(B), "quantile workspace too small");
  return launch_quantile_abs(d_x, d_out, B, n, q, d_workspace, (hipStream_t)stream);
}

int kd_cfg_combine(const float* d_cond, const float* d_null, float* d_out, float cond_scale, int64_t n,
                   void* stream) {
  KD_REQUIRE(d_cond && d_null && d_out && n >= 0, "kd_cfg_combine: null argument");
  return launch_cfg_combine(d_cond, d_null, d_out, cond_scale, n, (hipStream_t)stream);
}

int kd_philox_normal(float* d_out, int64_t n, uint64_t seed, uint64_t stream_id, void* stream) {
  return launch_philox_normal(d_out, n, seed, stream_id, (hipStream_t)stream);
}
int kd_philox_normal_rows(float* d_out, int B, int64_t n, const uint64_t* seeds, uint64_t stream_id, void* stream) {
  return launch_philox_normal_rows(d_out, B, n, seeds, stream_id, (hipStream_t)stream);
}
int kd_sample_start(float* d_x, int B, int C, int S, float scale, uint64_t seed, const uint64_t* seeds, const float* d_noise,
                    const float* d_init, int Hs, int Ws, void* stream) {
  return launch_sample_start(d_x, B, C, S, scale, seed, seeds, d_noise, d_init, Hs, Ws, (hipStream_t)stream);
}

int kd_tiles_gather(const float* d_canvas, float* d_tiles, int B, int C, int Hc, int Wc, int S, const int* origins_yx,
                    void* stream) {
  return launch_tiles_gather(d_canvas, d_tiles, B, C, Hc, Wc, S, origins_yx, (hipStream_t)stream);
}
int kd_tiles_fuse_update(float* d_x, float* d_x0bar, const float* d_x0_tiles, const float* d_thr, const int* d_tile_of, int N,
                         int C, int S, int st, int ny, int nx, int ramp, float A, float B, float P, float Sn,
                         const float* d_noise, uint64_t seed, uint64_t stream_id, void* stream) {
  return kd_tiles_fuse_update_known(d_x, d_x0bar, d_x0bar, d_x0_tiles, d_thr, d_tile_of, N, C, S, st, ny, nx, ramp, A, B, P, Sn,
                                    d_noise, seed, stream_id, 0, 0.0f, 0.0f, nullptr, 0, nullptr, nullptr, 0.0f, 0.0f, nullptr, 0,
                                    stream);
}
int kd_tiles_cond_gather(const float* d_src, int Cs, int W, float* d_tiles, int B, int S, const int* shifts_yx, int top,
                         const int* d_win_of, const int* d_centre_of, float fill, void* stream) {
  return launch_tiles_cond_gather(d_src, Cs, W, d_tiles, B, S, shifts_yx, top, d_win_of, d_centre_of, fill, (hipStream_t)stream);
}
int kd_tiles_gather_lowres(const float* d_prev, int Hp, int Wp, float* d_tiles, int B, int C, int Hc, int Wc, int S,
                           const int* origins_yx, float a, float s, const float* d_noise, uint64_t seed, uint64_t stream_id,
                           void* stream) {
  return launch_tiles_gather_lowres(d_prev, Hp, Wp, d_tiles, B, C, Hc, Wc, S, origins_yx, a, s, d_noise, seed, stream_id,
                                    (hipStream_t)stream);
}
int kd_tiles_finalize(const float* d_x, const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, float* d_out, int Ho,
                      int Wo, int oy, int ox, void* stream) {
  return kd_tiles_finalize_known(d_x, d_tile_of, N, C, S, st, ny, nx, d_out, Ho, Wo, oy, ox, nullptr, nullptr, stream);
}
// the C structs of the canvas sources as the launchers take them; a NULL source stays NULL
static const TileImage* tile_image_of(const kd_tiles_image_t* in, TileImage* out) {
  if (!in) return nullptr;
  *out = TileImage{in->d, in->H, in->W, in->row_stride, in->plane_stride};
  return out;
}
static const TileMask* tile_mask_of(const kd_tiles_mask_t* in, TileMask* out) {
  if (!in) return nullptr;
  *out = TileMask{in->d, in->H, in->W, in->row_stride};
  return out;
}
int kd_tiles_start(float* d_x, int C, int Hc, int Wc, float scale, const float* d_noise, uint64_t seed,
                   const kd_tiles_image_t* init, const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, float mix_a,
                   float mix_s, const float* d_mix_noise, uint64_t mix_stream_id, void* stream) {
  TileImage in, kn;
  TileMask mk;
  const TileMix mix{tile_image_of(known, &kn), tile_mask_of(mask, &mk), mix_a, mix_s, d_mix_noise, mix_stream_id};
  return launch_tiles_start(d_x, C, Hc, Wc, scale, d_noise, seed, tile_image_of(init, &in), mix, (hipStream_t)stream);
}
int kd_tiles_fuse_update_known(float* d_x, const float* d_hist, float* d_x0bar_out, const float* d_x0_tiles, const float* d_thr,
                               const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, int ramp, float A, float B,
                               float P, float Sn, const float* d_noise, uint64_t seed, uint64_t stream_id, int renoise,
                               float rn_a, float rn_b, const float* d_rn_noise, uint64_t rn_stream_id,
                               const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, float mix_a, float mix_s,
                               const float* d_mix_noise, uint64_t mix_stream_id, void* stream) {
  return kd_tiles_fuse_update_hist2(d_x, d_hist, d_x0bar_out, d_x0_tiles, d_thr, d_tile_of, N, C, S, st, ny, nx, ramp, A, B, P, Sn,
                                    d_noise, seed, stream_id, renoise, rn_a, rn_b, d_rn_noise, rn_stream_id, known, mask, mix_a,
                                    mix_s, d_mix_noise, mix_stream_id, nullptr, 0.0f, stream);
}
int kd_tiles_fuse_update_hist2(float* d_x, const float* d_hist, float* d_x0bar_out, const float* d_x0_tiles, const float* d_thr,
                               const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, int ramp, float A, float B,
                               float P, float Sn, const float* d_noise, uint64_t seed, uint64_t stream_id, int renoise,
                               float rn_a, float rn_b, const float* d_rn_noise, uint64_t rn_stream_id,
                               const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, float mix_a, float mix_s,
                               const float* d_mix_noise, uint64_t mix_stream_id, const float* d_hist2, float P2, void* stream) {
  TileImage kn;
  TileMask mk;
  const TileMix mix{tile_image_of(known, &kn), tile_mask_of(mask, &mk), mix_a, mix_s, d_mix_noise, mix_stream_id};
  return launch_tiles_fuse_update(d_x, d_hist, d_x0bar_out, d_x0_tiles, d_thr, d_tile_of, N, C, S, st, ny, nx, ramp, A, B, P,
                                  Sn, d_noise, seed, stream_id, renoise, rn_a, rn_b, d_rn_noise, rn_stream_id, mix,
                                  (hipStream_t)stream, d_hist2, P2);
}
// the finish over the canvas rows [y_lo, y_hi); y_hi < 0 is the launcher's "through the last row"
static int tiles_finalize(const float* d_x, const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, float* d_out, int Ho,
                          int Wo, int oy, int ox, const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, int y_lo, int y_hi,
                          void* stream) {
  TileImage kn;
  TileMask mk;
  return launch_tiles_finalize(d_x, d_tile_of, N, C, S, st, ny, nx, d_out, Ho, Wo, oy, ox, tile_image_of(known, &kn),
                               tile_mask_of(mask, &mk), y_lo, y_hi, (hipStream_t)stream);
}
int kd_tiles_finalize_known(const float* d_x, const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, float* d_out,
                            int Ho, int Wo, int oy, int ox, const kd_tiles_image_t* known, const kd_tiles_mask_t* mask,
                            void* stream) {
  return tiles_finalize(d_x, d_tile_of, N, C, S, st, ny, nx, d_out, Ho, Wo, oy, ox, known, mask, 0, -1, stream);
}
int kd_tiles_finalize_rows(const float* d_x, const int* d_tile_of, int N, int C, int S, int st, int ny, int nx, float* d_out,
                           int Ho, int Wo, int oy, int ox, const kd_tiles_image_t* known, const kd_tiles_mask_t* mask, int y_lo,
                           int y_hi, void* stream) {
  KD_REQUIRE(y_hi >= 0, "tiles finalize rows: y_hi must not be negative");
  return tiles_finalize(d_x, d_tile_of, N, C, S, st, ny, nx, d_out, Ho, Wo, oy, ox, known, mask, y_lo, y_hi, stream);
}
int kd_tiles_rows_copy(const float* d_src, int src_tiles, int src_rows, float* d_dst, int dst_tiles, int dst_rows,
                       const float* d_thr_src, float* d_thr_dst, int n, int C, int S, const int* desc, void* stream) {
  return launch_tiles_rows_copy(d_src, src_tiles, src_rows, d_dst, dst_tiles, dst_rows, d_thr_src, d_thr_dst, n, C, S, desc,
                                (hipStream_t)stream);
}

}  // extern "C"
