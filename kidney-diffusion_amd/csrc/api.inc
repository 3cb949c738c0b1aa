// Sampler loop and the extern "C" entry points declared in include/kd_engine.h.
namespace kd {

// skip_cond: the conditioning ops (kd_unet::op_is_cond) are left out - their outputs were restored from the table
static int run_forward(kd_unet* u, hipStream_t s, bool skip_cond = false) {
  const size_t n = u->ops.size();
  for (size_t i = 0; i < n; ++i) {
    if (skip_cond && u->op_is_cond[i]) continue;
    if (u->ops[i](s)) return 1;
  }
  return 0;
}
static int run_cond_ops(kd_unet* u, hipStream_t s) {
  const size_t n = u->ops.size();
  for (size_t i = 0; i < n; ++i)
    if (u->op_is_cond[i] && u->ops[i](s)) return 1;
  return 0;
}
// step-invariant work (the init conv's share over the cond / low-res planes): once per sampling call
static int run_static(kd_unet* u, hipStream_t s) {
  for (auto& op : u->static_ops)
    if (op(s)) return 1;
  return 0;
}

// cond_scale 0 (zero-initialised struct) and 1 both mean "no guidance"
static inline bool cfg_on(const kd_sample_args_t* a) { return a->cond_scale != 0.0f && a->cond_scale != 1.0f; }

struct SamplerCtx {
  StepTables tb;
  int T, R;
  bool cond_tab = false;   // the iteration restores the conditioning from kd_unet::cond_tab instead of computing it
};

// the sampler scratch both samplers use (UNet output, x0 estimate, thresholds, iteration, seed, quantile workspace)
static int sampler_scratch(kd_unet* u) {
  const int B = u->cfg.batch, S = u->cfg.image_size;
  const size_t img_bytes = (size_t)B * 3 * S * S * sizeof(float);
  if (!u->s_pred) {
    KD_HIP_CHECK(hipMalloc((void**)&u->s_pred, img_bytes));
    KD_HIP_CHECK(hipMalloc((void**)&u->s_x0, img_bytes));
    KD_HIP_CHECK(hipMalloc((void**)&u->s_thresh, (size_t)B * sizeof(float)));
    KD_HIP_CHECK(hipMalloc((void**)&u->s_time, (size_t)B * sizeof(float)));
    KD_HIP_CHECK(hipMalloc((void**)&u->s_iter, sizeof(int)));
    KD_HIP_CHECK(hipMalloc((void**)&u->s_seed, sizeof(uint64_t)));
    KD_HIP_CHECK(hipMalloc(&u->s_qws, quantile_ws_bytes(B)));
  }
  if (u->self_cond && !u->s_sc) {
    KD_HIP_CHECK(hipMalloc((void**)&u->s_sc, img_bytes));
    KD_HIP_CHECK(hipMemset(u->s_sc, 0, img_bytes));
  }
  return 0;
}
// self_cond plans: the carried x0 estimate starts as zeros (the library's self_cond = None) at the first step of a call;
// outside any captured graph
static int self_cond_reset(kd_unet* u, hipStream_t s) {
  if (!u->self_cond) return 0;
  const size_t bytes = (size_t)u->cfg.batch * 3 * u->cfg.image_size * u->cfg.image_size * sizeof(float);
  KD_HIP_CHECK(hipMemsetAsync(u->s_sc, 0, bytes, s));
  return 0;
}

static int sampler_prepare(kd_unet* u, const kd_schedule_t* sc, SamplerCtx& ctx, hipStream_t s) {
  if (sampler_scratch(u)) return 1;
  const int T = sc->T;
  KD_REQUIRE(T >= 1, "schedule must have at least one step");
  if (u->s_tables_cap < T) {
    if (u->s_tables) KD_HIP_CHECK(hipFree(u->s_tables));
    KD_HIP_CHECK(hipMalloc((void**)&u->s_tables, (size_t)9 * T * sizeof(float)));
    u->s_tables_cap = T;
    u->s_tables_host.clear();
    if (u->graph_exec) {  // the captured graph holds the old table pointers
      (void)hipGraphExecDestroy(u->graph_exec);
      u->graph_exec = nullptr;
    }
  }
  const float* src[9] = {sc->log_snr, sc->alpha, sc->sigma, sc->alpha_next, sc->sigma_next,
                         sc->c,       sc->noise_scale, sc->rn_a, sc->rn_b};
  const int cap = u->s_tables_cap;
  // The device tables are keyed on their CONTENT: a sampling call with the schedule of the previous one
  // (every patch of a grid, every k-range of a traced run) uploads nothing.  A changed schedule goes
  // through a pinned staging buffer with ONE asynchronous copy on the caller's stream, so it is ordered
  // behind the launches already queued there that still read the old tables.
  std::vector<float> host((size_t)9 * T, 0.0f);
  for (int i = 0; i < 9; ++i) {
    if (i < 7) KD_REQUIRE(src[i] != nullptr, "schedule arrays log_snr..noise_scale are required");
    if (src[i]) memcpy(host.data() + (size_t)i * T, src[i], (size_t)T * sizeof(float));
  }
  if (host != u->s_tables_host) {
    const size_t need = (size_t)9 * cap;
    // the previous upload may still be reading the staging buffer - on WHICHEVER stream it was issued (the grid
    // scheduler alternates one plan between the caller's stream and its side stream): wait for its event, not for `s`
    if (u->s_tables_ev) KD_HIP_CHECK(hipEventSynchronize(u->s_tables_ev));
    if (u->s_tables_pinned_floats < need) {
      if (u->s_tables_pinned) {
        KD_HIP_CHECK(hipHostFree(u->s_tables_pinned));
        u->s_tables_pinned = nullptr;
      }
      KD_HIP_CHECK(hipHostMalloc((void**)&u->s_tables_pinned, need * sizeof(float), hipHostMallocDefault));
      u->s_tables_pinned_floats = need;
    }
    memset(u->s_tables_pinned, 0, need * sizeof(float));
    for (int i = 0; i < 9; ++i) memcpy(u->s_tables_pinned + (size_t)i * cap, host.data() + (size_t)i * T, (size_t)T * sizeof(float));
    KD_HIP_CHECK(hipMemcpyAsync(u->s_tables, u->s_tables_pinned, need * sizeof(float), hipMemcpyHostToDevice, s));
    if (!u->s_tables_ev) KD_HIP_CHECK(hipEventCreateWithFlags(&u->s_tables_ev, hipEventDisableTiming));
    KD_HIP_CHECK(hipEventRecord(u->s_tables_ev, s));
    u->s_tables_host.swap(host);
  }
  float* t = u->s_tables;
  ctx.tb = StepTables{t, t + cap, t + 2 * cap, t + 3 * cap, t + 4 * cap, t + 5 * cap, t + 6 * cap, t + 7 * cap,
                      t + 8 * cap};
  ctx.T = T;
  return 0;
}

// The time conditioning of a step - sinusoidal embeddings, the two MLP trios, every ResnetBlock's FiLM scale / shift,
// the conditioning tokens and their cross-attention K / V - depends on the schedule index alone when there is no text
// conditioning and every sample carries the same low-res noise level (what Imagen.sample passes: one scalar for the
// batch).  It is then computed ONCE per schedule into a table [T][cond_bytes] and an iteration restores its row with one
// gather instead of 21 launches (SR UNet; ~60 for a batch-1 patch of stage 1) and the 113 MB time-MLP GEMM.  The table is
// keyed on the schedule's content, T and the low-res level, so every patch of a grid and every call of a traced run
// reuse it.  Same kernels on the same inputs: results are bit-identical with the table off (args->cond_table < 0).
// `key`: the content the rows are a function of (the DDPM step tables; the EDM tables for its 2N rows, ctx.tb.log_snr then
// pointing at its time inputs).
static int sampler_cond_table(kd_unet* u, const std::vector<float>& key, const kd_sample_args_t* a, SamplerCtx& ctx,
                              int k_begin, int k_end, hipStream_t s, bool force = false) {
  ctx.cond_tab = false;
  const bool lowres = u->cfg.lowres_cond != 0;
  if (a->cond_table < 0 || u->cond_bytes == 0 || u->cfg.text_tokens > 0 || cfg_on(a)) return 0;
  if (lowres && !a->lowres_log_snr_uniform) return 0;   // per-sample levels: computed in the step, as before
  const size_t need = (size_t)ctx.T * u->cond_bytes;
  const bool same = u->cond_tab != nullptr && u->cond_tab_bytes >= need && u->cond_tab_T == ctx.T &&
                    (int)u->cond_tab_row_ok.size() == ctx.T && u->cond_tab_sched == key &&
                    (!lowres || u->cond_tab_lowres == a->lowres_log_snr_value);
  if (!same) {
    // every row of the old table is stale from here on, whatever happens below
    u->cond_tab_row_ok.clear();
    u->cond_tab_valid = false;
    // Resident-size cap: args->cond_table_max_mb if given, else 4 GiB, and never more than 1/8 of the free HBM
    size_t cap = a->cond_table_max_mb > 0 ? (size_t)a->cond_table_max_mb << 20 : size_t(4) << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) cap = std::min(cap, (free_b + u->cond_tab_bytes) / 8);
    u->cond_tab_refused_bytes = 0;
    if (need > cap) {   // (reported: kd_unet_cond_table_refused_bytes - the launch count and the speed of the step differ)
      u->cond_tab_refused_bytes = (int64_t)need;
      return 0;
    }
    if (u->cond_tab_bytes < need) {
      if (u->cond_tab) {
        KD_HIP_CHECK(hipStreamSynchronize(s));   // (a replay of the old table may still be running)
        u->drop_graphs();   // the captured graphs hold the old table pointer
        KD_HIP_CHECK(hipFree(u->cond_tab));
        u->cond_tab = nullptr;
        u->cond_tab_bytes = 0;
      }
      if (hipMalloc((void**)&u->cond_tab, need) != hipSuccess) {
        (void)hipGetLastError();   // no room for the table: the step computes its conditioning itself
        u->cond_tab = nullptr;
        u->cond_tab_refused_bytes = (int64_t)need;
        return 0;
      }
      u->cond_tab_bytes = need;
    }
    u->cond_tab_sched = key;
    u->cond_tab_T = ctx.T;
    u->cond_tab_lowres = a->lowres_log_snr_value;
    u->cond_tab_row_ok.assign((size_t)ctx.T, 0);
  }
  // Rows are built on demand, for the steps this call walks: a 250-row table costs nothing to a call that runs 20 steps
  // of it, and every later call on the same schedule (every patch of a grid, the next k-range of a traced run) finds
  // its rows there.  B > 1: B schedule steps per run of the conditioning ops (see cond_scatter_kernel).
  const int B = u->cfg.batch;
  const bool rows = B > 1 && u->cond_rows_ok && u->d_cond_segs;
  const int chunk = rows ? B : 1;
  bool any = false;
  for (int k = k_begin; k < k_end && !any; ++k) any = force || !u->cond_tab_row_ok[k];
  if (any) {
    u->in_log_snr = u->s_time;
    u->in_lowres_log_snr = a->d_lowres_log_snr;
    u->in_text_tokens = nullptr;
    u->in_text_hiddens = nullptr;
    // device time of the build: two events recorded here and read when somebody asks (kd_unet_cond_table_build_ms) -
    // the sampling path itself never waits for them (ADVICE r4: a traced run builds rows in every call)
    if (!u->cond_ev0) KD_HIP_CHECK(hipEventCreate(&u->cond_ev0));
    if (!u->cond_ev1) KD_HIP_CHECK(hipEventCreate(&u->cond_ev1));
    u->cond_ev_pending = false;
    KD_HIP_CHECK(hipEventRecord(u->cond_ev0, s));
    int rc = 0, built = 0, runs = 0;
    for (int k0 = (k_begin / chunk) * chunk; k0 < k_end && !rc; k0 += chunk) {
      const int k1 = std::min(k0 + chunk, ctx.T);
      bool need_it = force;
      for (int k = k0; k < k1 && !need_it; ++k) need_it = !u->cond_tab_row_ok[k];
      if (!need_it) continue;
      for (int k = k0; k < k1; ++k) u->cond_tab_row_ok[k] = 0;
      ++runs;
      if (rows) {
        rc = launch_fill_time_rows(ctx.tb.log_snr, k0, ctx.T, u->s_time, B, s);
        if (!rc) rc = run_cond_ops(u, s);
        if (!rc)
          rc = launch_cond_scatter((const float*)u->cond_ws, (float*)u->cond_tab, u->d_cond_segs, (int)u->cond_segs.size(),
                                   u->cond_row_total, B, k0, ctx.T, (int64_t)(u->cond_bytes / 4), s);
      } else {
        rc = launch_iter_set(u->s_iter, k0 * ctx.R, s);
        if (!rc) rc = launch_fill_time(ctx.tb.log_snr, u->s_iter, ctx.R, u->s_time, B, s);
        if (!rc) rc = run_cond_ops(u, s);
        if (!rc && hipMemcpyAsync(u->cond_tab + (size_t)k0 * u->cond_bytes, u->cond_ws, u->cond_bytes, hipMemcpyDeviceToDevice,
                                  s) != hipSuccess) {
          set_error("cond table: device copy failed");
          rc = 1;
        }
      }
      if (!rc)
        for (int k = k0; k < k1; ++k) u->cond_tab_row_ok[k] = 1, ++built;
    }
    if (!rc && hipEventRecord(u->cond_ev1, s) == hipSuccess) {
      u->cond_ev_pending = true;
      u->cond_tab_build_rows = built;
      u->cond_tab_build_runs = runs;
    }
    if (rc) return 1;
  }
  u->cond_tab_valid = true;
  ctx.cond_tab = true;
  return 0;
}

static int emit_iteration(kd_unet* u, const SamplerCtx& ctx, const kd_sample_args_t* a, float* d_img,
                          hipStream_t s) {
  const int B = u->cfg.batch, S = u->cfg.image_size, R = ctx.R;
  const int64_t hw = (int64_t)S * S, per = 3 * hw;
  const bool inpaint = a->d_inpaint_images != nullptr;
  if (inpaint)
    if (launch_inpaint_mix(d_img, a->d_inpaint_images, a->d_inpaint_masks, a->d_noise_inpaint, B * per, u->s_seed,
                           ctx.tb, u->s_iter, R, B, 3, hw, s))
      return 1;
  if (launch_fill_time(ctx.tb.log_snr, u->s_iter, R, u->s_time, B, s)) return 1;
  u->in_x = d_img;
  u->in_lowres = a->d_lowres;
  u->in_cond = a->d_cond_images;
  u->in_log_snr = u->s_time;
  u->in_lowres_log_snr = a->d_lowres_log_snr;
  u->in_text_tokens = a->d_text_tokens;
  u->in_text_hiddens = a->d_text_hiddens;
  u->in_self_cond = u->s_sc;   // (nullptr unless self_cond; both guidance forwards read the same estimate)
  u->out = u->s_pred;
  if (ctx.cond_tab)
    if (launch_cond_gather(u->cond_tab, u->cond_ws, u->cond_bytes, u->s_iter, R, s)) return 1;
  if (run_forward(u, s, ctx.cond_tab)) return 1;
  if (cfg_on(a)) {  // classifier-free guidance: second forward on the null conditioning
    u->in_text_tokens = a->d_null_text_tokens;
    u->in_text_hiddens = a->d_null_text_hiddens;
    u->out = u->s_pred_null;
    if (run_forward(u, s)) return 1;
    if (launch_cfg_combine(u->s_pred, u->s_pred_null, u->s_pred, a->cond_scale, B * per, s)) return 1;
  }
  if (launch_x0(d_img, u->s_pred, u->s_x0, ctx.tb, u->s_iter, R, a->objective, B * per, s)) return 1;
  if (a->dynamic_threshold)
    if (launch_quantile_abs(u->s_x0, u->s_thresh, B, per, a->percentile, u->s_qws, s)) return 1;
  if (launch_ddpm_update(d_img, u->s_x0, u->s_thresh, a->d_noise_step, B * per, u->s_seed, ctx.tb, u->s_iter, R,
                         a->dynamic_threshold, B, per, s, u->s_sc))
    return 1;
  if (inpaint && R > 1)
    if (launch_renoise(d_img, a->d_noise_renoise, B * per, u->s_seed, ctx.tb, u->s_iter, R, ctx.T, B, per, s))
      return 1;
  return launch_iter_inc(u->s_iter, s);
}

static std::vector<uint64_t> graph_key_of(const kd_sample_args_t* a, const float* d_img, int T, int R, bool cond_tab) {
  auto p = [](const void* x) { return (uint64_t)(uintptr_t)x; };
  uint64_t pct;
  float f = a->percentile;
  memcpy(&pct, &f, sizeof(float));
  return {p(d_img), p(a->d_lowres), p(a->d_lowres_log_snr), p(a->d_cond_images), p(a->d_text_tokens),
          p(a->d_text_hiddens), p(a->d_inpaint_images), p(a->d_inpaint_masks), p(a->d_noise_step),
          p(a->d_noise_inpaint), p(a->d_noise_renoise), (uint64_t)a->objective,
          (uint64_t)a->dynamic_threshold, pct & 0xFFFFFFFFull, (uint64_t)T, (uint64_t)R,
          p(a->d_null_text_tokens), p(a->d_null_text_hiddens), (uint64_t)(a->cond_scale * 65536.0f),
          (uint64_t)cond_tab};
}

static int sample_steps(kd_unet* u, const kd_schedule_t* sc, const kd_sample_args_t* a, float* d_img, int k_begin,
                        int k_end, hipStream_t s) {
  KD_REQUIRE(u && sc && a && d_img, "null argument");
  KD_REQUIRE((a->d_inpaint_images == nullptr) == (a->d_inpaint_masks == nullptr),
             "inpaint_images and inpaint_masks must be given together");
  KD_REQUIRE(a->objective >= 0 && a->objective <= 2, "unknown prediction objective");
  SamplerCtx ctx;
  ctx.R = a->d_inpaint_images ? (a->resample_times < 1 ? 1 : a->resample_times) : 1;
  if (sampler_prepare(u, sc, ctx, s)) return 1;
  if (cfg_on(a)) {
    KD_REQUIRE(a->d_null_text_tokens && a->d_null_text_hiddens && a->d_text_tokens && a->d_text_hiddens,
               "cond_scale != 1 needs the conditional and the null text conditioning");
    if (!u->s_pred_null)
      KD_HIP_CHECK(hipMalloc((void**)&u->s_pred_null,
                             (size_t)u->cfg.batch * 3 * u->cfg.image_size * u->cfg.image_size * sizeof(float)));
  }
  KD_REQUIRE(0 <= k_begin && k_begin <= k_end && k_end <= ctx.T, "step range out of bounds");
  if (ctx.R > 1) KD_REQUIRE(sc->rn_a && sc->rn_b, "re-noise tables are required when resampling");
  const int n_iter = (k_end - k_begin) * ctx.R;
  if (k_begin == 0 && self_cond_reset(u, s)) return 1;   // k_begin > 0 continues from what the plan holds
  if (launch_iter_set(u->s_iter, k_begin * ctx.R, s)) return 1;
  if (launch_seed_set(u->s_seed, a->seed, s)) return 1;
  u->in_lowres = a->d_lowres;
  u->in_cond = a->d_cond_images;
  if (run_static(u, s)) return 1;  // conditioning planes are constant over the loop
  if (sampler_cond_table(u, u->s_tables_host, a, ctx, k_begin, k_end, s)) return 1;
  if (launch_iter_set(u->s_iter, k_begin * ctx.R, s)) return 1;
  if (!a->use_graph) {
    for (int i = 0; i < n_iter; ++i)
      if (emit_iteration(u, ctx, a, d_img, s)) return 1;
    return 0;
  }
  std::vector<uint64_t> key = graph_key_of(a, d_img, ctx.T, ctx.R, ctx.cond_tab);
  if (!u->graph_exec || key != u->graph_key) {
    if (u->graph_exec) {
      (void)hipGraphExecDestroy(u->graph_exec);
      u->graph_exec = nullptr;
    }
    // Capture on an engine-owned stream (the caller's may be the legacy null stream, which cannot be
    // captured); capturing only records the launches, the graph itself is launched on `s`.
    if (!u->cap_stream) KD_HIP_CHECK(hipStreamCreateWithFlags(&u->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    KD_HIP_CHECK(hipStreamBeginCapture(u->cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = emit_iteration(u, ctx, a, d_img, u->cap_stream);
    hipError_t e = hipStreamEndCapture(u->cap_stream, &graph);
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return 1;
    }
    if (e != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      KD_HIP_CHECK(e);
    }
    e = hipGraphInstantiate(&u->graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) u->graph_exec = nullptr;
    KD_HIP_CHECK(e);
    u->graph_key = key;
  }
  for (int i = 0; i < n_iter; ++i) KD_HIP_CHECK(hipGraphLaunch(u->graph_exec, s));
  return 0;
}


// ------------------------------------------------------------------------------ EDM Heun sampler
// Per-step tables of kd_edm_schedule_t -> u->e_tables [16][N] (stride N, so that c_noise_hat and c_noise_next form one
// [2N] time table for the conditioning table).  Content-keyed: an unchanged schedule uploads nothing.
static const int EDM_NTAB = 15;
static int edm_prepare(kd_unet* u, const kd_edm_schedule_t* sc, EdmTables& tb, hipStream_t s) {
  const int B = u->cfg.batch, S = u->cfg.image_size;
  const size_t img_bytes = (size_t)B * 3 * S * S * sizeof(float);
  const int N = sc->N;
  KD_REQUIRE(N >= 1, "EDM schedule must have at least one step");
  const float* src[EDM_NTAB] = {sc->sigma,      sc->sigma_hat,  sc->sigma_next, sc->churn,       sc->euler_step,
                                sc->heun_step,  sc->renoise,    sc->c_in_hat,   sc->c_skip_hat,  sc->c_out_hat,
                                sc->c_in_next,  sc->c_skip_next, sc->c_out_next, sc->c_noise_hat, sc->c_noise_next};
  std::vector<float> host((size_t)EDM_NTAB * N + 1);
  for (int i = 0; i < EDM_NTAB; ++i) {
    KD_REQUIRE(src[i] != nullptr, "every array of kd_edm_schedule_t is required");
    memcpy(host.data() + (size_t)i * N, src[i], (size_t)N * sizeof(float));
  }
  host[(size_t)EDM_NTAB * N] = sc->S_noise;   // (part of the key only)
  for (int k = 0; k + 1 < N; ++k)   // the Heun kernel re-noises by step index: only the last step may skip the correction
    KD_REQUIRE(src[2][k] != 0.0f, "EDM schedule: sigma_next == 0 before the last step");
  if (!u->e_xhat) {
    KD_HIP_CHECK(hipMalloc((void**)&u->e_xhat, img_bytes));
    KD_HIP_CHECK(hipMalloc((void**)&u->e_d, img_bytes));
    KD_HIP_CHECK(hipMalloc((void**)&u->e_in, img_bytes));
  }
  const int need = EDM_NTAB * N;
  if (host != u->e_tables_host) {
    if (u->e_tables_ev) KD_HIP_CHECK(hipEventSynchronize(u->e_tables_ev));   // the staging buffer's last upload
    if (u->e_tables_cap < need) {   // (graphs captured on the old tables are re-captured: their key holds the address)
      KD_HIP_CHECK(hipStreamSynchronize(s));   // replays on `s` may still read the old tables
      if (u->e_tables) KD_HIP_CHECK(hipFree(u->e_tables));
      if (u->e_tables_pinned) KD_HIP_CHECK(hipHostFree(u->e_tables_pinned));
      u->e_tables = nullptr;
      u->e_tables_pinned = nullptr;
      u->e_tables_cap = 0;
      KD_HIP_CHECK(hipMalloc((void**)&u->e_tables, (size_t)need * sizeof(float)));
      KD_HIP_CHECK(hipHostMalloc((void**)&u->e_tables_pinned, (size_t)need * sizeof(float), hipHostMallocDefault));
      u->e_tables_cap = need;
    }
    memcpy(u->e_tables_pinned, host.data(), (size_t)need * sizeof(float));
    KD_HIP_CHECK(hipMemcpyAsync(u->e_tables, u->e_tables_pinned, (size_t)need * sizeof(float), hipMemcpyHostToDevice, s));
    if (!u->e_tables_ev) KD_HIP_CHECK(hipEventCreateWithFlags(&u->e_tables_ev, hipEventDisableTiming));
    KD_HIP_CHECK(hipEventRecord(u->e_tables_ev, s));
    u->e_tables_host.swap(host);
  }
  const float* t = u->e_tables;
  const float** dst[EDM_NTAB] = {&tb.sigma,     &tb.sigma_hat,   &tb.sigma_next, &tb.churn,       &tb.euler_step,
                                 &tb.heun_step, &tb.renoise,     &tb.c_in_hat,   &tb.c_skip_hat,  &tb.c_out_hat,
                                 &tb.c_in_next, &tb.c_skip_next, &tb.c_out_next, &tb.c_noise_hat, &tb.c_noise_next};
  for (int i = 0; i < EDM_NTAB; ++i) *dst[i] = t + (size_t)i * N;
  return 0;
}

// UNet forward j of the step (0: at sigma_hat, 1: at sigma_next) on u->e_in -> s_pred (+ the guidance forward), then
// den = c_skip x + c_out net -> s_x0 and its per-sample quantile -> s_thresh
static int edm_forward(kd_unet* u, const SamplerCtx& ctx, const EdmTables& tb, const kd_sample_args_t* a, const float* x,
                       int j, hipStream_t s) {
  const int B = u->cfg.batch, S = u->cfg.image_size, R = ctx.R, N = ctx.T / 2;
  const int64_t per = (int64_t)3 * S * S;
  if (launch_fill_time(j ? tb.c_noise_next : tb.c_noise_hat, u->s_iter, R, u->s_time, B, s)) return 1;
  u->in_x = u->e_in;
  u->in_lowres = a->d_lowres;
  u->in_cond = a->d_cond_images;
  u->in_log_snr = u->s_time;
  u->in_lowres_log_snr = a->d_lowres_log_snr;
  u->in_text_tokens = a->d_text_tokens;
  u->in_text_hiddens = a->d_text_hiddens;
  u->in_self_cond = u->s_sc;
  u->out = u->s_pred;
  if (ctx.cond_tab)   // rows [0, N): time input at sigma_hat, [N, 2N): at sigma_next
    if (launch_cond_gather(u->cond_tab + (size_t)j * N * u->cond_bytes, u->cond_ws, u->cond_bytes, u->s_iter, R, s))
      return 1;
  if (run_forward(u, s, ctx.cond_tab)) return 1;
  if (cfg_on(a)) {
    u->in_text_tokens = a->d_null_text_tokens;
    u->in_text_hiddens = a->d_null_text_hiddens;
    u->out = u->s_pred_null;
    if (run_forward(u, s)) return 1;
    if (launch_cfg_combine(u->s_pred, u->s_pred_null, u->s_pred, a->cond_scale, B * per, s)) return 1;
  }
  if (launch_edm_precond_out(x, u->s_pred, u->s_x0, j ? tb.c_skip_next : tb.c_skip_hat, j ? tb.c_out_next : tb.c_out_hat,
                             u->s_iter, R, B * per, s))
    return 1;
  if (a->dynamic_threshold)
    if (launch_quantile_abs(u->s_x0, u->s_thresh, B, per, a->percentile, u->s_qws, s)) return 1;
  return 0;
}

// One EDM iteration: churn, forward at sigma_hat, Euler; with `heun` the forward at sigma_next and the correction
// (+ re-noise).  Everything on `s`, in order: no side streams (a captured graph with parallel branches can crash the
// runtime's replay).
static int emit_edm_iteration(kd_unet* u, const SamplerCtx& ctx, const EdmTables& tb, float s_noise,
                              const kd_sample_args_t* a, float* d_img, bool heun, hipStream_t s) {
  const int B = u->cfg.batch, S = u->cfg.image_size, R = ctx.R, N = ctx.T / 2;
  const int64_t hw = (int64_t)S * S, per = 3 * hw;
  const bool inpaint = a->d_inpaint_images != nullptr;
  if (launch_edm_churn(d_img, u->e_xhat, u->e_in, a->d_inpaint_images, a->d_inpaint_masks, a->d_noise_step, B * per,
                       u->s_seed, tb, s_noise, u->s_iter, R, B, 3, hw, s))
    return 1;
  if (edm_forward(u, ctx, tb, a, u->e_xhat, 0, s)) return 1;
  // self_cond: Euler leaves the first forward's thresholded estimate for the Heun forward (and, on the last step, for
  // the caller); Heun leaves the second's for the next step
  if (launch_edm_euler(u->e_xhat, u->s_x0, u->s_thresh, u->e_d, d_img, u->e_in, tb, u->s_iter, R, a->dynamic_threshold, B,
                       per, s, u->s_sc))
    return 1;
  if (heun) {
    if (edm_forward(u, ctx, tb, a, d_img, 1, s)) return 1;
    if (launch_edm_heun(d_img, u->e_xhat, u->e_d, u->s_x0, u->s_thresh, a->d_noise_renoise, B * per, u->s_seed, tb,
                        u->s_iter, R, N, inpaint && R > 1, a->dynamic_threshold, B, per, s, u->s_sc))
      return 1;
  }
  return launch_iter_inc(u->s_iter, s);
}

static int edm_sample_steps(kd_unet* u, const kd_edm_schedule_t* sc, const kd_sample_args_t* a, float* d_img, int k_begin,
                            int k_end, hipStream_t s) {
  KD_REQUIRE(u && sc && a && d_img, "null argument");
  KD_REQUIRE((a->d_inpaint_images == nullptr) == (a->d_inpaint_masks == nullptr),
             "inpaint_images and inpaint_masks must be given together");
  SamplerCtx ctx;
  ctx.R = a->d_inpaint_images ? (a->resample_times < 1 ? 1 : a->resample_times) : 1;
  if (sampler_scratch(u)) return 1;
  EdmTables tb{};
  if (edm_prepare(u, sc, tb, s)) return 1;
  const int N = sc->N;
  ctx.T = 2 * N;   // rows of the conditioning table; its time inputs: c_noise_hat | c_noise_next
  ctx.tb = StepTables{};
  ctx.tb.log_snr = tb.c_noise_hat;
  if (cfg_on(a)) {
    KD_REQUIRE(a->d_null_text_tokens && a->d_null_text_hiddens && a->d_text_tokens && a->d_text_hiddens,
               "cond_scale != 1 needs the conditional and the null text conditioning");
    if (!u->s_pred_null)
      KD_HIP_CHECK(hipMalloc((void**)&u->s_pred_null,
                             (size_t)u->cfg.batch * 3 * u->cfg.image_size * u->cfg.image_size * sizeof(float)));
  }
  KD_REQUIRE(0 <= k_begin && k_begin <= k_end && k_end <= N, "step range out of bounds");
  if (k_begin == 0 && self_cond_reset(u, s)) return 1;
  if (launch_seed_set(u->s_seed, a->seed, s)) return 1;
  u->in_lowres = a->d_lowres;
  u->in_cond = a->d_cond_images;
  if (run_static(u, s)) return 1;
  // rows k of both halves for the steps walked (the rows in between come along; each row is built once per schedule)
  if (sampler_cond_table(u, u->e_tables_host, a, ctx, k_begin, k_end > k_begin ? N + k_end : k_begin, s)) return 1;
  if (launch_iter_set(u->s_iter, k_begin * ctx.R, s)) return 1;
  for (int k = k_begin; k < k_end; ++k) {
    const bool heun = sc->sigma_next[k] != 0.0f;
    if (!a->use_graph) {
      for (int r = 0; r < ctx.R; ++r)
        if (emit_edm_iteration(u, ctx, tb, sc->S_noise, a, d_img, heun, s)) return 1;
      continue;
    }
    const int g = heun ? 0 : 1;
    std::vector<uint64_t> key = graph_key_of(a, d_img, ctx.T, ctx.R, ctx.cond_tab);
    uint32_t sn_bits;
    memcpy(&sn_bits, &sc->S_noise, sizeof(float));
    key.push_back((uint64_t)(uintptr_t)u->e_tables);   // (the stride N of the tables is in the key as T = 2N)
    key.push_back(sn_bits);
    if (!u->e_graph[g] || key != u->e_graph_key[g]) {
      if (u->e_graph[g]) {
        (void)hipGraphExecDestroy(u->e_graph[g]);
        u->e_graph[g] = nullptr;
      }
      // captured on the engine-owned stream (one stream, no forks), replayed on `s`
      if (!u->cap_stream) KD_HIP_CHECK(hipStreamCreateWithFlags(&u->cap_stream, hipStreamNonBlocking));
      hipGraph_t graph = nullptr;
      KD_HIP_CHECK(hipStreamBeginCapture(u->cap_stream, hipStreamCaptureModeThreadLocal));
      int rc = emit_edm_iteration(u, ctx, tb, sc->S_noise, a, d_img, heun, u->cap_stream);
      hipError_t e = hipStreamEndCapture(u->cap_stream, &graph);
      if (rc || e != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        if (rc) return 1;
        KD_HIP_CHECK(e);
      }
      e = hipGraphInstantiate(&u->e_graph[g], graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (e != hipSuccess) u->e_graph[g] = nullptr;
      KD_HIP_CHECK(e);
      u->e_graph_key[g] = key;
    }
    for (int r = 0; r < ctx.R; ++r) KD_HIP_CHECK(hipGraphLaunch(u->e_graph[g], s));
  }
  return 0;
}

}  // namespace kd

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
  // plans of one UNet (other batch / image size) share its packed weights
  u->wstore = share_with ? share_with->wstore : std::make_shared<WeightStore>();
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
      bt.to_text = true;
      bt.cond_hoist = false;
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
  return u ? (int64_t)(u->ws_bytes + u->cond_bytes + u->cond_tab_bytes + u->wstore->pool.total) : 0;
}
int64_t kd_unet_weight_bytes(const kd_unet_t* u) { return u ? (int64_t)u->wstore->pool.total : 0; }
int64_t kd_unet_macs(const kd_unet_t* u) { return u ? u->macs : 0; }
int64_t kd_unet_mfma_macs(const kd_unet_t* u) { return u ? u->mfma_macs : 0; }
int64_t kd_unet_mfma_bf16_macs(const kd_unet_t* u) { return u ? u->mfma_bf16_macs : 0; }
int kd_unet_num_launches(const kd_unet_t* u) { return u ? (int)u->ops.size() : 0; }
float kd_unet_cond_table_build_ms(kd_unet_t* u, int* rows, int* runs) {
  if (rows) *rows = u ? u->cond_tab_build_rows : 0;
  if (runs) *runs = u ? u->cond_tab_build_runs : 0;
  if (u && u->cond_ev_pending) {   // the events of the last build: read here, never on the sampling path
    u->cond_ev_pending = false;
    float ms = -1.f;
    if (hipEventSynchronize(u->cond_ev1) == hipSuccess && hipEventElapsedTime(&ms, u->cond_ev0, u->cond_ev1) == hipSuccess)
      u->cond_tab_build_ms = ms;
    else
      (void)hipGetLastError();
  }
  return u ? u->cond_tab_build_ms : -1.f;
}
int64_t kd_unet_cond_table_refused_bytes(const kd_unet_t* u) { return u ? u->cond_tab_refused_bytes : 0; }
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
  u->in_x = d_x;
  u->in_lowres = d_lowres;
  u->in_cond = d_cond_images;
  u->in_log_snr = d_log_snr;
  u->in_lowres_log_snr = d_lowres_log_snr;
  u->in_text_tokens = d_text_tokens;
  u->in_text_hiddens = d_text_hiddens;
  u->in_self_cond = d_self_cond;   // (a plan without self_cond ignores it, as the library does)
  u->out = d_out;
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
  KD_REQUIRE(u && sched && args, "null argument");
  hipStream_t s = (hipStream_t)stream;
  SamplerCtx ctx;
  ctx.R = args->d_inpaint_images ? (args->resample_times < 1 ? 1 : args->resample_times) : 1;
  if (sampler_prepare(u, sched, ctx, s)) return 1;
  KD_REQUIRE(0 <= k_begin && k_begin <= k_end && k_end <= ctx.T, "step range out of bounds");
  u->cond_tab_build_rows = 0;
  if (sampler_cond_table(u, u->s_tables_host, args, ctx, k_begin, k_end, s, force != 0)) return 1;
  if (built) *built = ctx.cond_tab ? u->cond_tab_build_rows : 0;
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
// v-hat, after guidance) [B,3,S,S]; 1 the x0 estimate BEFORE the threshold clamp [B,3,S,S]; 2 the per-sample
// dynamic thresholds max(1, quantile) [B].  Stream-ordered device-to-device copy (parity checks: bench.py, tests).
int kd_sample_last(kd_unet_t* u, int which, float* d_out, void* stream) {
  if (!u || !d_out) {
    set_error("kd_sample_last: null argument");
    return 1;
  }
  KD_REQUIRE(u->s_pred, "kd_sample_last: no sampling step has run on this plan");
  KD_REQUIRE(which >= 0 && which <= 5,
             "kd_sample_last: which must be 0 (pred), 1 (x0), 2 (thresholds), 3 / 4 (EDM x_hat / d), 5 (self-cond planes)");
  KD_REQUIRE(which <= 2 || which == 5 || u->e_xhat, "kd_sample_last: no EDM step has run on this plan");
  KD_REQUIRE(which != 5 || u->s_sc, "kd_sample_last: which = 5 needs a plan with self_cond");
  const int B = u->cfg.batch, S = u->cfg.image_size;
  const float* src = which == 0 ? u->s_pred : which == 1 ? u->s_x0 : which == 2 ? u->s_thresh : which == 3 ? u->e_xhat
                   : which == 4 ? u->e_d : u->s_sc;
  const size_t bytes = (which == 2 ? (size_t)B : (size_t)B * 3 * S * S) * sizeof(float);
  KD_HIP_CHECK(hipMemcpyAsync(d_out, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// Seeds the self-conditioning estimate a self_cond plan carries (d_x_start [B,3,S,S], NULL = zeros), so that
// kd_sample_steps / kd_edm_sample_steps with k_begin > 0 continue from a chosen state.  Stream-ordered.
int kd_sample_set_self_cond(kd_unet_t* u, const float* d_x_start, void* stream) {
  if (!u) {
    set_error("kd_sample_set_self_cond: null argument");
    return 1;
  }
  KD_REQUIRE(u->self_cond, "kd_sample_set_self_cond: the plan was created without self_cond");
  if (sampler_scratch(u)) return 1;
  const size_t bytes = (size_t)u->cfg.batch * 3 * u->cfg.image_size * u->cfg.image_size * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  if (d_x_start)
    KD_HIP_CHECK(hipMemcpyAsync(u->s_sc, d_x_start, bytes, hipMemcpyDeviceToDevice, s));
  else
    KD_HIP_CHECK(hipMemsetAsync(u->s_sc, 0, bytes, s));
  return 0;
}

int kd_sample_finalize(kd_unet_t* u, const kd_sample_args_t* args, float* d_img, void* stream) {
  if (!u || !args || !d_img) {
    set_error("kd_sample_finalize: null argument");
    return 1;
  }
  return launch_finalize(d_img, args->d_inpaint_images, args->d_inpaint_masks, u->cfg.batch, 3,
                         (int64_t)u->cfg.image_size * u->cfg.image_size, (hipStream_t)stream);
}

// ---- single-kernel entry points (tests)
// act bit 8 (0x100) selects the row-run K layout used for the small-Cin init convs
int kd_conv2d_nhwc(const float* d_x, const float* d_w_oihw, const float* d_bias, float* d_y, int B, int Hi, int Wi,
                   int Cin, int Cout, int KH, int KW, int stride, int pad, int act, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool rowrun = (act & 0x100) != 0;
  const bool pixshuf = (act & 0x200) != 0;   // 1x1 conv + PixelShuffle(2): d_y is [B, 2 Ho, 2 Wo, Cout / 4]
  act &= 0xff;
  KD_REQUIRE(!pixshuf || (KH == 1 && KW == 1 && Cout % 4 == 0 && !rowrun), "pixel-shuffle test path: 1x1 conv, Cout % 4 == 0");
  float *wp = nullptr, *part = nullptr, *bp = nullptr;
  KD_HIP_CHECK(hipMalloc((void**)&wp, (size_t)Cout * Cin * KH * KW * sizeof(float)));
  if (pixshuf) KD_HIP_CHECK(hipMalloc((void**)&bp, (size_t)Cout * sizeof(float)));
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
    const int ks = conv_ksplit(p);  // small-M shapes take the split-K path, as in the plan
    if (ks > 1) KD_HIP_CHECK(hipMalloc((void**)&part, (size_t)ks * B * p.Ho * p.Wo * Cout * sizeof(float)));
    p.partial = part;
    rc = launch_conv_igemm(p, s);
  }
  hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(wp);
  if (part) (void)hipFree(part);
  if (bp) (void)hipFree(bp);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
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
  float *U = nullptr, *V = nullptr, *D = nullptr;
  KD_HIP_CHECK(hipMalloc((void**)&U, (size_t)16 * Cout * Cin * sizeof(float)));
  KD_HIP_CHECK(hipMalloc((void**)&V, (size_t)16 * Mt * Cin * sizeof(float)));
  KD_HIP_CHECK(hipMalloc((void**)&D, (size_t)16 * Mt * Cout * sizeof(float)));
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
    rc = launch_conv_igemm(p, s);
  }
  if (!rc) rc = launch_wino_out(D, d_bias, nullptr, 0, d_y, B, H, W, Cout, 0, Mt, s);
  hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(U);
  (void)hipFree(V);
  (void)hipFree(D);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
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
  struct Bufs {
    std::vector<void*> p;
    ~Bufs() {
      for (void* q : p) (void)hipFree(q);
    }
    int get(void** out, size_t bytes) {
      KD_HIP_CHECK(hipMalloc(out, bytes));
      p.push_back(*out);
      return 0;
    }
  } bufs;
  float *U = nullptr, *V = nullptr, *D = nullptr;
  double* seg = nullptr;
  if (bufs.get((void**)&U, (size_t)36 * Cout * Cin * sizeof(float))) return 1;
  void* U3 = nullptr;
  if (bufs.get((void**)&V, (size_t)36 * Mt * Cin * (gemm_bf16x3 == 1 ? 6 : sizeof(float)))) return 1;
  if (bufs.get((void**)&D, (size_t)36 * Mt * Cout * sizeof(float))) return 1;
  void* x3ws = nullptr;
  if (gemm_bf16x3 && bufs.get(&U3, (size_t)36 * Cout * Cin * 6)) return 1;
  if (gemm_bf16x3 && bufs.get(&x3ws, gemm_bf16x3_workspace_bytes())) return 1;
  if (gemm_bf16x3) KD_HIP_CHECK(hipMemsetAsync(x3ws, 0, gemm_bf16x3_workspace_bytes(), s));
  const int nchunk = (H / 4) * (W / 4);
  if (d_out_stats)
    if (bufs.get((void**)&seg, (size_t)B * (Cout / 16) * nchunk * 2 * sizeof(double))) return 1;
  int rc = launch_wino4_pack(d_w_oihw, U, Cout, Cin, s);
  if (!rc && gemm_bf16x3) {
    rc = launch_split3(U, U3, 36, Cout, Cin, s);
    if (!rc && gemm_bf16x3 == 1) rc = launch_wino4_in3(d_x, Cin, nullptr, nullptr, nullptr, nullptr, 0, V, B, H, W, Cin, 1, s);
    if (!rc && gemm_bf16x3 != 1) rc = launch_wino4_in(d_x, Cin, nullptr, nullptr, nullptr, nullptr, 0, V, B, H, W, Cin, 1, s);
    if (!rc) rc = launch_gemm_bf16x3(V, U3, D, 36, (int)Mt, Cout, Cin, x3ws, s, gemm_bf16x3 != 1);
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
    rc = launch_conv_igemm(p, s);
  }
  if (!rc) rc = launch_wino4_out(D, d_bias, d_res, Cout, d_y, Cout, seg, B, H, W, Cout, s);
  if (!rc && seg)   // the 16-channel segments of a group are adjacent: [B][G][(Cout / G / 16) nchunk][2]
    rc = launch_gn_finalize(seg, d_out_stats, (Cout / G / 16) * nchunk, B, G, (double)H * W * (Cout / G), eps, s);
  hipError_t e = hipStreamSynchronize(s);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
}

int kd_gemm_bf16x3(const float* d_a, const float* d_b, float* d_c, int G, int M, int N, int K, int a_planes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(gemm_bf16x3_ok(G, M, N, K), "kd_gemm_bf16x3 needs M % 256 == 0, N % 128 == 0, K % 32 == 0, operand planes < 4 GB");
  void *A3 = nullptr, *B3 = nullptr, *ws = nullptr;
  hipError_t e = hipMalloc(&B3, (size_t)G * N * K * 6);
  if (e == hipSuccess && a_planes) e = hipMalloc(&A3, (size_t)G * M * K * 6);   // (a_planes == 0: the loader waves split A)
  if (e == hipSuccess) e = hipMalloc(&ws, gemm_bf16x3_workspace_bytes());   // slabs of the left-over tiles' k-parts
  int rc = e != hipSuccess;
  if (!rc && a_planes) rc = launch_split3(d_a, A3, G, M, K, s);
  if (!rc) rc = launch_split3(d_b, B3, G, N, K, s);
  if (!rc) rc = launch_gemm_bf16x3(a_planes ? A3 : (const void*)d_a, B3, d_c, G, M, N, K, ws, s, !a_planes);
  hipError_t es = hipStreamSynchronize(s);
  (void)hipFree(A3);
  (void)hipFree(B3);
  (void)hipFree(ws);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  KD_HIP_CHECK(es);
  return 0;
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
  KD_REQUIRE(H > 0 && W > 0 && !(H & 1) && !(W & 1) && M < 0x7fffffff && gemm_bf16x3_epi_ok(M, O, K, e),
             "kd_downsample_bf16x3 needs even map sides, C % 16 == 0, B (H/2) (W/2) % 256 == 0, O % 128 == 0");
  // torch weight [O][4 C] with k = c 4 + tap  ->  [tap][O][C] (launch_pack_unshuffle)  ->  [O][tap C + c]  ->  planes
  float *wt = nullptr, *wk = nullptr;
  void *W3 = nullptr, *ws = nullptr;
  hipError_t er = hipMalloc((void**)&wt, (size_t)O * K * 4);
  if (er == hipSuccess) er = hipMalloc((void**)&wk, (size_t)O * K * 4);
  if (er == hipSuccess) er = hipMalloc(&W3, (size_t)O * K * 6);
  if (er == hipSuccess) er = hipMalloc(&ws, gemm_bf16x3_workspace_bytes());
  int rc = er != hipSuccess;
  if (!rc) rc = launch_pack_unshuffle(d_w, wt, O, C, s);
  for (int t = 0; t < 4 && !rc; ++t) rc = launch_copy_scale_rows(wt + (size_t)t * O * C, C, wk + (size_t)t * C, K, C, 1.0f, O, s);
  if (!rc) rc = launch_split3(wk, W3, 1, O, K, s);
  if (!rc) rc = launch_gemm_bf16x3(d_x, W3, d_y, 1, (int)M, O, K, ws, s, true, true, &e);
  hipError_t es = hipStreamSynchronize(s);
  (void)hipFree(wt);
  (void)hipFree(wk);
  (void)hipFree(W3);
  (void)hipFree(ws);
  if (rc) return rc;
  KD_HIP_CHECK(er);
  KD_HIP_CHECK(es);
  return 0;
}

int kd_linear_bf16x3_seg_rows(int M, int N, int K) { return gemm_bf16x3_ok(1, M, N, K) ? gemm_bf16x3_seg_rows(M, N, K) : 0; }

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
  KD_REQUIRE(gemm_bf16x3_epi_ok(M, N, K, e), "kd_linear_bf16x3 needs M % 256 == 0, N % 128 == 0, K % 32 == 0, row strides >= the "
                                             "rows, hw % 256 == 0 under a gate");
  void *W3 = nullptr, *ws = nullptr;
  hipError_t er = hipMalloc(&W3, (size_t)N * K * 6);
  if (er == hipSuccess) er = hipMalloc(&ws, gemm_bf16x3_workspace_bytes());
  int rc = er != hipSuccess;
  if (!rc) rc = launch_split3(d_w, W3, 1, N, K, s);
  if (!rc) rc = launch_gemm_bf16x3(d_x, W3, d_y, 1, M, N, K, ws, s, true, true, &e);
  hipError_t es = hipStreamSynchronize(s);
  (void)hipFree(W3);
  (void)hipFree(ws);
  if (rc) return rc;
  KD_HIP_CHECK(er);
  KD_HIP_CHECK(es);
  return 0;
}

int kd_gn_conv3x3_winograd_fused_nhwc(const float* d_x, const float* d_gamma, const float* d_beta,
                                      const float* d_scale_shift, const float* d_w_oihw, const float* d_bias,
                                      const float* d_res, float* d_y, int B, int H, int W, int Cin, int Cout, int G,
                                      float eps, float* d_out_stats, int ldx, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (ldx <= 0) ldx = Cin;
  // every shape check BEFORE the first allocation; the buffers live in one holder that frees them on every path
  KD_REQUIRE(wino_fused128_ok(B, H, W, Cin, Cout) && G > 0 && Cin % G == 0,
             "GroupNorm-fused Winograd path needs H % 8 == 0, W % 16 == 0, Cin % 4 == 0, Cin <= 2048, Cout % 128 == 0");
  KD_REQUIRE(ldx >= Cin && ldx % 4 == 0, "GroupNorm-fused Winograd path: input row stride must be >= Cin and a multiple of 4");
  KD_REQUIRE(!d_out_stats || (Cout % G == 0 && (Cout / G) % 16 == 0), "output statistics need (Cout / G) % 16 == 0");
  struct Bufs {
    std::vector<void*> p;
    ~Bufs() {
      for (void* q : p) (void)hipFree(q);
    }
    int get(void** out, size_t bytes) {
      KD_HIP_CHECK(hipMalloc(out, bytes));
      p.push_back(*out);
      return 0;
    }
  } bufs;
  float *U = nullptr, *stats = nullptr, *ab = nullptr;
  double* partial = nullptr;
  if (bufs.get((void**)&U, (size_t)16 * Cout * Cin * sizeof(float))) return 1;
  if (bufs.get((void**)&stats, (size_t)B * G * 2 * sizeof(float))) return 1;
  if (bufs.get((void**)&ab, (size_t)B * Cin * 2 * sizeof(float))) return 1;
  if (bufs.get((void**)&partial, gn_partial_bytes(B, H * W, Cin, G))) return 1;
  int rc = launch_wino_fused128_pack(d_w_oihw, U, Cout, Cin, s, WF_U_SCALE);
  if (!rc) rc = launch_gn_stats(d_x, ldx, stats, partial, B, H * W, Cin, G, eps, s);
  if (!rc) rc = launch_gn_fold(stats, d_gamma, d_beta, d_scale_shift, 2 * Cin, ab, B, Cin, G, s);
  double* opart = nullptr;
  if (d_out_stats)
    if (bufs.get((void**)&opart, (size_t)B * G * wino_fused_out_stats_chunks(H, W, Cout, G) * 2 * sizeof(double))) return 1;
  void* items = nullptr;
  if (bufs.get(&items, wino_fused128_items_count(B, H, W, Cout) * 16)) return 1;
  if (!rc) rc = launch_wino_fused128_items(items, B, H, W, Cout, s);
  if (!rc)
    rc = launch_wino_fused_gn128(d_x, ldx, ab, U, d_bias, d_res, Cout, d_y, B, H, W, Cin, Cout, opart, opart ? G : 0, items, s);
  if (!rc && opart)
    rc = launch_gn_finalize(opart, d_out_stats, (int)wino_fused_out_stats_chunks(H, W, Cout, G), B, G,
                            (double)H * W * (Cout / G), eps, s);
  hipError_t e = hipStreamSynchronize(s);   // (the holder frees the buffers after the launches have drained)
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
}

// ---- the pieces of a ResnetBlock the plan joins (engine.hip: skinny, gca, wino4_block, resnet; the gate_add after a
// GlobalContext gate), one host wrapper each around the plan's own launch_* calls with the plan's argument forms.  Every
// shape is checked before the first allocation; the buffers live in one holder that frees them on every path.
namespace {
struct EntryBufs {
  std::vector<void*> p;
  ~EntryBufs() {
    for (void* q : p) (void)hipFree(q);
  }
  int get(void** out, size_t bytes) {
    KD_HIP_CHECK(hipMalloc(out, bytes));
    p.push_back(*out);
    return 0;
  }
};
int entry_finish(int rc, hipStream_t s) {
  hipError_t e = hipStreamSynchronize(s);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
}
}  // namespace

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
  EntryBufs bufs;
  float *U = nullptr, *D = nullptr;
  void *V = nullptr, *U3 = nullptr, *ws = nullptr;
  if (bufs.get((void**)&U, (size_t)36 * Cout * Cin * sizeof(float))) return 1;
  if (bufs.get(&V, planes ? (size_t)36 * Mt * Cin * 6 : (size_t)36 * Mt * Cin * sizeof(float))) return 1;
  if (bufs.get((void**)&D, (size_t)36 * Mt * Cout * sizeof(float))) return 1;
  if (x3 && bufs.get(&U3, ((size_t)36 * Cout * Cin * 3 + 1) / 2 * sizeof(float))) return 1;
  if (x3 && bufs.get(&ws, gemm_bf16x3_workspace_bytes())) return 1;
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
      rc = launch_gemm_bf16x3(V, U3, D, 36, (int)Mt, Cout, Cin, ws, s, !planes, false);
      if (!rc && gemm_bf16x3_needs_sum(36, (int)Mt, Cout, Cin)) rc = launch_gemm_bf16x3_sum(D, 36, (int)Mt, Cout, Cin, ws, s);
    } else if (!rc) {
      ConvParams p{};
      p.x = (const float*)V; p.w = U; p.y = D;
      p.B = 1; p.Hi = 1; p.Wi = (int)(36 * Mt); p.Cin = Cin; p.ldx = Cin;
      p.Ho = 1; p.Wo = (int)(36 * Mt); p.Cout = Cout;
      p.KH = 1; p.KW = 1; p.stride = 1; p.pad = 0;
      p.out_mode = OUT_NHWC; p.ldy = Cout;
      p.wz_rows = (int)Mt; p.wz_count = 36;
      rc = launch_conv_igemm(p, s);
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
  hipStream_t s = (hipStream_t)stream;
  const int np = d_self_cond ? 6 : 3;
  KD_REQUIRE(d_x && d_w3 && d_w7 && d_w15 && d_y && iters >= 1, "kd_init_conv_planes_nchw: null argument or iters < 1");
  KD_REQUIRE(c0 >= 0 && c0 + np <= Itot, "kd_init_conv_planes_nchw: input channels c0 .. c0 + planes - 1 out of range");
  KD_REQUIRE(init_conv_fused_ok(S, n3, n7, n15, np), "init conv kernel: S % 32 == 0 and the weights must fit LDS");
  float* wp = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  KD_HIP_CHECK(hipMalloc((void**)&wp, init_conv_weight_floats(n3, n7, n15, np) * sizeof(float)));
  int rc = launch_init_conv_pack(d_w3, d_w7, d_w15, wp, n3, n7, n15, Itot, c0, np, s);
  if (!rc && ms) {
    rc = hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, s) != hipSuccess;
    if (rc) set_error("kd_init_conv_planes_nchw: event setup failed");
  }
  for (int i = 0; i < iters && !rc; ++i)
    rc = launch_init_conv(d_x, d_self_cond, np, wp, d_bias, d_res, d_y, n3 + n7 + n15, nullptr, B, S, n3, n7, n15, s);
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
  (void)hipFree(wp);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
}

int kd_groupnorm_silu_nhwc(const float* d_x, const float* d_gamma, const float* d_beta, const float* d_scale_shift,
                           float* d_y, int B, int HW, int C, int G, float eps, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  float* stats = nullptr;
  double* partial = nullptr;
  KD_HIP_CHECK(hipMalloc((void**)&stats, (size_t)B * G * 2 * sizeof(float)));
  KD_HIP_CHECK(hipMalloc((void**)&partial, gn_partial_bytes(B, HW, C, G)));
  int rc = launch_gn_stats(d_x, C, stats, partial, B, HW, C, G, eps, s);
  if (!rc) rc = launch_gn_apply_silu(d_x, C, stats, d_gamma, d_beta, d_scale_shift, 2 * C, d_y, B, HW, C, G, s);
  hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(stats);
  (void)hipFree(partial);
  if (rc) return rc;
  KD_HIP_CHECK(e);
  return 0;
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
  KD_REQUIRE(gemm_bf16x3_epi_ok(rows, N, C, e), "kd_layernorm_linear_bf16x3 needs rows % 256 == 0, N % 128 == 0, C % 32 == 0");
  void *W3 = nullptr, *ws = nullptr;
  hipError_t er = hipMalloc(&W3, (size_t)N * C * 6);
  if (er == hipSuccess) er = hipMalloc(&ws, gemm_bf16x3_workspace_bytes());
  int rc = er != hipSuccess;
  if (!rc) rc = launch_split3(d_w, W3, 1, N, C, s);
  if (!rc) rc = launch_layernorm(d_x, C, d_g, d_beta, nullptr, 0, (float*)d_planes, rows, C, eps, s, in_act, nullptr, nullptr, nullptr, 0, 1);
  if (!rc) rc = launch_gemm_bf16x3(d_planes, W3, d_y, 1, rows, N, C, ws, s, false, true, &e);
  hipError_t es = hipStreamSynchronize(s);
  (void)hipFree(W3);
  (void)hipFree(ws);
  if (rc) return rc;
  KD_HIP_CHECK(er);
  KD_HIP_CHECK(es);
  return 0;
}

int kd_attention(const float* d_q, const float* d_k, const float* d_v, float* d_out, int B, int Nq, int Nk, int H,
                 int Hkv, int D, void* stream) {
  KD_REQUIRE(D == 64, "kd_attention is built for D = 64");
  KVSeg s0{d_k, d_v, Hkv * D, Nk};
  KVSeg s1{nullptr, nullptr, 0, 0};
  return launch_attention(d_q, H * D, nullptr, nullptr, s0, s1, d_out, H * D, B, Nq, H, Hkv, 1.0f,
                          (hipStream_t)stream);
}

// launch_attention with every argument the plan passes it (engine.hip transformer() / cross_attn(), text_build.inc):
// learned null key / value, two K/V segments with their own row strides, q / out row strides, scale
int kd_attention_ex(const float* d_q, int ldq, const float* d_null_kv, const float* d_k0, const float* d_v0, int ld0, int n0,
                    const float* d_k1, const float* d_v1, int ld1, int n1, float* d_out, int ldo, int B, int Nq, int H, int Hkv,
                    float scale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_q && d_out && B > 0 && H > 0 && n0 >= 0 && n1 >= 0, "kd_attention_ex: null argument or bad sizes");
  KD_REQUIRE((n0 == 0 || (d_k0 && d_v0)) && (n1 == 0 || (d_k1 && d_v1)), "kd_attention_ex: a segment with keys needs k and v");
  KD_REQUIRE((((uintptr_t)d_q | (uintptr_t)d_null_kv | (uintptr_t)d_k0 | (uintptr_t)d_v0 | (uintptr_t)d_k1 | (uintptr_t)d_v1 |
               (uintptr_t)d_out) & 15) == 0, "kd_attention_ex: 16-byte aligned pointers");
  KVSeg s0{d_k0, d_v0, ld0, n0};
  KVSeg s1{d_k1, d_v1, ld1, n1};
  return entry_finish(launch_attention(d_q, ldq, d_null_kv, d_null_kv ? d_null_kv + 64 : nullptr, s0, s1, d_out, ldo, B,
                                       Nq, H, Hkv, scale, s), s);
}

int kd_l2norm_heads(float* d_x, int ld, int64_t rows, int heads, const float* d_scale_vec, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KD_REQUIRE(d_x && rows >= 0 && heads > 0 && ld >= heads * 64, "kd_l2norm_heads: null argument or ld < heads * 64");
  return entry_finish(launch_l2norm_heads(d_x, ld, rows, heads, d_scale_vec, s), s);
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

}  // extern "C"
