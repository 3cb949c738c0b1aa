// The DDPM and EDM sampler loops over the plan's forward (state: kd::Sampler, engine.hip; entry points: api.inc).
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

static inline size_t image_bytes(const kd_unet* u) {
  return (size_t)u->cfg.batch * u->cfg.channels * u->cfg.image_size * u->cfg.image_size * sizeof(float);
}

struct SamplerCtx {
  StepTables tb{};   // (EDM: log_snr alone, its [2N] time inputs - what the conditioning table's rows are a function of)
  int T = 0, R = 1;
  bool cond_tab = false;   // the iteration restores the conditioning from the table instead of computing it
};

// the one place that writes the per-call I/O the plan's ops read
static void set_inputs(kd_unet* u, const float* x, const kd_sample_args_t* a, const float* log_snr, const float* self_cond,
                       float* out) {
  u->in_x = x;
  u->in_lowres = a->d_lowres;
  u->in_cond = a->d_cond_images;
  u->in_log_snr = log_snr;
  u->in_lowres_log_snr = a->d_lowres_log_snr;
  u->in_text_tokens = a->d_text_tokens;
  u->in_text_hiddens = a->d_text_hiddens;
  u->in_self_cond = self_cond;   // (nullptr = zeros; a plan without self_cond ignores it, as the library does)
  u->out = out;
}

// what is missing of the scratch; the carried self-conditioning estimate starts as zeros
static int sampler_scratch(kd_unet* u, bool guidance = false, bool edm = false) {
  Sampler& m = u->smp;
  const int B = u->cfg.batch;
  const size_t img = image_bytes(u);
  auto need = [&](auto*& p, size_t bytes) { return p ? 0 : m.mem.get(&p, bytes); };
  if (need(m.pred, img) || need(m.x0, img) || need(m.thresh, (size_t)B * sizeof(float)) ||
      need(m.time, (size_t)B * sizeof(float)) || need(m.iter, sizeof(int)) ||
      need(m.seed, (size_t)(SEED_ROWS + B) * sizeof(uint64_t)) ||
      need(m.qws, quantile_ws_bytes(B)))
    return 1;
  if (guidance && need(m.pred_null, img)) return 1;
  if (edm && (need(m.xhat, img) || need(m.d, img) || need(m.net_in, img))) return 1;
  if (u->self_cond && !m.self_cond) {
    if (need(m.self_cond, img)) return 1;
    KD_HIP_CHECK(hipMemset(m.self_cond, 0, img));
  }
  return 0;
}
// self_cond plans: the carried x0 estimate starts as zeros (the library's self_cond = None) at the first step of a call;
// outside any captured graph
static int self_cond_reset(kd_unet* u, hipStream_t s) {
  if (!u->self_cond) return 0;
  KD_HIP_CHECK(hipMemsetAsync(u->smp.self_cond, 0, image_bytes(u), s));
  return 0;
}

// What every sampling entry shares: the argument checks, R, the scratch and - when an image is sampled - the plan's
// inputs, the seed and the step-invariant part of the forward.  d_img == nullptr: no sampling follows, nothing is
// launched (kd_sample_build_cond_table).  edm: the forward reads the step's preconditioned input, not the image.
static int begin_call(kd_unet* u, const void* sched, const kd_sample_args_t* a, float* d_img, bool edm, SamplerCtx& ctx,
                      hipStream_t s) {
  KD_REQUIRE(u && sched && a, "null argument");
  KD_REQUIRE((a->d_inpaint_images == nullptr) == (a->d_inpaint_masks == nullptr),
             "inpaint_images and inpaint_masks must be given together");
  ctx.R = a->d_inpaint_images ? (a->resample_times < 1 ? 1 : a->resample_times) : 1;
  if (sampler_scratch(u, d_img && cfg_on(a), edm)) return 1;
  Sampler& m = u->smp;
  if (!d_img) {   // the conditioning ops read the time inputs alone: the rest stays as the last forward left it
    set_inputs(u, u->in_x, a, m.time, u->in_self_cond, u->out);
    return 0;
  }
  if (cfg_on(a))
    KD_REQUIRE(a->d_null_text_tokens && a->d_null_text_hiddens && a->d_text_tokens && a->d_text_hiddens,
               "cond_scale != 1 needs the conditional and the null text conditioning");
  set_inputs(u, edm ? m.net_in : d_img, a, m.time, m.self_cond, m.pred);
  if (launch_seed_set(m.seed, a->seed, a->seeds, u->cfg.batch, s)) return 1;   // (every call: k_begin > 0 re-keys too)
  return run_static(u, s);   // conditioning planes are constant over the loop
}

// kd_schedule_t -> the DDPM step tables on the device [9][T]
static int ddpm_prepare(kd_unet* u, const kd_schedule_t* sc, SamplerCtx& ctx, hipStream_t s) {
  const int T = sc->T;
  KD_REQUIRE(T >= 1, "schedule must have at least one step");
  const float* src[9] = {sc->log_snr, sc->alpha, sc->sigma, sc->alpha_next, sc->sigma_next,
                         sc->c,       sc->noise_scale, sc->rn_a, sc->rn_b};
  std::vector<float> host((size_t)9 * T, 0.0f);
  for (int i = 0; i < 9; ++i) {
    if (i < 7) KD_REQUIRE(src[i] != nullptr, "schedule arrays log_snr..noise_scale are required");
    if (src[i]) memcpy(host.data() + (size_t)i * T, src[i], (size_t)T * sizeof(float));
  }
  if (u->smp.ddpm_tab.upload(std::move(host), s)) return 1;
  const float* t = u->smp.ddpm_tab.dev;
  ctx.tb = StepTables{t, t + T, t + 2 * T, t + 3 * T, t + 4 * T, t + 5 * T, t + 6 * T, t + 7 * T, t + 8 * T};
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
// pointing at its time inputs).  The plan's time inputs are set (set_inputs) when this runs.
static int sampler_cond_table(kd_unet* u, const std::vector<float>& key, const kd_sample_args_t* a, SamplerCtx& ctx,
                              int k_begin, int k_end, hipStream_t s, bool force = false) {
  Sampler& m = u->smp;
  CondTable& c = m.cond;
  ctx.cond_tab = false;
  const bool lowres = u->cfg.lowres_cond != 0;
  if (a->cond_table < 0 || u->cond_bytes == 0 || u->cfg.text_tokens > 0 || cfg_on(a)) return 0;
  if (lowres && !a->lowres_log_snr_uniform) return 0;   // per-sample levels: computed in the step, as before
  const size_t need = (size_t)ctx.T * u->cond_bytes;
  const bool same = c.tab != nullptr && c.bytes >= need && c.T == ctx.T && (int)c.row_ok.size() == ctx.T && c.sched == key &&
                    (!lowres || c.lowres == a->lowres_log_snr_value);
  if (!same) {
    // every row of the old table is stale from here on, whatever happens below
    c.row_ok.clear();
    // Resident-size cap: args->cond_table_max_mb if given, else 4 GiB, and never more than 1/8 of the free HBM
    size_t cap = a->cond_table_max_mb > 0 ? (size_t)a->cond_table_max_mb << 20 : size_t(4) << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) cap = std::min(cap, (free_b + c.bytes) / 8);
    c.refused_bytes = 0;
    if (need > cap) {   // (reported: kd_unet_cond_table_refused_bytes - the launch count and the speed of the step differ)
      c.refused_bytes = (int64_t)need;
      return 0;
    }
    if (c.bytes < need) {
      if (c.tab) {
        KD_HIP_CHECK(hipStreamSynchronize(s));   // (a replay of the old table may still be running)
        m.drop_graphs();   // the captured graphs hold the old table pointer
        KD_HIP_CHECK(hipFree(c.tab));
        c.tab = nullptr;
        c.bytes = 0;
      }
      if (hipMalloc((void**)&c.tab, need) != hipSuccess) {
        (void)hipGetLastError();   // no room for the table: the step computes its conditioning itself
        c.tab = nullptr;
        c.refused_bytes = (int64_t)need;
        return 0;
      }
      c.bytes = need;
    }
    c.sched = key;
    c.T = ctx.T;
    c.lowres = a->lowres_log_snr_value;
    c.row_ok.assign((size_t)ctx.T, 0);
  }
  // Rows are built on demand, for the steps this call walks: a 250-row table costs nothing to a call that runs 20 steps
  // of it, and every later call on the same schedule (every patch of a grid, the next k-range of a traced run) finds
  // its rows there.  B > 1: B schedule steps per run of the conditioning ops (see cond_scatter_kernel).
  const int B = u->cfg.batch;
  const bool rows = B > 1 && u->cond_rows_ok && u->d_cond_segs;
  const int chunk = rows ? B : 1;
  bool any = false;
  for (int k = k_begin; k < k_end && !any; ++k) any = force || !c.row_ok[k];
  if (any) {
    // device time of the build: two events recorded here and read when somebody asks (kd_unet_cond_table_build_ms) -
    // the sampling path itself never waits for them (ADVICE r4: a traced run builds rows in every call)
    if (!c.ev0) KD_HIP_CHECK(hipEventCreate(&c.ev0));
    if (!c.ev1) KD_HIP_CHECK(hipEventCreate(&c.ev1));
    c.ev_pending = false;
    KD_HIP_CHECK(hipEventRecord(c.ev0, s));
    int rc = 0, built = 0, runs = 0;
    for (int k0 = (k_begin / chunk) * chunk; k0 < k_end && !rc; k0 += chunk) {
      const int k1 = std::min(k0 + chunk, ctx.T);
      bool need_it = force;
      for (int k = k0; k < k1 && !need_it; ++k) need_it = !c.row_ok[k];
      if (!need_it) continue;
      for (int k = k0; k < k1; ++k) c.row_ok[k] = 0;
      ++runs;
      if (rows) {
        rc = launch_fill_time_rows(ctx.tb.log_snr, k0, ctx.T, m.time, B, s);
        if (!rc) rc = run_cond_ops(u, s);
        if (!rc)
          rc = launch_cond_scatter((const float*)u->cond_ws, (float*)c.tab, u->d_cond_segs, (int)u->cond_segs.size(),
                                   u->cond_row_total, B, k0, ctx.T, (int64_t)(u->cond_bytes / 4), s);
      } else {
        rc = launch_iter_set(m.iter, k0 * ctx.R, s);
        if (!rc) rc = launch_fill_time(ctx.tb.log_snr, m.iter, ctx.R, m.time, B, s);
        if (!rc) rc = run_cond_ops(u, s);
        if (!rc && hipMemcpyAsync(c.tab + (size_t)k0 * u->cond_bytes, u->cond_ws, u->cond_bytes, hipMemcpyDeviceToDevice,
                                  s) != hipSuccess) {
          set_error("cond table: device copy failed");
          rc = 1;
        }
      }
      if (!rc)
        for (int k = k0; k < k1; ++k) c.row_ok[k] = 1, ++built;
    }
    if (!rc && hipEventRecord(c.ev1, s) == hipSuccess) {
      c.ev_pending = true;
      c.build_rows = built;
      c.build_runs = runs;
    }
    if (rc) return 1;
  }
  ctx.cond_tab = true;
  return 0;
}

// One UNet forward of a step on x -> smp.pred: the conditioning row restored from the table (rows of this forward at
// cond_rows) or computed, and under classifier-free guidance the second forward on the null conditioning and the combine
static int guided_forward(kd_unet* u, const SamplerCtx& ctx, const kd_sample_args_t* a, const float* x, const char* cond_rows,
                          hipStream_t s) {
  Sampler& m = u->smp;
  set_inputs(u, x, a, m.time, m.self_cond, m.pred);
  if (ctx.cond_tab && launch_cond_gather(cond_rows, u->cond_ws, u->cond_bytes, m.iter, ctx.R, s)) return 1;
  if (run_forward(u, s, ctx.cond_tab)) return 1;
  if (!cfg_on(a)) return 0;
  kd_sample_args_t null_a = *a;   // (both forwards read the same self-conditioning estimate)
  null_a.d_text_tokens = a->d_null_text_tokens;
  null_a.d_text_hiddens = a->d_null_text_hiddens;
  set_inputs(u, x, &null_a, m.time, m.self_cond, m.pred_null);
  if (run_forward(u, s)) return 1;
  return launch_cfg_combine(m.pred, m.pred_null, m.pred, a->cond_scale, (int64_t)(image_bytes(u) / sizeof(float)), s);
}

// sv: the update of a few-step solver (its tables; hist = the kept estimate or nullptr; hist2 and coef_prev2 = the ring's
// second slot and the third-order coefficients, or nullptr) in place of the ancestral one
static int emit_iteration(kd_unet* u, const SamplerCtx& ctx, const kd_sample_args_t* a, float* d_img, hipStream_t s,
                          const SolverTables* sv = nullptr, float* hist = nullptr, float* hist2 = nullptr,
                          const float* coef_prev2 = nullptr) {
  Sampler& m = u->smp;
  const int B = u->cfg.batch, S = u->cfg.image_size, R = ctx.R, Ci = u->cfg.channels;
  const int64_t hw = (int64_t)S * S, per = Ci * hw;
  const bool inpaint = a->d_inpaint_images != nullptr;
  if (inpaint)
    if (launch_inpaint_mix(d_img, a->d_inpaint_images, a->d_inpaint_masks, a->d_noise_inpaint, B * per, m.seed, ctx.tb,
                           m.iter, R, B, Ci, hw, s))
      return 1;
  if (launch_fill_time(ctx.tb.log_snr, m.iter, R, m.time, B, s)) return 1;
  if (guided_forward(u, ctx, a, d_img, m.cond.tab, s)) return 1;
  if (launch_x0(d_img, m.pred, m.x0, ctx.tb, m.iter, R, a->objective, B * per, s)) return 1;
  if (a->dynamic_threshold)
    if (launch_quantile_abs(m.x0, m.thresh, B, per, a->percentile, m.qws, s)) return 1;
  if (sv) {
    if (launch_solver_update(d_img, m.x0, m.thresh, a->d_noise_step, B * per, m.seed, *sv, m.iter, R, a->dynamic_threshold, B,
                             per, s, hist, m.self_cond, hist2, coef_prev2))
      return 1;
  } else if (launch_ddpm_update(d_img, m.x0, m.thresh, a->d_noise_step, B * per, m.seed, ctx.tb, m.iter, R,
                                a->dynamic_threshold, B, per, s, m.self_cond)) {
    return 1;
  }
  if (inpaint && R > 1)
    if (launch_renoise(d_img, a->d_noise_renoise, B * per, m.seed, ctx.tb, m.iter, R, ctx.T, B, per, s)) return 1;
  return launch_iter_inc(m.iter, s);
}

// what a captured iteration depends on besides the content of device memory; `tables`: the schedule tables' address
static std::vector<uint64_t> graph_key_of(const kd_sample_args_t* a, const float* d_img, const float* tables, int T, int R,
                                          bool cond_tab) {
  auto p = [](const void* x) { return (uint64_t)(uintptr_t)x; };
  uint64_t pct;
  float f = a->percentile;
  memcpy(&pct, &f, sizeof(float));
  return {p(d_img), p(a->d_lowres), p(a->d_lowres_log_snr), p(a->d_cond_images), p(a->d_text_tokens),
          p(a->d_text_hiddens), p(a->d_inpaint_images), p(a->d_inpaint_masks), p(a->d_noise_step),
          p(a->d_noise_inpaint), p(a->d_noise_renoise), (uint64_t)a->objective,
          (uint64_t)a->dynamic_threshold, pct & 0xFFFFFFFFull, (uint64_t)T, (uint64_t)R,
          p(a->d_null_text_tokens), p(a->d_null_text_hiddens), (uint64_t)(a->cond_scale * 65536.0f),
          (uint64_t)cond_tab, p(tables)};
}

// n launches on `s` of the iteration emit(stream) records - the one captured in `g` when it was captured for `key`.
// Captured on an engine-owned stream (the caller's may be the legacy null stream, which cannot be captured): capturing
// only records the launches.  One stream, no forks: see emit_edm_iteration.
template <class Emit>
static int replay_or_capture(Sampler& m, StepGraph& g, const std::vector<uint64_t>& key, Emit emit, hipStream_t s, int n) {
  if (!g.exec || key != g.key) {
    g.drop();
    if (!m.cap_stream) KD_HIP_CHECK(hipStreamCreateWithFlags(&m.cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    KD_HIP_CHECK(hipStreamBeginCapture(m.cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = emit(m.cap_stream);
    hipError_t e = hipStreamEndCapture(m.cap_stream, &graph);
    if (!rc && e == hipSuccess) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return 1;
    if (e != hipSuccess) g.exec = nullptr;
    KD_HIP_CHECK(e);
    g.key = key;
  }
  for (int i = 0; i < n; ++i) KD_HIP_CHECK(hipGraphLaunch(g.exec, s));
  return 0;
}

static int sample_steps(kd_unet* u, const kd_schedule_t* sc, const kd_sample_args_t* a, float* d_img, int k_begin,
                        int k_end, hipStream_t s) {
  KD_REQUIRE(d_img, "null argument");
  SamplerCtx ctx;
  if (begin_call(u, sc, a, d_img, false, ctx, s)) return 1;
  KD_REQUIRE(a->objective >= 0 && a->objective <= 2, "unknown prediction objective");
  if (ddpm_prepare(u, sc, ctx, s)) return 1;
  KD_REQUIRE(0 <= k_begin && k_begin <= k_end && k_end <= ctx.T, "step range out of bounds");
  if (ctx.R > 1) KD_REQUIRE(sc->rn_a && sc->rn_b, "re-noise tables are required when resampling");
  Sampler& m = u->smp;
  if (k_begin == 0 && !a->keep_self_cond && self_cond_reset(u, s)) return 1;   // k_begin > 0 continues from what the plan holds
  if (sampler_cond_table(u, m.ddpm_tab.host, a, ctx, k_begin, k_end, s)) return 1;
  if (launch_iter_set(m.iter, k_begin * ctx.R, s)) return 1;
  const int n_iter = (k_end - k_begin) * ctx.R;
  auto emit = [&](hipStream_t st) { return emit_iteration(u, ctx, a, d_img, st); };
  if (a->use_graph)
    return replay_or_capture(m, m.ddpm_graph, graph_key_of(a, d_img, m.ddpm_tab.dev, ctx.T, ctx.R, ctx.cond_tab), emit, s, n_iter);
  for (int i = 0; i < n_iter; ++i)
    if (emit(s)) return 1;
  return 0;
}

// ------------------------------------------------------------------------------ few-step solvers (DDIM, DPM-Solver++ 2M / 3M)
// kd_solver_schedule_t -> its tables on the device [9][T]: log_snr, alpha, sigma, rn_a, rn_b, then the four coefficients;
// with a coef_prev2 that is not all zero (kd_solver3_schedule_t) a tenth row holds it and *d_prev2 points at it.
// *keeps: some step reads the previous step's estimate (coef_prev != 0), so the plan carries one.
static const int SOLVER_NTAB = 9;
static int solver_prepare(kd_unet* u, const kd_solver_schedule_t* sc, const float* coef_prev2, SamplerCtx& ctx, SolverTables& sv,
                          bool* keeps, const float** d_prev2, hipStream_t s) {
  const int T = sc->T;
  KD_REQUIRE(T >= 1, "schedule must have at least one step");
  const float* src[SOLVER_NTAB] = {sc->log_snr, sc->alpha,   sc->sigma,     sc->rn_a,      sc->rn_b,
                                   sc->coef_x,  sc->coef_x0, sc->coef_prev, sc->coef_noise};
  bool ring = false;   // an absent or all-zero coef_prev2 is the nine-row schedule, bit for bit
  for (int k = 0; coef_prev2 && k < T; ++k) ring = ring || coef_prev2[k] != 0.0f;
  std::vector<float> host((size_t)(SOLVER_NTAB + (ring ? 1 : 0)) * T, 0.0f);
  for (int i = 0; i < SOLVER_NTAB; ++i) {
    if (i < 3) KD_REQUIRE(src[i] != nullptr, "solver schedule arrays log_snr, alpha and sigma are required");
    if (i >= 5) KD_REQUIRE(src[i] != nullptr, "solver schedule arrays coef_x, coef_x0, coef_prev and coef_noise are required");
    if (src[i]) memcpy(host.data() + (size_t)i * T, src[i], (size_t)T * sizeof(float));
  }
  if (ring) memcpy(host.data() + (size_t)SOLVER_NTAB * T, coef_prev2, (size_t)T * sizeof(float));
  *keeps = ring;
  for (int k = 0; k < T; ++k) *keeps = *keeps || sc->coef_prev[k] != 0.0f;
  if (u->smp.solver_tab.upload(std::move(host), s)) return 1;
  const float* t = u->smp.solver_tab.dev;
  ctx.tb = StepTables{};   // what the shared kernels of an iteration read: the time input, alpha / sigma, the re-noise pair
  ctx.tb.log_snr = t;
  ctx.tb.alpha = t + T;
  ctx.tb.sigma = t + 2 * T;
  ctx.tb.rn_a = t + 3 * T;
  ctx.tb.rn_b = t + 4 * T;
  sv = SolverTables{t + 5 * T, t + 6 * T, t + 7 * T, t + 8 * T};
  *d_prev2 = ring ? t + (size_t)SOLVER_NTAB * T : nullptr;
  ctx.T = T;
  return 0;
}

// As sample_steps, the update being the solver's.  Tables and captured iterations are the solver path's own (solver_tab,
// solver_graph): a plan that alternates between samplers replays each one's graph.  The conditioning rows are a function
// of the time inputs alone, so they are keyed on log_snr: every solver at any eta shares the rows of one N-step schedule.
// coef_prev2 (kd_solver3_*; nullptr from kd_solver_*): the third-order term over the ring of two histories.
static int solver_sample_steps(kd_unet* u, const kd_solver_schedule_t* sc, const float* coef_prev2, const kd_sample_args_t* a,
                               float* d_img, int k_begin, int k_end, hipStream_t s) {
  KD_REQUIRE(d_img, "null argument");
  SamplerCtx ctx;
  if (begin_call(u, sc, a, d_img, false, ctx, s)) return 1;
  KD_REQUIRE(a->objective >= 0 && a->objective <= 2, "unknown prediction objective");
  SolverTables sv{};
  bool keeps = false;
  const float* d_prev2 = nullptr;
  if (solver_prepare(u, sc, coef_prev2, ctx, sv, &keeps, &d_prev2, s)) return 1;
  KD_REQUIRE(0 <= k_begin && k_begin <= k_end && k_end <= ctx.T, "step range out of bounds");
  if (ctx.R > 1) KD_REQUIRE(sc->rn_a && sc->rn_b, "re-noise tables are required when resampling");
  // the first two steps of a schedule are of order 1 and at most 2: they read nothing of what the ring holds
  if (d_prev2 && k_begin == 0)
    KD_REQUIRE(sc->coef_prev[0] == 0.0f && coef_prev2[0] == 0.0f && (ctx.T < 2 || coef_prev2[1] == 0.0f),
               "solver schedule: step 0 must be first order and step 1 at most second order (coef_prev[0], coef_prev2[0..1] == 0)");
  Sampler& m = u->smp;
  if (keeps && !m.hist) {   // zeros until a step keeps its estimate: a call that starts at a second-order step reads them
    if (m.mem.get(&m.hist, image_bytes(u))) return 1;
    KD_HIP_CHECK(hipMemsetAsync(m.hist, 0, image_bytes(u), s));
  }
  if (d_prev2 && !m.hist2) {   // the ring's second slot, with the first third-order call
    if (m.mem.get(&m.hist2, image_bytes(u))) return 1;
    KD_HIP_CHECK(hipMemsetAsync(m.hist2, 0, image_bytes(u), s));
  }
  float* hist = keeps ? m.hist : nullptr;
  float* hist2 = d_prev2 ? m.hist2 : nullptr;
  if (k_begin == 0 && !a->keep_self_cond && self_cond_reset(u, s)) return 1;   // k_begin > 0 continues from what the plan holds
  const std::vector<float> cond_key(m.solver_tab.host.begin(), m.solver_tab.host.begin() + ctx.T);
  if (sampler_cond_table(u, cond_key, a, ctx, k_begin, k_end, s)) return 1;
  if (launch_iter_set(m.iter, k_begin * ctx.R, s)) return 1;
  const int n_iter = (k_end - k_begin) * ctx.R;
  auto emit = [&](hipStream_t st) { return emit_iteration(u, ctx, a, d_img, st, &sv, hist, hist2, d_prev2); };
  if (a->use_graph)
    return replay_or_capture(m, m.solver_graph[d_prev2 ? 2 : keeps ? 1 : 0],
                             graph_key_of(a, d_img, m.solver_tab.dev, ctx.T, ctx.R, ctx.cond_tab), emit, s, n_iter);
  for (int i = 0; i < n_iter; ++i)
    if (emit(s)) return 1;
  return 0;
}

// ------------------------------------------------------------------------------ EDM Heun sampler
// Per-step tables of kd_edm_schedule_t on the device [15][N] (c_noise_hat and c_noise_next adjacent: one [2N] time table
// for the conditioning table), then S_noise (part of the key only)
static const int EDM_NTAB = 15;
static int edm_prepare(kd_unet* u, const kd_edm_schedule_t* sc, EdmTables& tb, hipStream_t s) {
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
  host[(size_t)EDM_NTAB * N] = sc->S_noise;
  for (int k = 0; k + 1 < N; ++k)   // the Heun kernel re-noises by step index: only the last step may skip the correction
    KD_REQUIRE(src[2][k] != 0.0f, "EDM schedule: sigma_next == 0 before the last step");
  if (u->smp.edm_tab.upload(std::move(host), s)) return 1;
  const float* t = u->smp.edm_tab.dev;
  const float** dst[EDM_NTAB] = {&tb.sigma,     &tb.sigma_hat,   &tb.sigma_next, &tb.churn,       &tb.euler_step,
                                 &tb.heun_step, &tb.renoise,     &tb.c_in_hat,   &tb.c_skip_hat,  &tb.c_out_hat,
                                 &tb.c_in_next, &tb.c_skip_next, &tb.c_out_next, &tb.c_noise_hat, &tb.c_noise_next};
  for (int i = 0; i < EDM_NTAB; ++i) *dst[i] = t + (size_t)i * N;
  return 0;
}

// UNet forward j of the step (0: at sigma_hat, 1: at sigma_next) on smp.net_in -> pred (+ the guidance forward), then
// den = c_skip x + c_out net -> x0 and its per-sample quantile -> thresh
static int edm_forward(kd_unet* u, const SamplerCtx& ctx, const EdmTables& tb, const kd_sample_args_t* a, const float* x,
                       int j, hipStream_t s) {
  Sampler& m = u->smp;
  const int B = u->cfg.batch, S = u->cfg.image_size, R = ctx.R, N = ctx.T / 2;
  const int64_t per = (int64_t)u->cfg.channels * S * S;
  if (launch_fill_time(j ? tb.c_noise_next : tb.c_noise_hat, m.iter, R, m.time, B, s)) return 1;
  // table rows [0, N): time input at sigma_hat, [N, 2N): at sigma_next
  const char* rows = ctx.cond_tab ? m.cond.tab + (size_t)j * N * u->cond_bytes : nullptr;
  if (guided_forward(u, ctx, a, m.net_in, rows, s)) return 1;
  if (launch_edm_precond_out(x, m.pred, m.x0, j ? tb.c_skip_next : tb.c_skip_hat, j ? tb.c_out_next : tb.c_out_hat, m.iter, R,
                             B * per, s))
    return 1;
  if (a->dynamic_threshold)
    if (launch_quantile_abs(m.x0, m.thresh, B, per, a->percentile, m.qws, s)) return 1;
  return 0;
}

// One EDM iteration: churn, forward at sigma_hat, Euler; with `heun` the forward at sigma_next and the correction
// (+ re-noise).  Everything on `s`, in order: no side streams (a captured graph with parallel branches can crash the
// runtime's replay).
static int emit_edm_iteration(kd_unet* u, const SamplerCtx& ctx, const EdmTables& tb, float s_noise,
                              const kd_sample_args_t* a, float* d_img, bool heun, hipStream_t s) {
  Sampler& m = u->smp;
  const int B = u->cfg.batch, S = u->cfg.image_size, R = ctx.R, N = ctx.T / 2, Ci = u->cfg.channels;
  const int64_t hw = (int64_t)S * S, per = Ci * hw;
  const bool inpaint = a->d_inpaint_images != nullptr;
  if (launch_edm_churn(d_img, m.xhat, m.net_in, a->d_inpaint_images, a->d_inpaint_masks, a->d_noise_step, B * per, m.seed, tb,
                       s_noise, m.iter, R, B, Ci, hw, s))
    return 1;
  if (edm_forward(u, ctx, tb, a, m.xhat, 0, s)) return 1;
  // self_cond: Euler leaves the first forward's thresholded estimate for the Heun forward (and, on the last step, for
  // the caller); Heun leaves the second's for the next step
  if (launch_edm_euler(m.xhat, m.x0, m.thresh, m.d, d_img, m.net_in, tb, m.iter, R, a->dynamic_threshold, B, per, s,
                       m.self_cond))
    return 1;
  if (heun) {
    if (edm_forward(u, ctx, tb, a, d_img, 1, s)) return 1;
    if (launch_edm_heun(d_img, m.xhat, m.d, m.x0, m.thresh, a->d_noise_renoise, B * per, m.seed, tb, m.iter, R, N,
                        inpaint && R > 1, a->dynamic_threshold, B, per, s, m.self_cond))
      return 1;
  }
  return launch_iter_inc(m.iter, s);
}

static int edm_sample_steps(kd_unet* u, const kd_edm_schedule_t* sc, const kd_sample_args_t* a, float* d_img, int k_begin,
                            int k_end, hipStream_t s) {
  KD_REQUIRE(d_img, "null argument");
  SamplerCtx ctx;
  if (begin_call(u, sc, a, d_img, true, ctx, s)) return 1;   // (a->objective is not read: EDM has one parameterisation)
  EdmTables tb{};
  if (edm_prepare(u, sc, tb, s)) return 1;
  const int N = sc->N;
  ctx.T = 2 * N;   // rows of the conditioning table; its time inputs: c_noise_hat | c_noise_next
  ctx.tb.log_snr = tb.c_noise_hat;
  KD_REQUIRE(0 <= k_begin && k_begin <= k_end && k_end <= N, "step range out of bounds");
  Sampler& m = u->smp;
  if (k_begin == 0 && !a->keep_self_cond && self_cond_reset(u, s)) return 1;
  // rows k of both halves for the steps walked (the rows in between come along; each row is built once per schedule)
  if (sampler_cond_table(u, m.edm_tab.host, a, ctx, k_begin, k_end > k_begin ? N + k_end : k_begin, s)) return 1;
  if (launch_iter_set(m.iter, k_begin * ctx.R, s)) return 1;
  std::vector<uint64_t> key = graph_key_of(a, d_img, m.edm_tab.dev, ctx.T, ctx.R, ctx.cond_tab);
  uint32_t sn_bits;
  memcpy(&sn_bits, &sc->S_noise, sizeof(float));
  key.push_back(sn_bits);
  for (int k = k_begin; k < k_end; ++k) {
    const bool heun = sc->sigma_next[k] != 0.0f;
    auto emit = [&](hipStream_t st) { return emit_edm_iteration(u, ctx, tb, sc->S_noise, a, d_img, heun, st); };
    if (a->use_graph) {
      if (replay_or_capture(m, m.edm_graph[heun ? 0 : 1], key, emit, s, ctx.R)) return 1;
      continue;
    }
    for (int r = 0; r < ctx.R; ++r)
      if (emit(s)) return 1;
  }
  return 0;
}

}  // namespace kd
