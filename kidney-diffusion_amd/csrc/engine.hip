// libkd_engine: UNet execution plan, sampler loop and the C ABI of include/kd_engine.h.
//
// The plan builder walks the same module tree the host-side `Unet` class declares
//  and emits a flat list of kernel launches with static shapes and
// static workspace offsets, so one denoising iteration can be captured into a hipGraph and
// replayed.  Feature maps are NHWC fp32; token tensors [B,N,C] are the same memory.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cstddef>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/kd_engine.h"
#include "common.h"

namespace kd {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

#define KD_THROW_IF(expr)                                          \
  do {                                                             \
    if ((expr) != 0) throw std::runtime_error(::kd::g_err);        \
  } while (0)
#define KD_HIP_THROW(expr)                                                                       \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess)                                                                        \
      throw std::runtime_error(std::string(#expr) + " failed: " + hipGetErrorString(_e));        \
  } while (0)

// ------------------------------------------------------------------------------ memory helpers
struct WeightPool {  // engine-owned HBM for weights, bump-allocated from 256 MiB slabs
  std::vector<void*> slabs;
  char* cur = nullptr;
  size_t left = 0, total = 0;
  float* alloc(size_t n_floats) {
    size_t bytes = (n_floats * sizeof(float) + 255) & ~size_t(255);
    if (bytes > left) {
      size_t slab = std::max(bytes, size_t(256) << 20);
      void* p = nullptr;
      KD_HIP_THROW(hipMalloc(&p, slab));
      slabs.push_back(p);
      cur = (char*)p;
      left = slab;
      total += slab;
    }
    float* r = (float*)cur;
    cur += bytes;
    left -= bytes;
    return r;
  }
  ~WeightPool() {
    for (void* p : slabs) (void)hipFree(p);
  }
};

// Packed weights of ONE UNet, shared by all its plans (batch / image-size variants made with
// kd_unet_create_shared): a packed form is produced the first time a plan asks for it.
struct WeightStore {
  WeightPool pool;
  std::unordered_map<std::string, float*> cache;
};

struct Arena {  // plan-time activation allocator with reuse (single in-order stream => safe)
  struct Blk {
    size_t off, size;
    bool free;
  };
  std::vector<Blk> blks;
  size_t end = 0, peak = 0;
  size_t alloc(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    if (bytes == 0) bytes = 256;
    for (size_t i = 0; i < blks.size(); ++i) {
      if (blks[i].free && blks[i].size >= bytes) {
        if (blks[i].size > bytes) {
          Blk rest{blks[i].off + bytes, blks[i].size - bytes, true};
          blks[i].size = bytes;
          blks.insert(blks.begin() + i + 1, rest);
        }
        blks[i].free = false;
        return blks[i].off;
      }
    }
    if (!blks.empty() && blks.back().free) {  // grow the trailing free block
      blks.back().size = bytes;
      blks.back().free = false;
      end = blks.back().off + bytes;
      peak = std::max(peak, end);
      return blks.back().off;
    }
    blks.push_back(Blk{end, bytes, false});
    end += bytes;
    peak = std::max(peak, end);
    return blks.back().off;
  }
  void release(size_t off) {
    for (size_t i = 0; i < blks.size(); ++i) {
      if (blks[i].off == off && !blks[i].free) {
        blks[i].free = true;
        if (i + 1 < blks.size() && blks[i + 1].free) {
          blks[i].size += blks[i + 1].size;
          blks.erase(blks.begin() + i + 1);
        }
        if (i > 0 && blks[i - 1].free) {
          blks[i - 1].size += blks[i].size;
          blks.erase(blks.begin() + i);
        }
        return;
      }
    }
    throw std::runtime_error("arena: release of unknown offset");
  }
};

struct T {  // NHWC tensor in the workspace, or a channel slice of one (a skip tensor living in its concat buffer)
  size_t off = 0;  // arena block: what the reference counts key on
  int B = 0, H = 0, W = 0, C = 0;
  int ld = 0;      // row stride in floats; 0 = dense (C)
  int coff = 0;    // first channel inside the block's rows
  bool x3p = false;  // not fp32 rows: the three bf16 planes [3][C / 16][rows][16] a LayerNorm left for the bf16x3 GEMM that reads it
  int64_t rows() const { return (int64_t)B * H * W; }
  int HW() const { return H * W; }
  int LD() const { return ld ? ld : C; }
  size_t at() const { return off + (size_t)coff * sizeof(float); }  // byte offset of (row 0, channel 0)
  bool dense() const { return LD() == C; }
  T slice(int c0, int n) const { T s = *this; s.ld = LD(); s.C = n; s.coff = coff + c0; return s; }  // channels [c0, c0 + n)
};

// ------------------------------------------------------------------------------ sampler state (sampler.inc)
// Device buffers that die with their owner: the sampler's scratch, the temporaries of a test entry point (api.inc)
struct DevBufs {
  std::vector<void*> p;
  ~DevBufs() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class P>
  int get(P** out, size_t bytes) {
    KD_HIP_CHECK(hipMalloc((void**)out, bytes));
    p.push_back(*out);
    return 0;
  }
};

// A device table keyed on its CONTENT: a sampling call with the schedule of the previous one (every patch of a grid,
// every k-range of a traced run) uploads nothing.  Changed content goes through a pinned staging buffer with ONE
// asynchronous copy on the caller's stream, so it is ordered behind the launches already queued there that still read
// the old content.  A table that grows moves: captured iterations carry its address in their key.
struct DeviceTable {
  float* dev = nullptr;
  float* pinned = nullptr;   // staging for the asynchronous upload
  size_t cap = 0;            // floats, of both
  std::vector<float> host;   // what `dev` holds
  hipEvent_t ev = nullptr;   // recorded behind the last upload from the staging buffer
  ~DeviceTable() {
    release();
    if (ev) (void)hipEventDestroy(ev);
  }
  void release() {
    if (dev) (void)hipFree(dev);
    if (pinned) (void)hipHostFree(pinned);
    dev = pinned = nullptr;
    cap = 0;
    host.clear();
  }
  int upload(std::vector<float>&& h, hipStream_t s) {
    if (h == host) return 0;
    // the previous upload may still be reading the staging buffer - on WHICHEVER stream it was issued (the grid
    // scheduler alternates one plan between the caller's stream and its side stream): wait for its event, not for `s`
    if (ev) KD_HIP_CHECK(hipEventSynchronize(ev));
    const size_t bytes = h.size() * sizeof(float);
    if (cap < h.size()) {
      KD_HIP_CHECK(hipStreamSynchronize(s));   // replays on `s` may still read the old table
      release();
      KD_HIP_CHECK(hipMalloc((void**)&dev, bytes));
      KD_HIP_CHECK(hipHostMalloc((void**)&pinned, bytes, hipHostMallocDefault));
      cap = h.size();
    }
    memcpy(pinned, h.data(), bytes);
    KD_HIP_CHECK(hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, s));
    if (!ev) KD_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    KD_HIP_CHECK(hipEventRecord(ev, s));
    host = std::move(h);
    return 0;
  }
};

// One captured sampler iteration and what it was captured for (sampler.inc: replay_or_capture)
struct StepGraph {
  hipGraphExec_t exec = nullptr;
  std::vector<uint64_t> key;
  ~StepGraph() { drop(); }
  void drop() {
    if (exec) (void)hipGraphExecDestroy(exec);
    exec = nullptr;
  }
};

// The per-schedule conditioning table (sampler.inc: sampler_cond_table) of the plan's cond region
struct CondTable {
  char* tab = nullptr;   // [T][cond_bytes]
  size_t bytes = 0;
  std::vector<float> sched;   // the schedule tables' content the rows were built for
  int T = 0;
  float lowres = 0.f;
  std::vector<char> row_ok;   // [T]: rows are built on demand, for the steps a call walks
  float build_ms = -1.f;      // device time and row count of the last build (kd_unet_cond_table_build_ms)
  int build_rows = 0, build_runs = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the last build; read lazily (ev_pending)
  bool ev_pending = false;
  int64_t refused_bytes = 0;   // > 0: the last sampling call wanted a table of this size and the cap / allocator refused
  ~CondTable() {
    if (tab) (void)hipFree(tab);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

struct Sampler {
  // scratch, allocated on first use at addresses that stay (the captured iterations hold them): UNet output, the
  // guidance forward's, x0 estimate, per-sample thresholds and times; EDM: x_hat, d and the UNet input of the step
  float *pred = nullptr, *pred_null = nullptr, *x0 = nullptr, *thresh = nullptr, *time = nullptr;
  float *xhat = nullptr, *d = nullptr, *net_in = nullptr;
  float* self_cond = nullptr;   // self_cond plans: the thresholded x0 estimate carried to the next forward [B,3,S,S]
  float* hist = nullptr;   // few-step solvers: the thresholded x0 estimate of the previous step [B,C,S,S]; with the first 2M call
  float* hist2 = nullptr;  // third-order solvers: with hist the two slots of a ring by step parity; with the first 3M call
  int* iter = nullptr;
  uint64_t* seed = nullptr;   // Philox keys [SEED_ROWS + B] (common.h), device-resident so the step graph does not depend on them
  void* qws = nullptr;
  DevBufs mem;
  DeviceTable ddpm_tab;   // 9 x T (kd_schedule_t)
  DeviceTable edm_tab;    // 15 x N (kd_edm_schedule_t), then S_noise
  DeviceTable solver_tab; // 9 x T (kd_solver_schedule_t), 10 x T with a coef_prev2 (kd_solver3_schedule_t)
  hipStream_t cap_stream = nullptr;
  StepGraph ddpm_graph, edm_graph[2];   // EDM: one per step kind (0: with the Heun correction, 1: without)
  StepGraph solver_graph[3];   // few-step solvers: 0 for a schedule that keeps no history (DDIM), 1 for one that does (2M), 2: the ring (3M)
  CondTable cond;
  void drop_graphs() {   // the conditioning table moved: every captured iteration holds its address
    ddpm_graph.drop();
    for (auto& g : edm_graph) g.drop();
    for (auto& g : solver_graph) g.drop();
  }
  ~Sampler() {
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
  }
};

}  // namespace kd

using namespace kd;

// ------------------------------------------------------------------------------ the UNet object
struct kd_unet {
  kd_unet_config_t cfg;
  std::vector<std::function<int(hipStream_t)>> ops;
  std::vector<std::string> op_label;  // per-op description + algorithmic MACs (kd_unet_profile)
  std::vector<int64_t> op_macs;
  std::vector<int64_t> op_mfma;  // MACs the op issues on the matrix cores (Winograd: 16/36 of op_macs, padded K)
  std::shared_ptr<WeightStore> wstore;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  int64_t macs = 0;       // algorithmic MACs of one forward as the reference computes it
  int64_t mfma_macs = 0;  // MACs the per-step conv / GEMM launches issue on the matrix cores
  int64_t mfma_bf16_macs = 0;  // ... bf16 MACs of the bf16x3 GEMMs (six per fp32 MAC; not part of mfma_macs)
  int time_cond_dim = 0;
  int self_cond = 0;   // Unet(self_cond=True): the init conv also reads in_self_cond (kd_unet_create_self_cond)
  // per level: LinearAttentionTransformerBlock at the attention slot where layer_attns is 0 (use_linear_attn); the level's
  // first ResnetBlocks' cross-attention is LinearCrossAttention (use_linear_cross_attn) - kd_unet_create_ext
  int lin_attn[KD_MAX_LEVELS] = {0};
  int lin_cross[KD_MAX_LEVELS] = {0};
  // the library's other resampling forms (kd_unet_ext_t): Downsample slots hold a CrossEmbedLayer (kernel sizes 2 and 4);
  // Upsample slots hold nearest x2 + conv3x3 instead of conv1x1 -> SiLU -> PixelShuffle
  int cross_embed_downsample = 0, upsample_nearest = 0;
  // Unet(combine_upsample_fmaps=True) (kd_unet_ext2_t): every up level's map goes through a Block of its own at full resolution
  // into the concat in front of final_res_block
  int combine_upsample_fmaps = 0;
  // Unet(layer_attns_depth=...) (kd_unet_ext3_t): (attention, feed-forward) pairs of level l's TransformerBlocks, >= 1
  int attn_depth[KD_MAX_LEVELS] = {1, 1, 1, 1, 1, 1, 1, 1};
  // the first and the last layer's structural switches (kd_unet_ext4_t), normalised: init_plain: one Conv2d of init_ks[0];
  // else a CrossEmbedLayer of the n_init_ks ascending sizes init_ks; final_ks: final_conv's kernel size; no_final_res:
  // final_conv reads the concat itself; skip_scale: 2^-1/2, or 1 with scale_skip_connection=False (then no scale pass runs)
  int init_plain = 0, n_init_ks = 3, init_ks[4] = {3, 7, 15, 0};
  int final_ks = 3, no_final_res = 0;
  int init_generic = 0;   // A/B: the init conv's per-step share on the generic conv path even where a one-kernel form applies
  float skip_scale = 0.70710678118654752440f;
  // per-call I/O (read by the ops at run time)
  const float *in_x = nullptr, *in_lowres = nullptr, *in_cond = nullptr, *in_log_snr = nullptr,
              *in_lowres_log_snr = nullptr, *in_text_tokens = nullptr, *in_text_hiddens = nullptr;
  const float* in_self_cond = nullptr;   // [B,3,S,S] or nullptr (zeros); read only by self_cond plans
  float* out = nullptr;
  // text-conditioning sub-plan (present iff cfg.cond_on_text && cfg.text_tokens > 0)
  std::vector<std::function<int(hipStream_t)>> text_ops;
  // step-invariant part of the forward (init conv over the cond / low-res planes): run once per
  // sampling call, before the captured per-step graph
  std::vector<std::function<int(hipStream_t)>> static_ops;
  int text_embed_dim = 0, max_text_len = 0;
  const float *in_text_embeds = nullptr, *in_text_mask = nullptr;
  int in_text_len = 0, in_text_drop = 0;
  float *out_text_tokens = nullptr, *out_text_hiddens = nullptr;
  kd::Sampler smp;   // sampler scratch, schedule tables, captured iterations, conditioning table (sampler.inc)

  // ---- step-invariant-per-schedule-index conditioning (time embeddings, FiLM scale / shift, time tokens and their
  // cross-attention K / V): ops flagged op_is_cond write only into the `cond_ws` region (offsets carry COND_FLAG); the
  // sampler can run them once per schedule step into `smp.cond` and replay a step with one gather instead
  static constexpr size_t COND_FLAG = size_t(1) << 62;
  std::vector<char> op_is_cond;
  char* cond_ws = nullptr;
  size_t cond_bytes = 0;
  // the tensors of the cond region (every one batch-major: the table is then built B schedule steps per run)
  std::vector<kd::CondSeg> cond_segs;
  bool cond_rows_ok = true;
  kd::CondSeg* d_cond_segs = nullptr;
  uint32_t cond_row_total = 0;
  void* x3_ws = nullptr;   // slabs of the bf16x3 GEMMs' left-over tiles, allocated with the first such layer (emit_x3_gemm)
  // CUs of the device the plan was built on, read once: every launch shape of the plan comes from this - its bf16x3 GEMMs
  // (X3Shape), its fp32 convs (ConvShape) and the persistent grids of the fused Winograd conv and the init convs
  int cus = 0;

  float* P(size_t off) const { return (float*)((off & COND_FLAG) ? cond_ws + (off & ~COND_FLAG) : ws + off); }
  ~kd_unet() {
    smp.drop_graphs();   // before the buffers they point into
    for (void* p : {(void*)ws, (void*)cond_ws, (void*)d_cond_segs, x3_ws})
      if (p) (void)hipFree(p);
  }
};

namespace kd {

// An address in the plan's workspace or cond region: known as a byte offset at build (the ops are emitted before either
// exists), a pointer once the op runs.  The null Ref (an absent residual, gate, partial buffer, FiLM row) yields nullptr.
struct Ref {
  const kd_unet* u = nullptr;
  size_t off = 0;   // as kd_unet::P takes it (COND_FLAG included)
  explicit operator bool() const { return u != nullptr; }
  float* f() const { return u ? u->P(off) : nullptr; }
  double* d() const { return (double*)f(); }
  Ref floats(int64_t n) const { return u ? Ref{u, off + (size_t)n * sizeof(float)} : Ref(); }   // moved on by n floats
  Ref doubles(int64_t n) const { return u ? Ref{u, off + (size_t)n * sizeof(double)} : Ref(); }
};

// ------------------------------------------------------------------------------ plan builder
struct Builder {
  kd_unet* u;
  Arena arena;
  std::unordered_map<std::string, std::pair<const float*, int64_t>> params;
  const kd_unet_config_t& cfg;
  int B;
  // batched time-MLP: every ResnetBlock's Linear(time_cond_dim, 2*dim_out) in one skinny GEMM
  std::vector<std::string> tmlp_prefixes;
  std::unordered_map<std::string, int> tmlp_off;
  int tmlp_total = 0;
  float *tmlp_w = nullptr, *tmlp_b = nullptr;
  T t_ss;  // [B, tmlp_total] scale|shift rows for all blocks
  // shared scratch
  T gn_stats_t, gn_partial_t;
  size_t gn_partial_max = 0;

  Builder(kd_unet* u_) : u(u_), cfg(u_->cfg), B(u_->cfg.batch) {}

  // ---- parameters
  bool has(const std::string& n) const { return params.count(n) != 0; }
  int64_t numel(const std::string& n) const {
    auto it = params.find(n);
    if (it == params.end()) throw std::runtime_error("missing parameter '" + n + "'");
    return it->second.second;
  }
  const float* raw(const std::string& n, int64_t expect = -1) {
    auto it = params.find(n);
    if (it == params.end()) throw std::runtime_error("missing parameter '" + n + "'");
    if (expect >= 0 && it->second.second != expect)
      throw std::runtime_error("parameter '" + n + "' has " + std::to_string(it->second.second) +
                               " elements, plan expects " + std::to_string(expect));
    return it->second.first;
  }
  // Engine-owned weight buffer `key` of this UNet: allocated and filled by `make(dst)` the first time any
  // plan of the UNet asks for it (the store is shared between plans, see kd_unet_create_shared).
  template <class F>
  float* cached(const std::string& key, size_t n_floats, F make) {
    auto& c = u->wstore->cache;
    auto it = c.find(key);
    if (it != c.end()) return it->second;
    float* dst = u->wstore->pool.alloc(n_floats);
    make(dst);
    c[key] = dst;
    return dst;
  }
  const float* P(const std::string& n, int64_t expect = -1) {  // engine-owned copy, torch layout
    const float* src = raw(n, expect);
    int64_t ne = numel(n);
    return cached("raw:" + n, (size_t)ne, [&](float* dst) {
      KD_HIP_THROW(hipMemcpyAsync(dst, src, (size_t)ne * sizeof(float), hipMemcpyDeviceToDevice, 0));
    });
  }
  const float* pack_conv(const std::string& n, int O, int I, int Ipad, int K) {
    const float* src = raw(n, (int64_t)O * I * K * K);
    return cached("tap:" + n + ":" + std::to_string(Ipad), (size_t)O * Ipad * K * K,
                  [&](float* dst) { KD_THROW_IF(launch_pack_oihw(src, dst, O, I, Ipad, K, K, 0)); });
  }

  const float* pack_conv_rowrun(const std::string& n, int O, int I, int Ipad, int K) {
    const float* src = raw(n, (int64_t)O * I * K * K);
    return cached("rowrun:" + n + ":" + std::to_string(Ipad), (size_t)O * Ipad * K * K,
                  [&](float* dst) { KD_THROW_IF(launch_pack_oihw_rowrun(src, dst, O, I, Ipad, K, K, 0)); });
  }

  const float* pack_conv_rowrun_sub(const std::string& n, int O, int Itot, int a0, int na, int b0, int nb, int Ipad,
                                    int K) {
    const float* src = raw(n, (int64_t)O * Itot * K * K);
    const std::string key = "rowrun_sub:" + n + ":" + std::to_string(a0) + "," + std::to_string(na) + "," +
                            std::to_string(b0) + "," + std::to_string(nb) + "," + std::to_string(Ipad);
    return cached(key, (size_t)O * Ipad * K * K, [&](float* dst) {
      KD_THROW_IF(launch_pack_oihw_rowrun_sub(src, dst, O, Itot, a0, na, b0, nb, Ipad, K, K, 0));
    });
  }

  // ---- where the ops being emitted go
  // Step: an ordinary per-step op (u->ops).
  // Cond: conditioning that depends on the inputs log_snr / lowres_log_snr / text only (never on x): in u->ops too, but
  //   flagged, and everything it allocates lives in the permanent cond region (bump-allocated, never reused), so the
  //   sampler can snapshot / restore that region per schedule step (kd::CondTable).
  // Static: step-invariant work, run once per sampling call (u->static_ops).
  // Text: the text-conditioning sub-plan (u->text_ops).
  enum class Phase { Step, Cond, Static, Text };
  Phase phase = Phase::Step;
  bool step_op() const { return phase == Phase::Step; }
  bool recorded() const { return phase == Phase::Step || phase == Phase::Cond; }   // in u->ops: a row of the profile
  struct PhaseScope {   // enters a phase; the previous one is back, once, when exit() is called or the scope ends (also by a throw)
    Builder& b;
    const Phase prev;
    bool exited = false;
    PhaseScope(Builder& b_, Phase p) : b(b_), prev(b_.phase) { b.phase = p; }
    PhaseScope(const PhaseScope&) = delete;
    void exit() {
      if (!exited) b.phase = prev;
      exited = true;
    }
    ~PhaseScope() { exit(); }
  };
  PhaseScope scope(Phase p) { return PhaseScope(*this, p); }
  // for what is a function of the conditioning tokens alone (their K / V): hoisted into the cond region, but for the text
  // sub-plan, which has none
  PhaseScope cond_scope() { return PhaseScope(*this, phase == Phase::Text ? Phase::Text : Phase::Cond); }

  // ---- activations
  size_t cond_end = 0;
  size_t cond_alloc(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    if (bytes == 0) bytes = 256;
    const size_t off = cond_end;
    cond_end += bytes;
    return kd_unet::COND_FLAG | off;
  }
  T alloc(int b, int h, int w, int c) {
    T t;
    t.B = b; t.H = h; t.W = w; t.C = c;
    const size_t bytes = (size_t)b * h * w * c * sizeof(float);
    if (phase == Phase::Cond) {
      t.off = cond_alloc(bytes);
      // batch-major: [B][...] as allocated, or a linear()'s flattened [1][1][B x tokens][N] (the batch still outermost)
      const size_t total = (size_t)b * h * w * c, row = total / (size_t)B;
      if ((b == B || (b == 1 && h == 1 && w % B == 0)) && row > 0 && row * B == total && row < (size_t(1) << 31))
        u->cond_segs.push_back(CondSeg{(uint32_t)((t.off & ~kd_unet::COND_FLAG) / 4), (uint32_t)row, 0});
      else
        u->cond_rows_ok = false;
      return t;
    }
    t.off = arena.alloc(bytes);
    refs[t.off] = 1;
    return t;
  }
  T alloc_bytes(size_t bytes) {
    T t;
    t.B = 1; t.H = 1; t.W = 1; t.C = (int)((bytes + 3) / 4);
    if (phase == Phase::Cond) {
      t.off = cond_alloc(bytes);
      u->cond_rows_ok = false;   // a cond tensor without batch rows: the table is built step by step
      return t;
    }
    t.off = arena.alloc(bytes);
    refs[t.off] = 1;
    return t;
  }
  // every builder function returns a tensor owned by the caller (refcount 1) and never releases
  // its inputs; skip connections take an extra reference with retain().
  std::unordered_map<size_t, int> refs;
  void retain(const T& t) {
    if (t.off & kd_unet::COND_FLAG) return;
    refs[t.off] += 1;
  }
  void free(const T& t) {
    if (t.off & kd_unet::COND_FLAG) return;   // the cond region is permanent
    auto it = refs.find(t.off);
    if (it == refs.end() || it->second <= 0) throw std::runtime_error("plan: release of a dead tensor");
    if (--it->second == 0) {
      refs.erase(it);
      arena.release(t.off);
      drop_seg_block(t.off);
    }
  }
  // ---- the addresses an op captures (Ref).  at: (row 0, channel 0) of t, the first channel of a slice; base: row 0 of the
  // block t lives in, for launches that take the channel offset on its own; a nullptr tensor gives the null Ref
  Ref at(const T& t) const { return Ref{u, t.at()}; }
  Ref base(const T& t) const { return Ref{u, t.off}; }
  Ref at(const T* t) const { return t ? at(*t) : Ref(); }
  // image b0 of the map t (a launch over a set of images starts at the set's first)
  Ref image(const T& t, int b0) const { return at(t).floats((int64_t)b0 * t.HW() * t.LD()); }
  Ref image(const T* t, int b0) const { return t ? image(*t, b0) : Ref(); }
  // image b0's FiLM scale | shift row of t_ss from column ss_col on (ss_col < 0: no FiLM, the null Ref) and t_ss's row stride
  struct Film { Ref row; int ld; };
  Film film(int ss_col, int b0 = 0) const { return {ss_col >= 0 ? at(t_ss).floats((int64_t)b0 * tmlp_total + ss_col) : Ref(), tmlp_total}; }
  // image b0's share of a partial buffer add_seg() reserved at workspace offset `off`: [B][nseg][nchunk][2] doubles
  Ref seg_at(size_t off, int nseg = 0, int nchunk = 0, int b0 = 0) const { return Ref{u, off}.doubles((int64_t)b0 * nseg * nchunk * 2); }
  // ---- GroupNorm partials handed from the kernel that writes a map to the layer that normalises it (SegSrc,
  // common.h): per tensor (keyed by its workspace offset) up to two channel ranges with their partial buffers.
  struct SegPart {
    size_t off = 0;   // partial buffer [B][nseg][nchunk][2] doubles
    int nseg = 0, nchunk = 0, c0 = 0;
    float scale = 1.0f, ab_mul = 1.0f;
    bool owned = true;   // false: the buffer belongs to another tensor's list (a copied skip tensor) that outlives this one
  };
  struct SegList {
    size_t block = 0;   // arena block of the tensor: the partials die with it
    std::vector<SegPart> parts;
  };
  std::unordered_map<size_t, SegList> seg_of;   // key: T::at() - a slice and its buffer have different keys
  const bool x3_planes_on = kd_switch("KD_X3_PLANES", 1) != 0;   // LayerNorm outputs read by one bf16x3 GEMM: in plane form
  void drop_seg_block(size_t block) {
    for (auto it = seg_of.begin(); it != seg_of.end();) {
      if (it->second.block == block) {
        for (auto& sp : it->second.parts)
          if (sp.owned) arena.release(sp.off);
        it = seg_of.erase(it);
      } else {
        ++it;
      }
    }
  }
  // `to` is a copy of `from` that dies first: it may use from's partials
  void share_seg(const T& from, const T& to) {
    auto it = seg_of.find(from.at());
    if (it == seg_of.end()) return;
    SegList l = it->second;
    l.block = to.off;
    for (auto& sp : l.parts) sp.owned = false;
    seg_of[to.at()] = l;
  }
  // a skip slice joins the concat that holds it: its partials become channels [c0, ..) of the whole buffer `to`
  void move_seg(const T& from, const T& to, int c0, float scale, float ab_mul) {
    auto it = seg_of.find(from.at());
    if (it == seg_of.end()) return;
    SegList moved = it->second;
    seg_of.erase(it);
    SegList& dst = seg_of[to.at()];
    dst.block = to.off;
    for (auto sp : moved.parts) {
      sp.c0 += c0;
      sp.scale *= scale;
      sp.ab_mul *= ab_mul;
      dst.parts.push_back(sp);
    }
  }
  // reserves the partial buffer of channels [c0, c0 + 16 nseg) of tensor t; returns its workspace offset
  size_t add_seg(const T& t, int c0, int nseg, int nchunk, float scale = 1.0f, float ab_mul = 1.0f) {
    SegPart sp;
    sp.off = arena.alloc((size_t)t.B * nseg * nchunk * 2 * sizeof(double));
    sp.nseg = nseg; sp.nchunk = nchunk; sp.c0 = c0; sp.scale = scale; sp.ab_mul = ab_mul;
    SegList& l = seg_of[t.at()];
    l.block = t.off;
    l.parts.push_back(sp);
    return sp.off;
  }
  // the sources covering ALL C channels of x in order (at most two), or false
  // (G: the GroupNorm's groups, 0 = cfg.resnet_groups)
  bool seg_sources(const T& x, SegPart (&out)[2], int& n, int G = 0) const {
    n = 0;
    if (G <= 0) G = cfg.resnet_groups;
    if (x.C % G || (x.C / G) % 16) return false;
    auto it = seg_of.find(x.at());
    if (it == seg_of.end()) return false;
    std::vector<SegPart> v = it->second.parts;
    std::sort(v.begin(), v.end(), [](const SegPart& a, const SegPart& b) { return a.c0 < b.c0; });
    int c = 0;
    for (auto& sp : v) {
      if (sp.c0 != c || n == 2) return false;
      out[n++] = sp;
      c += 16 * sp.nseg;
    }
    return c == x.C;
  }
  // emits the GroupNorm statistics of x into gn_stats_t - from the producer's partials when x has them (then
  // `ab` != nullptr also gets the folded affine in the same launch and true is returned), else by a pass over x
  bool emit_gn_stats(const T& x, const float* gamma, const float* beta, int ss_col, const T* ab) {
    const int G = cfg.resnet_groups, Bx = x.B, HW = x.HW(), C = x.C;
    SegPart sp[2];
    int n = 0;
    const Ref st = at(gn_stats_t);
    if (seg_sources(x, sp, n)) {
      const SegPart a = sp[0], b2 = n > 1 ? sp[1] : SegPart();
      const Ref pa = seg_at(a.off), pb = n > 1 ? seg_at(b2.off) : Ref(), abr = at(ab);
      const Film ss = film(ss_col);
      emit([=](hipStream_t s) {
        SegSrc s0{pa.d(), a.nseg, a.nchunk, a.c0, a.scale, a.ab_mul};
        SegSrc s1{pb.d(), b2.nseg, b2.nchunk, b2.c0, b2.scale, b2.ab_mul};
        return launch_gn_fold_seg(s0, s1, gamma, beta, ss.row.f(), ss.ld, abr.f(), st.f(), Bx, C, G, (double)HW * (C / G), 1e-5f, s);
      }, "gn fold seg HW" + std::to_string(HW) + " C" + std::to_string(C));
      return ab != nullptr;
    }
    if (gn_partial_bytes(Bx, HW, C, G) > gn_partial_max) throw std::runtime_error("gn partial scratch too small");
    const Ref xr = at(x), part = at(gn_partial_t);
    const int ldx = x.LD();
    emit([=](hipStream_t s) {
      return launch_gn_stats(xr.f(), ldx, st.f(), part.d(), Bx, HW, C, G, 1e-5f, s);
    }, "gn stats HW" + std::to_string(HW) + " C" + std::to_string(C));
    return false;
  }
  const float* P_(const std::string& n) { return P(n); }
  void emit(std::function<int(hipStream_t)> f, std::string label = "op", int64_t macs = 0) {
    if (!recorded()) {
      (phase == Phase::Text ? u->text_ops : u->static_ops).push_back(std::move(f));
      return;
    }
    u->ops.push_back(std::move(f));
    u->op_label.push_back(std::move(label));
    u->op_macs.push_back(macs);
    u->op_mfma.push_back(0);
    u->op_is_cond.push_back(phase == Phase::Cond ? 1 : 0);
  }
  // the MACs of the op just emitted: m as the reference computes it (the text sub-plan's are not the UNet's; the step-invariant
  // share of the init conv counts although it runs once per sampling call), `issued` on the matrix cores per step
  void count_macs(int64_t m, int64_t issued) {
    if (phase != Phase::Text) u->macs += m;
    if (recorded()) {
      u->mfma_macs += issued;
      u->op_mfma.back() = issued;
    }
  }

  // ---- conv / GEMM emission
  struct ConvOpt {
    int act = ACT_NONE;
    const T* res = nullptr;       // y += res
    const T* gate_src = nullptr;  // y += gate_src * gate
    const T* gate = nullptr;
    int out_mode = OUT_NHWC;
    const T* dst = nullptr;  // write into channel slice [yoff, yoff+Cout) of dst
    int yoff = 0;
    int cin_logical = -1;
    bool out_external = false;  // OUT_NCHW into u->out
    bool rowrun = false;        // small-Cin wide-window conv: weights from pack_conv_rowrun
    int res_coff = 0;           // channel offset into res (res row stride stays res->C)
    int64_t macs_override = -1; // algorithmic MACs when the launch computes padded / re-associated work
    int wz_rows = 0;            // batched 1x1 GEMM over the Winograd positions (ConvParams::wz_rows)
    int wz_count = 16;          // ... 16 positions of F(2x2,3x3), 36 of F(4x4,3x3)
    bool want_seg = false;      // the output feeds a GroupNorm: leave its partials in the epilogue where possible
    int seg_c0 = -1, seg_cn = 0;  // channel range of y the partial buffer spans (default: this launch's own range);
                                  // launches filling slices of one tensor name the same span and share the buffer
    int* seg_nchunk = nullptr;    // out: chunks per image of the GroupNorm partials the launch leaves, 0 = none
  };
  // What every layer on the bf16x3 kernel's epilogue form (kernels_gemm_bf16x3.hip) must pass: a default-algorithm plan's
  // ordinary step op, whole tiles and at least 64 of them, K of at least min_k where the launch runs whole rounds, and the
  // epilogue's own conditions for the launch shape this plan will use
  bool x3_epi_layer_ok(int64_t M, int Cout, int K, int min_k, const X3Epi& e) const {
    if (cfg.gemm_bf16x3 < 0 || cfg.conv_algo != 0 || cfg.x3_linear < 0 || !step_op()) return false;
    if (Cout % 128 || M % 256 || (M / 256) * (Cout / 128) < 64) return false;   // below 64 tiles the k-parts get too short
    // measured per launch against conv_buf_kernel at batch 16 (profiles/README.md, round 5): K >= 256 wins wherever the
    // launch runs whole rounds (256 -> 128 on the 256 x 256 map 748 -> 645 us); with fewer tiles than CUs every tile is cut
    // in k and a second launch adds the parts (10-15 us): K = 512 then only draws level (45.5 against 45.7 us), K >= 1024 wins
    // (K = 128 where the launch runs whole rounds: the 128 -> 512 upsample conv of the 128 x 128 map 455 -> 388 us)
    const X3Shape sh = gemm_bf16x3_shape(1, (int)M, Cout, K, u->cus);
    const bool cut = sh.needs_sum();
    if (K < (cfg.x3_linear > 0 ? cfg.x3_linear : cut ? 256 : min_k)) return false;
    if (cfg.x3_linear == 0 && K < 1024 && cut) return false;
    return gemm_bf16x3_epi_ok(M, Cout, K, e, sh);
  }
  // a 1x1 conv / token GEMM that runs on it
  bool x3_linear_ok(const T& x, int Cout, int K, int stride, int pad, const ConvOpt& o) const {
    if (K != 1 || stride != 1 || pad != 0 || o.rowrun || o.wz_rows || o.out_external) return false;
    if (o.out_mode != OUT_NHWC && o.out_mode != OUT_PIXSHUF) return false;
    if (o.gate_src && o.res) return false;
    if (x.C % 32 || (x.coff & 3)) return false;   // (the launch wants 16-byte aligned rows of A)
    X3Epi e;
    e.lda = x.LD();
    if (x.x3p && (!x.dense() || x.coff)) return false;
    e.ldy = o.dst ? o.dst->LD() : (o.out_mode == OUT_PIXSHUF ? Cout / 4 : Cout);
    e.res = o.res ? (const float*)16 : nullptr;
    e.ldres = o.res ? o.res->LD() : 0;
    e.gate_src = o.gate_src ? (const float*)16 : nullptr;
    e.gate = o.gate_src ? (const float*)16 : nullptr;
    e.ldgs = o.gate_src ? o.gate_src->LD() : 0;
    e.hw = x.H * x.W;
    e.act = o.act;
    e.pixshuf_wo = o.out_mode == OUT_PIXSHUF ? x.W : 0;
    return x3_epi_layer_ok(x.rows(), Cout, x.C, 128, e);
  }
  // images per launch of a 1x1 conv on the bf16x3 kernel: the whole batch, or - where the maps of the whole batch pass the
  // 2 GB its 32-bit offsets span (unet3's outer levels at batch 8) - the largest divisor of the batch that fits; 0 = not on it
  // (cfg.wino4_max_images, the test knob, cuts these launches too)
  int x3_linear_images(const T& x, int Cout, int K, int stride, int pad, const ConvOpt& o) const {
    const bool whole = x3_linear_ok(x, Cout, K, stride, pad, o);
    const int cap = cfg.wino4_max_images > 0 && whole ? cfg.wino4_max_images : x.B;
    if (whole && cap >= x.B) return x.B;
    if (x.B < 2 || x.x3p || cfg.x3_linear != 0) return whole ? x.B : 0;
    for (int ns = 2; ns <= x.B; ++ns) {
      if (x.B % ns) continue;
      T xs = x;
      xs.B = x.B / ns;
      if (xs.B <= cap && x3_linear_ok(xs, Cout, K, stride, pad, o)) return xs.B;
    }
    return whole ? x.B : 0;
  }
  // One bf16x3 GEMM of the plan, C[G][M][N] = A[G][M][K] W3[G][N][K]^T with A at `a` and C at `c` of the workspace: the
  // slabs of the k-parts (with the first such layer), the launch with the shape this plan's CU count gives, its MACs
  // (`macs` algorithmic, 6 G M N K bf16 issued), and the launch that adds the k-parts where that shape cuts tiles (its own
  // op: the whole chip adds them).  epi_of: yields the X3Epi at run time (the epilogue form, G = 1; applied by the summing
  // launch where there is one), or nullptr.  Rows of the profile: `stem` x3 (without an epilogue: `stem` gemm bf16x3) and
  // `stem` x3 sum, each followed by `shape`
  template <class EpiOf>
  void emit_x3_gemm(Ref a, const void* W3, Ref c, int G, int64_t M, int N, int K, bool a_f32, EpiOf epi_of,
                    const std::string& stem, const std::string& shape, int64_t macs) {
    constexpr bool has_epi = !std::is_same<EpiOf, std::nullptr_t>::value;
    if (!u->x3_ws) KD_HIP_THROW(hipMalloc(&u->x3_ws, gemm_bf16x3_workspace_bytes()));
    const X3Shape sh = gemm_bf16x3_shape(G, (int)M, N, K, u->cus);
    void* const x3_ws = u->x3_ws;   // (allocated once per plan, above: the address stays)
    auto launch = [=](hipStream_t s, bool sum) {   // the GEMM, or the launch that adds its k-parts
      X3Epi e;
      const X3Epi* ep = nullptr;
      if constexpr (has_epi) {
        e = epi_of();
        ep = &e;
      }
      if (sum) return launch_gemm_bf16x3_sum(c.f(), G, (int)M, N, K, sh, x3_ws, s, ep);
      return launch_gemm_bf16x3(a.f(), W3, c.f(), G, (int)M, N, K, sh, x3_ws, s, a_f32, false, ep);
    };
    emit([=](hipStream_t s) { return launch(s, false); }, stem + (has_epi ? " x3" : " gemm bf16x3") + shape, macs);
    u->macs += macs;
    u->op_mfma.back() = 6 * G * M * N * K;   // bf16 MACs
    u->mfma_bf16_macs += u->op_mfma.back();
    if (sh.needs_sum()) emit([=](hipStream_t s) { return launch(s, true); }, stem + " x3 sum" + shape);
  }
  T conv(const T& x, const float* w, const float* bias, int Cout, int K, int stride, int pad, const ConvOpt& o) {
    if (x.x3p && !x3_linear_ok(x, Cout, K, stride, pad, o))
      throw std::runtime_error("plan: a tensor in plane form reached a layer that is not a bf16x3 GEMM");
    int Ho = (x.H + 2 * pad - K) / stride + 1, Wo = (x.W + 2 * pad - K) / stride + 1;
    T y;
    if (o.dst) {
      y = *o.dst;
    } else if (o.out_mode == OUT_PIXSHUF) {
      y = alloc(x.B, 2 * Ho, 2 * Wo, Cout / 4);
    } else if (o.out_external) {
      y = T();
      y.B = x.B; y.H = Ho; y.W = Wo; y.C = Cout;
    } else {
      y = alloc(x.B, Ho, Wo, Cout);
    }
    ConvParams p{};
    p.w = w; p.bias = bias;
    p.B = x.B; p.Hi = x.H; p.Wi = x.W; p.Cin = x.C; p.ldx = x.LD();
    p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
    p.KH = K; p.KW = K; p.stride = stride; p.pad = pad;
    if (o.rowrun) {  // weights packed [KH][Cout][KW*C]: a kernel row is one contiguous K run (kernels_conv.hip)
      p.KW = 1;
      p.Cin = K * x.C;
      p.rr_cin = x.C;
    }
    p.wz_rows = o.wz_rows;
    p.wz_count = o.wz_rows > 0 ? o.wz_count : 0;
    p.act = o.act; p.out_mode = o.out_mode;
    p.ldy = (o.out_mode == OUT_NHWC || o.out_mode == OUT_PIXSHUF) ? y.LD() : 0;
    p.yoff = y.coff + o.yoff;   // (a slice destination: channels count from the slice's first)
    p.ldres = o.res ? o.res->LD() : 0;
    p.ldgs = o.gate_src ? o.gate_src->LD() : 0;
    const bool ext = o.out_external;
    const int res_coff = o.res_coff, o_yoff = o.yoff;
    const int Bset = x3_linear_images(x, Cout, K, stride, pad, o);   // > 0: on the bf16x3 kernel, this many images per launch
    // The launch shape, decided here once: what the plan knows of the pointers at its build is a fact (arena offsets count
    // from a hipMalloc base, every block starts on 256 bytes; weights have their addresses; an output the plan does not own
    // stays off the 16-byte path).  The scratch, the partials and the launch below all follow this one value
    const int seg_c0 = o.seg_c0 >= 0 ? o.seg_c0 : o.yoff;   // in channels of the tensor y (a slice counts from its own first)
    p.seg_c0 = y.coff + seg_c0;                              // block channel of the partial buffer's segment 0
    auto al16 = [](bool aligned, unsigned bit) { return aligned ? bit : 0u; };
    ConvPtrs ptrs;
    ptrs.has = CONV_Y | CONV_PARTIAL | (bias ? CONV_BIAS : 0) | (o.res ? CONV_RES : 0) | (o.gate_src ? CONV_GATE_SRC : 0) |
               (o.gate ? CONV_GATE : 0);
    ptrs.al16 = CONV_PARTIAL | al16(!ext && y.off % 16 == 0, CONV_Y) | al16((uintptr_t)bias % 16 == 0, CONV_BIAS) |
                al16(o.res && (o.res->at() + (size_t)res_coff * sizeof(float)) % 16 == 0, CONV_RES) |
                al16(o.gate_src && o.gate_src->at() % 16 == 0, CONV_GATE_SRC) | al16(o.gate && o.gate->at() % 16 == 0, CONV_GATE);
    const ConvShape sh = conv_shape(p, ptrs, u->cus);
    // small-M layers (batch-1 patches): split-K scratch, released right after the launch is recorded
    // (one in-order stream: the next op that reuses the block runs after the reduction)
    const int ks = sh.ksplit;
    T part;
    if (ks > 1) {   // (scratch of this launch pair, not conditioning state: never in the cond region / table)
      auto ph = scope(phase == Phase::Cond ? Phase::Step : phase);
      part = alloc_bytes((size_t)ks * x.B * Ho * Wo * Cout * sizeof(float));
    }
    const Ref partial = ks > 1 ? at(part) : Ref();
    // GroupNorm partials of the output, left by the epilogue (channels [yoff, yoff + Cout) of y, or the Cout / 4
    // shuffled channels): several launches filling slices of one tensor (init conv) share the chunk count
    size_t sego = 0;
    int seg_nseg = 0, seg_nchunk = 0;
    if (o.want_seg && !ext && step_op()) {
      const int cw = o.out_mode == OUT_PIXSHUF ? Cout / 4 : Cout;
      const int span = o.seg_c0 >= 0 ? o.seg_cn : cw;
      // (the bf16x3 form of a 1x1 conv whose tiles are cut in k leaves its partials from the summing launch, a chunk per 8 rows)
      const bool lin3 = Bset > 0;
      int nchunk = sh.seg_chunks > 0 && lin3 && o.out_mode == OUT_NHWC
                       ? Ho * Wo / gemm_bf16x3_shape(1, Bset * Ho * Wo, Cout, x.C, u->cus).seg_rows()
                       : sh.seg_chunks;
      // (the bf16x3 PixelShuffle epilogue takes maps 16 pixels wide - conv_buf_kernel's wants 32 - with the same chunks: four
      // sub-positions per 32 input pixels)
      if (lin3 && o.out_mode == OUT_PIXSHUF && nchunk == 0 && (Ho * Wo) % 32 == 0 && ((Cout >> 2) & 31) == 0)
        nchunk = (Ho * Wo / 32) * 4;
      if (nchunk > 0 && cw % 16 == 0 && span % 16 == 0 && o.yoff >= seg_c0 && o.yoff + cw <= seg_c0 + span) {
        SegPart* have = nullptr;
        auto it = seg_of.find(y.at());
        if (it != seg_of.end())
          for (auto& sp : it->second.parts)
            if (sp.c0 == seg_c0 && sp.nseg == span / 16 && sp.nchunk == nchunk) have = &sp;
        seg_nseg = span / 16;
        seg_nchunk = nchunk;
        sego = have ? have->off : add_seg(y, seg_c0, seg_nseg, nchunk);
      }
    }
    if (o.seg_nchunk) *o.seg_nchunk = seg_nseg ? seg_nchunk : 0;
    // ---- token GEMMs / 1x1 convs with K >= 512 as fp32 products on the bf16 matrix pipe (kernels_gemm_bf16x3.hip,
    // epilogue form: bias / residual / gate, strided rows; weights split into planes once per plan, the fp32 activations by
    // the kernel's loader waves; GroupNorm partials of the output where no tile is cut in k).  Layers with an activation
    // stay on conv_buf_kernel; cfg.conv_algo != 0 (the direct-convolution plans of the tests) too
    if (Bset > 0) {
      const int64_t M = (int64_t)Bset * Ho * Wo;   // rows of one launch: Bset images (the whole batch but for maps past 2 GB)
      const int Cin = x.C;
      const float* W3 = cached("x3lin:" + std::to_string((uintptr_t)w) + ":" + std::to_string(Cout) + "x" + std::to_string(Cin),
                               ((size_t)Cout * Cin * 3 + 1) / 2,
                               [&](float* dst) { KD_THROW_IF(launch_split3(w, dst, 1, Cout, Cin, 0)); });
      X3Epi base;
      base.bias = bias;
      base.ldres = p.ldres;
      base.ldgs = p.ldgs;
      base.hw = Ho * Wo;
      base.ldy = p.ldy;
      base.lda = p.ldx;
      base.act = o.act;
      base.pixshuf_wo = o.out_mode == OUT_PIXSHUF ? Wo : 0;
      const int seg_coff = o_yoff - seg_c0;
      for (int b0 = 0; b0 < x.B; b0 += Bset) {
        // (every per-image address is that of the set's first image)
        const Ref res = image(o.res, b0).floats(res_coff), gs = image(o.gate_src, b0), gate = image(o.gate, b0);
        const Ref seg = seg_nseg ? seg_at(sego, seg_nseg, seg_nchunk, b0) : Ref();
        auto epi_of = [=]() {
          X3Epi e = base;
          e.res = res.f();
          e.gate_src = gs.f();
          e.gate = gate.f();
          if (seg) {   // the output feeds a GroupNorm: its partials from the epilogue (of the summing launch where tiles are cut in k)
            e.seg = seg.d();
            e.seg_nseg = seg_nseg;
            e.seg_coff = seg_coff;
          }
          return e;
        };
        const std::string shape = " M" + std::to_string(M) + " Cin" + std::to_string(Cin) + " Cout" + std::to_string(Cout);
        const int64_t m = o.macs_override >= 0 ? o.macs_override : M * Cout * Cin;
        // (planes: written by the LayerNorm in front, the loader waves only move them)
        emit_x3_gemm(image(x, b0), W3, image(y, b0).floats(o_yoff), 1, M, Cout, Cin, !x.x3p, epi_of, "conv k1", shape, m);
      }   // sets of images
      if (ks > 1) free(part);
      return y;
    }
    const Ref xr = at(x), yr = base(y), res = at(o.res).floats(res_coff), gs = at(o.gate_src), gate = at(o.gate);
    const Ref seg = seg_nseg ? seg_at(sego) : Ref();
    const kd_unet* io = u;   // the plan's output buffer is a per-call argument, read when the op runs
    emit([=](hipStream_t s) {
      ConvParams q = p;
      q.x = xr.f();
      q.y = ext ? io->out : yr.f();
      q.res = res.f();
      q.gate_src = gs.f();
      q.gate = gate.f();
      q.partial = partial.f();
      if (seg) {
        q.seg_partial = seg.d();
        q.seg_nseg = seg_nseg;
      }
      return launch_conv_igemm(q, sh, s);
    });
    if (ks > 1) free(part);
    int cin = o.cin_logical > 0 ? o.cin_logical : x.C;
    int64_t m = o.macs_override >= 0 ? o.macs_override : (int64_t)x.B * Ho * Wo * Cout * cin * K * K;
    if (recorded()) {
      u->op_label.back() = "conv k" + std::to_string(K) + " s" + std::to_string(stride) + " M" +
                           std::to_string((int64_t)x.B * Ho * Wo) + " Cin" + std::to_string(x.C) + " Cout" +
                           std::to_string(Cout);
      u->op_macs.back() = m;
    }
    count_macs(m, (int64_t)x.B * Ho * Wo * Cout * p.Cin * p.KH * p.KW);
    return y;
  }
  // x, res and dst of a token GEMM as the [1][1][rows][C] maps conv() and x3_linear_ok() take (`o` points into this)
  struct FlatLinear {
    T x, res, dst;
    ConvOpt o;
    static T flat(const T& t) {
      T f = t;
      f.B = 1; f.H = 1; f.W = (int)t.rows();
      return f;
    }
    FlatLinear(const T& x_, const T* res_, const T* dst_, int act) : x(flat(x_)) {
      o.act = act;
      if (res_) {
        res = flat(*res_);
        o.res = &res;
      }
      if (dst_) {
        dst = flat(*dst_);
        o.dst = &dst;
      }
    }
    FlatLinear(const FlatLinear&) = delete;
  };
  // token GEMM y[M,N] = x[M,K] @ w[N,K]^T
  // `dst`: write into this tensor (a slice of a wider buffer: a skip tensor in its concat slot) instead of a new one
  T linear(const T& x, const float* w, const float* bias, int N, int act = ACT_NONE, const T* res = nullptr,
           const T* dst = nullptr) {
    const FlatLinear f(x, res, dst, act);
    T y = conv(f.x, w, bias, N, 1, 1, 0, f.o);
    y.B = x.B; y.H = x.H; y.W = x.W;
    return y;
  }
  // small-M linear on [M,K] rows living at x of the workspace (row stride ldx) -> [M,N] at y (row stride ldy)
  void skinny(Ref x, int ldx, const float* w, const float* bias, Ref y, int ldy, int M, int K, int N, int in_act, int act) {
    emit([=](hipStream_t s) {
      return launch_linear_skinny(x.f(), ldx, w, bias, y.f(), ldy, M, K, N, in_act, act, s);
    }, "skinny M" + std::to_string(M) + " K" + std::to_string(K) + " N" + std::to_string(N), (int64_t)M * K * N);
    if (phase != Phase::Text) u->macs += (int64_t)M * K * N;
  }

  // in_act: applied to x on the way in (ACT_GELU: the feed-forward's GELU when its GEMM stores the raw product);
  // g2 / y2: a second LayerNorm of the result in the same pass (y2 = LN(y) g2)
  // planes & 1 / & 2: y / y2 is read by one bf16x3 GEMM and nothing else - left as that kernel's three bf16 planes
  T layernorm(const T& x, const float* g, const float* beta, const T* res = nullptr, int in_act = ACT_NONE,
              const float* g2 = nullptr, T* y2 = nullptr, bool want_seg = false, int planes = 0) {
    if (!x3_planes_on || x.C % 16 || x.C > 4096 || !step_op()) planes = 0;
    auto alloc_out = [&](bool pl) {
      if (!pl) return alloc(x.B, x.H, x.W, x.C);
      T t = alloc_bytes((size_t)x.rows() * x.C * 6);
      t.B = x.B; t.H = x.H; t.W = x.W; t.C = x.C;
      t.x3p = true;
      return t;
    };
    if ((planes & 1) && want_seg) throw std::runtime_error("plan: GroupNorm partials of a LayerNorm output in plane form");
    T y = alloc_out(planes & 1);
    if (g2) *y2 = alloc_out(planes & 2);
    int rows = (int)x.rows(), C = x.C, ldx = x.LD(), ldres = res ? res->LD() : 0;
    // the output feeds a GroupNorm (the ResnetBlock's block2 behind its cross-attention): one chunk of partials per pixel
    const int hw = x.HW();
    const bool sg = want_seg && step_op() && C % 16 == 0 && C <= 4096 && x.B * hw == rows;
    const Ref seg = sg ? seg_at(add_seg(y, 0, C / 16, hw)) : Ref();
    const Ref xr = at(x), yr = at(y), rr = at(res), y2r = g2 ? at(*y2) : Ref();
    emit([=](hipStream_t s) {
      return launch_layernorm(xr.f(), ldx, g, beta, rr.f(), ldres, yr.f(), rows, C, 1e-5f, s, in_act, g2, y2r.f(), seg.d(), hw, planes);
    }, std::string(g2 ? "ln x2 rows" : "ln rows") + std::to_string(rows) + " C" + std::to_string(C) + (planes ? " planes" : ""));
    return y;
  }
  // would linear(x, .., N) run on the bf16x3 kernel (x3_linear_ok on the flattened rows)?
  // (x stands for a dense tensor of its shape: the LayerNorm output the GEMM will read)
  bool linear_is_x3(const T& x, int N, const T* res = nullptr, const T* dst = nullptr) const {
    FlatLinear f(x, res, dst, ACT_NONE);
    f.x.ld = 0; f.x.coff = 0;
    return x3_linear_ok(f.x, N, 1, 1, 0, f.o);
  }

  // GroupNorm -> [FiLM: scale/shift rows of t_ss at column ss_col] -> SiLU as its own pass (layers the fused conv
  // does not take)
  T gn_silu(const T& x, const std::string& prefix, int ss_col) {
    const float* gamma = P(prefix + ".weight", x.C);
    const float* beta = P(prefix + ".bias", x.C);
    int G = cfg.resnet_groups;
    T y = alloc(x.B, x.H, x.W, x.C);
    emit_gn_stats(x, gamma, beta, ss_col, nullptr);
    const Ref xr = at(x), yr = at(y), st = at(gn_stats_t);
    const Film ss = film(ss_col);
    int Bx = x.B, HW = x.HW(), C = x.C, ldx = x.LD();
    emit([=](hipStream_t s) {
      return launch_gn_apply_silu(xr.f(), ldx, st.f(), gamma, beta, ss.row.f(), ss.ld, yr.f(), Bx, HW, C, G, s);
    }, "gn apply HW" + std::to_string(HW) + " C" + std::to_string(C));
    return y;
  }

  // ---- attention similarity variants (cfg.attn_qk_norm, include/kd_engine.h)
  // (D = 0 in these helpers: cfg.attn_dim_head; cross_attn() passes the head width its module's weights have)
  float attn_scale(int D = 0) const {
    return cfg.attn_qk_norm == 1 ? 16.0f : cfg.attn_qk_norm == 2 ? 8.0f : 1.0f / sqrtf((float)(D ? D : cfg.attn_dim_head));
  }
  // in place on a workspace tensor: normalise (and scale) the `heads` dim_head-wide segments at the start of each row
  void qk_norm(const T& t, int ld, int heads, const float* scale_vec, int D = 0) {
    const Ref tr = at(t);   // (a column slice of a wider buffer: the fused q / kv projection)
    int64_t rows = t.rows();
    if (!D) D = cfg.attn_dim_head;
    emit([=](hipStream_t s) { return launch_l2norm_heads(tr.f(), ld, rows, heads, D, scale_vec, s); },
         "qk l2norm rows" + std::to_string(rows) + " heads" + std::to_string(heads));
  }
  const float* q_scale_of(const std::string& pre, int D = 0) { return cfg.attn_qk_norm == 2 ? P(pre + ".q_scale", D ? D : cfg.attn_dim_head) : nullptr; }
  const float* k_scale_of(const std::string& pre, int D = 0) { return cfg.attn_qk_norm == 2 ? P(pre + ".k_scale", D ? D : cfg.attn_dim_head) : nullptr; }
  // learned null key / value [2][D]; with qk-norm the key row is normalised (and scaled) once, at plan build
  const float* null_kv_of(const std::string& pre, int D = 0) {
    if (!D) D = cfg.attn_dim_head;
    const float* raw_nkv = P(pre + ".null_kv", 2 * D);
    if (!cfg.attn_qk_norm) return raw_nkv;
    const float* ks = k_scale_of(pre, D);
    return cached("null_kv_qknorm" + std::to_string(cfg.attn_qk_norm) + ":" + pre, (size_t)2 * D, [&](float* dst) {
      KD_HIP_THROW(hipMemcpyAsync(dst, raw_nkv, (size_t)2 * D * sizeof(float), hipMemcpyDeviceToDevice, 0));
      KD_THROW_IF(launch_l2norm_heads(dst, 2 * D, 1, 1, D, ks, 0));
    });
  }

  // ---- modules
  // cross attention of feature tokens to the conditioning tokens c [B,Nc,cond_dim]; returns attn(x)+x
  // Its heads are what the module's weights say (null_kv [2][D], to_q [H D][dim]): the library builds mid_block1 / mid_block2
  // without the UNet's attention kwargs - 8 heads of 64 whatever attn_heads / attn_dim_head - and every other ResnetBlock with
  // them.
  T cross_attn(const T& x, const std::string& pre, const T& c) {
    const int dim = x.C, D = (int)(numel(pre + ".null_kv") / 2), inner = (int)(numel(pre + ".to_q.weight") / dim);
    if (D != 32 && D != 64 && D != 128)
      throw std::runtime_error("'" + pre + "': the attention kernels are built for dim_head 32, 64 and 128");
    const int H = inner / D;
    if (H < 1 || H * D != inner) throw std::runtime_error("'" + pre + ".to_q.weight' is no whole number of heads");
    T xn = layernorm(x, P(pre + ".norm.g", dim), nullptr);
    T q = linear(xn, P(pre + ".to_q.weight", (int64_t)inner * dim), nullptr, inner);
    free(xn);
    T kv;
    {   // K / V of the conditioning tokens: a function of c alone (cond region, see Phase::Cond)
      auto ph = cond_scope();
      kv = linear(c, P(pre + ".to_kv.weight", (int64_t)2 * inner * c.C), nullptr, 2 * inner);
      if (cfg.attn_qk_norm) qk_norm(kv, 2 * inner, H, k_scale_of(pre, D), D);
    }
    const float* nkv = null_kv_of(pre, D);
    if (cfg.attn_qk_norm) qk_norm(q, inner, H, q_scale_of(pre, D), D);
    T o = alloc(x.B, x.H, x.W, inner);
    {
      const Ref qr = at(q), kr = at(kv), vr = kr.floats(inner), outr = at(o);
      int Bx = x.B, Nq = x.HW(), Nc = c.HW();
      float scale = attn_scale(D);
      emit([=](hipStream_t s) {
        KVSeg s0{kr.f(), vr.f(), 2 * inner, Nc};
        KVSeg s1{nullptr, nullptr, 0, 0};
        return launch_attention(qr.f(), inner, nkv, nkv + D, s0, s1, outr.f(), inner, Bx, Nq, H, H, D, scale, s);
      }, "xattn Nq" + std::to_string(Nq) + " Nk" + std::to_string(Nc + 1));
      u->macs += (int64_t)Bx * H * Nq * (Nc + 1) * D * 2;
    }
    free(q);
    free(kv);
    T proj = linear(o, P(pre + ".to_out.0.weight", (int64_t)dim * inner), nullptr, dim);
    free(o);
    T y = layernorm(proj, P(pre + ".to_out.1.g", dim), nullptr, &x, ACT_NONE, nullptr, nullptr, true);   // block2's GroupNorm reads it
    free(proj);
    return y;
  }

  // TransformerBlock: `depth` times x = attn(x, ctx) + x ; x = ff(x) + x, parameters `<pre>.layers.{i}.{0,1}.*`.  Every
  // layer has its own context K / V (a cond-region launch each); only the last layer's final GEMM writes into `dst`.
  // plain: the residual attention of earlier library versions (cfg.mid_attn_plain): parameters `<pre>.fn.fn.*`,
  // x = attn(x) + x and no feed-forward
  T transformer(const T& x, const std::string& pre, const T* ctx, const T* dst = nullptr, bool plain = false, int depth = 1) {
    if (plain) return transformer_layer(x, pre + ".fn.fn", std::string(), ctx, dst, true);
    if (depth < 1) throw std::runtime_error("plan: TransformerBlock depth must be at least 1");
    T cur = x;
    for (int i = 0; i < depth; ++i) {
      const std::string l = pre + ".layers." + std::to_string(i);
      T y = transformer_layer(cur, l + ".0", l + ".1", ctx, i == depth - 1 ? dst : nullptr, false);
      if (i > 0) free(cur);   // (x itself is the caller's)
      cur = y;
    }
    return cur;
  }
  // one (attention `a`, feed-forward `f`) pair of it
  T transformer_layer(const T& x, const std::string& a, const std::string& f, const T* ctx, const T* dst, bool plain) {
    int H = cfg.attn_heads, D = cfg.attn_dim_head, inner = H * D, dim = x.C;
    const bool qkv1 = cfg.conv_algo == 0 && kd_switch("KD_QKV_FUSED", 1) != 0;
    // (one reader - the fused q / k / v GEMM: where that runs on the bf16x3 kernel the LayerNorm leaves its planes)
    T xn = layernorm(x, P(a + ".norm.g", dim), nullptr, nullptr, ACT_NONE, nullptr, nullptr, false,
                     qkv1 && linear_is_x3(x, inner + 2 * D) ? 1 : 0);
    // to_q and to_kv read the same rows: one GEMM over the stacked weights [inner + 2 D][dim], q and k / v are column
    // slices of its output (the attention kernel takes row strides) - one launch less and fuller tiles
    const float* wq = P(a + ".to_q.weight", (int64_t)inner * dim);
    const float* wkv = P(a + ".to_kv.weight", (int64_t)2 * D * dim);
    T q, kv, qkv;
    if (qkv1) {
      const float* wqkv = cached("qkv:" + a, (size_t)(inner + 2 * D) * dim, [&](float* dst) {
        KD_HIP_THROW(hipMemcpyAsync(dst, wq, (size_t)inner * dim * sizeof(float), hipMemcpyDeviceToDevice, 0));
        KD_HIP_THROW(hipMemcpyAsync(dst + (size_t)inner * dim, wkv, (size_t)2 * D * dim * sizeof(float), hipMemcpyDeviceToDevice, 0));
      });
      qkv = linear(xn, wqkv, nullptr, inner + 2 * D);
      q = qkv;
      q.C = inner; q.ld = inner + 2 * D; q.coff = 0;
      kv = qkv;
      kv.C = 2 * D; kv.ld = inner + 2 * D; kv.coff = inner;
    } else {
      q = linear(xn, wq, nullptr, inner);
      kv = linear(xn, wkv, nullptr, 2 * D);
    }
    free(xn);
    T ckv;
    bool has_ctx = ctx != nullptr;
    if (has_ctx) {   // K / V of the context tokens: a function of c alone (cond region)
      auto ph = cond_scope();
      T cn = layernorm(*ctx, P(a + ".to_context.0.weight", ctx->C), P(a + ".to_context.0.bias", ctx->C));
      ckv = linear(cn, P(a + ".to_context.1.weight", (int64_t)2 * D * ctx->C), P(a + ".to_context.1.bias", 2 * D),
                   2 * D);
      free(cn);
      if (cfg.attn_qk_norm) qk_norm(ckv, 2 * D, 1, k_scale_of(a));
    }
    const float* nkv = null_kv_of(a);
    if (cfg.attn_qk_norm) {
      qk_norm(q, q.LD(), H, q_scale_of(a));
      qk_norm(kv, kv.LD(), 1, k_scale_of(a));
    }
    T o = alloc(x.B, x.H, x.W, inner);
    {
      const Ref qr = at(q), kr = at(kv), outr = at(o), ck = has_ctx ? at(ckv) : Ref();
      int Bx = x.B, N = x.HW(), Nc = has_ctx ? ctx->HW() : 0;
      const int ldq = q.LD(), ldkv = kv.LD();
      float scale = attn_scale();
      emit([=](hipStream_t s) {
        KVSeg s0{nullptr, nullptr, 0, 0};
        if (ck) s0 = KVSeg{ck.f(), ck.floats(D).f(), 2 * D, Nc};
        KVSeg s1{kr.f(), kr.floats(D).f(), ldkv, N};
        return launch_attention(qr.f(), ldq, nkv, nkv + D, s0, s1, outr.f(), inner, Bx, N, H, 1, D, scale, s);
      }, "attn N" + std::to_string(N));
      u->macs += (int64_t)Bx * H * N * (N + Nc + 1) * D * 2;
    }
    if (qkv1) {
      free(qkv);
    } else {
      free(q);
      free(kv);
    }
    if (has_ctx) free(ckv);
    T proj = linear(o, P(a + ".to_out.0.weight", (int64_t)dim * inner), nullptr, dim);
    free(o);
    if (plain) {
      T x1 = layernorm(proj, P(a + ".to_out.1.g", dim), nullptr, &x);
      free(proj);
      return x1;
    }
    // x1 = LN(proj) g + x and the feed-forward's first LayerNorm h0 = LN(x1) g' in one pass over the rows
    T h0;
    // the hidden width is what the block's own weights say: the library builds mid_attn with TransformerBlock's default
    // ff_mult = 2 whatever the UNet's ff_mult (cfg.ff_mult_x2) is, and the levels' blocks with the UNet's
    const int64_t ff_ne = numel(f + ".1.weight");
    if (ff_ne % dim || (ff_ne / dim) % 4) throw std::runtime_error("'" + f + ".1.weight' is no [4 n][" + std::to_string(dim) + "] matrix");
    const int hidden = (int)(ff_ne / dim);
    const bool gelu_late = linear_is_x3(proj, hidden);   // (h0 has proj's shape)
    T x1 = layernorm(proj, P(a + ".to_out.1.g", dim), nullptr, &x, ACT_NONE, P(f + ".0.g", dim), &h0, false, gelu_late ? 2 : 0);
    free(proj);
    // feed forward: Linear -> GELU -> LayerNorm -> Linear.  Where the first GEMM runs on the bf16x3 kernel (no activation
    // in its epilogue) it stores the raw product and the LayerNorm applies the GELU on the way in: the same function on the
    // same values
    T h1 = linear(h0, P(f + ".1.weight", (int64_t)hidden * dim), nullptr, hidden, gelu_late ? ACT_NONE : ACT_GELU);
    free(h0);
    T h2 = layernorm(h1, P(f + ".3.g", hidden), nullptr, nullptr, gelu_late ? ACT_GELU : ACT_NONE, nullptr, nullptr, false,
                     linear_is_x3(h1, dim, &x1, dst) ? 1 : 0);
    free(h1);
    T y = linear(h2, P(f + ".4.weight", (int64_t)dim * hidden), nullptr, dim, ACT_NONE, &x1, dst);
    free(h2);
    free(x1);
    return y;
  }

  // GlobalContext gate [B,1,1,C]
  T gca(const T& h, const std::string& pre) {
    int C = h.C, hid = std::max(3, C / 2);
    const float* wk = P(pre + ".to_k.weight", C);
    const float* bk = P(pre + ".to_k.bias", 1);
    const float* w0 = P(pre + ".net.0.weight", (int64_t)hid * C);
    const float* b0 = P(pre + ".net.0.bias", hid);
    const float* w2 = P(pre + ".net.2.weight", (int64_t)C * hid);
    const float* b2 = P(pre + ".net.2.bias", C);
    int Bx = h.B, HW = h.HW();
    const Ref hr = at(h);
    if (gca_gate_fused_ok(C, hid) && h.B > 1 && kd_switch("KD_GCA_FUSED", 1)) {   // (a batch-1 patch: one workgroup would stream the weights alone)
      T scratch = alloc_bytes(gca_scratch_floats(h.B, h.HW(), C) * sizeof(float));
      T gate = alloc(h.B, 1, 1, C);
      const Ref sr = at(scratch), gr = at(gate);
      emit([=](hipStream_t s) {
        return launch_gca_gate(hr.f(), wk, bk, sr.f(), w0, b0, hid, w2, b2, gr.f(), Bx, HW, C, s);
      }, "gca_gate HW" + std::to_string(HW) + " C" + std::to_string(C));
      u->macs += (int64_t)Bx * HW * C * 2 + (int64_t)Bx * C * hid * 2;
      free(scratch);
      return gate;
    }
    T logits = alloc(h.B, h.H, h.W, 1);
    T pooled = alloc(h.B, 1, 1, C);
    T scratch = alloc_bytes(gca_scratch_floats(h.B, h.HW(), C) * sizeof(float));
    const Ref lr = at(logits), pr = at(pooled), sr = at(scratch);
    emit([=](hipStream_t s) {
      return launch_gca_pool(hr.f(), wk, bk, lr.f(), pr.f(), sr.f(), Bx, HW, C, s);
    }, "gca_pool HW" + std::to_string(HW) + " C" + std::to_string(C));
    u->macs += (int64_t)Bx * HW * C * 2;
    free(logits);
    free(scratch);
    T hidden = alloc(h.B, 1, 1, hid);
    skinny(at(pooled), C, w0, b0, at(hidden), hid, h.B, C, hid, ACT_NONE, ACT_SILU);
    free(pooled);
    T gate = alloc(h.B, 1, 1, C);
    skinny(at(hidden), hid, w2, b2, at(gate), C, h.B, hid, C, ACT_NONE, ACT_SIGMOID);
    free(hidden);
    return gate;
  }

  // ---- The path of a ResnetBlock 3x3 conv, the `Block` = GroupNorm -> [FiLM] -> SiLU -> conv3x3 (gn_conv3x3): Winograd
  // F(4x4,3x3) as 36 batched GEMMs (wino4_block), F(2x2,3x3) as 16 batched GEMMs (wino_block), the fused F(2x2,3x3) kernel
  // with the GroupNorm folded in (fwino_gn_conv), or gn_silu + the direct conv.  Decided here alone: resnet() dispatches on
  // it, and SkipStack::pop (unet_build.inc) asks it whether the layer takes a skip concat's 2^-1/2 itself - Wino4 through its
  // input transform's affine, WinoFused through the GroupNorm partials' ab_mul (SegPart); the other two read the skip half
  // scaled in memory.
  enum class Conv3x3 { Wino4, WinoGemm, WinoFused, Direct };
  struct Conv3x3Choice { Conv3x3 algo; int images; };   // images: Wino4's images per launch set (wino4_images)
  Conv3x3Choice conv3x3_choice(const T& x, int cout) const {
    const int images = wino4_images(x, cout);
    if (images > 0) return {Conv3x3::Wino4, images};
    const bool fused = fwino_ok(x, cout);
    // Winograd F(2x2,3x3) as batched GEMMs (kernels_wino.hip).  Worth it where the 2.25x smaller GEMM outweighs moving 4x
    // the map through the transforms: measured on MI355X, Cin >= 256 wins and Cin = 128 loses (profiles/README.md).
    // cfg.conv_algo: 0 auto, 1 never, >= 32 explicit Cin threshold (experiments, tests).
    auto gemm_ok = [&] {
      if (cfg.conv_algo == 1 || cfg.conv_algo == 4) return false;
      const int min_cin = cfg.conv_algo >= 32 ? cfg.conv_algo : 256;
      // the fused kernel (fwino_ok) takes every layer whose map it can tile and whose launch fills the chip, up to the
      // Cin its affine table holds.  Measured on the 64->256 UNet, ms/step with the hand-over at Cin <= 0 / 256 / 512 /
      // 1024 / all: 48.1 / 44.8 / 44.5 / 45.1 / 45.3 with the eight-wave kernel of round 1 (its Cin = 1024 launches lost
      // to the batched GEMMs), 37.59 / 37.36 / 37.40 at <= 512 / 1024 / 2048 with the persistent sixteen-wave kernel
      // (300 us against 265 + 40 + 21 for GEMM + transforms).
      if (cfg.conv_algo < 32 && fused) return false;
      if ((x.H & 1) || (x.W & 1) || x.C < min_cin || x.C % 32 || cout <= 32 || cout % 4) return false;
      const int64_t Mt = (int64_t)x.B * (x.H / 2) * (x.W / 2);
      return Mt % 256 == 0 && 16 * Mt < 0x7fffffff && (int64_t)16 * cout * x.C * 4 < 0x7fffffff;
    };
    if (gemm_ok()) return {Conv3x3::WinoGemm, 0};
    // the fused kernel with the GroupNorm folded in: the per-image affine table sits in LDS, one image's map under 2^31 bytes
    if (fused && x.C <= wino_fused_gn_max_cin() && x.C % cfg.resnet_groups == 0 && (int64_t)x.H * x.W * x.LD() * 4 < 0x7fffffff)
      return {Conv3x3::WinoFused, 0};
    return {Conv3x3::Direct, 0};
  }
  // ---- fused Winograd F(2x2,3x3) + GroupNorm / FiLM / SiLU (kernels_wino_fused128.hip): every ResnetBlock 3x3 conv
  // whose map the kernel can tile (H % 8, W % 16, Cout % 128: all reference configs; a reduced-width model's narrow
  // levels take the batched-GEMM or the direct path).  cfg.conv_algo 0: wherever the shape fits and the launch fills
  // the chip; 1 and 2: never (2 = the batched-GEMM Winograd path only); 3: wherever the shape fits (tests).
  bool fwino_ok(const T& x, int cout) const {
    if (cfg.conv_algo == 1 || cfg.conv_algo == 2) return false;
    if (x.C < 32 || !wino_fused128_ok(x.B, x.H, x.W, x.C, cout)) return false;
    if (cfg.conv_algo == 3) return true;
    return (int64_t)x.B * (x.H / 16) * (x.W / 16) * (cout / 64) >= 256;  // one workgroup per CU and round
  }
  // ---- Winograd F(4x4,3x3) (kernels_wino4.hip): 36 batched GEMMs over tiles of 4x4 outputs, 4x fewer MFMA issues than
  // the direct conv and 1.78x fewer than F(2x2,3x3), for V / D transform buffers of 2.25x the map.  cfg.conv_algo 0:
  // layers with Cin >= cfg.wino43_min_cin (default 512) whose GEMMs fill the chip - measured against the fused
  // F(2x2,3x3) kernel at batch 16 (profiles/README.md); 4: wherever the shape fits (tests); 1 / 2 / 3 / >= 32: never.
  // images per launch set of a F(4x4,3x3) layer: the whole batch where the rule below takes it, otherwise (default plan with
  // the bf16x3 GEMMs) the largest divisor of the batch whose V / D / maps stay inside what a buffer resource spans (4 GB) -
  // unet3's 512 x 512 and 1024 x 1024 levels at batch 8, which otherwise fall back to the fused F(2x2,3x3) kernel; 0 = not a
  // F(4x4,3x3) layer
  int wino4_images(const T& x, int cout) const {
    const int cap = cfg.wino4_max_images > 0 ? cfg.wino4_max_images : x.B;
    if (cap >= x.B && wino4_whole_ok(x, cout)) return x.B;
    if (cap >= x.B && (cfg.conv_algo != 0 || cfg.wino43_min_cin != 0 || cfg.gemm_bf16x3 < 0 || !recorded())) return 0;
    if (cap < x.B && !wino4_whole_ok(x, cout)) return 0;   // (the test knob cuts layers the plan takes, nothing else)
    for (int ns = 2; ns <= x.B; ++ns) {
      if (x.B % ns) continue;
      T xs = x;
      xs.B = x.B / ns;
      if (xs.B > cap || (int64_t)xs.B * x.H * x.W * x.LD() * 4 >= ((int64_t)1 << 32)) continue;
      const int64_t Mt = (int64_t)xs.B * (x.H / 4) * (x.W / 4);
      if (cap >= x.B && ((x.H & 3) || (x.W & 3) || !gemm_bf16x3_ok(36, Mt, cout, x.C))) continue;
      if (wino4_whole_ok(xs, cout)) return xs.B;
    }
    return 0;
  }
  bool wino4_whole_ok(const T& x, int cout) const {
    if (cfg.conv_algo != 0 && cfg.conv_algo != 4) return false;
    if (cfg.wino43_min_cin < 0 && cfg.conv_algo == 0) return false;
    if ((x.H & 3) || (x.W & 3) || x.C % 32 || cout % 64 || cout < 64) return false;
    const int64_t Mt = (int64_t)x.B * (x.H / 4) * (x.W / 4);
    if (Mt % 128 || 36 * Mt >= 0x7fffffff || (int64_t)36 * cout * x.C * 4 >= 0x7fffffff) return false;
    if (cfg.conv_algo == 4) return true;
    if ((36 * Mt / 128) * (cout / 64) < 512) return false;   // the 36 GEMMs must fill the chip
    // default threshold Cin >= 512.  Below it the transform passes (6.5 x the map through HBM) eat the GEMM saving:
    // same-box A/B against the fused F(2x2,3x3) kernel at batch 16: 256 -> 256 at 64 x 64 299 -> 286 us (-4 %, not
    // worth six times the per-conv rounding error), 256 -> 128 at 128 x 128 626 -> 737 (+18 %), at 256 x 256 +17 %
    // (round 4, with the input transform 13 % faster: Cin = 256 on the 64 x 64 level alone, 9 layers, gives 32.74 -> 32.59 ms
    // per forward - 0.5 % for six times those layers' rounding error: the threshold stays at 512)
    // With the position GEMMs on the bf16 pipe (bf16x3, 1.5 x the fp32 MFMA rate) the hand-over moves down to Cin >= 256
    // on maps of up to 65536 pixels - same box, per layer: 256 -> 256 at 64 x 64 (batch 16) 330 us fused F(2x2,3x3) against
    // 129 + 82 + 48 (GEMM + transforms), nine layers, -0.64 ms per forward; the larger maps stay: 256 -> 128 at 128 x 128
    // 688 against 256 + 378 + ~100, at 256 x 256 2618 against 934 + 1514 + ~400 (the transforms write 3.4 x the map)
    int thr = cfg.wino43_min_cin > 0 ? cfg.wino43_min_cin : 512;
    // (round 5: 256 -> 256 on larger maps as well - unet3's 256 x 256 level at batch 8, 524288 pixels: 2.62 ms fused against
    // 8 x (117 + 78 + 49 + 12) us for the same pixels at batch 1; what loses above 65536 pixels is Cout = 128, whose GEMMs
    // are half as wide for the same transform traffic)
    // (later in round 5, with the input transform's loads issued together - 185 -> 121 us at 65536 pixels x 512 channels -
    // Cout = 128 wins as well: 256 -> 128 at 128 x 128 698 us fused against 241 + 258 + 80, at 256 x 256 2639 against 1031 + 934
    // + 299; same-box bench 27.81 / 27.89 -> 27.56 / 27.62 ms: the rule is Cin >= 256 wherever the bf16x3 GEMM takes the shape)
    // (end of round 5: Cin = 128 too, with V of those HBM-bound layers kept in fp32 - wino4_block -: 128 -> 128 at 256 x 256
    // 1509 us fused against 332 + 608 + 333, at 128 x 128 375 against 88 + 166 + 88)
    if (cfg.wino43_min_cin == 0 && cfg.gemm_bf16x3 >= 0 && gemm_bf16x3_ok(36, Mt, cout, x.C)) thr = 128;
    return x.C >= thr;
  }
  // Bx images per set of launches (wino4_images): V and D are one set's, the sets run one after the other.
  // skip_c0 >= 0: channels [skip_c0, ..) of x hold an unscaled skip tensor the layer must see times skip_scale: the input
  // transform folds the factor into its affine (the statistics come from partials that carry the scale: SkipStack::pop)
  T wino4_block(const T& x, int Bx, const std::string& gn_prefix, int ss_col, const std::string& conv_prefix, int Cout,
                const T* res, int skip_c0, float skip_scale) {
    const int Cin = x.C, G = cfg.resnet_groups, H = x.H, W = x.W, HW = x.HW(), nset = x.B / Bx;
    const int64_t Mt = (int64_t)Bx * (H / 4) * (W / 4);
    const float* gamma = P(gn_prefix + ".weight", Cin);
    const float* beta = P(gn_prefix + ".bias", Cin);
    const float* bias = P(conv_prefix + ".bias", Cout);
    const float* wsrc = raw(conv_prefix + ".weight", (int64_t)Cout * Cin * 9);
    float* U = cached("wino4:" + conv_prefix, (size_t)36 * Cout * Cin,
                      [&](float* dst) { KD_THROW_IF(launch_wino4_pack(wsrc, dst, Cout, Cin, 0)); });
    emit_gn_stats(x, gamma, beta, ss_col, nullptr);
    // the 36 GEMMs as fp32-class products on the bf16 matrix pipe (kernels_gemm_bf16x3.hip) where the shape fits its tile
    const bool x3 = cfg.gemm_bf16x3 >= 0 && recorded() && gemm_bf16x3_ok(36, Mt, Cout, Cin);
    // V written as planes by the input transform, or as fp32, split by the GEMM's loader waves on the way into LDS: the
    // transform then writes a third less and is that much faster, but the loaders' vector work beside the MFMA waves costs a
    // GEMM that is bound by the matrix pipe 10-15 %.  Per layer (same box, batch 16, transform + GEMM in us, planes / fp32;
    // with the loader waves' loads three stages in flight, kernels_gemm_bf16x3.hip):
    //   128 -> 128 at 256 x 256 480 + 568 / 336 + 526    256 -> 128 at 256 x 256 1028 + 935 / 671 + 858
    //   128 -> 128 at 128 x 128 118 + 168 / 90 + 146     256 -> 128 at 128 x 128 241 + 256 / 164 + 238
    //   256 -> 256 at 64 x 64 65.5 + 112 / 50.5 + 121    512 -> 256 at 64 x 64 123 + 190 / 90 + 215
    //   512 -> 512 at 32 x 32 28.5 + 103 / 25.5 + 115    1024 -> 1024 at 16 x 16 19.6 + 102 / 16.8 + 113
    // fp32 wins where the GEMM itself waits for HBM - few MACs per byte of V and D: Cin Cout / (6 Cin + 4 Cout) < 40 (12.8 ...
    // 32 for the rows that win, 51 upwards for those that lose).  cfg.gemm_bf16x3: 0 = by that rule, 1 = planes, 2 = fp32
    const bool v_f32 = cfg.gemm_bf16x3 == 2 || (cfg.gemm_bf16x3 == 0 && (int64_t)Cin * Cout < 40 * (6 * (int64_t)Cin + 4 * Cout));
    const bool x3_planes = x3 && !v_f32;
    T V = x3_planes ? alloc_bytes((size_t)36 * Mt * Cin * 6) : alloc(1, 1, (int)(36 * Mt), Cin);
    T D = alloc(1, 1, (int)(36 * Mt), Cout);
    T y = alloc(x.B, H, W, Cout);
    const std::string shape = " M" + std::to_string((int64_t)Bx * HW) + " Cin" + std::to_string(Cin) + " Cout" +
                              std::to_string(Cout);
    const bool sg = Cout % 64 == 0;   // GroupNorm partials of y for whichever layer normalises it next
    const int seg_nchunk = (H / 4) * (W / 4);
    const size_t sgo_all = sg ? add_seg(y, 0, Cout / 16, seg_nchunk) : 0;
    const Ref vr = at(V), dr = at(D);
    for (int st = 0; st < nset; ++st) {
      const int b0 = st * Bx;   // first image of the set
      {
        const Ref xr = image(x, b0), sr = at(gn_stats_t).floats((int64_t)b0 * G * 2);
        const Film ss = film(ss_col, b0);
        const int ldx = x.LD();
        emit([=](hipStream_t s) {
          if (x3_planes)
            return launch_wino4_in3(xr.f(), ldx, sr.f(), gamma, beta, ss.row.f(), ss.ld, vr.f(), Bx, H, W, Cin, G, s, skip_c0, skip_scale);
          return launch_wino4_in(xr.f(), ldx, sr.f(), gamma, beta, ss.row.f(), ss.ld, vr.f(), Bx, H, W, Cin, G, s, skip_c0, skip_scale);
        }, (x3_planes ? "wino4_in3" : "wino4_in") + shape);
      }
      if (x3) {
        const float* U3 = cached("wino4x3:" + conv_prefix, ((size_t)36 * Cout * Cin * 3 + 1) / 2,
                                 [&](float* dst) { KD_THROW_IF(launch_split3(U, dst, 36, Cout, Cin, 0)); });
        // (the algorithmic MACs of the 3x3 conv it replaces)
        emit_x3_gemm(vr, U3, dr, 36, Mt, Cout, Cin, !x3_planes, nullptr, "wino4", shape, (int64_t)Bx * HW * Cout * Cin * 9);
      } else {
        ConvOpt o;
        o.wz_rows = (int)Mt;
        o.wz_count = 36;
        o.dst = &D;
        o.macs_override = (int64_t)Bx * HW * Cout * Cin * 9;   // the algorithmic MACs of the 3x3 conv it replaces
        conv(V, U, nullptr, Cout, 1, 1, 0, o);
        if (recorded()) u->op_label.back() = "wino4 gemm" + shape;
      }
      {
        const Ref seg = sg ? seg_at(sgo_all, Cout / 16, seg_nchunk, b0) : Ref(), yr = image(y, b0), rr = image(res, b0);
        const int ldres = res ? res->LD() : 0;
        emit([=](hipStream_t s) {
          return launch_wino4_out(dr.f(), bias, rr.f(), ldres, yr.f(), Cout, seg.d(), Bx, H, W, Cout, s);
        }, "wino4_out" + shape);
      }
    }   // sets
    free(V);
    free(D);
    return y;
  }

  T wino_block(const T& x, const std::string& gn_prefix, int ss_col, const std::string& conv_prefix, int Cout,
               const T* res) {
    const int Cin = x.C, G = cfg.resnet_groups, Bx = x.B, H = x.H, W = x.W, HW = x.HW();
    const int64_t Mt = (int64_t)Bx * (H / 2) * (W / 2);
    const float* gamma = P(gn_prefix + ".weight", Cin);
    const float* beta = P(gn_prefix + ".bias", Cin);
    const float* bias = P(conv_prefix + ".bias", Cout);
    const float* wsrc = raw(conv_prefix + ".weight", (int64_t)Cout * Cin * 9);
    float* U = cached("wino:" + conv_prefix, (size_t)16 * Cout * Cin,
                      [&](float* dst) { KD_THROW_IF(launch_wino_pack(wsrc, dst, Cout, Cin, 0)); });
    // The map can be walked in slices of tiles (V and D are 4x the slice each) to bound the workspace:
    // cfg.wino_slice_mb caps V+D per slice.  Default: one slice - slices small enough to stay in the
    // 256 MB Infinity Cache were measured and are slower (56.5 ms/step unsliced, 59.3 at 96 MB,
    // 57.5 at 192 MB): the cache does not turn the V/D round trip into hits.
    const int64_t slice_mb = cfg.wino_slice_mb;
    int64_t nt_slice = Mt;
    if (slice_mb > 0) {
      nt_slice = (slice_mb << 20) / (64 * (int64_t)(Cin + Cout)) / 256 * 256;
      nt_slice = std::min(Mt, std::max<int64_t>(nt_slice, 256));
    }
    emit_gn_stats(x, gamma, beta, ss_col, nullptr);
    T V = alloc(1, 1, (int)(16 * nt_slice), Cin);
    T D = alloc(1, 1, (int)(16 * nt_slice), Cout);
    T y = alloc(Bx, H, W, Cout);
    // GroupNorm partials of y from the output transform (one chunk per 2x2 tile) for whichever layer normalises it next
    const bool sg = Cout % 16 == 0;
    const Ref seg = sg ? seg_at(add_seg(y, 0, Cout / 16, (H / 2) * (W / 2))) : Ref();
    const std::string shape = " M" + std::to_string((int64_t)Bx * HW) + " Cin" + std::to_string(Cin) + " Cout" +
                              std::to_string(Cout);
    const Ref xr = at(x), vr = at(V), dr = at(D), yr = at(y), rr = at(res), st = at(gn_stats_t);
    const Film ss = film(ss_col);
    const int ldx = x.LD(), ldres = res ? res->LD() : 0;
    for (int64_t t0 = 0; t0 < Mt; t0 += nt_slice) {
      const int64_t nt = std::min(nt_slice, Mt - t0);
      emit([=](hipStream_t s) {
        return launch_wino_in(xr.f(), ldx, st.f(), gamma, beta, ss.row.f(), ss.ld, vr.f(), Bx, H, W, Cin, G, t0, nt, s);
      }, "wino_in" + shape);
      T Vs = V, Ds = D;
      Vs.W = (int)(16 * nt);
      Ds.W = (int)(16 * nt);
      ConvOpt o;
      o.wz_rows = (int)nt;
      o.dst = &Ds;
      o.macs_override = nt * 4 * Cout * Cin * 9;  // algorithmic MACs of the share of the 3x3 conv it replaces
      conv(Vs, U, nullptr, Cout, 1, 1, 0, o);
      if (recorded()) u->op_label.back() = "wino gemm" + shape;
      emit([=](hipStream_t s) {
        return launch_wino_out(dr.f(), bias, rr.f(), ldres, yr.f(), Bx, H, W, Cout, t0, nt, s, seg.d());
      }, "wino_out" + shape);
    }
    free(V);
    free(D);
    return y;
  }

  // The fused F(2x2,3x3) layer straight from the un-normalised block input: GroupNorm statistics, the per-(image, channel)
  // affine fold, and the fused kernel that applies GroupNorm / FiLM / SiLU to the raw patch in LDS
  // (wino_fused_gn_kernel): the activated map is never written.
  T fwino_gn_conv(const T& x, const std::string& gn_prefix, int ss_col, const std::string& conv_prefix, int Cout,
                  const T* res) {
    const int Cin = x.C, G = cfg.resnet_groups, Bx = x.B, H = x.H, W = x.W;
    const float* gamma = P(gn_prefix + ".weight", Cin);
    const float* beta = P(gn_prefix + ".bias", Cin);
    const float* bias = P(conv_prefix + ".bias", Cout);
    const float* wsrc = raw(conv_prefix + ".weight", (int64_t)Cout * Cin * 9);
    float* U = cached("winof_gn128:" + conv_prefix, (size_t)16 * Cout * Cin,
                      [&](float* dst) { KD_THROW_IF(launch_wino_fused128_pack(wsrc, dst, Cout, Cin, 0, WF_U_SCALE)); });
    T ab = alloc_bytes((size_t)Bx * Cin * 2 * sizeof(float));
    T y = alloc(Bx, H, W, Cout);
    const Ref abr = at(ab);
    // statistics: from the partials x's producer left (one launch gives the folded affine too), else a pass over x
    if (!emit_gn_stats(x, gamma, beta, ss_col, &ab)) {
      const Ref st = at(gn_stats_t);
      const Film ss = film(ss_col);
      emit([=](hipStream_t s) { return launch_gn_fold(st.f(), gamma, beta, ss.row.f(), ss.ld, abr.f(), Bx, Cin, G, s); },
           "gn fold C" + std::to_string(Cin));
    }
    // the epilogue leaves the partials of y for whichever GroupNorm reads it next (block2, or the next block)
    const bool so_ = Cout % 16 == 0;
    const Ref seg = so_ ? seg_at(add_seg(y, 0, Cout / 16, (int)wino_fused_out_stats_chunks(H, W, Cout, Cout / 16))) : Ref();
    const Ref xr = at(x), yr = at(y), rr = at(res);
    const int ldres = res ? res->LD() : 0, ldx = x.LD();
    const int64_t m = (int64_t)Bx * H * W * Cout * Cin * 9;
    // id -> (image, y0, x0, slab) of the kernel's work items: one table per map shape, shared by the layers
    const std::string shape_key = std::to_string(Bx) + "x" + std::to_string(H) + "x" + std::to_string(W) + "x" + std::to_string(Cout);
    const float* items = cached("winof128_items:" + shape_key, wino_fused128_items_count(Bx, H, W, Cout) * 4,
                                [&](float* dst) { KD_THROW_IF(launch_wino_fused128_items(dst, Bx, H, W, Cout, 0)); });
    const int cus = u->cus;
    emit([=](hipStream_t s) {
      return launch_wino_fused_gn128(xr.f(), ldx, abr.f(), U, bias, rr.f(), ldres, yr.f(), Bx, H, W, Cin, Cout, seg.d(),
                                     so_ ? Cout / 16 : 0, items, cus, s);
    }, "wino fused M" + std::to_string((int64_t)Bx * H * W) + " Cin" + std::to_string(Cin) + " Cout" +
           std::to_string(Cout), m);
    free(ab);
    count_macs(m, (int64_t)Bx * H * W * 4 * Cout * ((Cin / 4 + 3) / 4 * 16));
    return y;
  }

  // The `Block` `pre` (.groupnorm, .project) of a ResnetBlock on the path conv3x3_choice picks.  free_x: x dies here, released
  // once the layer has read it.  skip_c0 / skip_scale: see resnet() (Wino4 takes them; WinoFused has them in the partials).
  T gn_conv3x3(const T& x, bool free_x, const std::string& pre, int ss_col, int Cout, const T* res, int skip_c0 = -1,
               float skip_scale = 1.0f) {
    const Conv3x3Choice c = conv3x3_choice(x, Cout);
    if (skip_c0 >= 0 && c.algo != Conv3x3::Wino4 && c.algo != Conv3x3::WinoFused)
      throw std::runtime_error("plan: folded skip scale on a conv path that cannot apply it: " + pre);
    const std::string gn = pre + ".groupnorm", cv = pre + ".project";
    T y;
    switch (c.algo) {
      case Conv3x3::Wino4: y = wino4_block(x, c.images, gn, ss_col, cv, Cout, res, skip_c0, skip_scale); break;
      case Conv3x3::WinoGemm: y = wino_block(x, gn, ss_col, cv, Cout, res); break;
      case Conv3x3::WinoFused: y = fwino_gn_conv(x, gn, ss_col, cv, Cout, res); break;
      case Conv3x3::Direct: {
        T a = gn_silu(x, gn, ss_col);
        if (free_x) free(x);   // before the conv allocates its output, which may take x's place
        ConvOpt o;
        o.res = res;          // y + res folded into the conv epilogue
        o.want_seg = true;    // the next GroupNorm reads y (block1 behind a cross-attention: none does, harmless)
        y = conv(a, pack_conv(cv + ".weight", Cout, a.C, a.C, 3), P(cv + ".bias", Cout), Cout, 3, 1, 1, o);
        free(a);
        return y;
      }
    }
    if (free_x) free(x);
    return y;
  }

  // ResnetBlock.  Does NOT free x.
  // ct: the buffer of the skip concat that follows this block ([B,H,W,dim_out + skip channels]); when the
  // block ends in its 1x1 skip conv, that conv writes the block output straight into the first dim_out
  // channels of ct and ct is returned (concat_skip then only adds the skip half); otherwise ct is ignored
  // out_slot: a channel slice (of the concat buffer this block's output will later be part of as the skip half);
  // a block that ends in gate_add writes its output there and returns the slice; otherwise out_slot is ignored.
  // skip_c0 >= 0: x is a concat whose channels [skip_c0, ..) hold an UNSCALED skip tensor that the layer must see
  // scaled by skip_scale: the GroupNorm gets it through the partials' scale (SegPart), the 1x1 skip conv through
  // weights whose columns were scaled at plan build.
  // out_seg: false for the last producer in front of a final conv that reads it directly (final_resnet_block=False): no
  // GroupNorm normalises that output, so its ResnetBlock / upsample does not leave partials
  struct ResnetOpt {
    const T *ct = nullptr, *out_slot = nullptr;
    int skip_c0 = -1;
    float skip_scale = 1.0f;
    bool out_seg = true;
  };
  T resnet(const T& x, const std::string& pre, int dim_out, const T* ctx, bool use_gca, const ResnetOpt& ro) {
    bool has_cross = has(pre + ".cross_attn.to_q.weight");
    if (has_cross && !ctx) throw std::runtime_error("cross-attention block without conditioning tokens: " + pre);
    int dim_in = x.C;
    T h = gn_conv3x3(x, false, pre + ".block1", -1, dim_out, nullptr, ro.skip_c0, ro.skip_scale);
    if (has_cross) {
      T h2 = lin_cross_pre.count(pre) ? linear_cross_attn(h, pre + ".cross_attn", *ctx) : cross_attn(h, pre + ".cross_attn", *ctx);
      free(h);
      h = h2;
    }
    auto it = tmlp_off.find(pre);
    int ss_col = it != tmlp_off.end() ? it->second : -1;
    bool has_res_conv = has(pre + ".res_conv.weight");
    T h2 = gn_conv3x3(h, true, pre + ".block2", ss_col, dim_out, (!use_gca && !has_res_conv) ? &x : nullptr);
    if (!use_gca && !has_res_conv) return h2;
    if (ro.skip_c0 >= 0 && !has_res_conv) throw std::runtime_error("plan: folded skip scale without a skip conv: " + pre);
    const float* w_res = nullptr;
    if (has_res_conv) {
      w_res = P(pre + ".res_conv.weight", (int64_t)dim_out * dim_in);
      if (ro.skip_c0 >= 0) {   // columns of the skip channels times skip_scale
        const float* src = w_res;
        w_res = cached("res_conv_skipscaled:" + pre + ":" + std::to_string(ro.skip_c0), (size_t)dim_out * dim_in, [&](float* dst) {
          KD_THROW_IF(launch_copy_scale_rows(src, dim_in, dst, dim_in, dim_in, 1.0f, dim_out, 0));
          KD_THROW_IF(launch_copy_scale_rows(dst + ro.skip_c0, dim_in, dst + ro.skip_c0, dim_in, dim_in - ro.skip_c0, ro.skip_scale,
                                             dim_out, 0));
        });
      }
    }
    T out;
    if (use_gca) {
      T gate = gca(h2, pre + ".gca");
      if (has_res_conv) {
        ConvOpt o;
        o.gate_src = &h2;
        o.gate = &gate;
        o.want_seg = ro.out_seg;
        if (ro.ct) o.dst = ro.ct;
        out = conv(x, w_res, P(pre + ".res_conv.bias", dim_out), dim_out, 1, 1, 0, o);
      } else {
        out = ro.out_slot ? *ro.out_slot : alloc(x.B, x.H, x.W, dim_out);
        if (out.C != dim_out) throw std::runtime_error("plan: output slot of the wrong width: " + pre);
        const Ref ar = at(h2), gr = at(gate), rr = at(x), yr = at(out);
        int Bx = x.B, HW = x.HW(), ldr = x.LD(), ldy = out.LD();
        const bool sg = ro.out_seg && dim_out % 16 == 0;   // GroupNorm partials of `out` for the block that reads it
        const Ref seg = sg ? seg_at(add_seg(out, 0, dim_out / 16, gate_add_chunks(Bx, HW))) : Ref();
        emit([=](hipStream_t s) {
          return launch_gate_add(ar.f(), gr.f(), rr.f(), ldr, yr.f(), ldy, seg.d(), Bx, HW, dim_out, s);
        }, "gate_add HW" + std::to_string(HW) + " C" + std::to_string(dim_out));
      }
      free(gate);
    } else {  // res_conv without gca: out = conv1x1(x) + h2
      ConvOpt o;
      o.res = &h2;
      o.want_seg = ro.out_seg;
      if (ro.ct) o.dst = ro.ct;
      out = conv(x, w_res, P(pre + ".res_conv.bias", dim_out), dim_out, 1, 1, 0, o);
    }
    free(h2);
    return out;
  }

  // the Downsample (pixel-unshuffle + conv1x1 = a 2 x 2 / stride-2 conv) on the bf16x3 kernel: its fp32-A loader gathers the
  // four input pixels of an output pixel (X3Epi::a_tap_c), K = 4 C
  X3Epi downsample_x3_epi(const T& x, int ldy) const {
    X3Epi e;
    e.lda = x.LD();
    e.ldy = ldy;
    e.a_tap_c = x.C;
    e.a_wi = x.W;
    e.a_hi = x.H;
    e.hw = (x.H / 2) * (x.W / 2);
    return e;
  }
  // ldy: row stride of the output (0 = Cout; a CrossEmbedLayer's 2 x 2 half fills a channel slice of the level's map)
  bool downsample_x3_ok(const T& x, int Cout, int ldy = 0) const {
    if ((x.H & 1) || (x.W & 1) || x.C % 16) return false;
    return x3_epi_layer_ok((int64_t)x.B * (x.H / 2) * (x.W / 2), Cout, 4 * x.C, 256, downsample_x3_epi(x, ldy ? ldy : Cout));
  }
  // dst: write channels [0, Cout) of this map (of dst->C >= Cout channels, whose GroupNorm partials the launch's buffer then
  // spans: the launches filling the other channels find it under the same span) instead of a new one; seg_nchunk: as ConvOpt's
  T downsample_x3(const T& x, const std::string& pre, const float* w_taps /*[tap][O][C]*/, const float* bias, int Cout,
                  const T* dst = nullptr, int* seg_nchunk = nullptr) {
    const int C = x.C, K = 4 * C, Ho = x.H / 2, Wo = x.W / 2;
    const int64_t M = (int64_t)x.B * Ho * Wo;
    // B operand [O][K] with k = tap C + c, then its three planes
    const float* W3 = cached("x3down:" + pre, ((size_t)Cout * K * 3 + 1) / 2, [&](float* dst) {
      float* wk = nullptr;
      KD_HIP_THROW(hipMalloc((void**)&wk, (size_t)Cout * K * sizeof(float)));
      int rc = 0;
      for (int t = 0; t < 4 && !rc; ++t)
        rc = launch_copy_scale_rows(w_taps + (size_t)t * Cout * C, C, wk + (size_t)t * C, K, C, 1.0f, Cout, 0);
      if (!rc) rc = launch_split3(wk, dst, 1, Cout, K, 0);
      hipError_t er = hipDeviceSynchronize();
      (void)hipFree(wk);
      KD_THROW_IF(rc);
      KD_HIP_THROW(er);
    });
    T y = dst ? *dst : alloc(x.B, Ho, Wo, Cout);
    const X3Epi base = downsample_x3_epi(x, y.LD());
    // the output feeds the GroupNorm of the level's first ResnetBlock: partials from the epilogue
    const int span = y.C;   // channels the partial buffer covers
    const bool sg = Cout % 16 == 0 && span % 16 == 0 && (Ho * Wo) % 32 == 0;
    const int nchunk = sg ? Ho * Wo / gemm_bf16x3_shape(1, (int)M, Cout, K, u->cus).seg_rows() : 0;
    if (seg_nchunk) *seg_nchunk = nchunk;
    const Ref seg = sg ? seg_at(add_seg(y, 0, span / 16, nchunk)) : Ref();
    auto epi_of = [=]() {
      X3Epi e = base;
      e.bias = bias;
      if (seg) {
        e.seg = seg.d();
        e.seg_nseg = span / 16;
      }
      return e;
    };
    const std::string shape = " M" + std::to_string(M) + " Cin" + std::to_string(C) + " Cout" + std::to_string(Cout);
    emit_x3_gemm(at(x), W3, at(y), 1, M, Cout, K, true, epi_of, "conv k2", shape, M * Cout * K);
    return y;
  }
  T downsample(const T& x, const std::string& pre, int dim_out) {  // pixel-unshuffle + conv1x1 == 2x2/s2 conv
    if (u->cross_embed_downsample) return cross_embed_downsample(x, pre, dim_out);
    if (cfg.downsample_conv4) {   // earlier library versions: Conv2d(dim, dim_out, 4, stride 2, pad 1)
      ConvOpt o4;
      o4.want_seg = true;
      return conv(x, pack_conv(pre + ".weight", dim_out, x.C, x.C, 4), P(pre + ".bias", dim_out), dim_out, 4, 2, 1, o4);
    }
    const float* src = raw(pre + ".1.weight", (int64_t)dim_out * 4 * x.C);
    const int C = x.C;
    float* w = cached("unshuffle:" + pre, (size_t)dim_out * 4 * C,
                      [&](float* dst) { KD_THROW_IF(launch_pack_unshuffle(src, dst, dim_out, C, 0)); });
    if (downsample_x3_ok(x, dim_out)) return downsample_x3(x, pre, w, P(pre + ".1.bias", dim_out), dim_out);
    ConvOpt o;
    o.want_seg = true;   // feeds the GroupNorm of the level's first ResnetBlock
    return conv(x, w, P(pre + ".1.bias", dim_out), dim_out, 2, 2, 0, o);
  }
  // `Unet(cross_embed_downsample=True)`: CrossEmbedLayer(d, (2, 4), dim_out, stride 2) = cat(Conv2d(d, dim_out / 2, 2, stride 2),
  // Conv2d(d, dim_out - dim_out / 2, 4, stride 2, pad 1)): two launches into the channel halves of one map - the 2 x 2 half
  // on the path downsample() picks for that Cout, the 4 x 4 half on the generic conv as the downsample_conv4 fork - that
  // share one buffer of GroupNorm partials where their chunks agree (else the first ResnetBlock takes its statistics itself)
  T cross_embed_downsample(const T& x, const std::string& pre, int dim_out) {
    if (dim_out & 1) throw std::runtime_error("cross_embed_downsample: odd dim_out " + std::to_string(dim_out) + " at " + pre);
    if ((x.H & 1) || (x.W & 1)) throw std::runtime_error("cross_embed_downsample: odd map at " + pre);
    const int d2 = dim_out / 2, d4 = dim_out - d2, C = x.C;
    const float* w2 = pack_conv(pre + ".convs.0.weight", d2, C, C, 2);   // [tap = kh 2 + kw][O][C]: downsample()'s tap layout
    const float* b2 = P(pre + ".convs.0.bias", d2);
    T y = alloc(x.B, x.H / 2, x.W / 2, dim_out);
    int chunks2 = 0, chunks4 = 0;   // of the partials each half leaves
    if (downsample_x3_ok(x, d2, dim_out)) {
      downsample_x3(x, pre + ".convs.0", w2, b2, d2, &y, &chunks2);
    } else {
      ConvOpt o2;
      o2.seg_nchunk = &chunks2;
      o2.dst = &y;
      o2.want_seg = true;
      o2.seg_c0 = 0;
      o2.seg_cn = dim_out;
      conv(x, w2, b2, d2, 2, 2, 0, o2);
    }
    ConvOpt o4;
    o4.seg_nchunk = &chunks4;
    o4.dst = &y;
    o4.yoff = d2;
    o4.want_seg = true;
    o4.seg_c0 = 0;
    o4.seg_cn = dim_out;
    conv(x, pack_conv(pre + ".convs.1.weight", d4, C, C, 4), P(pre + ".convs.1.bias", d4), d4, 4, 2, 1, o4);
    // one buffer over all dim_out channels, filled by both launches - or none
    auto it = seg_of.find(y.at());
    if (it != seg_of.end() && (it->second.parts.size() != 1 || chunks2 == 0 || chunks2 != chunks4)) {
      for (auto& sp : it->second.parts)
        if (sp.owned) arena.release(sp.off);
      seg_of.erase(it);
    }
    return y;
  }
  // `Unet(pixel_shuffle_upsample=False)`: nn.Upsample(scale 2, nearest) -> Conv2d(d, dim_out, 3, padding 1), no activation, as
  // four phase GEMMs over the low-res map (kernels_resample.hip).  ct as upsample().  The kernel leaves no GroupNorm
  // partials: the next ResnetBlock takes its statistics with the launch it uses for any producer without them.  A shape
  // the kernel does not take is refused here, at build, with the condition it misses.
  T upsample_nearest(const T& x, const std::string& pre, int dim_out, const T* ct = nullptr) {
    const int C = x.C;
    const float* wsrc = raw(pre + ".1.weight", (int64_t)dim_out * C * 9);
    const float* b = P(pre + ".1.bias", dim_out);
    T y = ct ? *ct : alloc(x.B, 2 * x.H, 2 * x.W, dim_out);
    if (y.B != x.B || y.H != 2 * x.H || y.W != 2 * x.W) throw std::runtime_error("plan: upsample target of the wrong shape");
    if (const char* why = upsample_nearest_refusal(x.LD(), y.LD(), y.coff, x.B, x.H, x.W, C, dim_out))
      throw std::runtime_error(std::string(why) + " (" + pre + ": Cin " + std::to_string(C) + ", Cout " + std::to_string(dim_out) + ")");
    if ((x.coff & 3)) throw std::runtime_error("upsample_nearest_conv3x3: input channel offset must be a multiple of 4 (" + pre + ")");
    const float* wp = cached("upnearest_w:" + pre, upsample_nearest_weight_floats(C, dim_out),
                             [&](float* dst) { KD_THROW_IF(launch_upsample_nearest_pack(wsrc, dst, dim_out, C, 0)); });
    const Ref xr = at(x), yr = base(y);   // (the launch takes y's first channel as yoff)
    const int ldx = x.LD(), ldy = y.LD(), yoff = y.coff, Bx = x.B, H = x.H, W = x.W;
    const int64_t M = (int64_t)Bx * H * W;
    const int64_t m = 4 * M * dim_out * C * 9;
    emit([=](hipStream_t s) {
      return launch_upsample_nearest_conv3x3(xr.f(), ldx, wp, b, yr.f(), ldy, yoff, Bx, H, W, C, dim_out, s);
    }, "upsample nearest conv3 M" + std::to_string(M) + " Cin" + std::to_string(C) + " Cout" + std::to_string(dim_out), m);
    count_macs(m, 4 * M * dim_out * 4 * C);
    return y;
  }
  T upsample(const T& x, const std::string& pre, int dim_out, const T* ct, bool out_seg) {  // conv1x1 -> SiLU -> PixelShuffle(2)
    if (u->upsample_nearest) return upsample_nearest(x, pre, dim_out, ct);
    const float* wsrc = raw(pre + ".net.0.weight", (int64_t)4 * dim_out * x.C);
    const float* bsrc = raw(pre + ".net.0.bias", 4 * dim_out);
    const int C = x.C;
    float* b = nullptr;  // weight and bias are permuted together: the bias buffer is cached under its own key
    float* w = cached("shuffle_w:" + pre, (size_t)4 * dim_out * C, [&](float* dst) {
      b = cached("shuffle_b:" + pre, (size_t)4 * dim_out, [](float*) {});
      KD_THROW_IF(launch_pack_shuffle(wsrc, bsrc, dst, b, dim_out, C, 0));
    });
    if (!b) b = cached("shuffle_b:" + pre, (size_t)4 * dim_out, [](float*) {});
    ConvOpt o;
    o.act = ACT_SILU;
    o.out_mode = OUT_PIXSHUF;
    o.want_seg = out_seg;
    if (ct) o.dst = ct;   // straight into the first dim_out channels of the following skip concat
    return conv(x, w, b, 4 * dim_out, 1, 1, 0, o);
  }
  // ---- `Unet(combine_upsample_fmaps=True)`: `upsample_combiner.fmap_convs.i`, the library's Block with its own default of
  // 8 groups and no FiLM, over up level i's map f brought to the full resolution by nearest upsampling with the integer
  // factor s, into channels [yoff, yoff + dim) of the concat `cat` in front of final_res_block.  s >= 2: one launch of the
  // class kernel over the LOW-RES map (kernels_upcombine.hip) - the statistics of the upsampled map are those of f, every
  // pixel being replicated s^2 times; where f's producer left partials that tile 16-channel groups they are folded to the
  // per-(image, channel) affine the kernel applies on load, else GroupNorm + SiLU run over f into a low-res temporary.
  // s = 1 (the last level of a UNet that is not memory_efficient): GroupNorm + SiLU, then the conv on the generic path.
  // A shape the kernel does not take is refused here, at build.
  static constexpr int COMBINE_GROUPS = 8;
  T gn_silu_plain(const T& x, const float* gamma, const float* beta, int G) {
    const int Bx = x.B, HW = x.HW(), C = x.C, ldx = x.LD();
    if (C % G || (C / G) % 4) throw std::runtime_error("upsample_combiner: GroupNorm(" + std::to_string(G) + ") needs groups of 4 n channels, C = " + std::to_string(C));
    T st = alloc_bytes((size_t)Bx * G * 2 * sizeof(float)), part = alloc_bytes(gn_partial_bytes(Bx, HW, C, G));
    T y = alloc(x.B, x.H, x.W, C);
    const Ref xr = at(x), yr = at(y), sr = at(st), pr = at(part);
    emit([=](hipStream_t s) { return launch_gn_stats(xr.f(), ldx, sr.f(), pr.d(), Bx, HW, C, G, 1e-5f, s); },
         "gn stats HW" + std::to_string(HW) + " C" + std::to_string(C));
    emit([=](hipStream_t s) { return launch_gn_apply_silu(xr.f(), ldx, sr.f(), gamma, beta, nullptr, 0, yr.f(), Bx, HW, C, G, s); },
         "gn apply HW" + std::to_string(HW) + " C" + std::to_string(C));
    free(st);
    free(part);
    return y;
  }
  void combine_fmap(const T& f, int i, int scale, const T& cat, int yoff) {
    const int G = COMBINE_GROUPS, dim = cfg.dim, Cin = f.C, Bx = f.B, H = f.H, W = f.W;
    const std::string pre = "upsample_combiner.fmap_convs." + std::to_string(i);
    const float* gamma = P(pre + ".groupnorm.weight", Cin);
    const float* beta = P(pre + ".groupnorm.bias", Cin);
    const float* bias = P(pre + ".project.bias", dim);
    if (cat.B != Bx || cat.H != scale * H || cat.W != scale * W || scale < 1)
      throw std::runtime_error("plan: " + pre + ": the map is no integer fraction of the full resolution");
    if (scale == 1) {
      T a = gn_silu_plain(f, gamma, beta, G);
      ConvOpt o;
      o.dst = &cat;
      o.yoff = yoff;
      conv(a, pack_conv(pre + ".project.weight", dim, Cin, Cin, 3), bias, dim, 3, 1, 1, o);
      free(a);
      return;
    }
    if (const char* why = upsample_scale_refusal(f.LD(), cat.LD(), cat.coff + yoff, Bx, H, W, Cin, dim, scale))
      throw std::runtime_error(std::string(why) + " (" + pre + ": Cin " + std::to_string(Cin) + ", Cout " + std::to_string(dim) + ")");
    if ((f.coff & 3)) throw std::runtime_error("upsample_nearest_gn_conv3x3: input channel offset must be a multiple of 4 (" + pre + ")");
    const float* wsrc = raw(pre + ".project.weight", (int64_t)dim * Cin * 9);
    const float* wp = cached("upcombine_w:" + pre, upsample_scale_weight_floats(Cin, dim),
                             [&](float* dst) { KD_THROW_IF(launch_upsample_scale_pack(wsrc, dst, dim, Cin, 0)); });
    SegPart sp[2];
    int nsp = 0;
    bool fold = Cin % G == 0 && (Cin / G) % 16 == 0 && seg_sources(f, sp, nsp, G);
    for (int k = 0; k < nsp; ++k) fold = fold && sp[k].scale == 1.0f && sp[k].ab_mul == 1.0f;   // (the map as it is in memory)
    T src = f, ab;
    if (fold) {
      ab = alloc_bytes((size_t)Bx * Cin * 2 * sizeof(float));
      const SegPart a = sp[0], b2 = nsp > 1 ? sp[1] : SegPart();
      const Ref pa = seg_at(a.off), pb = nsp > 1 ? seg_at(b2.off) : Ref(), abr = at(ab);
      const int HW = f.HW();
      emit([=](hipStream_t s) {
        SegSrc s0{pa.d(), a.nseg, a.nchunk, a.c0, a.scale, a.ab_mul};
        SegSrc s1{pb.d(), b2.nseg, b2.nchunk, b2.c0, b2.scale, b2.ab_mul};
        return launch_gn_fold_seg(s0, s1, gamma, beta, nullptr, 0, abr.f(), nullptr, Bx, Cin, G, (double)HW * (Cin / G), 1e-5f, s);
      }, "gn fold seg HW" + std::to_string(HW) + " C" + std::to_string(Cin));
    } else {
      src = gn_silu_plain(f, gamma, beta, G);
    }
    const Ref xr = at(src), abr = fold ? at(ab) : Ref(), yr = base(cat);
    const int ldx = src.LD(), ldy = cat.LD(), yo = cat.coff + yoff;
    const int64_t M = (int64_t)Bx * H * W;
    const int64_t m = M * scale * scale * dim * Cin * 9;
    emit([=](hipStream_t s) {
      return launch_upsample_scale_conv3x3(xr.f(), ldx, abr.f(), wp, bias, yr.f(), ldy, yo, Bx, H, W, Cin, dim, scale, s);
    }, "upsample combine s=" + std::to_string(scale) + " M" + std::to_string(M) + " Cin" + std::to_string(Cin) + " Cout" +
           std::to_string(dim) + (fold ? " affine" : ""), m);
    count_macs(m, M * dim * Cin * (scale == 2 ? 16 : 25));
    free(fold ? ab : src);
  }
  T concat_skip(const T& x, const T& skip, float scale) {
    T y = alloc(x.B, x.H, x.W, x.C + skip.C);
    int Ca = x.C, Cb = skip.C, lda = x.LD(), ldb = skip.LD();
    int64_t rows = x.rows();
    const Ref ar = at(x), br = at(skip), ya = at(y), yb = ya.floats(Ca);
    emit([=](hipStream_t s) {
      if (launch_copy_scale_rows(ar.f(), lda, ya.f(), Ca + Cb, Ca, 1.0f, rows, s)) return 1;
      return launch_copy_scale_rows(br.f(), ldb, yb.f(), Ca + Cb, Cb, scale, rows, s);
    }, "concat rows" + std::to_string(rows) + " C" + std::to_string(Ca + Cb));
    return y;
  }
  // the same when x's producer already wrote its Ca channels into y (resnet / upsample with ct = &y)
  void concat_skip_tail(const T& y, int Ca, const T& skip, float scale) {
    const Ref br = at(skip), yb = at(y).floats(Ca);
    int Cb = skip.C, ldb = skip.LD(), ldy = y.LD();
    int64_t rows = y.rows();
    emit([=](hipStream_t s) {
      return launch_copy_scale_rows(br.f(), ldb, yb.f(), ldy, Cb, scale, rows, s);
    }, "concat tail rows" + std::to_string(rows) + " C" + std::to_string(Ca + Cb));
  }
  // x into the first x.C channels of the concat buffer ct (whose skip half is already there)
  void concat_head(const T& ct, const T& x, const char* what = "concat head") {
    const Ref ar = at(x), yr = at(ct);
    int Ca = x.C, lda = x.LD(), ldy = ct.LD();
    int64_t rows = x.rows();
    emit([=](hipStream_t s) { return launch_copy_scale_rows(ar.f(), lda, yr.f(), ldy, Ca, 1.0f, rows, s); },
         std::string(what) + " rows" + std::to_string(rows) + " C" + std::to_string(Ca));
  }
  // in place: channels [c0, c0 + n) of t times scale (a skip half whose consumer cannot fold the scale)
  void scale_slice(const T& t, int c0, int n, float scale) {
    const Ref tr = at(t).floats(c0);
    int ld = t.LD();
    int64_t rows = t.rows();
    emit([=](hipStream_t s) {
      return launch_copy_scale_rows(tr.f(), ld, tr.f(), ld, n, scale, rows, s);
    }, "scale slice rows" + std::to_string(rows) + " C" + std::to_string(n));
  }

  void collect_time_mlps() {
    std::vector<std::string> names;
    const std::string suffix = ".time_mlp.1.weight";
    for (auto& kv : params) {
      const std::string& n = kv.first;
      if (n.size() > suffix.size() && n.compare(n.size() - suffix.size(), suffix.size(), suffix) == 0)
        names.push_back(n.substr(0, n.size() - suffix.size()));
    }
    std::sort(names.begin(), names.end());
    int tcd = u->time_cond_dim;
    int total = 0;
    for (auto& pre : names) {
      int64_t ne = numel(pre + suffix);
      if (ne % tcd) throw std::runtime_error("time_mlp weight of unexpected shape: " + pre);
      tmlp_off[pre] = total;
      total += (int)(ne / tcd);
    }
    tmlp_total = total;
    tmlp_prefixes = names;
    if (total == 0) return;
    tmlp_w = cached("time_mlps_w", (size_t)total * tcd, [&](float* dst) {
      for (auto& pre : names) {
        int64_t ne = numel(pre + suffix);
        KD_HIP_THROW(hipMemcpyAsync(dst + (size_t)tmlp_off[pre] * tcd, raw(pre + suffix), (size_t)ne * 4,
                                    hipMemcpyDeviceToDevice, 0));
      }
    });
    tmlp_b = cached("time_mlps_b", (size_t)total, [&](float* dst) {
      for (auto& pre : names) {
        int64_t ne = numel(pre + suffix);
        KD_HIP_THROW(hipMemcpyAsync(dst + tmlp_off[pre], raw(pre + ".time_mlp.1.bias", ne / tcd),
                                    (size_t)(ne / tcd) * 4, hipMemcpyDeviceToDevice, 0));
      }
    });
  }

  // one time-conditioning trio: log_snr[B] -> (t [B,tcd] written/accumulated, tokens into c rows)
  void time_trio(const std::string& hid, const std::string& cond, const std::string& tok, bool lowres,
                 const T& t_out, const T& c_tok, int tok_row, const T& emb, const T& hidden) {
    int tcd = u->time_cond_dim, half = cfg.sinu_dim / 2, sw = cfg.sinu_dim + 1;
    int cd = cfg.cond_dim, ntt = cfg.num_time_tokens, ntok = c_tok.H * c_tok.W;
    const float* sw_w = P(hid + ".0.weights", half);
    const kd_unet* io = u;   // the per-call inputs are read when the op runs
    const Ref er = at(emb);
    int Bx = B;
    emit([=](hipStream_t s) {
      const float* t = lowres ? io->in_lowres_log_snr : io->in_log_snr;
      if (!t) {
        set_error(lowres ? "lowres_log_snr is required by this UNet" : "log_snr is required");
        return 1;
      }
      return launch_sinu_emb(t, sw_w, er.f(), Bx, half, s);
    });
    skinny(er, sw, P(hid + ".1.weight", (int64_t)tcd * sw), P(hid + ".1.bias", tcd), at(hidden), tcd, B, sw,
           tcd, ACT_NONE, ACT_SILU);
    // tokens: [B, ntt*cd] written at row tok_row of c (row stride ntok*cd per batch)
    skinny(at(hidden), tcd, P(tok + ".0.weight", (int64_t)cd * ntt * tcd), P(tok + ".0.bias", cd * ntt),
           at(c_tok).floats((int64_t)tok_row * cd), ntok * cd, B, tcd, cd * ntt, ACT_NONE, ACT_NONE);
    skinny(at(hidden), tcd, P(cond + ".0.weight", (int64_t)tcd * tcd), P(cond + ".0.bias", tcd), at(t_out), tcd, B,
           tcd, tcd, ACT_NONE, ACT_NONE);
  }

  // linear attention (linattn_build.inc): the ResnetBlocks whose cross-attention is LinearCrossAttention, by prefix
  std::unordered_set<std::string> lin_cross_pre;
  T linear_attn_block(const T& x, const std::string& pre, const T* ctx, const T* dst = nullptr);
  T linear_cross_attn(const T& x, const std::string& pre, const T& c);
  T feed_forward_tail(const T& x, const T& proj, const std::string& g_out, const std::string& f, const T* dst);
  // ---- the UNet walk (unet_build.inc): build() is the list of these stages
  void step(T& x, const T& y) { free(x); x = y; }  // x <- y
  struct Model {   // the per-model constants, computed once by model()
    int dim = 0, L = 0, S = 0, tcd = 0, Ci = 0;   // Ci: image channels (x, the self-conditioning and low-res images, the output)
    std::vector<int> dims;                        // dim, then every level's width
    bool combine = false, keep_init = false, final_res = true;
    // cat_w: combine_upsample_fmaps: width of the concat in front of final_res_block, [x: dim | up level 0 (deepest) .. L - 1:
    // dim each | init conv residual: dim]; fin_w: channels of the map the final conv reads
    int cat_w = 0, fin_w = 0;
    float skip_scale = 1.0f;
  };
  struct FinalConv {   // prepared by final_conv_setup() at the top, emitted by final_conv() at the bottom
    int ks = 3, cin = 0, w = 0, n = 0;   // kernel size, weight input channels, channels read from x, GEMM columns
    const float* bias = nullptr;
    float* w_packed = nullptr;
    T stat;   // has_static: the low-res planes' share [B, Ci, S, S], written once per sampling call
    bool has_static = false;
  };
  struct InitConv {
    T x;      // the init conv's output map
    T stat;   // hoist: the cond / low-res planes' share, written once per sampling call and released at the end
    bool hoist = false;
  };
  // The skip tensors of the down path and the protocol "a producer may write straight into the concat that follows it"
  struct SkipStack {
    Builder& b;
    std::vector<T> hiddens;
    T ct;                  // the offer: concat buffer handed to the next producer
    bool have_ct = false, ct_owned = false;   // ct_owned: allocated by the offer (else it is the skip's own buffer)
    int ct_ca = 0;         // channels the producer contributes
    explicit SkipStack(Builder& b_) : b(b_) {}
    // every hidden of a level is later concatenated behind dim_out channels of the up path: its producer writes it into
    // channels [dim_out, dim_out + x.C) of that buffer
    T make_slot(const T& x, int dim_out) { return b.alloc(x.B, x.H, x.W, dim_out + x.C).slice(dim_out, x.C); }
    void push(const T& x) { b.retain(x); hiddens.push_back(x); }
    void push(T& x, const T& y, const T* slot);      // x <- y, produced into `slot` or not; then retained
    void push_copy(const T& x, int dim_out);
    const T* offer(int Bc, int Hc, int Wc, int Ca);
    void drop_offer() { if (have_ct && ct_owned) b.free(ct); have_ct = false; }
    int pop(T& x, int dim_out, float skip_scale);
    static T whole(T s) { s.C = s.ld; s.ld = 0; s.coff = 0; return s; }   // the buffer a skip slice lives in
    void finish() const;              // the end-of-walk checks
  };
  struct Combiner {
    Builder& b;
    const Model& m;
    T cat, head;           // the concat in front of final_res_block at full width (from the last level on); its channels [0, dim)
    std::vector<T> maps;   // each level's map after its attention slot
    bool head_here = false, head_resnet = false;   // the last level's attention block / last ResnetBlock writes the head in place
    Combiner(Builder& b_, const Model& m_) : b(b_), m(m_) {}
    void open(const T& x, const T& init_residual, int dim_out, bool ups, bool attn);
    const T* resnet_target() const { return head_resnet ? &cat : nullptr; }
    const T* attn_target() const { return head_here ? &head : nullptr; }
    void took_head(T& x) const { if (head_resnet && x.off == cat.off) x = head; }   // the ResnetBlock wrote into the concat
    void keep(const T& x) { if (m.combine) { b.retain(x); maps.push_back(x); } }   // the map lives on to the tail, as a skip does
    void close(T& x);
  };
  Model model();
  void gn_scratch(const Model& m);
  FinalConv final_conv_setup(const Model& m);
  T conditioning(const Model& m);
  InitConv init_conv(const Model& m);
  void down_path(const Model& m, T& x, const T& c, SkipStack& skips);
  void middle(const Model& m, T& x, const T& c);
  void up_path(const Model& m, T& x, const T& c, SkipStack& skips, Combiner& comb, const T& init_residual);
  void tail(const Model& m, T& x, const T& c, Combiner& comb, const T& init_residual);
  void final_conv(const Model& m, const FinalConv& f, const T& x);
  void release(const T& x, const FinalConv& fin, const InitConv& init);
  void build();
  void build_text();
};

}  // namespace kd

#include "unet_build.inc"  // Builder::build(): the walk over the module tree
#include "linattn_build.inc"  // Builder: LinearAttentionTransformerBlock and LinearCrossAttention
#include "text_build.inc"  // Builder::build_text(): step-invariant text conditioning
#include "sampler.inc"     // DDPM and EDM sampler loops
#include "api.inc"         // extern "C" entry points

