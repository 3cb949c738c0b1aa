// Sampler-side kernels: x0 prediction, per-sample 0.95-quantile (radix select), the fused DDPM
// reverse step (threshold clamp + posterior mean + noise add, noise either from a tensor or
// from in-kernel Philox4x32-10), the update of the few-step solvers (DDIM, DPM-Solver++(2M / 3M) and their SDE forms), the RePaint inpaint mix /
// re-noise and the final clamp.
//
// Every kernel reads the current iteration index from device memory (d_iter) and looks its
// per-step scalars up in device tables, so that one captured hipGraph serves all T*R
// iterations.  iteration it -> timestep k = it / R, resample slot ri = it % R (r = R-1-ri).
//
// The kernels that draw noise walk the batch with blockIdx.y = image and read their Philox key through noise_key():
// one key and one counter over the whole batch tensor, or a key per image with the counter inside the image.
#include "common.h"

#pragma clang fp contract(off)  // keep mul/add separate so that the arithmetic follows torch's op order
#include "philox.h"

namespace kd {

static inline int grid_for(int64_t n_items) {
  int64_t b = (n_items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ------------------------------------------------------------------------- Philox4x32-10 normals (philox.h)
// stream ids: purpose in the top 32 bits, iteration in the low 32
__device__ __forceinline__ uint64_t stream_id(uint32_t purpose, uint32_t it) { return ((uint64_t)purpose << 32) | it; }
enum { PURPOSE_STEP = 1, PURPOSE_INPAINT = 2, PURPOSE_RENOISE = 3, PURPOSE_EDM_CHURN = 4, PURPOSE_EDM_RENOISE = 5,
       PURPOSE_USER = 16 };

__global__ void philox_normal_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t sid) {
  int64_t n4 = (n + 3) / 4;
  for (int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += (int64_t)gridDim.x * blockDim.x) {
    f32x4 z = philox_normal4(seed, sid, (uint64_t)i4);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i4 * 4 + e < n) out[i4 * 4 + e] = z[e];
  }
}
int launch_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t sid, hipStream_t s) {
  hipLaunchKernelGGL(philox_normal_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, s, out, n, seed, sid);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// Row b of out[B][n] from (seeds[b], sid) with the counter running inside the row: what philox_normal_kernel writes for
// (n, seeds[b], sid).  The keys travel as a kernel argument, SEED_CHUNK rows per launch.
struct SeedChunk {
  uint64_t v[SEED_CHUNK];
};
__global__ __launch_bounds__(256) void philox_normal_rows_kernel(float* __restrict__ out, int64_t n4, SeedChunk seeds,
                                                                 uint64_t sid) {
  const uint64_t seed = seeds.v[blockIdx.y];
  float* row = out + (int64_t)blockIdx.y * n4 * 4;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n4; j += (int64_t)gridDim.x * blockDim.x)
    *(f32x4*)(row + j * 4) = philox_normal4(seed, sid, (uint64_t)j);
}
// grid of the kernels that walk [B][per4] with blockIdx.y = image: as many blocks as grid_for gives the flat walk
static inline dim3 grid_rows(int64_t per4, int B) {
  const int cap = 4096 / B < 1 ? 1 : 4096 / B;
  const int gx = grid_for(per4);
  return dim3((unsigned)(gx > cap ? cap : gx), (unsigned)B);
}
int launch_philox_normal_rows(float* out, int B, int64_t n, const uint64_t* seeds, uint64_t sid, hipStream_t s) {
  KD_REQUIRE(out != nullptr && seeds != nullptr, "philox rows: null argument");
  KD_REQUIRE(B >= 1 && n >= 4 && n % 4 == 0, "philox rows: the row length must be a positive multiple of 4");
  KD_REQUIRE(((uintptr_t)out & 15) == 0, "philox rows: out must be 16-byte aligned");
  for (int b0 = 0; b0 < B; b0 += SEED_CHUNK) {
    const int nb = std::min(B - b0, (int)SEED_CHUNK);
    SeedChunk c{};
    for (int b = 0; b < nb; ++b) c.v[b] = seeds[b0 + b];
    hipLaunchKernelGGL(philox_normal_rows_kernel, grid_rows(n / 4, nb), dim3(256), 0, s, out + (int64_t)b0 * n, n / 4, c, sid);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// The start of a stage: x[b,c,y,x] = scale * z + (2 * init[b,c,sy,sx] - 1), one float4 of x per thread and Philox call.
// z is the draw of kd_philox_normal (per_image == 0: key keys.v[0], counter over the whole batch tensor) or of
// kd_philox_normal_rows (per_image != 0: key keys.v[image of the launch], counter inside the image), or it is read from
// `noise`.  The source pixel follows torch's nearest rule, min((int)floorf(dst * ((float)in / (float)out)), in - 1), the
// ratios ry / rx divided in fp32 by the host; the gather is scalar, so the source rows need no alignment.  The pointers
// are those of the launch's first image; b0 is that image's index in the batch (the counter of the whole-batch stream).
__global__ __launch_bounds__(256) void sample_start_kernel(float* __restrict__ out, const float* __restrict__ noise,
                                                           const float* __restrict__ init, int C, int S, int Hs, int Ws,
                                                           float ry, float rx, float scale, SeedChunk keys, int per_image,
                                                           int64_t b0, uint64_t sid) {
  const int b = blockIdx.y;
  const int64_t plane = (int64_t)S * S, per4 = C * plane / 4;
  const uint64_t seed = keys.v[per_image ? b : 0];
  const uint64_t ctr0 = per_image ? 0 : (uint64_t)((b0 + b) * per4);
  float* row = out + (int64_t)b * per4 * 4;
  const float* zrow = noise ? noise + (int64_t)b * per4 * 4 : nullptr;
  const float* src = init ? init + (int64_t)b * C * Hs * Ws : nullptr;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < per4; j += (int64_t)gridDim.x * blockDim.x) {
    f32x4 z = zrow ? *(const f32x4*)(zrow + j * 4) : philox_normal4(seed, sid, ctr0 + (uint64_t)j);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = z[e] * scale;
    if (src) {
      int c = (int)(j * 4 / plane);   // (c, y, x) of the float4's first element; a float4 may cross a row or a plane
      const int rem = (int)(j * 4 - c * plane);
      int y = rem / S, x = rem - y * S;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int sy = min((int)floorf((float)y * ry), Hs - 1);
        const int sx = min((int)floorf((float)x * rx), Ws - 1);
        float t = 2.0f * src[((int64_t)c * Hs + sy) * Ws + sx];
        t = t - 1.0f;
        o[e] = o[e] + t;
        if (++x == S) {
          x = 0;
          if (++y == S) {
            y = 0;
            ++c;   // (c == C only behind the image's last element: not read)
          }
        }
      }
    }
    *(f32x4*)(row + j * 4) = o;
  }
}
int launch_sample_start(float* out, int B, int C, int S, float scale, uint64_t seed, const uint64_t* seeds, const float* noise,
                        const float* init, int Hs, int Ws, hipStream_t s) {
  KD_REQUIRE(out != nullptr, "sample start: null output");
  KD_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && C <= 1024 && S >= 1 && S <= 16384,
             "sample start: batch, channels or image size out of range");
  const int64_t n = (int64_t)C * S * S;
  KD_REQUIRE(n % 4 == 0, "sample start: the row length C * S * S must be a multiple of 4");
  KD_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)noise & 15) == 0, "sample start: out and noise must be 16-byte aligned");
  KD_REQUIRE(init == nullptr || (Hs >= 1 && Ws >= 1 && Hs <= 16384 && Ws <= 16384), "sample start: source size out of range");
  const float ry = init ? (float)Hs / (float)S : 1.0f, rx = init ? (float)Ws / (float)S : 1.0f;
  const bool per_image = seeds != nullptr && noise == nullptr;
  const uint64_t sid = ((uint64_t)PURPOSE_USER << 32) | 2;   // the caller's x_T stream (include/kd_engine.h)
  const int step = per_image ? (int)SEED_CHUNK : B;   // per-image keys travel as a kernel argument, SEED_CHUNK per launch
  for (int b0 = 0; b0 < B; b0 += step) {
    const int nb = std::min(B - b0, step);
    SeedChunk keys{};
    keys.v[0] = seed;
    for (int b = 0; per_image && b < nb; ++b) keys.v[b] = seeds[b0 + b];
    hipLaunchKernelGGL(sample_start_kernel, grid_rows(n / 4, nb), dim3(256), 0, s, out + (int64_t)b0 * n,
                       noise ? noise + (int64_t)b0 * n : nullptr, init ? init + (int64_t)b0 * C * Hs * Ws : nullptr, C, S, Hs,
                       Ws, ry, rx, scale, keys, per_image ? 1 : 0, (int64_t)b0, sid);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// The key block in device memory (Sampler::seed): [SEED_BATCH] keys the whole batch tensor, the counter being the float4
// index over all B images; [SEED_MODE] != 0 switches to one key per image, [SEED_ROWS + b], with the counter running
// inside the image - image b then draws what a batch-1 call keyed seeds[b] draws.  Both words are read by the kernels,
// so one captured step serves either mode and any keys.
struct NoiseKey {
  uint64_t seed;
  uint64_t ctr0;   // counter of the image's first float4
};
__device__ __forceinline__ NoiseKey noise_key(const uint64_t* __restrict__ d_seed, int b, int64_t per4) {
  NoiseKey k;
  if (d_seed[SEED_MODE] != 0) {
    k.seed = d_seed[SEED_ROWS + b];
    k.ctr0 = 0;
  } else {
    k.seed = d_seed[SEED_BATCH];
    k.ctr0 = (uint64_t)((int64_t)b * per4);
  }
  return k;
}
// four draws for float4 j of image b (flat float4 index i4 = b * per4 + j)
__device__ __forceinline__ f32x4 noise4(const float* noise, int64_t noise_stride, NoiseKey key, uint32_t purpose, int it,
                                        int64_t i4, int64_t j) {
  if (noise) return *(const f32x4*)(noise + (int64_t)it * noise_stride + i4 * 4);
  return philox_normal4(key.seed, stream_id(purpose, (uint32_t)it), key.ctr0 + (uint64_t)j);
}

// ------------------------------------------------------------------------- per-step helpers
__global__ void fill_time_kernel(const float* __restrict__ table, const int* __restrict__ d_iter, int R,
                                 float* __restrict__ out, int B) {
  int i = threadIdx.x;
  if (i < B) out[i] = table[*d_iter / R];
}
int launch_fill_time(const float* table, const int* d_iter, int R, float* out, int B, hipStream_t s) {
  KD_REQUIRE(B <= 1024, "batch too large for fill_time");
  hipLaunchKernelGGL(fill_time_kernel, dim3(1), dim3(((B + 63) / 64) * 64), 0, s, table, d_iter, R, out, B);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// cond region of schedule step (*d_iter / R) out of the per-schedule table -> the live cond region (16 bytes per thread)
__global__ __launch_bounds__(256) void cond_gather_kernel(const float4* __restrict__ tab, float4* __restrict__ dst, int64_t n16,
                                                          const int* __restrict__ d_iter, int R) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) dst[i] = tab[(int64_t)(*d_iter / R) * n16 + i];
}
int launch_cond_gather(const void* tab, void* dst, size_t bytes, const int* d_iter, int R, hipStream_t s) {
  KD_REQUIRE(tab != nullptr && dst != nullptr, "cond gather: no table");
  KD_REQUIRE(bytes % 16 == 0 && (((uintptr_t)tab | (uintptr_t)dst) & 15) == 0, "cond gather: 16-byte granules");
  const int64_t n16 = (int64_t)(bytes / 16);
  hipLaunchKernelGGL(cond_gather_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, (const float4*)tab, (float4*)dst, n16,
                     d_iter, R);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- building the per-schedule conditioning table B schedule steps at a time.  The conditioning ops are row-wise
// over the batch (time MLPs, token LayerNorm, K / V projections: sample b's rows depend on sample b's log-SNR alone), so a
// run whose B samples carry B DIFFERENT schedule steps yields in row b what a run at step k0 + b yields in every row;
// the scatter writes row b of every tensor into all B rows of table entry k0 + b.  Same kernels, same tile shapes, same
// per-row arithmetic as the in-step path: the table is bit-identical to one built step by step.
__global__ void fill_time_rows_kernel(const float* __restrict__ table, int k0, int T, float* __restrict__ out, int B) {
  const int i = threadIdx.x;
  if (i < B) out[i] = table[min(k0 + i, T - 1)];
}
int launch_fill_time_rows(const float* table, int k0, int T, float* out, int B, hipStream_t s) {
  KD_REQUIRE(B <= 1024 && T > 0, "batch too large for fill_time_rows");
  hipLaunchKernelGGL(fill_time_rows_kernel, dim3(1), dim3(((B + 63) / 64) * 64), 0, s, table, k0, T, out, B);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void cond_scatter_kernel(const float* __restrict__ ws, float* __restrict__ tab,
                                                           const CondSeg* __restrict__ segs, int nseg, uint32_t row_total, int B,
                                                           int k0, int T, int64_t cond_floats) {
  const int b = blockIdx.y, k = k0 + b;
  if (k >= T) return;
  float* row = tab + (int64_t)k * cond_floats;
  for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < row_total; e += gridDim.x * 256) {
    int lo = 0, hi = nseg - 1;   // last segment whose start <= e
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].start <= e) lo = mid; else hi = mid - 1;
    }
    const CondSeg sg = segs[lo];
    const uint32_t j = e - sg.start;
    const float v = ws[(size_t)sg.off4 + (size_t)b * sg.row4 + j];
    float* dst = row + sg.off4 + j;
    for (int b2 = 0; b2 < B; ++b2) dst[(size_t)b2 * sg.row4] = v;
  }
}
int launch_cond_scatter(const float* ws, float* tab, const CondSeg* d_segs, int nseg, uint32_t row_total, int B, int k0, int T,
                        int64_t cond_floats, hipStream_t s) {
  KD_REQUIRE(ws && tab && d_segs && nseg > 0 && row_total > 0, "cond scatter: empty conditioning region");
  const unsigned gx = (unsigned)std::min<uint32_t>((row_total + 255) / 256, 1024);
  hipLaunchKernelGGL(cond_scatter_kernel, dim3(gx, (unsigned)B), dim3(256), 0, s, ws, tab, d_segs, nseg, row_total, B, k0, T,
                     cond_floats);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

__global__ void iter_inc_kernel(int* d_iter) { *d_iter += 1; }
__global__ void iter_set_kernel(int* d_iter, int v) { *d_iter = v; }
__global__ void seed_set_kernel(uint64_t* d_seed, uint64_t v, uint64_t per_image) {
  d_seed[SEED_BATCH] = v;
  d_seed[SEED_MODE] = per_image;
}
__global__ void seed_rows_kernel(uint64_t* d_rows, SeedChunk c, int n) {
  if ((int)threadIdx.x < n) d_rows[threadIdx.x] = c.v[threadIdx.x];
}
// seeds: host pointer to B keys or nullptr; they travel as kernel arguments, so the caller's array is free on return
int launch_seed_set(uint64_t* d_seed, uint64_t value, const uint64_t* seeds, int B, hipStream_t s) {
  hipLaunchKernelGGL(seed_set_kernel, dim3(1), dim3(1), 0, s, d_seed, value, (uint64_t)(seeds != nullptr));
  for (int b0 = 0; seeds && b0 < B; b0 += SEED_CHUNK) {
    const int nb = std::min(B - b0, (int)SEED_CHUNK);
    SeedChunk c{};
    for (int b = 0; b < nb; ++b) c.v[b] = seeds[b0 + b];
    hipLaunchKernelGGL(seed_rows_kernel, dim3(1), dim3(64), 0, s, d_seed + SEED_ROWS + b0, c, nb);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_iter_set(int* d_iter, int value, hipStream_t s) {
  hipLaunchKernelGGL(iter_set_kernel, dim3(1), dim3(1), 0, s, d_iter, value);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_iter_inc(int* d_iter, hipStream_t s) {
  hipLaunchKernelGGL(iter_inc_kernel, dim3(1), dim3(1), 0, s, d_iter);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// x0 from the model output: noise: (x - sigma*eps)/max(alpha,1e-8) ; v: alpha*x - sigma*v
__global__ void x0_kernel(const float* __restrict__ x, const float* __restrict__ pred, float* __restrict__ x0,
                          StepTables tb, const int* __restrict__ d_iter, int R, int objective, int64_t n4) {
  const int k = *d_iter / R;
  const float alpha = tb.alpha[k], sigma = tb.sigma[k];
  const float alpha_c = fmaxf(alpha, 1e-8f);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 xv = *(const f32x4*)(x + i * 4), pv = *(const f32x4*)(pred + i * 4), o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (objective == 0) o[e] = (xv[e] - sigma * pv[e]) / alpha_c;
      else if (objective == 1) o[e] = alpha * xv[e] - sigma * pv[e];
      else o[e] = pv[e];
    }
    *(f32x4*)(x0 + i * 4) = o;
  }
}
int launch_x0(const float* x, const float* pred, float* x0, const StepTables& tb, const int* d_iter, int R,
              int objective, int64_t n, hipStream_t s) {
  KD_REQUIRE(n % 4 == 0, "image element count must be a multiple of 4");
  hipLaunchKernelGGL(x0_kernel, dim3(grid_for(n / 4)), dim3(256), 0, s, x, pred, x0, tb, d_iter, R, objective,
                     n / 4);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- quantile of |x| (radix select)
// torch.quantile semantics: rank = q*(n-1) in fp32, lo = floor(rank), result = lerp(v[lo], v[lo+1], rank-lo)
// on the ascending order statistics.  |x| >= 0, so the fp32 bit pattern orders like the value:
// four 8-bit MSB-first histogram passes pin v[lo] exactly; v[lo+1] is v[lo] if the last bin holds
// more than k_rem+1 elements, else the smallest value above v[lo] (one min pass).
struct QState {
  uint32_t prefix;   // bits fixed so far (high bits)
  uint32_t k_rem;    // rank still to resolve inside the prefix bucket
  uint32_t eq_count; // after the last pass: elements equal to v[lo]
  uint32_t next_bits;// min bits strictly above v[lo]
};
// workspace layout per call: QState[B] | hist[4][B][256] (uint32)
size_t quantile_ws_bytes(int B) { return (size_t)B * sizeof(QState) + (size_t)4 * B * 256 * sizeof(uint32_t); }

__global__ void q_init_kernel(QState* st, uint32_t* hist, int B, uint32_t k) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * B * 256) hist[i] = 0;
  if (i < B) {
    st[i].prefix = 0;
    st[i].k_rem = k;
    st[i].eq_count = 0;
    st[i].next_bits = 0xFFFFFFFFu;
  }
}

__global__ __launch_bounds__(256) void q_hist_kernel(const float* __restrict__ x, const QState* __restrict__ st,
                                                     uint32_t* __restrict__ hist, int64_t n, int pass) {
  __shared__ uint32_t h[256];
  const int b = blockIdx.y;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t prefix = st[b].prefix;
  const int shift = 24 - 8 * pass;
  const uint32_t himask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
  const uint32_t* xb = (const uint32_t*)(x + (int64_t)b * n);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint32_t bits = xb[i] & 0x7FFFFFFFu;
    if ((bits & himask) == prefix) atomicAdd(&h[(bits >> shift) & 255u], 1u);
  }
  __syncthreads();
  uint32_t c = h[threadIdx.x];
  if (c) atomicAdd(&hist[((int64_t)pass * gridDim.y + b) * 256 + threadIdx.x], c);
}

// The digit of this pass: the bin d with cum(d) <= k < cum(d) + h[d].  One wave per sample, 4 bins per lane and a
// shuffle prefix sum (the first form walked the 256 bins in one thread: 256 dependent loads, 18 us per pass, four
// passes per denoising step).
__global__ __launch_bounds__(64) void q_scan_kernel(QState* st, const uint32_t* __restrict__ hist, int B, int pass) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const uint32_t* h = hist + ((int64_t)pass * B + b) * 256;
  const uint32_t k = st[b].k_rem;
  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = h[4 * lane + j];
  const uint32_t mine = (c[0] + c[1]) + (c[2] + c[3]);
  uint32_t incl = mine;   // inclusive prefix sum over the lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
    if (lane >= off) incl += o;
  }
  uint32_t cum = incl - mine;   // bins before this lane's four
  // the lane that holds the digit: cum <= k < incl (exactly one lane when k < n; lane 63 otherwise, as before)
  const bool here = (k >= cum && k < incl) || (lane == 63 && k >= incl);
  if (here) {
    int d = 4 * lane;
    for (int j = 0; j < 4; ++j) {
      if (k < cum + c[j] || j == 3) {
        d = 4 * lane + j;
        break;
      }
      cum += c[j];
    }
    st[b].prefix |= (uint32_t)d << (24 - 8 * pass);
    st[b].k_rem = k - cum;
    if (pass == 3) st[b].eq_count = h[d];
  }
}

__global__ __launch_bounds__(256) void q_next_kernel(const float* __restrict__ x, QState* st, int64_t n) {
  const int b = blockIdx.y;
  const uint32_t v = st[b].prefix;
  const uint32_t* xb = (const uint32_t*)(x + (int64_t)b * n);
  uint32_t best = 0xFFFFFFFFu;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint32_t bits = xb[i] & 0x7FFFFFFFu;
    if (bits > v && bits < best) best = bits;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t o = (uint32_t)__shfl_xor((int)best, off, 64);
    best = o < best ? o : best;
  }
  if ((threadIdx.x & 63) == 0 && best != 0xFFFFFFFFu) atomicMin(&st[b].next_bits, best);
}

__global__ void q_final_kernel(const QState* __restrict__ st, float* __restrict__ out, int B, float w) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float lo = __uint_as_float(st[b].prefix);
  float hi = lo;
  if (w > 0.f && !(st[b].k_rem + 1 < st[b].eq_count)) hi = __uint_as_float(st[b].next_bits);
  float diff = hi - lo;
  out[b] = (w < 0.5f) ? lo + w * diff : hi - diff * (1.0f - w);  // torch lerp
}

int launch_quantile_abs(const float* x, float* out, int B, int64_t n, float q, void* ws, hipStream_t s) {
  KD_REQUIRE(n >= 1 && n < (1ll << 31), "quantile: n out of range");
  KD_REQUIRE(q >= 0.f && q <= 1.f, "quantile: q must be in [0,1]");
  QState* st = (QState*)ws;
  uint32_t* hist = (uint32_t*)((char*)ws + (size_t)B * sizeof(QState));
  float rank = q * (float)(n - 1);  // fp32, as torch computes it
  float lo_f = floorf(rank);
  uint32_t k = (uint32_t)lo_f;
  float w = rank - lo_f;
  if ((int64_t)k >= n - 1) {  // q == 1
    k = (uint32_t)(n - 1);
    w = 0.f;
  }
  int init_threads = 4 * B * 256;
  hipLaunchKernelGGL(q_init_kernel, dim3((init_threads + 255) / 256), dim3(256), 0, s, st, hist, B, k);
  int gx = (int)((n + 256 * 16 - 1) / (256 * 16));
  if (gx < 1) gx = 1;
  if (gx > 256) gx = 256;
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(q_hist_kernel, dim3(gx, B), dim3(256), 0, s, x, st, hist, n, pass);
    hipLaunchKernelGGL(q_scan_kernel, dim3(B), dim3(64), 0, s, st, hist, B, pass);
  }
  hipLaunchKernelGGL(q_next_kernel, dim3(gx, B), dim3(256), 0, s, x, st, n);
  hipLaunchKernelGGL(q_final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, st, out, B, w);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- fused DDPM reverse step
// x0c = clamp(x0,-s,s)/s ; mean = alpha_next*(x*(1-c)/alpha + c*x0c) ; x = mean + noise_scale*N(0,1)
__global__ void ddpm_update_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                   const float* __restrict__ s_thresh, const float* __restrict__ noise,
                                   int64_t noise_stride, const uint64_t* __restrict__ d_seed, StepTables tb,
                                   const int* __restrict__ d_iter, int R, int dynamic_threshold, int64_t per4,
                                   float* __restrict__ sc_out) {
  const int b = blockIdx.y;   // one grid row per image: no division splits the flat index
  const NoiseKey key = noise_key(d_seed, b, per4);  // device-resident: the captured step graph is seed-independent
  const int it = *d_iter;
  const int k = it / R;
  const float alpha = tb.alpha[k], alpha_next = tb.alpha_next[k], c = tb.c[k], ns = tb.noise_scale[k];
  const float one_minus_c = 1.0f - c;
  float s = 1.0f;
  if (dynamic_threshold) s = fmaxf(s_thresh[b], 1.0f);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < per4; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)b * per4 + j;
    f32x4 xv = *(const f32x4*)(x + i * 4), x0v = *(const f32x4*)(x0 + i * 4);
    f32x4 z = noise4(noise, noise_stride, key, PURPOSE_STEP, it, i, j), o, xsv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xs = fminf(fmaxf(x0v[e], -s), s) / s;
      xsv[e] = xs;
      float mean = alpha_next * (xv[e] * one_minus_c / alpha + c * xs);
      o[e] = mean + ns * z[e];
    }
    *(f32x4*)(x + i * 4) = o;
    if (sc_out) *(f32x4*)(sc_out + i * 4) = xsv;   // self-conditioning: the next step's UNet reads this x_start
  }
}
int launch_ddpm_update(float* x, const float* x0, const float* s_thresh, const float* noise, int64_t noise_stride,
                       const uint64_t* d_seed, const StepTables& tb, const int* d_iter, int R, int dynamic_threshold, int B,
                       int64_t per, hipStream_t s, float* sc_out) {
  KD_REQUIRE(per % 4 == 0, "per-sample element count must be a multiple of 4");
  KD_REQUIRE(B >= 1 && B <= 65535, "batch out of range for the per-image grid");
  hipLaunchKernelGGL(ddpm_update_kernel, grid_rows(per / 4, B), dim3(256), 0, s, x, x0, s_thresh, noise,
                     noise_stride, d_seed, tb, d_iter, R, dynamic_threshold, per / 4, sc_out);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- fused few-step solver update
// DDIM(eta), DPM-Solver++(2M / 3M) and the SDE forms of 2M and 3M in one form:
//     x = A_k x + B_k x0c + P_k h1 + Q_k h2 + S_k N(0,1)
// x0c the thresholded estimate of ddpm_update_kernel, h1 / h2 the x0c that steps k - 1 / k - 2 kept.  The host puts the
// solver into the tables (kd_solver_schedule_t, kd_solver3_schedule_t).  A term whose coefficient is 0 is left out, operand
// unread: no draw for a deterministic step, and no read of a history on a step of lower order - the first two steps a call
// walks read nothing an earlier call left.  A history takes this step's x0c in the last resample slot only, so all R
// resamples of step k read the estimates of steps k - 1 and k - 2; in place, each thread behind its own read.
//   RING == false (no Q table): one history `hist`, h1 - today's 2M and DDIM, arguments and arithmetic unchanged.
//   RING == true: `hist` and `hist2` are the two slots of a ring indexed by the step's parity, read from the iteration
//   counter - h1 in slot (k - 1) & 1, h2 in slot k & 1, which then takes x0c - so one captured step serves every step.
template <bool RING>
__device__ __forceinline__ void solver_update_body(float* __restrict__ x, const float* __restrict__ x0,
                                                   const float* __restrict__ s_thresh, const float* __restrict__ noise,
                                                   int64_t noise_stride, const uint64_t* __restrict__ d_seed,
                                                   const SolverTables& tb, const int* __restrict__ d_iter, int R,
                                                   int dynamic_threshold, int64_t per4, float* hist, float* hist2,
                                                   const float* __restrict__ coef_prev2, float* __restrict__ sc_out) {
  const int b = blockIdx.y;
  const NoiseKey key = noise_key(d_seed, b, per4);
  const int it = *d_iter;
  const int k = it / R, ri = it - k * R;
  const float ca = tb.coef_x[k], cb = tb.coef_x0[k], cp = tb.coef_prev[k], cs = tb.coef_noise[k];
  const float cq = RING ? coef_prev2[k] : 0.0f;
  float* h1 = hist;    // the estimate of step k - 1
  float* h2 = hist2;   // of step k - 2; takes this step's
  if (RING) {
    h1 = (k & 1) ? hist : hist2;
    h2 = (k & 1) ? hist2 : hist;
  }
  float* kept = RING ? h2 : h1;
  const bool use_prev = h1 != nullptr && cp != 0.0f, use_prev2 = RING && cq != 0.0f, use_noise = cs != 0.0f;
  const bool keep = kept != nullptr && ri == R - 1;
  float s = 1.0f;
  if (dynamic_threshold) s = fmaxf(s_thresh[b], 1.0f);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < per4; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)b * per4 + j;
    f32x4 xv = *(const f32x4*)(x + i * 4), x0v = *(const f32x4*)(x0 + i * 4), o, xsv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xs = fminf(fmaxf(x0v[e], -s), s) / s;
      xsv[e] = xs;
      o[e] = ca * xv[e] + cb * xs;
    }
    if (use_prev) {
      f32x4 hv = *(const f32x4*)(h1 + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + cp * hv[e];
    }
    if (use_prev2) {
      f32x4 hv = *(const f32x4*)(h2 + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + cq * hv[e];
    }
    if (use_noise) {
      f32x4 z = noise4(noise, noise_stride, key, PURPOSE_STEP, it, i, j);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + cs * z[e];
    }
    *(f32x4*)(x + i * 4) = o;
    if (keep) *(f32x4*)(kept + i * 4) = xsv;
    if (sc_out) *(f32x4*)(sc_out + i * 4) = xsv;   // self-conditioning: the next step's UNet reads this x_start
  }
}
__global__ void solver_update_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                     const float* __restrict__ s_thresh, const float* __restrict__ noise,
                                     int64_t noise_stride, const uint64_t* __restrict__ d_seed, SolverTables tb,
                                     const int* __restrict__ d_iter, int R, int dynamic_threshold, int64_t per4,
                                     float* hist, float* __restrict__ sc_out) {
  solver_update_body<false>(x, x0, s_thresh, noise, noise_stride, d_seed, tb, d_iter, R, dynamic_threshold, per4, hist, nullptr,
                            nullptr, sc_out);
}
__global__ void solver3_update_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                      const float* __restrict__ s_thresh, const float* __restrict__ noise,
                                      int64_t noise_stride, const uint64_t* __restrict__ d_seed, SolverTables tb,
                                      const int* __restrict__ d_iter, int R, int dynamic_threshold, int64_t per4,
                                      float* hist, float* hist2, const float* __restrict__ coef_prev2,
                                      float* __restrict__ sc_out) {
  solver_update_body<true>(x, x0, s_thresh, noise, noise_stride, d_seed, tb, d_iter, R, dynamic_threshold, per4, hist, hist2,
                           coef_prev2, sc_out);
}
// hist2 != nullptr: the ring form (coef_prev2 and hist given too); else today's launch
int launch_solver_update(float* x, const float* x0, const float* s_thresh, const float* noise, int64_t noise_stride,
                         const uint64_t* d_seed, const SolverTables& tb, const int* d_iter, int R, int dynamic_threshold,
                         int B, int64_t per, hipStream_t s, float* hist, float* sc_out, float* hist2, const float* coef_prev2) {
  KD_REQUIRE(per % 4 == 0, "per-sample element count must be a multiple of 4");
  KD_REQUIRE(B >= 1 && B <= 65535, "batch out of range for the per-image grid");
  if (hist2) {
    KD_REQUIRE(hist != nullptr && coef_prev2 != nullptr && hist != hist2, "solver update: the ring needs two histories and coef_prev2");
    hipLaunchKernelGGL(solver3_update_kernel, grid_rows(per / 4, B), dim3(256), 0, s, x, x0, s_thresh, noise, noise_stride,
                       d_seed, tb, d_iter, R, dynamic_threshold, per / 4, hist, hist2, coef_prev2, sc_out);
  } else {
    hipLaunchKernelGGL(solver_update_kernel, grid_rows(per / 4, B), dim3(256), 0, s, x, x0, s_thresh, noise, noise_stride,
                       d_seed, tb, d_iter, R, dynamic_threshold, per / 4, hist, sc_out);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- inpainting (RePaint-style)
// x = x*(1-m) + (alpha_t*inp + sigma_t*noise)*m        (mask [B,1,HW], image [B,C,HW])
__global__ void inpaint_mix_kernel(float* __restrict__ x, const float* __restrict__ inp,
                                   const float* __restrict__ mask, const float* __restrict__ noise,
                                   int64_t noise_stride, const uint64_t* __restrict__ d_seed, StepTables tb,
                                   const int* __restrict__ d_iter, int R, int64_t hw4, int64_t per4) {
  const int b = blockIdx.y;
  const NoiseKey key = noise_key(d_seed, b, per4);
  const int it = *d_iter;
  const int k = it / R;
  const float alpha = tb.alpha[k], sigma = tb.sigma[k];
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < per4; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)b * per4 + j, p4 = j % hw4;   // (the mask has one plane per image)
    f32x4 m = *(const f32x4*)(mask + (b * hw4 + p4) * 4);
    f32x4 xv = *(const f32x4*)(x + i * 4), iv = *(const f32x4*)(inp + i * 4);
    f32x4 z = noise4(noise, noise_stride, key, PURPOSE_INPAINT, it, i, j), o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float noised = alpha * iv[e] + sigma * z[e];
      o[e] = m[e] != 0.f ? noised : xv[e];  // img*~mask + noised*mask with a boolean mask
    }
    *(f32x4*)(x + i * 4) = o;
  }
}
int launch_inpaint_mix(float* x, const float* inp, const float* mask, const float* noise, int64_t noise_stride,
                       const uint64_t* d_seed, const StepTables& tb, const int* d_iter, int R, int B, int C, int64_t hw,
                       hipStream_t s) {
  KD_REQUIRE(hw % 4 == 0, "H*W must be a multiple of 4");
  KD_REQUIRE(B >= 1 && B <= 65535, "batch out of range for the per-image grid");
  hipLaunchKernelGGL(inpaint_mix_kernel, grid_rows(C * hw / 4, B), dim3(256), 0, s, x, inp, mask, noise,
                     noise_stride, d_seed, tb, d_iter, R, hw / 4, C * hw / 4);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// re-noise t_next -> t after a non-final resample:  x = x*rn_a + noise*rn_b   (skipped when r == 0 or last k)
__global__ void renoise_kernel(float* __restrict__ x, const float* __restrict__ noise, int64_t noise_stride,
                               const uint64_t* __restrict__ d_seed, StepTables tb,
                               const int* __restrict__ d_iter, int R, int T, int64_t per4) {
  const int b = blockIdx.y;
  const NoiseKey key = noise_key(d_seed, b, per4);
  const int it = *d_iter;
  const int k = it / R, ri = it - k * R;
  if (ri == R - 1 || k == T - 1) return;
  const float a = tb.rn_a[k], bco = tb.rn_b[k];
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < per4; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)b * per4 + j;
    f32x4 xv = *(const f32x4*)(x + i * 4);
    f32x4 z = noise4(noise, noise_stride, key, PURPOSE_RENOISE, it, i, j), o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = xv[e] * a + z[e] * bco;
    *(f32x4*)(x + i * 4) = o;
  }
}
int launch_renoise(float* x, const float* noise, int64_t noise_stride, const uint64_t* d_seed, const StepTables& tb,
                   const int* d_iter, int R, int T, int B, int64_t per, hipStream_t s) {
  KD_REQUIRE(per % 4 == 0, "per-sample element count must be a multiple of 4");
  KD_REQUIRE(B >= 1 && B <= 65535, "batch out of range for the per-image grid");
  hipLaunchKernelGGL(renoise_kernel, grid_rows(per / 4, B), dim3(256), 0, s, x, noise, noise_stride, d_seed, tb,
                     d_iter, R, T, per / 4);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- EDM Heun sampler (ElucidatedImagen)
// One step k (iteration it, k = it / R):  x_hat = x + churn_k * (S_noise * N(0,1))  [known pixels: inp + the same
// added noise]; den = thr(c_skip(sh) x_hat + c_out(sh) net(c_in(sh) x_hat)); d = (x_hat - den) / sh;
// x_next = x_hat + (sn - sh) d; Heun: den2 = thr(c_skip(sn) x_next + c_out(sn) net(c_in(sn) x_next)),
// d2 = (x_next - den2) / sn, x = x_hat + 0.5 (sn - sh) (d + d2) (+ RePaint re-noise).  The host computes every
// per-step scalar as the library does (python doubles for sh / churn / step sizes, fp32 torch ops for the c_*).

// x_hat (inpaint mix included) -> xh, and c_in(sh) * x_hat -> net_in (the UNet's input)
__global__ void edm_churn_kernel(const float* __restrict__ x, float* __restrict__ xh, float* __restrict__ net_in,
                                 const float* __restrict__ inp, const float* __restrict__ mask,
                                 const float* __restrict__ noise, int64_t noise_stride, const uint64_t* __restrict__ d_seed,
                                 EdmTables tb, float s_noise, const int* __restrict__ d_iter, int R, int64_t hw4,
                                 int64_t per4) {
  const int b = blockIdx.y;
  const NoiseKey key = noise_key(d_seed, b, per4);
  const int it = *d_iter;
  const int k = it / R;
  const float churn = tb.churn[k], c_in = tb.c_in_hat[k];
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < per4; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)b * per4 + j;
    f32x4 xv = *(const f32x4*)(x + i * 4);
    f32x4 z = noise4(noise, noise_stride, key, PURPOSE_EDM_CHURN, it, i, j), o, ci;
    f32x4 m = {0.f, 0.f, 0.f, 0.f}, iv = {0.f, 0.f, 0.f, 0.f};
    if (inp) {
      const int64_t p4 = j % hw4;
      m = *(const f32x4*)(mask + (b * hw4 + p4) * 4);
      iv = *(const f32x4*)(inp + i * 4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float added = churn * (s_noise * z[e]);
      o[e] = m[e] != 0.f ? iv[e] + added : xv[e] + added;   // x_hat*~mask + (inp + added)*mask, boolean mask
      ci[e] = c_in * o[e];
    }
    *(f32x4*)(xh + i * 4) = o;
    *(f32x4*)(net_in + i * 4) = ci;
  }
}
int launch_edm_churn(const float* x, float* xh, float* net_in, const float* inp, const float* mask, const float* noise,
                     int64_t noise_stride, const uint64_t* d_seed, const EdmTables& tb, float s_noise, const int* d_iter,
                     int R, int B, int C, int64_t hw, hipStream_t s) {
  KD_REQUIRE(hw % 4 == 0, "H*W must be a multiple of 4");
  KD_REQUIRE(B >= 1 && B <= 65535, "batch out of range for the per-image grid");
  hipLaunchKernelGGL(edm_churn_kernel, grid_rows(C * hw / 4, B), dim3(256), 0, s, x, xh, net_in, inp, mask, noise,
                     noise_stride, d_seed, tb, s_noise, d_iter, R, hw / 4, C * hw / 4);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// den = c_skip[k] * x + c_out[k] * net   (before the threshold: the x0 estimate kd_sample_last reports)
__global__ void edm_precond_out_kernel(const float* __restrict__ x, const float* __restrict__ net, float* __restrict__ den,
                                       const float* __restrict__ c_skip_tab, const float* __restrict__ c_out_tab,
                                       const int* __restrict__ d_iter, int R, int64_t n4) {
  const int k = *d_iter / R;
  const float c_skip = c_skip_tab[k], c_out = c_out_tab[k];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 xv = *(const f32x4*)(x + i * 4), nv = *(const f32x4*)(net + i * 4), o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = c_skip * xv[e] + c_out * nv[e];
    *(f32x4*)(den + i * 4) = o;
  }
}
int launch_edm_precond_out(const float* x, const float* net, float* den, const float* c_skip_tab, const float* c_out_tab,
                           const int* d_iter, int R, int64_t n, hipStream_t s) {
  KD_REQUIRE(n % 4 == 0, "image element count must be a multiple of 4");
  hipLaunchKernelGGL(edm_precond_out_kernel, dim3(grid_for(n / 4)), dim3(256), 0, s, x, net, den, c_skip_tab, c_out_tab,
                     d_iter, R, n / 4);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

__device__ __forceinline__ float edm_thr(float v, float s) { return fminf(fmaxf(v, -s), s) / s; }

// Euler: d = (x_hat - thr(den)) / sh -> d_out ; x_next = x_hat + (sn - sh) d -> x ; c_in(sn) x_next -> net_in
__global__ void edm_euler_kernel(const float* __restrict__ xh, const float* __restrict__ den,
                                 const float* __restrict__ s_thresh, float* __restrict__ d_out, float* __restrict__ x,
                                 float* __restrict__ net_in, EdmTables tb, const int* __restrict__ d_iter, int R,
                                 int dynamic_threshold, int64_t per4, int64_t total4, float* __restrict__ sc_out) {
  const int k = *d_iter / R;
  const float sh = tb.sigma_hat[k], step = tb.euler_step[k], c_in = tb.c_in_next[k];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
    const float s = dynamic_threshold ? fmaxf(s_thresh[i / per4], 1.0f) : 1.0f;
    f32x4 hv = *(const f32x4*)(xh + i * 4), dv = *(const f32x4*)(den + i * 4), d, xn, ci, tv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tv[e] = edm_thr(dv[e], s);
      d[e] = (hv[e] - tv[e]) / sh;
      xn[e] = hv[e] + step * d[e];
      ci[e] = c_in * xn[e];
    }
    *(f32x4*)(d_out + i * 4) = d;
    *(f32x4*)(x + i * 4) = xn;
    *(f32x4*)(net_in + i * 4) = ci;
    if (sc_out) *(f32x4*)(sc_out + i * 4) = tv;   // self-conditioning: the Heun forward (or the next step) reads it
  }
}
int launch_edm_euler(const float* xh, const float* den, const float* s_thresh, float* d_out, float* x, float* net_in,
                     const EdmTables& tb, const int* d_iter, int R, int dynamic_threshold, int B, int64_t per,
                     hipStream_t s, float* sc_out) {
  KD_REQUIRE(per % 4 == 0, "per-sample element count must be a multiple of 4");
  const int64_t total4 = (int64_t)B * per / 4;
  hipLaunchKernelGGL(edm_euler_kernel, dim3(grid_for(total4)), dim3(256), 0, s, xh, den, s_thresh, d_out, x, net_in, tb,
                     d_iter, R, dynamic_threshold, per / 4, total4, sc_out);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// Heun: d2 = (x_next - thr(den2)) / sn ; x = x_hat + 0.5 (sn - sh) (d + d2) ; RePaint re-noise x += (s - sn) N(0,1)
// after every resample but the last (r == 0) and never on the last step.  x holds x_next on entry (in place).
__global__ void edm_heun_kernel(float* __restrict__ x, const float* __restrict__ xh, const float* __restrict__ d_in,
                                const float* __restrict__ den, const float* __restrict__ s_thresh,
                                const float* __restrict__ noise, int64_t noise_stride, const uint64_t* __restrict__ d_seed,
                                EdmTables tb, const int* __restrict__ d_iter, int R, int N, int renoise,
                                int dynamic_threshold, int64_t per4, float* __restrict__ sc_out) {
  const int b = blockIdx.y;
  const NoiseKey key = noise_key(d_seed, b, per4);
  const int it = *d_iter;
  const int k = it / R, ri = it - k * R;
  const bool rn = renoise && ri != R - 1 && k != N - 1;
  const float sn = tb.sigma_next[k], step = tb.heun_step[k], rs = tb.renoise[k];
  const float s = dynamic_threshold ? fmaxf(s_thresh[b], 1.0f) : 1.0f;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < per4; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)b * per4 + j;
    f32x4 xv = *(const f32x4*)(x + i * 4), hv = *(const f32x4*)(xh + i * 4), dv = *(const f32x4*)(d_in + i * 4),
          nv = *(const f32x4*)(den + i * 4), o, tv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tv[e] = edm_thr(nv[e], s);
      const float d2 = (xv[e] - tv[e]) / sn;
      o[e] = hv[e] + step * (dv[e] + d2);
    }
    if (sc_out) *(f32x4*)(sc_out + i * 4) = tv;   // self-conditioning: the next step's first forward reads it
    if (rn) {
      f32x4 z = noise4(noise, noise_stride, key, PURPOSE_EDM_RENOISE, it, i, j);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + rs * z[e];
    }
    *(f32x4*)(x + i * 4) = o;
  }
}
int launch_edm_heun(float* x, const float* xh, const float* d_in, const float* den, const float* s_thresh,
                    const float* noise, int64_t noise_stride, const uint64_t* d_seed, const EdmTables& tb,
                    const int* d_iter, int R, int N, int renoise, int dynamic_threshold, int B, int64_t per,
                    hipStream_t s, float* sc_out) {
  KD_REQUIRE(per % 4 == 0, "per-sample element count must be a multiple of 4");
  KD_REQUIRE(B >= 1 && B <= 65535, "batch out of range for the per-image grid");
  hipLaunchKernelGGL(edm_heun_kernel, grid_rows(per / 4, B), dim3(256), 0, s, x, xh, d_in, den, s_thresh, noise,
                     noise_stride, d_seed, tb, d_iter, R, N, renoise, dynamic_threshold, per / 4, sc_out);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// final: clamp(-1,1); paste known pixels; (x+1)/2
__global__ void finalize_kernel(float* __restrict__ x, const float* __restrict__ inp,
                                const float* __restrict__ mask, int C, int64_t hw4, int64_t total4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4;
       i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 xv = *(const f32x4*)(x + i * 4), o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fminf(fmaxf(xv[e], -1.0f), 1.0f);
    if (inp) {
      int64_t plane = i / hw4, p4 = i - plane * hw4;
      int64_t b = plane / C;
      f32x4 m = *(const f32x4*)(mask + (b * hw4 + p4) * 4), iv = *(const f32x4*)(inp + i * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = m[e] != 0.f ? iv[e] : o[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (o[e] + 1.0f) * 0.5f;
    *(f32x4*)(x + i * 4) = o;
  }
}
int launch_finalize(float* x, const float* inp, const float* mask, int B, int C, int64_t hw, hipStream_t s) {
  int64_t total4 = (int64_t)B * C * hw / 4;
  hipLaunchKernelGGL(finalize_kernel, dim3(grid_for(total4)), dim3(256), 0, s, x, inp, mask, C, hw / 4, total4);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
