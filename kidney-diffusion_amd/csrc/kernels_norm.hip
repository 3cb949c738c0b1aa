// HBM-bound normalisation / elementwise kernels on NHWC fp32 feature maps.
// All of them move 16 B per lane and reduce with wavefront (64-lane) shuffles.
#include "common.h"
#include "epilogue.h"

namespace kd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + expf(-v)); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------------- GroupNorm statistics
// grid (chunks, G, B).  Each block sums x and x^2 (fp64 accumulators: CDNA runs fp64 VALU at
// full rate and the kernel is HBM-bound) over its pixel slice of group g, writes one partial.
constexpr int GN_ROWS_PER_BLOCK = 256;

__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, int ldx,
                                                         double* __restrict__ partial, float* __restrict__ stats,
                                                         int HW, int C, int G, double count, float eps) {
  const int g = blockIdx.y, b = blockIdx.z, chunk = blockIdx.x;
  const int Cg = C / G;
  const int Cg4 = Cg >> 2;
  const int p0 = chunk * GN_ROWS_PER_BLOCK;
  const int p1 = min(HW, p0 + GN_ROWS_PER_BLOCK);
  const float* base = x + ((int64_t)b * HW) * ldx + g * Cg;
  double s = 0.0, ss = 0.0;
  const int total = (p1 - p0) * Cg4;
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    int row = idx / Cg4, c4 = idx - row * Cg4;
    f32x4 v = *(const f32x4*)(base + (int64_t)(p0 + row) * ldx + c4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double d = (double)v[e];
      s += d;
      ss += d * d;
    }
  }
  __shared__ double red[2][4];
  s = wave_sum_d(s);
  ss = wave_sum_d(ss);
  int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = s;
    red[1][wave] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    double tss = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (gridDim.x == 1) {  // small map: this workgroup saw the whole group, no finalize launch needed
      double mean = ts / count;
      double var = tss / count - mean * mean;
      if (var < 0.0) var = 0.0;
      stats[(b * G + g) * 2] = (float)mean;
      stats[(b * G + g) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
      return;
    }
    int64_t o = (((int64_t)b * G + g) * gridDim.x + chunk) * 2;
    partial[o] = ts;
    partial[o + 1] = tss;
  }
}

__global__ void gn_finalize_kernel(const double* __restrict__ partial, float* __restrict__ stats, int chunks,
                                   int BG, double count, float eps) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BG) return;
  double s = 0.0, ss = 0.0;
  for (int c = 0; c < chunks; ++c) {
    s += partial[((int64_t)i * chunks + c) * 2];
    ss += partial[((int64_t)i * chunks + c) * 2 + 1];
  }
  double mean = s / count;
  double var = ss / count - mean * mean;
  if (var < 0.0) var = 0.0;
  stats[i * 2] = (float)mean;
  stats[i * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

size_t gn_partial_bytes(int B, int HW, int C, int G) {
  int chunks = (HW + GN_ROWS_PER_BLOCK - 1) / GN_ROWS_PER_BLOCK;
  return (size_t)B * G * chunks * 2 * sizeof(double);
}

int launch_gn_stats(const float* x, int ldx, float* stats, double* partial, int B, int HW, int C, int G,
                    float eps, hipStream_t s) {
  KD_REQUIRE(C % G == 0 && (C / G) % 4 == 0 && ldx % 4 == 0, "GroupNorm needs (C/G) % 4 == 0");
  int chunks = (HW + GN_ROWS_PER_BLOCK - 1) / GN_ROWS_PER_BLOCK;
  const double count = (double)HW * (C / G);
  hipLaunchKernelGGL(gn_partial_kernel, dim3(chunks, G, B), dim3(256), 0, s, x, ldx, partial, stats, HW, C, G, count,
                     eps);
  // (a single-launch version in which the last workgroup to arrive reduces the partials was measured:
  //  its per-workgroup __threadfence - an L2 write-back on this multi-XCD part - cost 12 ms per step)
  if (chunks > 1) {
    int BG = B * G;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3((BG + 63) / 64), dim3(64), 0, s, partial, stats, chunks, BG, count,
                       eps);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// many partials per (b, g) (the fused conv's epilogue leaves one per workgroup wave): one workgroup per (b, g),
// thread t sums entries t, t + 256, ... and the 256 sums are folded pairwise - a fixed order either way
__global__ __launch_bounds__(256) void gn_finalize_wide_kernel(const double* __restrict__ partial, float* __restrict__ stats,
                                                               int chunks, double count, float eps) {
  __shared__ double sh[2][256];
  const int i = blockIdx.x, t = threadIdx.x;
  double s = 0.0, ss = 0.0;
  for (int c = t; c < chunks; c += 256) {
    s += partial[((int64_t)i * chunks + c) * 2];
    ss += partial[((int64_t)i * chunks + c) * 2 + 1];
  }
  sh[0][t] = s;
  sh[1][t] = ss;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double mean = sh[0][0] / count;
    double var = sh[1][0] / count - mean * mean;
    if (var < 0.0) var = 0.0;
    stats[i * 2] = (float)mean;
    stats[i * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

int launch_gn_finalize(const double* partial, float* stats, int chunks, int B, int G, double count, float eps,
                       hipStream_t s) {
  const int BG = B * G;
  if (chunks >= 64) {
    hipLaunchKernelGGL(gn_finalize_wide_kernel, dim3(BG), dim3(256), 0, s, partial, stats, chunks, count, eps);
    KD_HIP_CHECK(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((BG + 63) / 64), dim3(64), 0, s, partial, stats, chunks, BG, count, eps);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- GroupNorm apply
// y = silu( ((x-mean)*rstd*gamma + beta) * (scale+1) + shift ), folded to silu(x*A + Bc) per (b,c).
constexpr int GA_ROWS_PER_BLOCK = 64;  // upper bound; small maps use fewer rows per workgroup (see launch)

__global__ __launch_bounds__(256) void gn_apply_silu_kernel(const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ scale_shift,
                                                            int ld_ss, float* __restrict__ y, int HW, int C,
                                                            int G, int rows_per_block) {
  const int b = blockIdx.y;
  const int C4 = C >> 2;
  const int W = C4 < 256 ? C4 : 256;
  const int RP = 256 / W;
  const int rsub = threadIdx.x / W;
  if (rsub >= RP) return;
  const int Cg = C / G;
  const int p0 = blockIdx.x * rows_per_block;
  const int p1 = min(HW, p0 + rows_per_block);
  for (int c4 = threadIdx.x - rsub * W; c4 < C4; c4 += W) {
    float A[4], Bc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int c = c4 * 4 + e;
      int g = c / Cg;
      float mean = stats[(b * G + g) * 2], rstd = stats[(b * G + g) * 2 + 1];
      float a = rstd * gamma[c];
      float bb = beta[c] - mean * a;
      if (scale_shift) {
        float sc = scale_shift[(int64_t)b * ld_ss + c] + 1.0f;
        float sh = scale_shift[(int64_t)b * ld_ss + C + c];
        a *= sc;
        bb = bb * sc + sh;
      }
      A[e] = a;
      Bc[e] = bb;
    }
    for (int row = p0 + rsub; row < p1; row += RP) {
      int64_t pix = (int64_t)b * HW + row;
      f32x4 v = *(const f32x4*)(x + pix * ldx + c4 * 4);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = silu_f(v[e] * A[e] + Bc[e]);
      *(f32x4*)(y + pix * C + c4 * 4) = o;
    }
  }
}

int launch_gn_apply_silu(const float* x, int ldx, const float* stats, const float* gamma, const float* beta,
                         const float* scale_shift, int ld_ss, float* y, int B, int HW, int C, int G,
                         hipStream_t s) {
  KD_REQUIRE(C % 4 == 0 && ldx % 4 == 0, "GroupNorm apply needs C % 4 == 0");
  // aim at >= 512 workgroups: a batch-1 patch at the 8x8 level would otherwise run on ONE workgroup
  int rpb = (int)(((int64_t)B * HW + 511) / 512);
  rpb = rpb < 1 ? 1 : (rpb > GA_ROWS_PER_BLOCK ? GA_ROWS_PER_BLOCK : rpb);
  int chunks = (HW + rpb - 1) / rpb;
  hipLaunchKernelGGL(gn_apply_silu_kernel, dim3(chunks, B), dim3(256), 0, s, x, ldx, stats, gamma, beta,
                     scale_shift, ld_ss, y, HW, C, G, rpb);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- LayerNorm (one wave per row)
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int ldx,
                                                        const float* __restrict__ g,
                                                        const float* __restrict__ beta,
                                                        const float* __restrict__ res, int ldres,
                                                        float* __restrict__ y, int rows, int C, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + (int64_t)row * ldx;
  float* yr = y + (int64_t)row * C;
  const int C4 = C >> 2;
  float s = 0.f;
  for (int c4 = lane; c4 < C4; c4 += 64) {
    f32x4 v = *(const f32x4*)(xr + c4 * 4);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = wave_sum_f(s) / (float)C;
  float ss = 0.f;
  for (int c4 = lane; c4 < C4; c4 += 64) {
    f32x4 v = *(const f32x4*)(xr + c4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float d = v[e] - mean;
      ss += d * d;
    }
  }
  const float var = wave_sum_f(ss) / (float)C;
  const float rstd = 1.0f / sqrtf(var + eps);
  for (int c4 = lane; c4 < C4; c4 += 64) {
    f32x4 v = *(const f32x4*)(xr + c4 * 4);
    f32x4 gg = *(const f32x4*)(g + c4 * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (v[e] - mean) * rstd * gg[e];
    if (beta) {
      f32x4 bb = *(const f32x4*)(beta + c4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] += bb[e];
    }
    if (res) {
      f32x4 rr = *(const f32x4*)(res + (int64_t)row * ldres + c4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] += rr[e];
    }
    *(f32x4*)(yr + c4 * 4) = o;
  }
}

// The same with the row held in registers (C <= 256 NV floats: one wave per row, NV float4 per lane) - one read of x
// instead of three -, an optional activation applied to x on the way in (GELU: the feed-forward's Linear -> GELU ->
// LayerNorm, with the GEMM storing the raw product; same function on the same values as the GEMM epilogue's: bit-equal),
// and an optional SECOND LayerNorm of the result (gain g2, output y2): the TransformerBlock's x1 = LN(proj) g + x followed
// by h0 = LN(x1) g2 in one pass over the row.
typedef float f32x2n __attribute__((ext_vector_type(2)));

// FULL: C == 256 NV - no lane is past the row, so the loads carry no bounds branch and hipcc issues them together (with the
// branch every load got a full wait behind it: 85 waits for 17 loads at C = 1024).  Gains / added maps come in groups of four
// float4 per lane.
template <int NV, bool FULL>
__global__ __launch_bounds__(256) void layernorm_reg_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ g,
                                                            const float* __restrict__ beta, const float* __restrict__ res,
                                                            int ldres, float* __restrict__ y, int rows, int C, float eps,
                                                            int in_act, const float* __restrict__ g2, float* __restrict__ y2,
                                                            double* __restrict__ seg, int seg_hw, int planes) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + (int64_t)row * ldx;
  const int C4 = C >> 2;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  // planes & 1: y, & 2: y2 leave as the three bf16 planes of the bf16x3 GEMM's A operand, [3][C / 16][rows][16]
  // (kernels_gemm_bf16x3.hip): the lane's four values are a quarter of a 32-byte plane row - 8 bytes per plane
  auto put_planes = [&](float* dst, int c4, const f32x4& o) {
    uint32_t h0, m0, l0, h1, m1, l1;
    x3_split(f32x2n{o[0], o[1]}, h0, m0, l0);
    x3_split(f32x2n{o[2], o[3]}, h1, m1, l1);
    typedef unsigned int u32x2n __attribute__((ext_vector_type(2)));
    const int64_t plane = (int64_t)rows * C / 2;   // dwords per plane
    uint32_t* q = (uint32_t*)dst + (((int64_t)(c4 >> 2) * rows + row) * 8 + (c4 & 3) * 2);
    *(u32x2n*)q = u32x2n{h0, h1};
    *(u32x2n*)(q + plane) = u32x2n{m0, m1};
    *(u32x2n*)(q + 2 * plane) = u32x2n{l0, l1};
  };
  auto in = [&](int i) { return FULL || lane + 64 * i < C4; };
  // a lane past the row reads the row's first float4 instead (valid memory) and is masked wherever it would count
  auto ld4 = [&](const float* p, int i) { return *(const f32x4*)(p + (in(i) ? lane + 64 * i : 0) * 4); };
  f32x4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = ld4(xr, i);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (in_act != ACT_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = ep_act(v[i][e], in_act);
    }
    if (!in(i)) v[i] = z4;
    if (in(i)) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  }
  const float mean = wave_sum_f(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (in(i)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[i][e] - mean;
        ss += d * d;
      }
    }
  const float rstd = 1.0f / sqrtf(wave_sum_f(ss) / (float)C + eps);
  float s2 = 0.f;
  constexpr int GRP = NV < 4 ? NV : 4;
#pragma unroll
  for (int i0 = 0; i0 < NV; i0 += GRP) {
    f32x4 gg[GRP], bb[GRP], rr[GRP];
#pragma unroll
    for (int k = 0; k < GRP; ++k) gg[k] = ld4(g, i0 + k);
    if (beta) {
#pragma unroll
      for (int k = 0; k < GRP; ++k) bb[k] = ld4(beta, i0 + k);
    }
    if (res) {
#pragma unroll
      for (int k = 0; k < GRP; ++k) rr[k] = ld4(res + (int64_t)row * ldres, i0 + k);
    }
#pragma unroll
    for (int k = 0; k < GRP; ++k) {
      const int i = i0 + k, c4 = lane + 64 * i;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * gg[k][e];
      if (beta) o += bb[k];
      if (res) o += rr[k];
      if (in(i)) {
        if (planes & 1) put_planes(y, c4, o);
        else *(f32x4*)(y + (int64_t)row * C + c4 * 4) = o;
        v[i] = o;
        s2 += (o[0] + o[1]) + (o[2] + o[3]);
      }
      if (seg) {
        // GroupNorm partials of y for the layer that normalises it (SegSrc, common.h): one chunk per pixel; the four lanes
        // 4 j .. 4 j + 3 hold the 16 channels of segment j + 16 i (whole waves get here: C4 % 4 == 0, lanes past the row add zeros)
        double d1 = in(i) ? (double)((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) : 0.0;
        double d2 = in(i) ? (double)fmaf(v[i][0], v[i][0], fmaf(v[i][1], v[i][1], fmaf(v[i][2], v[i][2], v[i][3] * v[i][3]))) : 0.0;
        d1 += __shfl_xor(d1, 1, 64);
        d2 += __shfl_xor(d2, 1, 64);
        d1 += __shfl_xor(d1, 2, 64);
        d2 += __shfl_xor(d2, 2, 64);
        if (in(i) && (lane & 3) == 0) {
          const int b = row / seg_hw, pix = row - b * seg_hw;
          double* o2 = seg + (((int64_t)b * (C >> 4) + (c4 >> 2)) * seg_hw + pix) * 2;
          o2[0] = d1;
          o2[1] = d2;
        }
      }
    }
  }
  if (!g2) return;
  const float mean2 = wave_sum_f(s2) / (float)C;
  float ss2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (in(i)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[i][e] - mean2;
        ss2 += d * d;
      }
    }
  const float rstd2 = 1.0f / sqrtf(wave_sum_f(ss2) / (float)C + eps);
#pragma unroll
  for (int i0 = 0; i0 < NV; i0 += GRP) {
    f32x4 gg[GRP];
#pragma unroll
    for (int k = 0; k < GRP; ++k) gg[k] = ld4(g2, i0 + k);
#pragma unroll
    for (int k = 0; k < GRP; ++k) {
      const int i = i0 + k;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean2) * rstd2 * gg[k][e];
      if (in(i)) {
        if (planes & 2) put_planes(y2, lane + 64 * i, o);
        else *(f32x4*)(y2 + (int64_t)row * C + (lane + 64 * i) * 4) = o;
      }
    }
  }
}

int launch_layernorm(const float* x, int ldx, const float* g, const float* beta, const float* res, int ldres, float* y,
                     int rows, int C, float eps, hipStream_t s, int in_act, const float* g2, float* y2, double* seg, int seg_hw,
                     int planes) {
  KD_REQUIRE(!planes || (C % 16 == 0 && C <= 4096 && (planes & ~3) == 0 && (!(planes & 2) || g2)),
             "LayerNorm: plane-form output needs C % 16 == 0, C <= 4096");
  KD_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && (!res || ldres % 4 == 0), "LayerNorm needs C % 4 == 0");
  KD_REQUIRE((g2 == nullptr) == (y2 == nullptr), "LayerNorm: the second normalisation needs its gain and its output");
  KD_REQUIRE(!seg || (C % 16 == 0 && C <= 4096 && seg_hw > 0 && rows % seg_hw == 0),
             "LayerNorm: output statistics need C % 16 == 0, C <= 4096 and whole images");
  const dim3 grid((rows + 3) / 4), block(256);
#define KD_LN(NV_)                                                                                                              \
  do {                                                                                                                          \
    if (C == 256 * NV_)                                                                                                         \
      hipLaunchKernelGGL((layernorm_reg_kernel<NV_, true>), grid, block, 0, s, x, ldx, g, beta, res, ldres, y, rows, C, eps, in_act, \
                         g2, y2, seg, seg_hw, planes);                                                                          \
    else                                                                                                                        \
      hipLaunchKernelGGL((layernorm_reg_kernel<NV_, false>), grid, block, 0, s, x, ldx, g, beta, res, ldres, y, rows, C, eps,     \
                         in_act, g2, y2, seg, seg_hw, planes);                                                                  \
  } while (0)
  if (C <= 256) KD_LN(1);
  else if (C <= 512) KD_LN(2);
  else if (C <= 1024) KD_LN(4);
  else if (C <= 2048) KD_LN(8);
  else if (C <= 4096) KD_LN(16);
  else {
    KD_REQUIRE(in_act == ACT_NONE && !g2 && !planes, "LayerNorm rows above 4096 channels: plain form only");
    hipLaunchKernelGGL(layernorm_kernel, grid, block, 0, s, x, ldx, g, beta, res, ldres, y, rows, C, eps);
  }
#undef KD_LN
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- gate / add
static inline int grid_for(int64_t n_items) {
  int64_t b = (n_items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}
// y = a * gate[b][c] + r, NHWC.  r and y may be channel slices of wider tensors (row strides ldr / ldy: a skip
// tensor that already lives in the buffer of the concat it will be part of).  seg != nullptr: the kernel also
// leaves the GroupNorm partials of y for the layer that reads it - per image, 16-channel segment and pixel chunk
// one (sum, sum of squares) in fp64, [B][C/16][gridDim.x][2], summed in a fixed order (launch_gn_fold_seg), so
// the next GroupNorm needs no statistics pass over y.
__global__ __launch_bounds__(256) void gate_add_kernel(const float* __restrict__ a, const float* __restrict__ gate,
                                                       const float* __restrict__ r, int ldr, float* __restrict__ y,
                                                       int ldy, double* __restrict__ seg, int HW, int C, int rpb) {
  __shared__ double sh[2][64];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int C4 = C >> 2;
  const int Wd = C4 < 256 ? C4 : 256;
  const int RP = 256 / Wd;
  const int rsub = threadIdx.x / Wd, col = threadIdx.x - rsub * Wd;
  const bool active = rsub < RP;
  const int p0 = chunk * rpb, p1 = min(HW, p0 + rpb);
  const int nseg = C >> 4, segw = Wd >> 2;
  for (int c4b = 0; c4b < C4; c4b += Wd) {
    const int c4 = c4b + col;
    double s1 = 0.0, s2 = 0.0;
    if (active && c4 < C4) {
      f32x4 g = {1.f, 1.f, 1.f, 1.f};
      if (gate) g = *(const f32x4*)(gate + ((int64_t)b * C4 + c4) * 4);
      for (int row = p0 + rsub; row < p1; row += RP) {
        const int64_t pix = (int64_t)b * HW + row;
        f32x4 v = *(const f32x4*)(a + (pix * C4 + c4) * 4);
        const f32x4 rr = *(const f32x4*)(r + pix * ldr + c4 * 4);
        v = v * g + rr;
        *(f32x4*)(y + pix * ldy + c4 * 4) = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double d = (double)v[e];
          s1 += d;
          s2 += d * d;
        }
      }
    }
    if (seg) {   // (block-uniform)
      s1 += __shfl_xor(s1, 1, 64);
      s2 += __shfl_xor(s2, 1, 64);
      s1 += __shfl_xor(s1, 2, 64);
      s2 += __shfl_xor(s2, 2, 64);
      if (active && (col & 3) == 0) {
        sh[0][rsub * segw + (col >> 2)] = s1;
        sh[1][rsub * segw + (col >> 2)] = s2;
      }
      __syncthreads();
      const int sg = (c4b >> 2) + threadIdx.x;
      if (threadIdx.x < segw && sg < nseg) {
        double t1 = 0.0, t2 = 0.0;
        for (int q = 0; q < RP; ++q) {
          t1 += sh[0][q * segw + threadIdx.x];
          t2 += sh[1][q * segw + threadIdx.x];
        }
        double* o = seg + (((int64_t)b * nseg + sg) * nchunk + chunk) * 2;
        o[0] = t1;
        o[1] = t2;
      }
      __syncthreads();
    }
  }
}
// pixel rows per workgroup of launch_gate_add: the partial layout of `seg` has gate_add_chunks(B, HW) chunks
static inline int gate_add_rpb(int B, int HW) {
  int rpb = (int)(((int64_t)B * HW + 2047) / 2048);
  return rpb < 8 ? 8 : (rpb > 64 ? 64 : rpb);
}
int gate_add_chunks(int B, int HW) {
  const int rpb = gate_add_rpb(B, HW);
  return (HW + rpb - 1) / rpb;
}
int launch_gate_add(const float* a, const float* gate, const float* r, int ldr, float* y, int ldy, double* seg, int B,
                    int HW, int C, hipStream_t s) {
  KD_REQUIRE(C % 4 == 0 && ldr % 4 == 0 && ldy % 4 == 0, "gate_add needs C % 4 == 0");
  KD_REQUIRE(!seg || C % 16 == 0, "gate_add: segment statistics need C % 16 == 0");
  const int rpb = gate_add_rpb(B, HW);
  hipLaunchKernelGGL(gate_add_kernel, dim3((HW + rpb - 1) / rpb, B), dim3(256), 0, s, a, gate, r, ldr, y, ldy, seg, HW, C,
                     rpb);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// GroupNorm statistics from segment partials, and the per-(image, channel) affine the normalisation (+ FiLM)
// folds to, in ONE launch (was gn_finalize + gn_fold).  The input of the GroupNorm is the channel concat of up
// to two sources; source i covers channels [c0, c0 + 16 nseg) and is seen by the layer as `scale` * x (skip
// connections enter scaled by 2^-1/2).  If the consuming kernel reads the UNSCALED source, `ab_mul` = scale
// moves the factor into the affine (A x' + B with x' = ab_mul x), else ab_mul = 1.  One workgroup per
// (group, image): the partials are summed thread-strided and folded pairwise - a fixed order.
constexpr int GFS_T = 1024;   // threads of gn_fold_seg_kernel (a batch-1 1024^2 map has 32768 partials per segment)
__global__ __launch_bounds__(GFS_T) void gn_fold_seg_kernel(SegSrc s0, SegSrc s1, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ scale_shift, int ld_ss,
                                                          float* __restrict__ ab, float* __restrict__ stats, int C, int G,
                                                          double count, float eps) {
  __shared__ double sh[2][GFS_T];
  const int g = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int Cg = C / G, c_lo = g * Cg, c_hi = c_lo + Cg;
  double a1 = 0.0, a2 = 0.0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const SegSrc& sc = k ? s1 : s0;
    if (!sc.partial) continue;
    const int lo = max(c_lo, sc.c0), hi = min(c_hi, sc.c0 + 16 * sc.nseg);
    if (lo >= hi) continue;
    const int sa = (lo - sc.c0) >> 4, se = (hi - sc.c0) >> 4;
    const int64_t n = (int64_t)(se - sa) * sc.nchunk;
    const double* base = sc.partial + (((int64_t)b * sc.nseg + sa) * sc.nchunk) * 2;
    // four independent chains per thread (four 16-byte loads in flight), folded in a fixed order
    double l1[4] = {0.0, 0.0, 0.0, 0.0}, l2[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = t;
    for (; i + 3 * GFS_T < n; i += 4 * GFS_T) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double2 v = *(const double2*)(base + 2 * (i + q * GFS_T));
        l1[q] += v.x;
        l2[q] += v.y;
      }
    }
    for (; i < n; i += GFS_T) {
      l1[0] += base[2 * i];
      l2[0] += base[2 * i + 1];
    }
    a1 += (double)sc.scale * ((l1[0] + l1[1]) + (l1[2] + l1[3]));
    a2 += (double)sc.scale * (double)sc.scale * ((l2[0] + l2[1]) + (l2[2] + l2[3]));
  }
  sh[0][t] = a1;
  sh[1][t] = a2;
  __syncthreads();
  for (int w = GFS_T / 2; w > 0; w >>= 1) {
    if (t < w) {
      sh[0][t] += sh[0][t + w];
      sh[1][t] += sh[1][t + w];
    }
    __syncthreads();
  }
  const double mean_d = sh[0][0] / count;
  double var = sh[1][0] / count - mean_d * mean_d;
  if (var < 0.0) var = 0.0;
  const float mean = (float)mean_d, rstd = (float)(1.0 / sqrt(var + (double)eps));
  if (stats && t == 0) {
    stats[(b * G + g) * 2] = mean;
    stats[(b * G + g) * 2 + 1] = rstd;
  }
  if (!ab) return;
  for (int c = c_lo + t; c < c_hi; c += GFS_T) {
    float a = rstd * gamma[c];
    float bb = beta[c] - mean * a;
    if (scale_shift) {
      const float sc = scale_shift[(int64_t)b * ld_ss + c] + 1.0f;
      const float sft = scale_shift[(int64_t)b * ld_ss + C + c];
      a *= sc;
      bb = bb * sc + sft;
    }
    const float m = (s1.partial && c >= s1.c0 && c < s1.c0 + 16 * s1.nseg) ? s1.ab_mul : s0.ab_mul;
    ab[2 * ((int64_t)b * C + c)] = a * m * WF_AB_SCALE;   // (the fused kernel's activation form, common.h)
    ab[2 * ((int64_t)b * C + c) + 1] = bb * WF_AB_SCALE;
  }
}
int launch_gn_fold_seg(SegSrc s0, SegSrc s1, const float* gamma, const float* beta, const float* scale_shift, int ld_ss,
                       float* ab, float* stats, int B, int C, int G, double count, float eps, hipStream_t s) {
  KD_REQUIRE(s0.partial && C % G == 0 && (C / G) % 16 == 0, "gn_fold_seg: groups must be multiples of 16 channels");
  KD_REQUIRE(s0.c0 == 0 && s0.c0 + 16 * s0.nseg + (s1.partial ? 16 * s1.nseg : 0) == C &&
                 (!s1.partial || s1.c0 == 16 * s0.nseg),
             "gn_fold_seg: the sources must tile the channels");
  hipLaunchKernelGGL(gn_fold_seg_kernel, dim3(G, B), dim3(GFS_T), 0, s, s0, s1, gamma, beta, scale_shift, ld_ss, ab, stats, C,
                     G, count, eps);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// dst[row][0..C) = src[row][0..C) * scale with row strides (concat head copy; in-place scaling of a skip slice)
__global__ void copy_scale_rows_kernel(const float* __restrict__ src, int lds_, float* __restrict__ dst, int ldd, int C4,
                                       float scale, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / C4;
    const int c4 = (int)(idx - row * C4);
    f32x4 v = *(const f32x4*)(src + row * lds_ + c4 * 4);
    v *= scale;
    *(f32x4*)(dst + row * ldd + c4 * 4) = v;
  }
}
int launch_copy_scale_rows(const float* src, int ld_src, float* dst, int ld_dst, int C, float scale, int64_t rows,
                           hipStream_t s) {
  KD_REQUIRE(C % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0, "copy_scale_rows needs multiples of 4 channels");
  const int64_t total = rows * (C / 4);
  hipLaunchKernelGGL(copy_scale_rows_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, ld_src, dst, ld_dst, C / 4, scale,
                     total);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y,
                           int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = a[i] + b[i];
}
int launch_add(const float* a, const float* b, float* y, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(add_kernel, dim3(grid_for(n)), dim3(256), 0, s, a, b, y, n);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

__global__ void act_kernel(const float* __restrict__ a, float* __restrict__ y, int64_t n, int act) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = a[i];
    if (act == ACT_SILU) v = silu_f(v);
    else if (act == ACT_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    else if (act == ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
    y[i] = v;
  }
}
int launch_act(const float* a, float* y, int64_t n, int act, hipStream_t s) {
  hipLaunchKernelGGL(act_kernel, dim3(grid_for(n)), dim3(256), 0, s, a, y, n, act);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- init image assembly
// NCHW planes (cond | x | lowres) -> NHWC [B][HW][Cpad], zero padded.  Channel order follows
// Unet.forward: x = cat(x, lowres); x = cat(cond_images, x)   (SURVEY A.1 / §3.2).
__global__ void pack_init_kernel(const float* __restrict__ cond, int Cc, const float* __restrict__ x, int Cx,
                                 const float* __restrict__ lowres, int Cl, float* __restrict__ y, int Cpad,
                                 int64_t HW, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t pix = idx;  // b*HW + p
    int64_t b = pix / HW, p = pix - b * HW;
    float* o = y + pix * Cpad;
    int c = 0;
    for (int i = 0; i < Cc; ++i) o[c++] = cond[(b * Cc + i) * HW + p];
    if (x)  // x == nullptr: only the step-invariant planes (cond | lowres) are packed
      for (int i = 0; i < Cx; ++i) o[c++] = x[(b * Cx + i) * HW + p];
    for (int i = 0; i < Cl; ++i) o[c++] = lowres[(b * Cl + i) * HW + p];
    for (; c < Cpad; ++c) o[c] = 0.f;
  }
}
int launch_pack_init(const float* cond, int Cc, const float* x, int Cx, const float* lowres, int Cl, float* y, int Cpad,
                     int B, int HW, hipStream_t s) {
  KD_REQUIRE(Cc + (x ? Cx : 0) + Cl <= Cpad, "pack init: the planes do not fit the padded pixel");
  int64_t total = (int64_t)B * HW;
  hipLaunchKernelGGL(pack_init_kernel, dim3(grid_for(total)), dim3(256), 0, s, cond, Cc, x, Cx, lowres, Cl, y, Cpad,
                     (int64_t)HW, total);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

__global__ void copy_rows_kernel(const float* __restrict__ src, int64_t sbs, int lds_, float* __restrict__ dst,
                                 int64_t dbs, int ldd, int rows, int C, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(idx % C);
    int64_t t = idx / C;
    int r = (int)(t % rows);
    int64_t b = t / rows;
    dst[b * dbs + (int64_t)r * ldd + c] = src[b * sbs + (int64_t)r * lds_ + c];
  }
}
int launch_copy_rows(const float* src, int64_t sbs, int ld_src, float* dst, int64_t dbs, int ld_dst, int rows,
                     int C, int B, hipStream_t s) {
  int64_t total = (int64_t)B * rows * C;
  if (total == 0) return 0;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, sbs, ld_src, dst, dbs, ld_dst,
                     rows, C, total);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_bcast_row(const float* src, float* dst, int64_t dst_bstride, int C, int B, hipStream_t s) {
  return launch_copy_rows(src, 0, C, dst, dst_bstride, C, 1, C, B, s);
}

// ab[b][c] = (A, B) with GroupNorm(+FiLM)(x)[b][c] = A x + B (same arithmetic as gn_apply_silu_kernel)
__global__ __launch_bounds__(256) void gn_fold_kernel(const float* __restrict__ stats, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta,
                                                      const float* __restrict__ scale_shift, int ld_ss,
                                                      float* __restrict__ ab, int B, int C, int G) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * C) return;
  const int b = idx / C, c = idx - b * C;
  const int g = c / (C / G);
  const float mean = stats[(b * G + g) * 2], rstd = stats[(b * G + g) * 2 + 1];
  float a = rstd * gamma[c];
  float bb = beta[c] - mean * a;
  if (scale_shift) {
    const float sc = scale_shift[(int64_t)b * ld_ss + c] + 1.0f;
    const float sh = scale_shift[(int64_t)b * ld_ss + C + c];
    a *= sc;
    bb = bb * sc + sh;
  }
  ab[2 * idx] = a * WF_AB_SCALE;   // the fused kernel's activation works on -log2(e) (A x + B)
  ab[2 * idx + 1] = bb * WF_AB_SCALE;
}

int launch_gn_fold(const float* stats, const float* gamma, const float* beta, const float* scale_shift, int ld_ss,
                   float* ab, int B, int C, int G, hipStream_t s) {
  KD_REQUIRE(C % G == 0, "gn_fold: C % G");
  hipLaunchKernelGGL(gn_fold_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, stats, gamma, beta, scale_shift, ld_ss, ab,
                     B, C, G);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}


}  // namespace kd
