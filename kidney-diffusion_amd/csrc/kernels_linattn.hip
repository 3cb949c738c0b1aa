// Linear attention of imagen-pytorch (LinearAttention, LinearCrossAttention) on NHWC tokens, dim_head = 64:
//   ctx[b,h] = sum_n softmax_n(k)[n,d] v[n,e]   (one 64 x 64 block per image and head)
//   out[n]   = act(softmax_d(q[n]) * scale . ctx[b,h])
// Three kernels carry the per-step work: the depthwise 3x3 conv of q | k | v (with online-softmax partials of k per token
// chunk), the context reduction (split over token chunks, summed in a fixed order: no atomics, run-to-run bit-identical)
// and the apply.  Both products run on the fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products and sums).
#include <math.h>

#include "common.h"

namespace kd {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int LA_D = 64;        // dim_head
constexpr int LA_TN = 32;       // tokens per LDS tile of the context reduction
constexpr int LA_NS = 80;       // LDS row stride (floats) of [token][64] tiles read as 4 rows x 16 columns: conflict-free
constexpr int LA_QS = 68;       // LDS row stride of the apply's q tile, read as 16 rows x 4 columns: conflict-free
constexpr int LA_PART = LA_D * LA_D + 2 * LA_D;   // floats per (image, head, split) of the reduction's workspace

// online softmax: fold (m2, s2) - a max and the sum of exp(x - m2) - into (m, s)
__device__ __forceinline__ void la_fold(float& m, float& s, float m2, float s2) {
  if (m2 > m) {
    s = s * expf(m - m2) + s2;
    m = m2;
  } else {
    s += s2 * expf(m2 - m);
  }
}

// [9][3 inner] tap-major depthwise weights from the three [inner][1][3][3] tensors of to_q.2 / to_k.2 / to_v.2
__global__ void la_pack_dw_kernel(const float* __restrict__ wq, const float* __restrict__ wk, const float* __restrict__ wv,
                                  float* __restrict__ dst, int inner) {
  const int C3 = 3 * inner;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * C3) return;
  const int tap = i / C3, c = i - tap * C3;
  const float* src = c < inner ? wq : c < 2 * inner ? wk : wv;
  dst[i] = src[(size_t)(c % inner) * 9 + tap];
}

// column xx of rows py - 1 .. py + 1 of a [H][W][C3] map (channel offset applied), zeros outside the map: the loads read
// the clamped pixel and the value is selected (a select of addresses would put the zeros in scratch memory)
__device__ __forceinline__ float4 la_pick(bool in, float4 v) {
  return make_float4(in ? v.x : 0.f, in ? v.y : 0.f, in ? v.z : 0.f, in ? v.w : 0.f);
}
__device__ __forceinline__ void la_column(const float* __restrict__ xb, int H, int W, int C3, int py, int xx, float4& c0,
                                          float4& c1, float4& c2) {
  const bool in_x = xx >= 0 && xx < W;
  const int xc = min(max(xx, 0), W - 1), y0 = max(py - 1, 0), y2 = min(py + 1, H - 1);
  c0 = la_pick(in_x && py >= 1, *(const float4*)(xb + ((size_t)y0 * W + xc) * C3));
  c1 = la_pick(in_x, *(const float4*)(xb + ((size_t)py * W + xc) * C3));
  c2 = la_pick(in_x && py + 1 < H, *(const float4*)(xb + ((size_t)y2 * W + xc) * C3));
}

// y = depthwise 3x3 (zero padding) of x, both [B][H][W][3 inner] dense.  Block: 128 threads x 4 channels over the
// LA_CHUNK tokens of one chunk of one image (grid.x = B x nchunk, grid.y = channel blocks of 512).  Each thread slides a
// 3 x 3 window of float4 along the row (three loads per token; the next column is loaded before the current token is
// summed).  Threads of k's channels [inner, 2 inner) also leave part[b][chunk][c - inner] = (max, sum of exp(k - max))
// over the chunk's tokens.
__global__ __launch_bounds__(128) void la_dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ y, float2* __restrict__ part, int H, int W,
                                                        int inner, int nchunk) {
  const int C3 = 3 * inner;
  const int b = blockIdx.x / nchunk, ch = blockIdx.x - b * nchunk;
  const int c = (blockIdx.y * 128 + threadIdx.x) * 4;
  if (c >= C3) return;
  const int HW = H * W;
  const int t0 = ch * LA_CHUNK, t1 = min(t0 + LA_CHUNK, HW);
  float4 wr[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wr[t] = *(const float4*)(w + (size_t)t * C3 + c);
  const float* xb = x + (size_t)b * HW * C3 + c;
  float* yb = y + (size_t)b * HW * C3 + c;
  const bool is_k = c >= inner && c < 2 * inner;
  float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = t0; t < t1;) {   // the chunk's row segments
    const int py = t / W, px0 = t - py * W, n = min(t1 - t, W - px0);
    float4 win[3][3];   // [row][column] of the window around (py, px0 + i)
    la_column(xb, H, W, C3, py, px0 - 1, win[0][0], win[1][0], win[2][0]);
    la_column(xb, H, W, C3, py, px0, win[0][1], win[1][1], win[2][1]);
    la_column(xb, H, W, C3, py, px0 + 1, win[0][2], win[1][2], win[2][2]);
    for (int i = 0; i < n; ++i) {
      // the next token's new column, issued before this token's sums
      float4 nxt[3];
      la_column(xb, H, W, C3, py, px0 + i + 2, nxt[0], nxt[1], nxt[2]);
      float4 acc = zero;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 v = win[r][q], ww = wr[r * 3 + q];
          acc.x = fmaf(v.x, ww.x, acc.x);
          acc.y = fmaf(v.y, ww.y, acc.y);
          acc.z = fmaf(v.z, ww.z, acc.z);
          acc.w = fmaf(v.w, ww.w, acc.w);
        }
      *(float4*)(yb + (size_t)(t + i) * C3) = acc;
      if (is_k) {
        la_fold(m0, s0, acc.x, 1.f);
        la_fold(m1, s1, acc.y, 1.f);
        la_fold(m2, s2, acc.z, 1.f);
        la_fold(m3, s3, acc.w, 1.f);
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        win[r][0] = win[r][1];
        win[r][1] = win[r][2];
        win[r][2] = nxt[r];
      }
    }
    t += n;
  }
  if (is_k) {
    float4* pb = (float4*)(part + ((size_t)b * nchunk + ch) * inner + (c - inner));
    pb[0] = make_float4(m0, s0, m1, s1);
    pb[1] = make_float4(m2, s2, m3, s3);
  }
}

// One (split, head, image): P[d][e] = sum over the split's tokens of exp(k[n][d] - m_s[d]) v[n][e], with m_s / S_s the
// max / sum of exp over those tokens folded from the chunk partials in chunk order.  ws block: P [64][64], m_s [64], S_s [64].
// Four waves, wave w the 16 rows d = 16 w ..; tiles of LA_TN tokens through LDS (exp applied on the way in).
__global__ __launch_bounds__(256) void la_ctx_reduce_kernel(const float* __restrict__ k, const float* __restrict__ v, int ld,
                                                            const float2* __restrict__ part, int HW, int inner, int nchunk,
                                                            int cps, float* __restrict__ ws, int nsplit) {
  __shared__ float sk[LA_TN * LA_NS], sv[LA_TN * LA_NS];
  __shared__ float sm[LA_D];
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c0 = sp * cps, c1 = min(c0 + cps, nchunk);
  float* out = ws + (((size_t)b * heads + h) * nsplit + sp) * LA_PART;
  if (tid < LA_D) {
    float m = -INFINITY, s = 0.f;
    for (int ch = c0; ch < c1; ++ch) {
      const float2 p = part[((size_t)b * nchunk + ch) * inner + h * LA_D + tid];
      la_fold(m, s, p.x, p.y);
    }
    sm[tid] = m;
    out[LA_D * LA_D + tid] = m;
    out[LA_D * LA_D + LA_D + tid] = s;
  }
  const int n0 = c0 * LA_CHUNK, n1 = min(c1 * LA_CHUNK, HW);
  const float* kb = k + (size_t)b * HW * ld + h * LA_D;
  const float* vb = v + (size_t)b * HW * ld + h * LA_D;
  f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
  for (int nt = n0; nt < n1; nt += LA_TN) {
    __syncthreads();   // sm written / the previous tile consumed
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = tid + r * 256;
      const int row = i >> 4, col = (i & 15) * 4;
      const int n = nt + row;
      float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < n1) {
        kk = *(const float4*)(kb + (size_t)n * ld + col);
        vv = *(const float4*)(vb + (size_t)n * ld + col);
        kk.x = expf(kk.x - sm[col]);
        kk.y = expf(kk.y - sm[col + 1]);
        kk.z = expf(kk.z - sm[col + 2]);
        kk.w = expf(kk.w - sm[col + 3]);
      }
      *(float4*)(sk + row * LA_NS + col) = kk;
      *(float4*)(sv + row * LA_NS + col) = vv;
    }
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < LA_TN; kt += 4) {
      const int n = kt + (lane >> 4);
      const float a = sk[n * LA_NS + wv * 16 + (lane & 15)];   // A[d][n]
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sv[n * LA_NS + j * 16 + (lane & 15)], acc[j], 0, 0, 0);
    }
  }
  // C/D: column e = 16 j + (lane & 15), row d = 16 wv + 4 (lane >> 4) + r
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(wv * 16 + (lane >> 4) * 4 + r) * LA_D + j * 16 + (lane & 15)] = acc[j][r];
}

// One (head, image): ctx[d][e] = (sum_s exp(m_s - M) P_s + [exp(nk - M) nv] + sum_j exp(ck_j - M) cv_j)[d][e] / S[d], the
// splits in index order, then the null key / value, then the context tokens.
__global__ __launch_bounds__(256) void la_ctx_combine_kernel(const float* __restrict__ ws, int nsplit,
                                                             const float* __restrict__ ck, const float* __restrict__ cv,
                                                             int ldc, int m, const float* __restrict__ nk,
                                                             const float* __restrict__ nv, float* __restrict__ ctx) {
  __shared__ float sM[LA_D], sInv[LA_D];
  const int h = blockIdx.x, b = blockIdx.y, heads = gridDim.x, tid = threadIdx.x;
  const float* wb = ws ? ws + ((size_t)b * heads + h) * nsplit * LA_PART : nullptr;
  const float* ckb = m > 0 ? ck + (size_t)b * m * ldc + h * LA_D : nullptr;
  const float* cvb = m > 0 ? cv + (size_t)b * m * ldc + h * LA_D : nullptr;
  if (tid < LA_D) {
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, wb[s * LA_PART + LA_D * LA_D + tid]);
    if (nk) M = fmaxf(M, nk[tid]);
    for (int j = 0; j < m; ++j) M = fmaxf(M, ckb[(size_t)j * ldc + tid]);
    float S = 0.f;
    for (int s = 0; s < nsplit; ++s)
      S += wb[s * LA_PART + LA_D * LA_D + LA_D + tid] * expf(wb[s * LA_PART + LA_D * LA_D + tid] - M);
    if (nk) S += expf(nk[tid] - M);
    for (int j = 0; j < m; ++j) S += expf(ckb[(size_t)j * ldc + tid] - M);
    sM[tid] = M;
    sInv[tid] = 1.0f / S;
  }
  __syncthreads();
  const int d = tid >> 2, e0 = (tid & 3) * 16;
  const float M = sM[d];
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* P = wb + s * LA_PART;
    const float f = expf(P[LA_D * LA_D + d] - M);
#pragma unroll
    for (int e = 0; e < 16; e += 4) {
      const float4 p = *(const float4*)(P + d * LA_D + e0 + e);
      acc[e] = fmaf(f, p.x, acc[e]);
      acc[e + 1] = fmaf(f, p.y, acc[e + 1]);
      acc[e + 2] = fmaf(f, p.z, acc[e + 2]);
      acc[e + 3] = fmaf(f, p.w, acc[e + 3]);
    }
  }
  if (nk) {
    const float f = expf(nk[d] - M);
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = fmaf(f, nv[e0 + e], acc[e]);
  }
  for (int j = 0; j < m; ++j) {
    const float f = expf(ckb[(size_t)j * ldc + d] - M);
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = fmaf(f, cvb[(size_t)j * ldc + e0 + e], acc[e]);
  }
  const float inv = sInv[d];
  float* o = ctx + (((size_t)b * heads + h) * LA_D + d) * LA_D + e0;
#pragma unroll
  for (int e = 0; e < 16; e += 4) *(float4*)(o + e) = make_float4(acc[e] * inv, acc[e + 1] * inv, acc[e + 2] * inv, acc[e + 3] * inv);
}

// One (64-token tile, head, image): out[n][h*64 + e] = act(sum_d softmax_d(q[n][h*64 + d]) scale ctx[b,h][d][e]).
// The q-softmax is taken on load (4 lanes per token row), ctx sits in LDS; wave w computes tokens 16 w .. 16 w + 15.
__global__ __launch_bounds__(256) void la_apply_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ ctx,
                                                       float* __restrict__ out, int ldo, int N, float scale, int silu) {
  __shared__ float sq[64 * LA_QS], sc[LA_D * LA_NS];
  const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z, heads = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* cb = ctx + ((size_t)b * heads + h) * LA_D * LA_D;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = tid + r * 256;
    const int row = i >> 4, col = (i & 15) * 4;
    *(float4*)(sc + row * LA_NS + col) = *(const float4*)(cb + row * LA_D + col);
  }
  {
    const int row = tid >> 2, cq = (tid & 3) * 16;
    const int n = t0 + row;
    float qv[16];
    if (n < N) {
      const float* qp = q + ((size_t)b * N + n) * ldq + h * LA_D + cq;
#pragma unroll
      for (int e = 0; e < 16; e += 4) {
        const float4 t = *(const float4*)(qp + e);
        qv[e] = t.x;
        qv[e + 1] = t.y;
        qv[e + 2] = t.z;
        qv[e + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) qv[e] = 0.f;
    }
    float mx = qv[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = fmaxf(mx, qv[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      qv[e] = expf(qv[e] - mx);
      sum += qv[e];
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    const float f = scale / sum;
#pragma unroll
    for (int e = 0; e < 16; e += 4)
      *(float4*)(sq + row * LA_QS + cq + e) = make_float4(qv[e] * f, qv[e + 1] * f, qv[e + 2] * f, qv[e + 3] * f);
  }
  __syncthreads();
  f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kt = 0; kt < LA_D; kt += 4) {
    const float a = sq[(wv * 16 + (lane & 15)) * LA_QS + kt + (lane >> 4)];   // A[n][d]
    const int d = kt + (lane >> 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sc[d * LA_NS + j * 16 + (lane & 15)], acc[j], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = t0 + wv * 16 + (lane >> 4) * 4 + r;
    if (n >= N) continue;
    float* op = out + ((size_t)b * N + n) * ldo + h * LA_D + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float o = acc[j][r];
      if (silu) o = o / (1.0f + expf(-o));
      op[j * 16] = o;
    }
  }
}

}  // namespace

int linattn_chunks(int HW) { return (HW + LA_CHUNK - 1) / LA_CHUNK; }

// splits per (image, head): enough blocks to fill the chip twice over (256 CUs), at least one chunk per split
int linattn_splits(int B, int heads, int HW) {
  const int nchunk = linattn_chunks(HW);
  if (nchunk == 0) return 0;
  const int want = (512 + B * heads - 1) / (B * heads);
  const int cps = (nchunk + std::min(std::max(want, 1), nchunk) - 1) / std::min(std::max(want, 1), nchunk);
  return (nchunk + cps - 1) / cps;
}

size_t linattn_ws_floats(int B, int heads, int HW) { return (size_t)B * heads * linattn_splits(B, heads, HW) * LA_PART; }

int launch_linattn_pack_dw(const float* wq, const float* wk, const float* wv, float* dst, int inner, hipStream_t s) {
  KD_REQUIRE(inner > 0 && inner % LA_D == 0, "linear attention: inner = heads x 64");
  const int n = 9 * 3 * inner;
  hipLaunchKernelGGL(la_pack_dw_kernel, dim3((n + 255) / 256), dim3(256), 0, s, wq, wk, wv, dst, inner);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_linattn_dwconv(const float* x, const float* w, float* y, float* part, int B, int H, int W, int inner,
                          hipStream_t s) {
  KD_REQUIRE(B > 0 && H > 0 && W > 0 && inner > 0 && inner % LA_D == 0, "linattn dwconv: B, H, W > 0, inner = heads x 64");
  KD_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) == 0, "linattn dwconv: 16-byte aligned buffers");
  KD_REQUIRE(x != y, "linattn dwconv: not in place");
  const int nchunk = linattn_chunks(H * W);
  KD_REQUIRE((int64_t)B * nchunk < (int64_t(1) << 31), "linattn dwconv: too many chunks");
  const int cblocks = (3 * inner / 4 + 127) / 128;
  hipLaunchKernelGGL(la_dwconv_kernel, dim3(B * nchunk, cblocks), dim3(128), 0, s, x, w, y, (float2*)part, H, W, inner,
                     nchunk);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_linattn_context(const float* k, const float* v, int ld, const float* part, int HW, const float* ck,
                           const float* cv, int ldc, int m, const float* nk, const float* nv, float* ws, float* ctx, int B,
                           int heads, hipStream_t s) {
  KD_REQUIRE(B > 0 && heads > 0 && HW >= 0 && m >= 0 && (HW > 0 || m > 0 || nk), "linattn context: no keys");
  KD_REQUIRE(!nk == !nv, "linattn context: null key and value together");
  KD_REQUIRE(m == 0 || (ck && cv && ldc >= heads * LA_D), "linattn context: context rows");
  KD_REQUIRE((((uintptr_t)ctx) & 15) == 0, "linattn context: 16-byte aligned output");
  const int nsplit = linattn_splits(B, heads, HW);
  if (nsplit > 0) {
    KD_REQUIRE(k && v && part && ws && ld % 4 == 0 && ld >= heads * LA_D, "linattn context: k / v rows, partials, workspace");
    KD_REQUIRE((((uintptr_t)k | (uintptr_t)v | (uintptr_t)ws) & 15) == 0, "linattn context: 16-byte aligned k / v");
    const int nchunk = linattn_chunks(HW);
    const int cps = (nchunk + nsplit - 1) / nsplit;
    hipLaunchKernelGGL(la_ctx_reduce_kernel, dim3(nsplit, heads, B), dim3(256), 0, s, k, v, ld, (const float2*)part, HW,
                       heads * LA_D, nchunk, cps, ws, nsplit);
    KD_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(la_ctx_combine_kernel, dim3(heads, B), dim3(256), 0, s, nsplit > 0 ? ws : nullptr, nsplit, ck, cv, ldc,
                     m, nk, nv, ctx);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_linattn_apply(const float* q, int ldq, const float* ctx, float* out, int ldo, int B, int N, int heads,
                         float scale, int silu, hipStream_t s) {
  KD_REQUIRE(B > 0 && N > 0 && heads > 0 && ldq % 4 == 0 && ldq >= heads * LA_D && ldo >= heads * LA_D,
             "linattn apply: B, N > 0, q rows of heads x 64 floats, 16-byte strides");
  KD_REQUIRE((((uintptr_t)q | (uintptr_t)ctx) & 15) == 0, "linattn apply: 16-byte aligned q / ctx");
  hipLaunchKernelGGL(la_apply_kernel, dim3((N + 63) / 64, heads, B), dim3(256), 0, s, q, ldq, ctx, out, ldo, N, scale, silu);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
