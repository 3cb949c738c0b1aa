// Final 3x3 convolution to the image's C = 1 .. 4 channels (Cout = C is far too narrow for an MFMA tile).
//
//   out[b][o][y][x] = bias[o] + sum_{c,kh,kw} in[b][y+kh-1][x+kw-1][c] * W[o][c][kh][kw]
//
// is evaluated as (1) a 1x1 GEMM on the matrix cores, P[pixel][o*9+tap] = sum_c feat[pixel][c] *
// W[o][c][tap] (9 C columns: 9 / 18 / 27 padded to 32, 36 padded to 48 - final_gemm_cols_k), and (2) the 9-tap
// gather-sum below, which also adds the step-invariant contribution of the low-res conditioning planes (`stat`,
// computed once per sampling call by final_static_kernel) and writes the NCHW prediction the sampler consumes.
// C <= 3 keeps the 32-column P and the launches of the 3-channel plans; C = 4 is the one width past 32 columns.
//
// Unet(final_conv_kernel_size=k), k = 1 | 5 | 7 (k = 3 keeps its own gather below, bit for bit): the same two steps with
// the (output, tap) columns n = o kp + tap, kp = k^2 rounded up to a multiple of 4 (28 | 52: every channel's columns start
// on a 16-byte boundary; the pad columns have zero weights; k = 3 keeps kp = 9, its gather reads column o 9 + tap), the row
// padded to a multiple of 16 and at least 32 columns (final_gemm_cols_k).  At k = 7 a pixel has up to 208 columns and a
// gather tile holding all of them would not fit LDS, so the k x k gather is tiled by OUTPUT CHANNEL: a workgroup stages the kp
// columns of one channel o over its halo patch (16-byte loads; kp + 1 = 29 | 53 floats per pixel in LDS, odd: conflict-free
// reads) and every lane of the first TW x ROWS threads sums its pixel's k^2 taps.  k = 1 has no taps to gather: out =
// (stat | bias) + P[pixel][o], no LDS.
#include "common.h"

namespace kd {

static bool final_k_ok(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }
static int final_kp(int k) { return k == 1 ? 1 : k == 3 ? 9 : (k * k + 3) & ~3; }   // columns per output channel
int final_gemm_cols_k(int ch, int k) {   // (k = 3: 32 columns; 48 at ch = 4)
  const int n = (final_kp(k) * ch + 15) / 16 * 16;
  return n < 32 ? 32 : n;
}

// w_oihw [ch][Ctot][k][k] -> packed [nf][C] rows n = o kp + tap for channels [0, C); rows with tap >= k^2 or o >= ch zero
__global__ void pack_final_k_kernel(const float* __restrict__ w, float* __restrict__ out, int Ctot, int C, int ch, int nf, int kk,
                                    int kp) {
  int total = nf * C;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx % C, n = idx / C;
    int o = n / kp, tap = n - o * kp;
    float v = 0.f;
    if (o < ch && tap < kk) v = w[((int64_t)o * Ctot + c) * kk + tap];
    out[idx] = v;
  }
}
int launch_pack_final_k(const float* w, float* out, int Ctot, int C, int ch, int k, hipStream_t s) {
  KD_REQUIRE(ch >= 1 && ch <= 4 && C >= 1 && C <= Ctot && final_k_ok(k), "final conv: 1 .. 4 image channels, kernel size 1, 3, 5 or 7");
  const int nf = final_gemm_cols_k(ch, k);
  hipLaunchKernelGGL(pack_final_k_kernel, dim3((nf * C + 255) / 256), dim3(256), 0, s, w, out, Ctot, C, ch, nf, k * k,
                     final_kp(k));
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// stat[b][o][y][x] = bias[o] + sum_{c<ch,taps} lowres[b][c][y+kh-ks/2][x+kw-ks/2] * w[o][c0+c][kh][kw]   (NCHW in/out; ks x ks taps)
__global__ void final_static_kernel(const float* __restrict__ lowres, const float* __restrict__ w,
                                    const float* __restrict__ bias, float* __restrict__ stat, int Ctot, int c0, int ch,
                                    int H, int W, int64_t total, int ks) {
  const int pad = ks >> 1, kk = ks * ks;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int x = (int)(idx % W);
    int64_t t = idx / W;
    int y = (int)(t % H);
    t /= H;
    int o = (int)(t % ch);
    int64_t b = t / ch;
    float acc = bias[o];
    for (int c = 0; c < ch; ++c)
      for (int kh = 0; kh < ks; ++kh) {
        int iy = y + kh - pad;
        if (iy < 0 || iy >= H) continue;
        for (int kw = 0; kw < ks; ++kw) {
          int ix = x + kw - pad;
          if (ix < 0 || ix >= W) continue;
          acc += lowres[((b * ch + c) * H + iy) * W + ix] * w[((int64_t)o * Ctot + c0 + c) * kk + kh * ks + kw];
        }
      }
    stat[idx] = acc;
  }
}
int launch_final_static(const float* lowres, const float* w, const float* bias, float* stat, int Ctot, int c0, int ch,
                        int B, int H, int W, hipStream_t s, int ks) {
  KD_REQUIRE(ch >= 1 && ch <= 4 && c0 >= 0 && c0 + ch <= Ctot, "final conv: 1 .. 4 low-res planes inside the weights");
  KD_REQUIRE(ks == 1 || ks == 3 || ks == 5 || ks == 7, "final conv: kernel size 1, 3, 5 or 7");
  int64_t total = (int64_t)B * ch * H * W;
  int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(final_static_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, lowres, w,
                     bias, stat, Ctot, c0, ch, H, W, total, ks);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// out[b][o][y][x] = (stat ? stat[b][o][y][x] : bias[o]) + sum_tap P[b][y+kh-1][x+kw-1][o*9+tap]
// One block per 4 rows x 64 pixels (a wave per row): the 6 x 66 pixel rows of P are staged in LDS
// with 16-B loads - every row of P is read 1.5 times (3 times with one-row blocks) -, then every lane sums its pixel's
// 9 CH values.  CH <= 3: all 32 columns of a row of P are
// staged (8 loads per pixel); CH = 4: the 36 used ones of its 48 (9 loads) - either way a pixel takes 36 floats of LDS,
// an odd multiple of 4 (conflict-free 4-B reads), and the tile stays within 64 KB (a row of 52 floats for all 48
// columns would take 80 KB and the second workgroup off the CU).
constexpr int FG_ROWS = 4, FG_LD = 36;
template <int CH>
__global__ __launch_bounds__(64 * FG_ROWS) void final_gather_kernel(const float* __restrict__ P, const float* __restrict__ stat,
                                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                                   int H, int W) {
  constexpr int NF = CH <= 3 ? 32 : 48;   // final_gemm_cols_k(CH, 3)
  constexpr unsigned NQ = CH <= 3 ? 8 : 9;     // 16-B pieces of a row of P that are staged
  static_assert(4 * NQ <= FG_LD && 9 * CH <= 4 * NQ && 4 * NQ <= NF, "final gather: staged columns");
  __shared__ __attribute__((aligned(16))) float tile[FG_ROWS + 2][66][FG_LD];  // padded rows: conflict-free 4-B reads
  const int segs = (W + 63) / 64, rgs = (H + FG_ROWS - 1) / FG_ROWS;
  const int seg = blockIdx.x % segs, rg = (blockIdx.x / segs) % rgs, b = blockIdx.x / (segs * rgs);
  const int x0 = seg * 64, y0 = rg * FG_ROWS, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  for (unsigned idx = threadIdx.x; idx < (FG_ROWS + 2) * 66 * NQ; idx += 64 * FG_ROWS) {
    int q = idx % NQ, px = (idx / NQ) % 66, r = idx / (66 * NQ);
    int iy = y0 + r - 1, ix = x0 + px - 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const f32x4*)(P + (((int64_t)b * H + iy) * W + ix) * NF + q * 4);
    *(f32x4*)&tile[r][px][q * 4] = v;
  }
  __syncthreads();
  const int x = x0 + lane, y = y0 + wv;
  if (x >= W || y >= H) return;
#pragma unroll
  for (int o = 0; o < CH; ++o) {
    const int64_t oi = (((int64_t)b * CH + o) * H + y) * W + x;
    float acc = stat ? stat[oi] : bias[o];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc += tile[wv + kh][lane + kw][o * 9 + kh * 3 + kw];
    out[oi] = acc;
  }
}
static int launch_final_gather(const float* P, const float* stat, const float* bias, float* out, int ch, int B, int H, int W,
                               hipStream_t s) {
  KD_REQUIRE(ch >= 1 && ch <= 4 && ((uintptr_t)P & 15) == 0, "final conv: 1 .. 4 image channels, 16-byte aligned P");
  const int segs = (W + 63) / 64, rgs = (H + FG_ROWS - 1) / FG_ROWS;
  const dim3 grid((unsigned)((int64_t)B * rgs * segs)), block(64 * FG_ROWS);
  switch (ch) {
    case 1: hipLaunchKernelGGL(final_gather_kernel<1>, grid, block, 0, s, P, stat, bias, out, H, W); break;
    case 2: hipLaunchKernelGGL(final_gather_kernel<2>, grid, block, 0, s, P, stat, bias, out, H, W); break;
    case 3: hipLaunchKernelGGL(final_gather_kernel<3>, grid, block, 0, s, P, stat, bias, out, H, W); break;
    default: hipLaunchKernelGGL(final_gather_kernel<4>, grid, block, 0, s, P, stat, bias, out, H, W); break;
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- the gathers of k = 1 | 5 | 7
// k = 1: out[b][o][y][x] = (stat ? stat : bias[o]) + P[b][y][x][o]
__global__ void final_cols_kernel(const float* __restrict__ P, const float* __restrict__ stat, const float* __restrict__ bias,
                                  float* __restrict__ out, int ch, int nf, int64_t hw, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pix = idx % hw, t = idx / hw;
    const int o = (int)(t % ch);
    const int64_t b = t / ch;
    out[idx] = (stat ? stat[idx] : bias[o]) + P[(b * hw + pix) * nf + o];
  }
}

// out[b][o][y][x] = (stat ? stat[b][o][y][x] : bias[o]) + sum_tap P[b][y+kh-K/2][x+kw-K/2][o KP + tap], one output channel
// and one TW x ROWS pixel tile per workgroup of NT >= TW ROWS threads (all stage, the first TW ROWS sum); tile
// [(ROWS + K - 1)][(TW + K - 1)][KP + 1] floats of dynamic LDS
template <int K, int TW, int ROWS, int NT>
__global__ __launch_bounds__(NT) void final_gather_k_kernel(const float* __restrict__ P, const float* __restrict__ stat,
                                                            const float* __restrict__ bias, float* __restrict__ out, int CH, int NF,
                                                            int H, int W) {
  constexpr int KP = (K * K + 3) & ~3, Q = KP / 4, LD = KP + 1, PW = TW + K - 1, PH = ROWS + K - 1, PAD = K / 2;
  static_assert((LD & 1) && NT >= TW * ROWS, "an odd pixel stride reads LDS free of bank conflicts");
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) float fk_tile[];
  const int segs = (W + TW - 1) / TW, rgs = (H + ROWS - 1) / ROWS;
  int t = blockIdx.x;
  const int seg = t % segs;
  t /= segs;
  const int rg = t % rgs;
  t /= rgs;
  const int o = t % CH, b = t / CH;
  const int x0 = seg * TW, y0 = rg * ROWS;
  const float* Po = P + (int64_t)b * H * W * NF + o * KP;   // 16-byte aligned: NF % 4 == 0, KP % 4 == 0
#pragma unroll 4
  for (int idx = threadIdx.x; idx < PH * PW * Q; idx += NT) {
    const int q = idx % Q, pp = idx / Q;
    const int px = pp % PW, r = pp / PW;
    const int iy = y0 + r - PAD, ix = x0 + px - PAD;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const f32x4*)(Po + ((int64_t)iy * W + ix) * NF + q * 4);
    float* d = fk_tile + pp * LD + q * 4;
    d[0] = v[0];
    d[1] = v[1];
    d[2] = v[2];
    d[3] = v[3];
  }
  __syncthreads();
  if (threadIdx.x >= TW * ROWS) return;
  const int lx = threadIdx.x % TW, ly = threadIdx.x / TW;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= W || y >= H) return;
  const int64_t oi = (((int64_t)b * CH + o) * H + y) * W + x;
  float acc = stat ? stat[oi] : bias[o];
#pragma unroll
  for (int kh = 0; kh < K; ++kh)
#pragma unroll
    for (int kw = 0; kw < K; ++kw) acc += fk_tile[((ly + kh) * PW + lx + kw) * LD + kh * K + kw];
  out[oi] = acc;
}
template <int K, int TW, int ROWS, int NT>
static int launch_final_gather_kt(const float* P, const float* stat, const float* bias, float* out, int ch, int nf, int B, int H,
                                  int W, hipStream_t s) {
  constexpr size_t smem = (size_t)(ROWS + K - 1) * (TW + K - 1) * (((K * K + 3) & ~3) + 1) * sizeof(float);
  static_assert(smem <= 160 * 1024, "final gather: the tile must fit LDS");
  const int64_t blocks = (int64_t)B * ch * ((H + ROWS - 1) / ROWS) * ((W + TW - 1) / TW);
  KD_REQUIRE(blocks < 0x7fffffff && nf % 4 == 0 && ((uintptr_t)P & 15) == 0, "final conv: too many tiles for one launch, or P not 16-byte aligned");
  KD_HIP_CHECK(hipFuncSetAttribute((const void*)final_gather_k_kernel<K, TW, ROWS, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)smem));
  hipLaunchKernelGGL((final_gather_k_kernel<K, TW, ROWS, NT>), dim3((unsigned)blocks), dim3(NT), smem, s, P, stat, bias, out, ch, nf,
                     H, W);
  return 0;
}
int launch_final_gather_k(const float* P, const float* stat, const float* bias, float* out, int ch, int k, int B, int H, int W,
                          hipStream_t s) {
  if (k == 3) return launch_final_gather(P, stat, bias, out, ch, B, H, W, s);
  KD_REQUIRE(ch >= 1 && ch <= 4 && final_k_ok(k) && B >= 1 && H >= 1 && W >= 1, "final conv: 1 .. 4 image channels, kernel size 1, 3, 5 or 7");
  const int nf = final_gemm_cols_k(ch, k);
  int rc = 0;
  if (k == 1) {
    const int64_t total = (int64_t)B * ch * H * W, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(final_cols_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, P, stat, bias, out, ch,
                       nf, (int64_t)H * W, total);
  } else if (k == 5) {
    rc = launch_final_gather_kt<5, 64, 4, 256>(P, stat, bias, out, ch, nf, B, H, W, s);
  } else {
    rc = launch_final_gather_kt<7, 32, 8, 512>(P, stat, bias, out, ch, nf, B, H, W, s);
  }
  if (rc) return rc;
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
