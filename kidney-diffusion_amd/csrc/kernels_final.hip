// Final 3x3 convolution to the image's C = 1 .. 4 channels (Cout = C is far too narrow for an MFMA tile).
//
//   out[b][o][y][x] = bias[o] + sum_{c,kh,kw} in[b][y+kh-1][x+kw-1][c] * W[o][c][kh][kw]
//
// is evaluated as (1) a 1x1 GEMM on the matrix cores, P[pixel][o*9+tap] = sum_c feat[pixel][c] *
// W[o][c][tap] (9 C columns: 9 / 18 / 27 padded to 32, 36 padded to 48 - final_gemm_cols), and (2) the 9-tap
// gather-sum below, which also adds the step-invariant contribution of the low-res conditioning planes (`stat`,
// computed once per sampling call by final_static_kernel) and writes the NCHW prediction the sampler consumes.
// C <= 3 keeps the 32-column P and the launches of the 3-channel plans; C = 4 is the one width past 32 columns.
#include "common.h"

namespace kd {

int final_gemm_cols(int ch) { return ch <= 3 ? 32 : 48; }

// w_oihw [ch][Ctot][3][3] -> packed [nf][C] rows n = o*9 + tap for channels [0, C); rows 9 ch .. nf - 1 zero
__global__ void pack_final_kernel(const float* __restrict__ w, float* __restrict__ out, int Ctot, int C, int ch, int nf) {
  int total = nf * C;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    int c = idx % C, n = idx / C;
    float v = 0.f;
    if (n < 9 * ch) {
      int o = n / 9, tap = n - o * 9;
      v = w[((int64_t)o * Ctot + c) * 9 + tap];
    }
    out[idx] = v;
  }
}
int launch_pack_final(const float* w, float* out, int Ctot, int C, int ch, hipStream_t s) {
  KD_REQUIRE(ch >= 1 && ch <= 4 && C >= 1 && C <= Ctot, "final conv: 1 .. 4 image channels");
  const int nf = final_gemm_cols(ch);
  hipLaunchKernelGGL(pack_final_kernel, dim3((nf * C + 255) / 256), dim3(256), 0, s, w, out, Ctot, C, ch, nf);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// stat[b][o][y][x] = bias[o] + sum_{c<ch,taps} lowres[b][c][y+kh-1][x+kw-1] * w[o][c0+c][kh][kw]   (NCHW in/out)
__global__ void final_static_kernel(const float* __restrict__ lowres, const float* __restrict__ w,
                                    const float* __restrict__ bias, float* __restrict__ stat, int Ctot, int c0, int ch,
                                    int H, int W, int64_t total) {
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
      for (int kh = 0; kh < 3; ++kh) {
        int iy = y + kh - 1;
        if (iy < 0 || iy >= H) continue;
        for (int kw = 0; kw < 3; ++kw) {
          int ix = x + kw - 1;
          if (ix < 0 || ix >= W) continue;
          acc += lowres[((b * ch + c) * H + iy) * W + ix] * w[((int64_t)o * Ctot + c0 + c) * 9 + kh * 3 + kw];
        }
      }
    stat[idx] = acc;
  }
}
int launch_final_static(const float* lowres, const float* w, const float* bias, float* stat, int Ctot, int c0, int ch,
                        int B, int H, int W, hipStream_t s) {
  KD_REQUIRE(ch >= 1 && ch <= 4 && c0 >= 0 && c0 + ch <= Ctot, "final conv: 1 .. 4 low-res planes inside the weights");
  int64_t total = (int64_t)B * ch * H * W;
  int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(final_static_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, lowres, w,
                     bias, stat, Ctot, c0, ch, H, W, total);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// out[b][o][y][x] = (stat ? stat[b][o][y][x] : bias[o]) + sum_tap P[b][y+kh-1][x+kw-1][o*9+tap]
// One block per 4 rows x 64 pixels (a wave per row): the 6 x 66 pixel rows of P are staged in LDS
// with 16-B loads - every row of P is read 1.5 times (3 times with the one-row blocks of rounds 1-3: 165 -> ~60 us at
// the headline shape) -, then every lane sums its pixel's 9 CH values.  CH <= 3: all 32 columns of a row of P are
// staged (8 loads per pixel); CH = 4: the 36 used ones of its 48 (9 loads) - either way a pixel takes 36 floats of LDS,
// an odd multiple of 4 (conflict-free 4-B reads), and the tile stays within 64 KB (a row of 52 floats for all 48
// columns would take 80 KB and the second workgroup off the CU).
constexpr int FG_ROWS = 4, FG_LD = 36;
template <int CH>
__global__ __launch_bounds__(64 * FG_ROWS) void final_gather_kernel(const float* __restrict__ P, const float* __restrict__ stat,
                                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                                   int H, int W) {
  constexpr int NF = CH <= 3 ? 32 : 48;   // final_gemm_cols(CH)
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
int launch_final_gather(const float* P, const float* stat, const float* bias, float* out, int ch, int B, int H, int W,
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

}  // namespace kd
