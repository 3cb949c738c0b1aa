// Nearest-neighbour x2 upsample followed by a 3x3 / pad-1 conv (the library's `pixel_shuffle_upsample=False` Upsample)
// in one kernel on fp32 MFMA, NHWC in and out.  The upsampled map is never written: output pixel (2y + p, 2x + q) is a
// 2 x 2 conv over the LOW-RES map with the 3x3 taps that fall on one input pixel summed,
//   rows  p = 0: {y - 1: w[0], y: w[1] + w[2]}     p = 1: {y: w[0] + w[1], y + 1: w[2]}     (columns the same with q)
// so the layer is four phase GEMMs with K = 4 Cin over the low-res pixels: 16 / 36 of the MACs of the conv over the
// upsampled map, and the input is read at low resolution.  Taps off the low-res map are zero (they are exactly the taps
// the 3x3 conv's zero padding would have met).
//
// A workgroup (4 waves) takes 8 x 16 low-res pixels x 64 output channels x the four phases; wave w owns rows 2w, 2w + 1
// of the tile (one 32-row MFMA tile) and keeps 4 phases x 2 column tiles of 32 x 32 accumulators.  Per k-step of 8
// input channels the workgroup stages the 10 x 18 pixel patch (halo of one) and the 16 summed tap matrices' [64][8]
// blocks in LDS; a lane then needs 9 patch vectors (3 x 3 shifts) and 32 weight vectors for 128 MFMAs.
#include "common.h"

namespace kd {

namespace {

typedef float up_f32x16 __attribute__((ext_vector_type(16)));
typedef float up_f32x4 __attribute__((ext_vector_type(4)));

constexpr int UP_TY = 8, UP_TX = 16;                 // low-res pixels of a workgroup's tile
constexpr int UP_PY = UP_TY + 2, UP_PX = UP_TX + 2;  // ... with the halo
constexpr int UP_NT = 64;                            // output channels of a tile
constexpr int UP_KC = 8;                             // input channels per k-step

// wp[t][n][c], t = ((p 2 + q) 2 + a) 2 + b: phase (p, q), tap (a, b) of its 2 x 2 conv = input pixel (y - 1 + p + a, x - 1 + q + b)
__global__ __launch_bounds__(256) void upsample_nearest_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int O, int I) {
  const int64_t n_total = (int64_t)16 * O * I;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_total) return;
  const int c = (int)(idx % I);
  const int n = (int)((idx / I) % O);
  const int t = (int)(idx / ((int64_t)I * O));
  const int p = t >> 3, q = (t >> 2) & 1, a = (t >> 1) & 1, b = t & 1;
  // kernel rows (columns) that land on tap a (b) of phase p (q): p = 0: {0}, {1, 2}; p = 1: {0, 1}, {2}
  const int kh0 = p == 0 ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 2), kh1 = p == 0 ? (a == 0 ? 0 : 2) : (a == 0 ? 1 : 2);
  const int kw0 = q == 0 ? (b == 0 ? 0 : 1) : (b == 0 ? 0 : 2), kw1 = q == 0 ? (b == 0 ? 0 : 2) : (b == 0 ? 1 : 2);
  const float* src = w + ((int64_t)n * I + c) * 9;
  float v = 0.f;
  for (int kh = kh0; kh <= kh1; ++kh)
    for (int kw = kw0; kw <= kw1; ++kw) v += src[kh * 3 + kw];
  wp[idx] = v;
}

__global__ __launch_bounds__(256) void upsample_nearest_conv3x3_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ wp,
                                                                       const float* __restrict__ bias, float* __restrict__ y, int ldy,
                                                                       int yoff, int B, int H, int W, int Cin, int Cout, int tiles_x,
                                                                       int tiles_y) {
  __shared__ up_f32x4 As[2][UP_PY * UP_PX];   // [channel half][patch pixel]: channels c0 + 4 h .. + 3
  __shared__ up_f32x4 Bs[2][16 * UP_NT];      // [channel half][tap matrix t][column]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
  const int x0 = tx * UP_TX, y0 = ty * UP_TY, n0 = blockIdx.y * UP_NT;
  const bool second = n0 + 32 < Cout;   // the tile's second 32 columns exist (Cout % 32 == 0)

  up_f32x16 acc[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[f][j][r] = 0.f;

  const int m = lane & 31, h = lane >> 5;
  const int a_base = (2 * wave + (m >> 4)) * UP_PX + (m & 15);   // the lane's pixel in the patch, before the tap shift
  const float* xb = x + (int64_t)b * H * W * ldx;

  for (int c0 = 0; c0 < Cin; c0 += UP_KC) {
    for (int i = tid; i < 2 * UP_PY * UP_PX; i += 256) {
      const int hh = i & 1, pix = i >> 1;
      const int iy = y0 - 1 + pix / UP_PX, ix = x0 - 1 + pix % UP_PX;
      up_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const up_f32x4*)(xb + ((int64_t)iy * W + ix) * ldx + c0 + 4 * hh);
      As[hh][pix] = v;
    }
#pragma unroll
    for (int i = 0; i < 2 * 16 * UP_NT / 256; ++i) {
      const int idx = tid + 256 * i;
      const int hh = idx & 1, row = idx >> 1;
      const int t = row / UP_NT, n = n0 + row % UP_NT;
      up_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < Cout) v = *(const up_f32x4*)(wp + ((int64_t)t * Cout + n) * Cin + c0 + 4 * hh);
      Bs[hh][row] = v;
    }
    __syncthreads();
    up_f32x4 a[9];
#pragma unroll
    for (int sy = 0; sy < 3; ++sy)
#pragma unroll
      for (int sx = 0; sx < 3; ++sx) a[sy * 3 + sx] = As[h][a_base + sy * UP_PX + sx];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) {
        const up_f32x4 av = a[((f >> 1) + (tp >> 1)) * 3 + (f & 1) + (tp & 1)];
        const up_f32x4 b0 = Bs[h][(f * 4 + tp) * UP_NT + m];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[f][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[k], b0[k], acc[f][0], 0, 0, 0);
        if (second) {
          const up_f32x4 b1 = Bs[h][(f * 4 + tp) * UP_NT + 32 + m];
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[f][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[k], b1[k], acc[f][1], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // Epilogue: each wave turns its tiles through 4 KB of LDS of its own (the weight stage is free after the last barrier), so
  // a lane finishes 4 consecutive channels of 4 pixels with 16-byte stores to the interleaved output positions.
  float* scratch = (float*)&Bs[0][0] + wave * 1024;
  const int rq = lane >> 3, c4 = (lane & 7) * 4;
  float* yb = y + (int64_t)b * (2 * H) * (2 * W) * ldy + yoff;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j == 1 && !second) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) scratch[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + m] = acc[f][j][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int nc = n0 + 32 * j + c4;
      const up_f32x4 bv = bias ? *(const up_f32x4*)(bias + nc) : up_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = rq + 8 * i;
        const int ly = y0 + 2 * wave + (row >> 4), lx = x0 + (row & 15);
        const up_f32x4 v = *(const up_f32x4*)(scratch + row * 32 + c4) + bv;
        if (ly < H && lx < W) *(up_f32x4*)(yb + ((int64_t)(2 * ly + (f >> 1)) * (2 * W) + 2 * lx + (f & 1)) * ldy + nc) = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
}

}  // namespace

const char* upsample_nearest_refusal(int ldx, int ldy, int yoff, int B, int H, int W, int Cin, int Cout) {
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return "upsample_nearest_conv3x3: empty shape";
  if (Cin % UP_KC) return "upsample_nearest_conv3x3: Cin must be a multiple of 8 (the kernel's k-step)";
  if (Cout % 32) return "upsample_nearest_conv3x3: Cout must be a multiple of 32 (one MFMA column tile)";
  if (ldx < Cin || (ldx & 3)) return "upsample_nearest_conv3x3: input row stride must be >= Cin and a multiple of 4";
  if (ldy < yoff + Cout || (ldy & 3) || (yoff & 3) || yoff < 0)
    return "upsample_nearest_conv3x3: output row stride / channel offset must hold Cout channels and be multiples of 4";
  const int64_t tiles = (int64_t)B * ((H + UP_TY - 1) / UP_TY) * ((W + UP_TX - 1) / UP_TX);
  if (tiles > 0x7fffffff) return "upsample_nearest_conv3x3: more than 2^31 tiles";
  return nullptr;
}

size_t upsample_nearest_weight_floats(int Cin, int Cout) { return (size_t)16 * Cout * Cin; }

int launch_upsample_nearest_pack(const float* w_oihw, float* wp, int O, int I, hipStream_t s) {
  const int64_t n = (int64_t)16 * O * I;
  hipLaunchKernelGGL(upsample_nearest_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_oihw, wp, O, I);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_upsample_nearest_conv3x3(const float* x, int ldx, const float* wp, const float* bias, float* y, int ldy, int yoff, int B,
                                    int H, int W, int Cin, int Cout, hipStream_t s) {
  if (const char* why = upsample_nearest_refusal(ldx, ldy, yoff, B, H, W, Cin, Cout)) {
    set_error(why);
    return 1;
  }
  KD_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)wp & 15) == 0 && ((uintptr_t)bias & 15) == 0,
             "upsample_nearest_conv3x3: 16-byte aligned pointers");
  const int tiles_x = (W + UP_TX - 1) / UP_TX, tiles_y = (H + UP_TY - 1) / UP_TY;
  const dim3 grid((unsigned)(B * tiles_y * tiles_x), (unsigned)((Cout + UP_NT - 1) / UP_NT));
  hipLaunchKernelGGL(upsample_nearest_conv3x3_kernel, grid, dim3(256), 0, s, x, ldx, wp, bias, y, ldy, yoff, B, H, W, Cin, Cout, tiles_x,
                     tiles_y);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
