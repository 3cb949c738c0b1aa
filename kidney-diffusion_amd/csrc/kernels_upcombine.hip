// Nearest-neighbour x s upsample (any integer s >= 2) -> [per-(image, channel) affine + SiLU] -> 3x3 / pad-1 conv in one kernel on
// fp32 MFMA, NHWC in and out: the Block of the library's UpsampleCombiner (`Unet(combine_upsample_fmaps=True)`) over an up
// level's map brought to full resolution.  The x2 kernel of kernels_resample.hip generalised: the upsampled map is never
// written, the tile (8 x 16 low-res pixels, 4 waves, k-steps of 8 input channels, a 10 x 18 patch in LDS) is the same.
#include "common.h"

namespace kd {

namespace {

typedef float up_f32x16 __attribute__((ext_vector_type(16)));
typedef float up_f32x4 __attribute__((ext_vector_type(4)));

constexpr int UP_TY = 8, UP_TX = 16;                 // low-res pixels of a workgroup's tile
constexpr int UP_PY = UP_TY + 2, UP_PX = UP_TX + 2;  // ... with the halo
constexpr int UP_KC = 8;                             // input channels per k-step

// Inside the s x s output block of low-res pixel (y, x) an output row is the block's first (reads rows {y - 1: w[0], y: w[1] + w[2]}), an interior one ({y: w[0] + w[1] + w[2]}) or its last
// ({y: w[0] + w[1], y + 1: w[2]}), columns the same: 3 x 3 classes, nine distinct values per (low-res pixel, output channel)
// whatever s is, from 5 x 5 = 25 summed tap matrices (sixteen of them the x2 kernel's).  The matrix work is 25 Cin Cout MACs
// per low-res pixel; the launch is bound by the s^2 stores per pixel.  s = 2 has no interior row or column: that
// instantiation holds the four corner classes only, on the x2 kernel's 64-column tile; the general one holds nine classes
// of 32 columns (144 accumulator registers).
constexpr int UPS_NM = 25;   // summed tap matrices: t = rt 5 + ct
// row (column) tap rt: 0 = first row's tap on y - 1 (w[0]); 1 = first row's on y (w[1] + w[2]); 2 = interior's on y (all
// three); 3 = last row's on y (w[0] + w[1]); 4 = last row's on y + 1 (w[2])
__host__ __device__ constexpr int ups_k0(int rt) { return rt == 1 ? 1 : rt == 4 ? 2 : 0; }
__host__ __device__ constexpr int ups_k1(int rt) { return rt == 0 ? 0 : rt == 3 ? 1 : 2; }
// class r (0 first, 1 interior, 2 last): its taps i = 0 .. ups_ntap(r) - 1, their patch shift (0: y - 1, 1: y, 2: y + 1) and rt
__host__ __device__ constexpr int ups_ntap(int r) { return r == 1 ? 1 : 2; }
__host__ __device__ constexpr int ups_shift(int r, int i) { return r == 0 ? i : r == 1 ? 1 : 1 + i; }
__host__ __device__ constexpr int ups_rt(int r, int i) { return r == 0 ? i : r == 1 ? 2 : 3 + i; }

// wp[t][n][c], t = rt 5 + ct
__global__ __launch_bounds__(256) void upsample_scale_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int O, int I) {
  const int64_t n_total = (int64_t)UPS_NM * O * I;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_total) return;
  const int c = (int)(idx % I);
  const int n = (int)((idx / I) % O);
  const int t = (int)(idx / ((int64_t)I * O));
  const int rt = t / 5, ct = t % 5;
  const float* src = w + ((int64_t)n * I + c) * 9;
  float v = 0.f;
  for (int kh = ups_k0(rt); kh <= ups_k1(rt); ++kh)
    for (int kw = ups_k0(ct); kw <= ups_k1(ct); ++kw) v += src[kh * 3 + kw];
  wp[idx] = v;
}

// S2: s == 2 (classes first / last only, two 32-column tiles per workgroup); else nine classes, one column tile.
// ab: [B][Cin][2] affine in launch_gn_fold_seg's form (times WF_AB_SCALE), or nullptr = x as it is
template <bool S2>
__global__ __launch_bounds__(256) void upsample_scale_conv3x3_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ ab,
                                                                     const float* __restrict__ wp, const float* __restrict__ bias,
                                                                     float* __restrict__ y, int ldy, int yoff, int B, int H, int W,
                                                                     int Cin, int Cout, int s, int tiles_x, int tiles_y) {
  constexpr int NR = S2 ? 2 : 3;       // row (column) classes held
  constexpr int NRT = S2 ? 4 : 5;      // row (column) taps staged
  constexpr int NCT = S2 ? 2 : 1;      // 32-column tiles
  constexpr int NT = 32 * NCT;
  __shared__ up_f32x4 As[2][UP_PY * UP_PX];      // [channel half][patch pixel]: channels c0 + 4 h .. + 3, activated
  __shared__ up_f32x4 Bs[2][NRT * NRT * NT];     // [channel half][staged tap matrix][column]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, b = tile / (tiles_x * tiles_y);
  const int x0 = tx * UP_TX, y0 = ty * UP_TY, n0 = blockIdx.y * NT;
  const bool second = NCT > 1 && n0 + 32 < Cout;   // the tile's second 32 columns exist (Cout % 32 == 0)

  up_f32x16 acc[NR * NR][NCT];
#pragma unroll
  for (int f = 0; f < NR * NR; ++f)
#pragma unroll
    for (int j = 0; j < NCT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[f][j][r] = 0.f;

  const int m = lane & 31, h = lane >> 5;
  const int a_base = (2 * wave + (m >> 4)) * UP_PX + (m & 15);   // the lane's pixel in the patch, before the tap shift
  const float* xb = x + (int64_t)b * H * W * ldx;
  const float* abb = ab ? ab + (int64_t)b * Cin * 2 : nullptr;

  for (int c0 = 0; c0 < Cin; c0 += UP_KC) {
    for (int i = tid; i < 2 * UP_PY * UP_PX; i += 256) {
      const int hh = i & 1, pix = i >> 1;
      const int iy = y0 - 1 + pix / UP_PX, ix = x0 - 1 + pix % UP_PX;
      up_f32x4 v = {0.f, 0.f, 0.f, 0.f};   // off the map: the conv's zero padding, AFTER the activation
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        v = *(const up_f32x4*)(xb + ((int64_t)iy * W + ix) * ldx + c0 + 4 * hh);
        if (abb) {
          const up_f32x4 ab0 = *(const up_f32x4*)(abb + 2 * (c0 + 4 * hh)), ab1 = *(const up_f32x4*)(abb + 2 * (c0 + 4 * hh) + 4);
          const float av[4] = {ab0[0], ab0[2], ab1[0], ab1[2]}, bv[4] = {ab0[1], ab0[3], ab1[1], ab1[3]};
#pragma unroll
          for (int k = 0; k < 4; ++k) {   // SiLU(z) = z / (1 + 2^u) on u = -log2(e) z
            const float u = av[k] * v[k] + bv[k];
            v[k] = WF_U_SCALE * u / (1.0f + exp2f(u));
          }
        }
      }
      As[hh][pix] = v;
    }
    for (int idx = tid; idx < 2 * NRT * NRT * NT; idx += 256) {
      const int hh = idx & 1, row = idx >> 1;
      const int lt = row / NT, n = n0 + row % NT;
      int rt = lt / NRT, ct = lt % NRT;
      if (S2) {   // staged taps 0, 1, 2, 3 = taps 0, 1, 3, 4
        rt += rt >> 1;
        ct += ct >> 1;
      }
      up_f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < Cout) v = *(const up_f32x4*)(wp + ((int64_t)(rt * 5 + ct) * Cout + n) * Cin + c0 + 4 * hh);
      Bs[hh][row] = v;
    }
    __syncthreads();
    up_f32x4 a[9];
#pragma unroll
    for (int sy = 0; sy < 3; ++sy)
#pragma unroll
      for (int sx = 0; sx < 3; ++sx) a[sy * 3 + sx] = As[h][a_base + sy * UP_PX + sx];
#pragma unroll
    for (int ri = 0; ri < NR; ++ri) {
#pragma unroll
      for (int ci = 0; ci < NR; ++ci) {
        const int r = S2 ? 2 * ri : ri, c = S2 ? 2 * ci : ci;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (i >= ups_ntap(r)) continue;
#pragma unroll
          for (int j2 = 0; j2 < 2; ++j2) {
            if (j2 >= ups_ntap(c)) continue;
            const int rt = ups_rt(r, i), ct = ups_rt(c, j2);
            const int lrt = S2 && rt > 2 ? rt - 1 : rt, lct = S2 && ct > 2 ? ct - 1 : ct;   // (taps 0, 1, 3, 4 -> 0, 1, 2, 3)
            const up_f32x4 av = a[ups_shift(r, i) * 3 + ups_shift(c, j2)];
            const up_f32x4 b0 = Bs[h][(lrt * NRT + lct) * NT + m];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              acc[ri * NR + ci][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[k], b0[k], acc[ri * NR + ci][0], 0, 0, 0);
            if (NCT > 1 && second) {
              const up_f32x4 b1 = Bs[h][(lrt * NRT + lct) * NT + 32 + m];
#pragma unroll
              for (int k = 0; k < 4; ++k)
                acc[ri * NR + ci][NCT - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[k], b1[k], acc[ri * NR + ci][NCT - 1], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();
  }

  // Epilogue: each wave turns a class's 32 x 32 tile through 4 KB of LDS of its own (the weight stage is free after the last
  // barrier), so a lane holds 4 consecutive channels of 4 low-res pixels, and stores each with 16 bytes to every pixel of
  // the class in that pixel's s x s block: eight lanes fill 128 contiguous bytes of an output row.
  float* scratch = (float*)&Bs[0][0] + wave * 1024;
  const int rq = lane >> 3, c4 = (lane & 7) * 4;
  const int Wo = s * W;
  float* yb = y + (int64_t)b * (s * H) * Wo * ldy + yoff;
#pragma unroll
  for (int ri = 0; ri < NR; ++ri) {
#pragma unroll
    for (int ci = 0; ci < NR; ++ci) {
      const int r = S2 ? 2 * ri : ri, c = S2 ? 2 * ci : ci;
      // the class's rows and columns inside the block
      const int dy0 = r == 0 ? 0 : r == 1 ? 1 : s - 1, dy1 = r == 0 ? 1 : r == 1 ? s - 1 : s;
      const int dx0 = c == 0 ? 0 : c == 1 ? 1 : s - 1, dx1 = c == 0 ? 1 : c == 1 ? s - 1 : s;
#pragma unroll
      for (int j = 0; j < NCT; ++j) {
        if (j == 1 && !second) continue;
#pragma unroll
        for (int q = 0; q < 16; ++q) scratch[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + m] = acc[ri * NR + ci][j][q];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int nc = n0 + 32 * j + c4;
        const up_f32x4 bv = bias ? *(const up_f32x4*)(bias + nc) : up_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = rq + 8 * i;
          const int ly = y0 + 2 * wave + (row >> 4), lx = x0 + (row & 15);
          const up_f32x4 v = *(const up_f32x4*)(scratch + row * 32 + c4) + bv;
          if (ly < H && lx < W) {
            for (int dy = dy0; dy < dy1; ++dy) {
              float* yrow = yb + ((int64_t)(s * ly + dy) * Wo + s * lx) * ldy + nc;
              for (int dx = dx0; dx < dx1; ++dx) *(up_f32x4*)(yrow + (int64_t)dx * ldy) = v;
            }
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
  }
}

}  // namespace

const char* upsample_scale_refusal(int ldx, int ldy, int yoff, int B, int H, int W, int Cin, int Cout, int s) {
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return "upsample_nearest_gn_conv3x3: empty shape";
  if (s < 2) return "upsample_nearest_gn_conv3x3: the scale must be an integer >= 2 (scale 1 is a plain conv3x3)";
  if (Cin % UP_KC) return "upsample_nearest_gn_conv3x3: Cin must be a multiple of 8 (the kernel's k-step)";
  if (Cout % 32) return "upsample_nearest_gn_conv3x3: Cout must be a multiple of 32 (one MFMA column tile)";
  if (ldx < Cin || (ldx & 3)) return "upsample_nearest_gn_conv3x3: input row stride must be >= Cin and a multiple of 4";
  if (ldy < yoff + Cout || (ldy & 3) || (yoff & 3) || yoff < 0)
    return "upsample_nearest_gn_conv3x3: output row stride / channel offset must hold Cout channels and be multiples of 4";
  const int64_t tiles = (int64_t)B * ((H + UP_TY - 1) / UP_TY) * ((W + UP_TX - 1) / UP_TX);
  if (tiles > 0x7fffffff) return "upsample_nearest_gn_conv3x3: more than 2^31 tiles";
  if ((int64_t)s * H > 0x7fffffff || (int64_t)s * W > 0x7fffffff || (int64_t)B * s * H * s * W > 0x7fffffff)
    return "upsample_nearest_gn_conv3x3: more than 2^31 output pixels";
  return nullptr;
}

size_t upsample_scale_weight_floats(int Cin, int Cout) { return (size_t)UPS_NM * Cout * Cin; }

int launch_upsample_scale_pack(const float* w_oihw, float* wp, int O, int I, hipStream_t s) {
  const int64_t n = (int64_t)UPS_NM * O * I;
  hipLaunchKernelGGL(upsample_scale_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_oihw, wp, O, I);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_upsample_scale_conv3x3(const float* x, int ldx, const float* ab, const float* wp, const float* bias, float* y, int ldy,
                                  int yoff, int B, int H, int W, int Cin, int Cout, int scale, hipStream_t s) {
  if (const char* why = upsample_scale_refusal(ldx, ldy, yoff, B, H, W, Cin, Cout, scale)) {
    set_error(why);
    return 1;
  }
  KD_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)wp & 15) == 0 && ((uintptr_t)bias & 15) == 0 &&
                 ((uintptr_t)ab & 15) == 0,
             "upsample_nearest_gn_conv3x3: 16-byte aligned pointers");
  const int tiles_x = (W + UP_TX - 1) / UP_TX, tiles_y = (H + UP_TY - 1) / UP_TY;
  const unsigned tiles = (unsigned)(B * tiles_y * tiles_x);
  if (scale == 2) {
    hipLaunchKernelGGL(upsample_scale_conv3x3_kernel<true>, dim3(tiles, (unsigned)((Cout + 63) / 64)), dim3(256), 0, s, x, ldx, ab, wp,
                       bias, y, ldy, yoff, B, H, W, Cin, Cout, scale, tiles_x, tiles_y);
  } else {
    hipLaunchKernelGGL(upsample_scale_conv3x3_kernel<false>, dim3(tiles, (unsigned)(Cout / 32)), dim3(256), 0, s, x, ldx, ab, wp, bias,
                       y, ldy, yoff, B, H, W, Cin, Cout, scale, tiles_x, tiles_y);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
