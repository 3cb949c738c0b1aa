// Fused-tile canvas sampling (MultiDiffusion / Mixture of Diffusers): the canvas of a stage is ONE noisy image
// [C, Hc, Wc]; at every schedule step every tile of an ny x nx lattice (tile size S, stride st, Hc = (ny - 1) st + S) is
// denoised by itself, the thresholded x0 estimates are averaged where tiles overlap and the solver update runs once, on the
// canvas.  Two kernels, both bound by memory: the gather canvas -> tiles, and the whole canvas step in one pass.
//
// S, st and hence every tile origin and Wc are multiples of 4: a float4 of a canvas row never straddles a tile edge, so
// every access below is one 16-byte load or store.
#include "common.h"

#pragma clang fp contract(off)  // mul and add stay apart: the expression and op order of solver_update_kernel
#include "philox.h"

namespace kd {

// ------------------------------------------------------------------------- canvas -> tiles
// Tile b of the launch = canvas[:, y0[b] : y0[b] + S, x0[b] : x0[b] + S].  The origins travel as a kernel argument (as the
// per-image seeds do), TILE_CHUNK tiles per launch: the caller's array is free on return.
enum { TILE_CHUNK = 32 };
struct TileOrigins {
  int y0[TILE_CHUNK];
  int x0[TILE_CHUNK];
};
__global__ __launch_bounds__(256) void tiles_gather_kernel(const float* __restrict__ canvas, float* __restrict__ tiles, int C,
                                                           int Hc, int Wc, int S, TileOrigins org) {
  const int b = blockIdx.y;
  const int S4 = S / 4;
  const int per4 = C * S * S4;   // (< 2^31: checked by the host)
  const int y0 = org.y0[b], x0 = org.x0[b];
  float* dst = tiles + (int64_t)b * per4 * 4;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < per4; j += gridDim.x * 256) {
    const int row = j / S4, xq = j - row * S4;   // row = c * S + y
    const int c = row / S, y = row - c * S;
    *(f32x4*)(dst + (int64_t)j * 4) = *(const f32x4*)(canvas + ((int64_t)c * Hc + y0 + y) * Wc + x0 + 4 * xq);
  }
}
int launch_tiles_gather(const float* canvas, float* tiles, int B, int C, int Hc, int Wc, int S, const int* origins_yx,
                        hipStream_t s) {
  KD_REQUIRE(canvas && tiles && origins_yx, "tiles gather: null argument");
  KD_REQUIRE(B >= 1 && C >= 1 && C <= 1024 && S >= 4 && S % 4 == 0, "tiles gather: needs B, C >= 1 and a tile size S % 4 == 0");
  KD_REQUIRE(Hc >= S && Wc >= S && Wc % 4 == 0 && Hc <= (1 << 20) && Wc <= (1 << 20), "tiles gather: canvas smaller than a tile, or Wc % 4 != 0");
  KD_REQUIRE((int64_t)C * S * S < (1ll << 31), "tiles gather: a tile must hold fewer than 2^31 elements");
  KD_REQUIRE((((uintptr_t)canvas | (uintptr_t)tiles) & 15) == 0, "tiles gather: canvas and tiles must be 16-byte aligned");
  for (int b = 0; b < B; ++b) {
    const int y0 = origins_yx[2 * b], x0 = origins_yx[2 * b + 1];
    KD_REQUIRE(y0 >= 0 && y0 + S <= Hc && x0 >= 0 && x0 + S <= Wc && x0 % 4 == 0,
               "tiles gather: a tile origin lies outside the canvas or its x0 is no multiple of 4");
  }
  const int per4 = C * S * (S / 4);
  for (int b0 = 0; b0 < B; b0 += TILE_CHUNK) {
    const int nb = std::min(B - b0, (int)TILE_CHUNK);
    TileOrigins org{};
    for (int b = 0; b < nb; ++b) {
      org.y0[b] = origins_yx[2 * (b0 + b)];
      org.x0[b] = origins_yx[2 * (b0 + b) + 1];
    }
    const int gx = std::max(1, std::min((per4 + 255) / 256, 8192 / nb));
    hipLaunchKernelGGL(tiles_gather_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, s, canvas,
                       tiles + (int64_t)b0 * per4 * 4, C, Hc, Wc, S, org);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- the canvas step
// Per canvas pixel, over the present tiles t that cover it, in ascending (row, column) order of their slots:
//   x0c_t = clamp(x0_t, -s_t, s_t) / s_t, s_t = max(thr_t, 1)          (thr == nullptr: s_t = 1)
//   x0bar = (sum w_t x0c_t) / (sum w_t)
//   x <- A x + B x0bar [+ P hist] [+ Sn z] ; hist <- x0bar               (hist: what x0bar held on entry)
// A term whose coefficient is 0 is left out, operand unread.  A pixel that no present tile covers is left alone in both
// buffers.  z: read from `noise`, or element (c Hc + y) Wc + x of Philox stream `sid` under `seed` - the bits
// kd_philox_normal writes over C Hc Wc elements, whatever the tiling.
// Pixel-centric, no atomics: a thread owns four consecutive x of one (c, y); a block row is one canvas row, so the row's
// slots and weights are uniform over the block.  At most TILE_COVER slots per axis (S <= TILE_COVER st).
enum { TILE_COVER = 3 };
struct TileGeom {
  int C, S, st, ny, nx, Hc, Wc;
  int ramp, ov;   // ramp != 0: w(y, x) = r(y) r(x), r(i) = min(i + 1, S - i, ov) / ov; else w = 1
  int N;          // tiles in x0_tiles
};
__device__ __forceinline__ float ramp_weight(int i, int S, int ov) { return (float)min(min(i + 1, S - i), ov) / (float)ov; }

__global__ __launch_bounds__(256) void tiles_fuse_update_kernel(float* __restrict__ x, float* __restrict__ x0bar,
                                                                const float* __restrict__ x0_tiles,
                                                                const float* __restrict__ thr, const int* __restrict__ tile_of,
                                                                TileGeom g, float A, float B, float P, float Sn,
                                                                const float* __restrict__ noise, uint64_t seed, uint64_t sid) {
  const int W4 = g.Wc / 4;
  const int xq = blockIdx.x * 256 + threadIdx.x;
  if (xq >= W4) return;
  const int xx = 4 * xq;
  // covering slot columns: q st <= xx < q st + S
  const int q_hi = min(xx / g.st, g.nx - 1), q_lo = xx < g.S ? 0 : (xx - g.S) / g.st + 1;
  const int rows = g.C * g.Hc;
  const int64_t tile_plane = (int64_t)g.S * g.S;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int c = row / g.Hc, y = row - c * g.Hc;
    const int r_hi = min(y / g.st, g.ny - 1), r_lo = y < g.S ? 0 : (y - g.S) / g.st + 1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, wsum = {0.f, 0.f, 0.f, 0.f};
    bool covered = false;
    for (int r = r_lo; r <= r_hi; ++r) {
      const int ly = y - r * g.st;
      const float wy = g.ramp ? ramp_weight(ly, g.S, g.ov) : 1.0f;
      for (int q = q_lo; q <= q_hi; ++q) {
        const int t = tile_of[r * g.nx + q];
        if (t < 0 || t >= g.N) continue;
        covered = true;
        const int lx = xx - q * g.st;
        const float s = thr ? fmaxf(thr[t], 1.0f) : 1.0f;
        const f32x4 v = *(const f32x4*)(x0_tiles + ((int64_t)t * g.C + c) * tile_plane + (int64_t)ly * g.S + lx);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xs = fminf(fmaxf(v[e], -s), s) / s;
          const float w = g.ramp ? wy * ramp_weight(lx + e, g.S, g.ov) : 1.0f;
          acc[e] = acc[e] + w * xs;
          wsum[e] = wsum[e] + w;
        }
      }
    }
    if (!covered) continue;
    const int64_t j4 = (int64_t)row * W4 + xq;
    f32x4 xv = *(const f32x4*)(x + j4 * 4), xb, o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      xb[e] = acc[e] / wsum[e];
      o[e] = A * xv[e] + B * xb[e];
    }
    if (P != 0.0f) {
      const f32x4 hv = *(const f32x4*)(x0bar + j4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + P * hv[e];
    }
    if (Sn != 0.0f) {
      const f32x4 z = noise ? *(const f32x4*)(noise + j4 * 4) : philox_normal4(seed, sid, (uint64_t)j4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + Sn * z[e];
    }
    *(f32x4*)(x + j4 * 4) = o;
    *(f32x4*)(x0bar + j4 * 4) = xb;
  }
}
int launch_tiles_fuse_update(float* x, float* x0bar, const float* x0_tiles, const float* thr, const int* tile_of, int N, int C,
                             int S, int st, int ny, int nx, int ramp, float A, float B, float P, float Sn, const float* noise,
                             uint64_t seed, uint64_t sid, hipStream_t s) {
  KD_REQUIRE(x && x0bar && x0_tiles && tile_of, "tiles fuse: null argument");
  KD_REQUIRE(N >= 1 && C >= 1 && C <= 1024 && ny >= 1 && nx >= 1 && N <= (int64_t)ny * nx, "tiles fuse: needs 1 <= N <= ny nx tiles and C >= 1");
  KD_REQUIRE(S >= 4 && S % 4 == 0 && st >= 4 && st % 4 == 0 && st <= S, "tiles fuse: needs S % 4 == 0, st % 4 == 0 and 4 <= st <= S");
  KD_REQUIRE(S <= TILE_COVER * st, "tiles fuse: more than 3 tiles per axis cover a pixel (S > 3 st)");
  const int64_t Hc = (int64_t)(ny - 1) * st + S, Wc = (int64_t)(nx - 1) * st + S;
  KD_REQUIRE(Hc <= (1 << 20) && Wc <= (1 << 20) && (int64_t)C * Hc < (1ll << 31) && (int64_t)ny * nx < (1ll << 31),
             "tiles fuse: canvas out of range");
  KD_REQUIRE((((uintptr_t)x | (uintptr_t)x0bar | (uintptr_t)x0_tiles | (uintptr_t)noise) & 15) == 0,
             "tiles fuse: x, x0bar, x0_tiles and noise must be 16-byte aligned");
  TileGeom g{C, S, st, ny, nx, (int)Hc, (int)Wc, ramp != 0, std::max(S - st, 1), N};
  const int W4 = (int)Wc / 4;
  const int64_t rows = (int64_t)C * Hc;
  hipLaunchKernelGGL(tiles_fuse_update_kernel, dim3((unsigned)((W4 + 255) / 256), (unsigned)std::min<int64_t>(rows, 65535)),
                     dim3(256), 0, s, x, x0bar, x0_tiles, thr, tile_of, g, A, B, P, Sn, noise, seed, sid);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
