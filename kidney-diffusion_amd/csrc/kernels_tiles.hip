// Fused-tile canvas sampling (MultiDiffusion / Mixture of Diffusers): the canvas of a stage is ONE noisy image
// [C, Hc, Wc]; at every schedule step every tile of an ny x nx lattice (tile size S, stride st, Hc = (ny - 1) st + S) is
// denoised by itself, the thresholded x0 estimates are averaged where tiles overlap and the solver update runs once, on the
// canvas.  Two kernels, both bound by memory: the gather canvas -> tiles, and the whole canvas step in one pass.  Three
// more make a stage stream at the sizes of a magnification level (canvas 40960^2): the conditioning tiles of a chunk cut
// straight out of the level above, the low-res conditioning tiles cut straight out of the previous stage's canvas, and
// the end of a stage written in place into a larger canvas - none of them leaves a canvas-sized temporary.
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
// Host side of the gathers.  `who` is the launcher's prefix in the requirement messages.
// The tile set of kd_tiles_gather / kd_tiles_gather_lowres: B tiles [C, S, S] at origins_yx [B][2] inside a canvas [C, Hc, Wc].
static int check_tile_origins(const std::string& who, const int* origins_yx, int B, int C, int Hc, int Wc, int S) {
  KD_REQUIRE(B >= 1 && C >= 1 && C <= 1024 && S >= 4 && S % 4 == 0, who + ": needs B, C >= 1 and a tile size S % 4 == 0");
  KD_REQUIRE(Hc >= S && Wc >= S && Wc % 4 == 0 && Hc <= (1 << 20) && Wc <= (1 << 20), who + ": canvas smaller than a tile, or Wc % 4 != 0");
  KD_REQUIRE((int64_t)C * S * S < (1ll << 31), who + ": a tile must hold fewer than 2^31 elements");
  for (int b = 0; b < B; ++b) {
    const int y0 = origins_yx[2 * b], x0 = origins_yx[2 * b + 1];
    KD_REQUIRE(y0 >= 0 && y0 + S <= Hc && x0 >= 0 && x0 + S <= Wc && x0 % 4 == 0,
               who + ": a tile origin lies outside the canvas or its x0 is no multiple of 4");
  }
  return 0;
}
// launch(b0, nb, org) for every pack of at most TILE_CHUNK of the B pairs yx [B][2]; org holds the pack's pairs.
template <class Launch>
static void for_tile_chunks(const int* yx, int B, Launch launch) {
  for (int b0 = 0; b0 < B; b0 += TILE_CHUNK) {
    const int nb = std::min(B - b0, (int)TILE_CHUNK);
    TileOrigins org{};
    for (int b = 0; b < nb; ++b) {
      org.y0[b] = yx[2 * (b0 + b)];
      org.x0[b] = yx[2 * (b0 + b) + 1];
    }
    launch(b0, nb, org);
  }
}
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
  if (check_tile_origins("tiles gather", origins_yx, B, C, Hc, Wc, S)) return 1;
  KD_REQUIRE((((uintptr_t)canvas | (uintptr_t)tiles) & 15) == 0, "tiles gather: canvas and tiles must be 16-byte aligned");
  const int per4 = C * S * (S / 4);
  for_tile_chunks(origins_yx, B, [&](int b0, int nb, const TileOrigins& org) {
    const int gx = std::max(1, std::min((per4 + 255) / 256, 8192 / nb));
    hipLaunchKernelGGL(tiles_gather_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, s, canvas,
                       tiles + (int64_t)b0 * per4 * 4, C, Hc, Wc, S, org);
  });
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- the canvas step: lattice, fusion, update
// Per canvas pixel, over the present tiles t that cover it, in ascending (row, column) order of their slots:
//   x0c_t = clamp(x0_t, -s_t, s_t) / s_t, s_t = max(thr_t, 1)          (thr == nullptr: s_t = 1)
//   x0bar = (sum w_t x0c_t) / (sum w_t)
//   x <- A x + B x0bar [+ P hist] [+ P2 hist2] [+ Sn z] ; x0bar_out <- x0bar
// A term whose coefficient is 0 is left out, operand unread.  A pixel that no present tile covers is left alone in both
// buffers.  z: read from `noise`, or element (c Hc + y) Wc + x of Philox stream `sid` under `seed` - the bits
// kd_philox_normal writes over C Hc Wc elements, whatever the tiling.
// Pixel-centric, no atomics: a thread owns four consecutive x of one (c, y); a block row is one canvas row, so the row's
// slots and weights are uniform over the block.  At most TILE_COVER slots per axis (S <= TILE_COVER st).  The kernel
// itself (tiles_fuse_update_kernel) stands below, behind the sources it mixes in.
enum { TILE_COVER = 3 };
// The launch grid of the canvas-shaped kernels (start, step, finish): a thread per float4 of a canvas row [Wc], block row
// blockIdx.y walks the C Hc rows in strides of gridDim.y.
static dim3 canvas_grid(int C, int Hc, int Wc) {
  return dim3((unsigned)((Wc / 4 + 255) / 256), (unsigned)std::min<int64_t>((int64_t)C * Hc, 65535));
}
struct TileGeom {
  int C, S, st, ny, nx, Hc, Wc;
  int ramp, ov;   // ramp != 0: w(y, x) = r(y) r(x), r(i) = min(i + 1, S - i, ov) / ov; else w = 1
  int N;          // tiles in x0_tiles
};
__device__ __forceinline__ float ramp_weight(int i, int S, int ov) { return (float)min(min(i + 1, S - i), ov) / (float)ov; }
// Host side of the canvas step and of the end of a stage: the lattice checked and as the kernels take it.
static int tile_lattice(const std::string& who, int N, int C, int S, int st, int ny, int nx, int ramp, TileGeom* g) {
  KD_REQUIRE(N >= 1 && C >= 1 && C <= 1024 && ny >= 1 && nx >= 1 && N <= (int64_t)ny * nx, who + ": needs 1 <= N <= ny nx tiles and C >= 1");
  KD_REQUIRE(S >= 4 && S % 4 == 0 && st >= 4 && st % 4 == 0 && st <= S, who + ": needs S % 4 == 0, st % 4 == 0 and 4 <= st <= S");
  KD_REQUIRE(S <= TILE_COVER * st, who + ": more than 3 tiles per axis cover a pixel (S > 3 st)");
  const int64_t Hc = (int64_t)(ny - 1) * st + S, Wc = (int64_t)(nx - 1) * st + S;
  KD_REQUIRE(Hc <= (1 << 20) && Wc <= (1 << 20) && (int64_t)C * Hc < (1ll << 31) && (int64_t)ny * nx < (1ll << 31),
             who + ": canvas out of range");
  *g = TileGeom{C, S, st, ny, nx, (int)Hc, (int)Wc, ramp != 0, std::max(S - st, 1), N};
  return 0;
}

// The covering slots of the float4 at (y, xx): rows r_lo .. r_hi, columns q_lo .. q_hi of the lattice.
struct TileCover {
  int r_lo, r_hi, q_lo, q_hi;
};
__device__ __forceinline__ TileCover tile_cover(const TileGeom& g, int y, int xx) {
  return TileCover{y < g.S ? 0 : (y - g.S) / g.st + 1, min(y / g.st, g.ny - 1), xx < g.S ? 0 : (xx - g.S) / g.st + 1,
                   min(xx / g.st, g.nx - 1)};
}
// whether a present tile covers the float4 at (y, xx)
__device__ __forceinline__ bool tile_covered(const int* __restrict__ tile_of, const TileGeom& g, int y, int xx) {
  const TileCover cv = tile_cover(g, y, xx);
  bool covered = false;
  for (int r = cv.r_lo; r <= cv.r_hi; ++r)
    for (int q = cv.q_lo; q <= cv.q_hi; ++q) {
      const int t = tile_of[r * g.nx + q];
      covered = covered || (t >= 0 && t < g.N);
    }
  return covered;
}
// x0bar of the float4 at (c, y, xx) into xb; false when no present tile covers it (xb is then not written).
__device__ __forceinline__ bool fuse_tiles(const float* __restrict__ x0_tiles, const float* __restrict__ thr,
                                           const int* __restrict__ tile_of, const TileGeom& g, int c, int y, int xx, f32x4& xb) {
  const TileCover cv = tile_cover(g, y, xx);
  const int64_t tile_plane = (int64_t)g.S * g.S;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, wsum = {0.f, 0.f, 0.f, 0.f};
  bool covered = false;
  for (int r = cv.r_lo; r <= cv.r_hi; ++r) {
    const int ly = y - r * g.st;
    const float wy = g.ramp ? ramp_weight(ly, g.S, g.ov) : 1.0f;
    for (int q = cv.q_lo; q <= cv.q_hi; ++q) {
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
  if (!covered) return false;
#pragma unroll
  for (int e = 0; e < 4; ++e) xb[e] = acc[e] / wsum[e];
  return true;
}
// The update of the float4 j4: A x + B x0bar [+ P hist] [+ P2 hist2] [+ Sn z], left to right.
__device__ __forceinline__ f32x4 canvas_update(const f32x4& xv, const f32x4& xb, const float* hist, const float* hist2, int64_t j4,
                                               float A, float B, float P, float P2, float Sn, const float* __restrict__ noise,
                                               uint64_t seed, uint64_t sid) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = A * xv[e] + B * xb[e];
  if (P != 0.0f) {
    const f32x4 hv = *(const f32x4*)(hist + j4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = o[e] + P * hv[e];
  }
  if (P2 != 0.0f) {
    const f32x4 hv = *(const f32x4*)(hist2 + j4 * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = o[e] + P2 * hv[e];
  }
  if (Sn != 0.0f) {
    const f32x4 z = noise ? *(const f32x4*)(noise + j4 * 4) : philox_normal4(seed, sid, (uint64_t)j4);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = o[e] + Sn * z[e];
  }
  return o;
}

// ------------------------------------------------------------------------- conditioning tiles from the level above
// The conditioning image of a tile is a window of the level above, `src` [Cs, W, W]: the image rolled by the tile's shift
// (sy, sx), filled where the roll wraps, cropped to the window at `top` and resized to S (ultra_res.grid
// .cond_images_for_grid, then resize_image_to).  Per axis, output coordinate p of a tile with shift sh:
//   w = map[p] (window coordinate), g = top + w;  filled = sh > 0 ? g < sh : g >= (W + sh) % W   (sh == 0: everything)
//   source index (g - sh) mod W
// Channels c < Cs read through `win_of`; channels Cs + c (the v2 centre crop, `centre_of` != nullptr) through `centre_of`.
// Data movement only.  The source x wraps and is unaligned: scalar loads, one 16-byte store.  A block row is one output
// row: filled_y is uniform over the block and a filled row stores `fill` without loading.  The maps live in device
// memory, where the host cannot check them: a map entry is clamped into [0, W - top - 1], so no entry reads outside src.
__global__ __launch_bounds__(256) void tiles_cond_gather_kernel(const float* __restrict__ src, int Cs, int W,
                                                                float* __restrict__ tiles, int S, int Ct, TileOrigins sh, int top,
                                                                const int* __restrict__ win_of,
                                                                const int* __restrict__ centre_of, float fill) {
  const int S4 = S / 4;
  const int xq = blockIdx.x * 256 + threadIdx.x;
  if (xq >= S4) return;
  const int b = blockIdx.z;
  const int sy = sh.y0[b], sx = sh.x0[b];
  const int wmax = W - top - 1;
  const int edge_x = sx > 0 ? sx : (W + sx) % W, edge_y = sy > 0 ? sy : (W + sy) % W;
  // the four source columns of this thread under either map
  int rx[2][4];
  bool fx[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int* map = m ? centre_of : win_of;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = top + (map ? min(max(map[4 * xq + e], 0), wmax) : 0);
      fx[m][e] = sx > 0 ? g < edge_x : g >= edge_x;
      int r = g - sx;
      r = r < 0 ? r + W : (r >= W ? r - W : r);
      rx[m][e] = r;
    }
  }
  const int rows = Ct * S;
  float* dst = tiles + (int64_t)b * rows * S;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int c = row / S, y = row - c * S;
    const int m = c >= Cs ? 1 : 0;
    const int g = top + min(max((m ? centre_of : win_of)[y], 0), wmax);
    const bool fy = sy > 0 ? g < edge_y : g >= edge_y;
    f32x4 o = {fill, fill, fill, fill};
    if (!fy) {
      int ry = g - sy;
      ry = ry < 0 ? ry + W : (ry >= W ? ry - W : ry);
      const float* line = src + ((int64_t)(c - m * Cs) * W + ry) * W;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (!fx[m][e]) o[e] = line[rx[m][e]];
    }
    *(f32x4*)(dst + (int64_t)row * S + 4 * xq) = o;
  }
}
int launch_tiles_cond_gather(const float* src, int Cs, int W, float* tiles, int B, int S, const int* shifts_yx, int top,
                             const int* win_of, const int* centre_of, float fill, hipStream_t s) {
  KD_REQUIRE(src && tiles && shifts_yx && win_of, "tiles cond gather: null argument");
  KD_REQUIRE(B >= 1 && Cs >= 1 && Cs <= 512 && S >= 4 && S % 4 == 0 && S <= (1 << 20),
             "tiles cond gather: needs B, Cs >= 1 and a tile size S % 4 == 0");
  KD_REQUIRE(W >= 1 && W <= (1 << 20) && top >= 0 && top < W, "tiles cond gather: source width or window offset out of range");
  const int Ct = centre_of ? 2 * Cs : Cs;
  KD_REQUIRE((int64_t)Ct * S * S < (1ll << 31), "tiles cond gather: a tile must hold fewer than 2^31 elements");
  KD_REQUIRE(((uintptr_t)tiles & 15) == 0, "tiles cond gather: tiles must be 16-byte aligned");
  for (int b = 0; b < B; ++b) {
    const int sy = shifts_yx[2 * b], sx = shifts_yx[2 * b + 1];
    KD_REQUIRE(sy > -W && sy < W && sx > -W && sx < W, "tiles cond gather: a shift must lie inside (-W, W)");
  }
  const int S4 = S / 4, rows = Ct * S;
  for_tile_chunks(shifts_yx, B, [&](int b0, int nb, const TileOrigins& sh) {
    hipLaunchKernelGGL(tiles_cond_gather_kernel, dim3((unsigned)((S4 + 255) / 256), (unsigned)std::min(rows, 8192), (unsigned)nb),
                       dim3(256), 0, s, src, Cs, W, tiles + (int64_t)b0 * rows * S, S, Ct, sh, top, win_of, centre_of, fill);
  });
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- low-res conditioning tiles from the previous canvas
// tiles[b, c, y, x] = a (2 prev[c, iy, ix] - 1) + s z[(c Hc + y0 + y) Wc + x0 + x]: the previous stage's canvas resized
// (nearest, the rule of sample_start_kernel: min((int)floorf(dst * ((float)in / (float)out)), in - 1), the ratios divided
// in fp32 by the host) to this stage's canvas [C, Hc, Wc], normalised and augmented - cut per tile without the canvas
// ever existing.  z is a property of the canvas element (read from `noise`, or the element of Philox stream `sid` under
// `seed`: x0 and Wc are multiples of 4, so a thread's four x are one float4 of the stream), so overlapping tiles see one
// conditioning on shared pixels.  Op order: 2 v, - 1, a *, s z, the sum; s == 0 leaves the term out, operand unread.
__global__ __launch_bounds__(256) void tiles_gather_lowres_kernel(const float* __restrict__ prev, int Hp, int Wp, float ry,
                                                                  float rx, float* __restrict__ tiles, int C, int Hc, int Wc,
                                                                  int S, TileOrigins org, float a, float s,
                                                                  const float* __restrict__ noise, uint64_t seed, uint64_t sid) {
  const int b = blockIdx.y;
  const int S4 = S / 4;
  const int per4 = C * S * S4;   // (< 2^31: checked by the host)
  const int y0 = org.y0[b], x0 = org.x0[b];
  float* dst = tiles + (int64_t)b * per4 * 4;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < per4; j += gridDim.x * 256) {
    const int row = j / S4, xq = j - row * S4;   // row = c * S + y
    const int c = row / S, y = row - c * S;
    const int iy = min((int)floorf((float)(y0 + y) * ry), Hp - 1);
    const float* line = prev + ((int64_t)c * Hp + iy) * Wp;
    const int64_t at = ((int64_t)c * Hc + y0 + y) * Wc + x0 + 4 * xq;   // canvas element of the float4's first x
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ix = min((int)floorf((float)(x0 + 4 * xq + e) * rx), Wp - 1);
      float t = 2.0f * line[ix];
      t = t - 1.0f;
      o[e] = a * t;
    }
    if (s != 0.0f) {
      const f32x4 z = noise ? *(const f32x4*)(noise + at) : philox_normal4(seed, sid, (uint64_t)(at / 4));
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = o[e] + s * z[e];
    }
    *(f32x4*)(dst + (int64_t)j * 4) = o;
  }
}
int launch_tiles_gather_lowres(const float* prev, int Hp, int Wp, float* tiles, int B, int C, int Hc, int Wc, int S,
                               const int* origins_yx, float a, float s, const float* noise, uint64_t seed, uint64_t sid,
                               hipStream_t st) {
  KD_REQUIRE(prev && tiles && origins_yx, "tiles gather lowres: null argument");
  if (check_tile_origins("tiles gather lowres", origins_yx, B, C, Hc, Wc, S)) return 1;
  KD_REQUIRE(Hp >= 1 && Wp >= 1 && Hp <= (1 << 20) && Wp <= (1 << 20), "tiles gather lowres: previous canvas out of range");
  KD_REQUIRE((((uintptr_t)tiles | (uintptr_t)noise) & 15) == 0, "tiles gather lowres: tiles and noise must be 16-byte aligned");
  const float ry = (float)Hp / (float)Hc, rx = (float)Wp / (float)Wc;
  const int per4 = C * S * (S / 4);
  for_tile_chunks(origins_yx, B, [&](int b0, int nb, const TileOrigins& org) {
    const int gx = std::max(1, std::min((per4 + 255) / 256, 8192 / nb));
    hipLaunchKernelGGL(tiles_gather_lowres_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, st, prev, Hp, Wp, ry, rx,
                       tiles + (int64_t)b0 * per4 * 4, C, Hc, Wc, S, org, a, s, noise, seed, sid);
  });
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- known pixels and an image start
// A canvas that keeps known pixels (RePaint at the level of the canvas) or starts from an image.  The known image, the init
// image and the mask are read at the canvas' size through the nearest rule of tiles_gather_lowres_kernel; a source is a
// base with strides, so a window of a level is read in place.  `vec`: source and canvas sizes agree and base and strides
// are aligned - the thread's four x are one 16-byte (image) or 4-byte (mask) load; otherwise scalar gathers.
struct ImgSrc {
  const float* d;
  int H, W;
  int64_t row, plane;
  float ry, rx;
  int vec;
};
struct MaskSrc {
  const unsigned char* d;
  int H, W;
  int64_t row;
  float ry, rx;
  int vec;
};
__device__ __forceinline__ f32x4 src_image4(const ImgSrc& s, int c, int y, int xx) {
  if (s.vec) return *(const f32x4*)(s.d + (int64_t)c * s.plane + (int64_t)y * s.row + xx);
  const int sy = min((int)floorf((float)y * s.ry), s.H - 1);
  const float* line = s.d + (int64_t)c * s.plane + (int64_t)sy * s.row;
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = line[min((int)floorf((float)(xx + e) * s.rx), s.W - 1)];
  return v;
}
// byte e of the word: the mask of x = xx + e
__device__ __forceinline__ uint32_t src_mask4(const MaskSrc& m, int y, int xx) {
  if (m.vec) return *(const uint32_t*)(m.d + (int64_t)y * m.row + xx);
  const int sy = min((int)floorf((float)y * m.ry), m.H - 1);
  const unsigned char* line = m.d + (int64_t)sy * m.row;
  uint32_t w = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) w |= (uint32_t)line[min((int)floorf((float)(xx + e) * m.rx), m.W - 1)] << (8 * e);
  return w;
}
__device__ __forceinline__ bool mask_at(uint32_t w, int e) { return ((w >> (8 * e)) & 0xffu) != 0; }
__device__ __forceinline__ bool mask_all(uint32_t w) { return mask_at(w, 0) && mask_at(w, 1) && mask_at(w, 2) && mask_at(w, 3); }
// The mix of one slot: x = m ? a (2 kn - 1) + s z : x; op order 2 v, - 1, a *, s z, the sum; s == 0 leaves z unread.
struct MixArgs {
  int on;
  ImgSrc kn;
  MaskSrc mk;
  float a, s;
  const float* noise;
  uint64_t sid;
};
// the known elements (mask word mw != 0) of the float4 j4 at (c, y, xx) replaced in o
__device__ __forceinline__ void mix_known(const MixArgs& m, uint32_t mw, int c, int y, int xx, int64_t j4, uint64_t seed, f32x4& o) {
  const f32x4 kv = src_image4(m.kn, c, y, xx);
  f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if (m.s != 0.0f) z = m.noise ? *(const f32x4*)(m.noise + j4 * 4) : philox_normal4(seed, m.sid, (uint64_t)j4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float t = 2.0f * kv[e];
    t = t - 1.0f;
    float v = m.a * t;
    if (m.s != 0.0f) v = v + m.s * z[e];
    if (mask_at(mw, e)) o[e] = v;
  }
}
// Host side: a source as the kernels take it.  Hc, Wc: the canvas it is seen at; `align`: bytes of the vector load.
template <class Src, class Dev>
static int tile_source(const std::string& who, const Src* in, int Hc, int Wc, int64_t plane, int align, Dev* out) {
  KD_REQUIRE(in->d != nullptr && in->H >= 1 && in->W >= 1 && in->H <= (1 << 20) && in->W <= (1 << 20),
             who + ": null base or size out of range");
  KD_REQUIRE(in->row >= in->W && plane >= 0, who + ": a row stride below the width, or a negative plane stride");
  out->d = in->d;
  out->H = in->H;
  out->W = in->W;
  out->row = in->row;
  out->ry = (float)in->H / (float)Hc;
  out->rx = (float)in->W / (float)Wc;
  out->vec = in->H == Hc && in->W == Wc && in->row % 4 == 0 && plane % 4 == 0 && ((uintptr_t)in->d & (align - 1)) == 0;
  return 0;
}
static int tile_image(const std::string& who, const TileImage* in, int Hc, int Wc, ImgSrc* out) {
  if (tile_source(who, in, Hc, Wc, in->plane, 16, out)) return 1;
  out->plane = in->plane;
  return 0;
}
static int tile_mix(const std::string& who, const TileMix& mix, int Hc, int Wc, MixArgs* m) {
  *m = MixArgs{};
  KD_REQUIRE((mix.known != nullptr) == (mix.mask != nullptr), who + ": the known image and the mask come together");
  if (!mix.known) return 0;
  KD_REQUIRE(((uintptr_t)mix.noise & 15) == 0, who + ": the mix noise must be 16-byte aligned");
  if (tile_image(who + " known image", mix.known, Hc, Wc, &m->kn)) return 1;
  if (tile_source(who + " mask", mix.mask, Hc, Wc, 0, 4, &m->mk)) return 1;
  m->on = 1;
  m->a = mix.a;
  m->s = mix.s;
  m->noise = mix.noise;
  m->sid = mix.sid;
  return 0;
}

// x of a stage in one launch: x = scale z [+ (2 init - 1)], then [the mix of the first slot].  z: `noise`, or element
// (c Hc + y) Wc + x of stream `sid` - with no image and no mask and scale 1 the bits of kd_philox_normal.  A float4 whose
// mask bytes are all set draws no z.
__global__ __launch_bounds__(256) void tiles_start_kernel(float* __restrict__ x, int C, int Hc, int Wc, float scale,
                                                          const float* __restrict__ noise, uint64_t seed, uint64_t sid,
                                                          int has_init, ImgSrc init, MixArgs mix) {
  const int W4 = Wc / 4;
  const int xq = blockIdx.x * 256 + threadIdx.x;
  if (xq >= W4) return;
  const int xx = 4 * xq;
  const int rows = C * Hc;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int c = row / Hc, y = row - c * Hc;
    const int64_t j4 = (int64_t)row * W4 + xq;
    const uint32_t mw = mix.on ? src_mask4(mix.mk, y, xx) : 0u;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (!mask_all(mw)) {
      const f32x4 z = noise ? *(const f32x4*)(noise + j4 * 4) : philox_normal4(seed, sid, (uint64_t)j4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = z[e] * scale;
      if (has_init) {
        const f32x4 iv = src_image4(init, c, y, xx);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = 2.0f * iv[e];
          t = t - 1.0f;
          o[e] = o[e] + t;
        }
      }
    }
    if (mw != 0u) mix_known(mix, mw, c, y, xx, j4, seed, o);
    *(f32x4*)(x + j4 * 4) = o;
  }
}
int launch_tiles_start(float* x, int C, int Hc, int Wc, float scale, const float* noise, uint64_t seed, const TileImage* init,
                       const TileMix& mix, hipStream_t s) {
  KD_REQUIRE(x != nullptr, "tiles start: null output");
  KD_REQUIRE(C >= 1 && C <= 1024 && Hc >= 1 && Wc >= 4 && Wc % 4 == 0 && Hc <= (1 << 20) && Wc <= (1 << 20) &&
                 (int64_t)C * Hc < (1ll << 31),
             "tiles start: canvas out of range, or Wc % 4 != 0");
  KD_REQUIRE((((uintptr_t)x | (uintptr_t)noise) & 15) == 0, "tiles start: x and noise must be 16-byte aligned");
  ImgSrc in{};
  if (init && tile_image("tiles start init image", init, Hc, Wc, &in)) return 1;
  MixArgs m;
  if (tile_mix("tiles start", mix, Hc, Wc, &m)) return 1;
  const uint64_t sid = (16ull << 32) | 2;   // the caller's x_T stream, as launch_sample_start (include/kd_engine.h)
  hipLaunchKernelGGL(tiles_start_kernel, canvas_grid(C, Hc, Wc), dim3(256), 0, s, x, C, Hc, Wc, scale, noise, seed, sid,
                     init ? 1 : 0, in, m);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- the canvas step: the kernel
// The canvas step and, with KNOWN, on the same pixel in the same pass [the re-noise x = x rn_a + z rn_b] then [the mix of
// the NEXT slot]: bit for bit the three passes one after the other.  Without KNOWN the re-noise, the mask load and the mix
// are compiled out.  hist (read when P != 0) or hist2 (read when P2 != 0; without HIST2 the term is compiled out) and
// x0bar_out may be one buffer - a thread reads and writes its own element - so none of them is restrict.  A float4 whose mask bytes are all set is known after the mix whatever the update gives: x is
// not read, nothing is drawn for the update; x0bar is written all the same.
template <bool KNOWN, bool HIST2>
__global__ __launch_bounds__(256) void tiles_fuse_update_kernel(float* __restrict__ x, const float* hist, const float* hist2,
                                                                float* x0bar_out,
                                                                const float* __restrict__ x0_tiles,
                                                                const float* __restrict__ thr, const int* __restrict__ tile_of,
                                                                TileGeom g, float A, float B, float P, float P2, float Sn,
                                                                const float* __restrict__ noise, uint64_t seed, uint64_t sid,
                                                                int renoise, float rn_a, float rn_b,
                                                                const float* __restrict__ rn_noise, uint64_t rn_sid, MixArgs mix) {
  const int W4 = g.Wc / 4;
  const int xq = blockIdx.x * 256 + threadIdx.x;
  if (xq >= W4) return;
  const int xx = 4 * xq;
  const int rows = g.C * g.Hc;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int c = row / g.Hc, y = row - c * g.Hc;
    f32x4 xb;
    if (!fuse_tiles(x0_tiles, thr, tile_of, g, c, y, xx, xb)) continue;
    const int64_t j4 = (int64_t)row * W4 + xq;
    const uint32_t mw = KNOWN && mix.on ? src_mask4(mix.mk, y, xx) : 0u;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (!mask_all(mw)) {
      o = canvas_update(*(const f32x4*)(x + j4 * 4), xb, hist, hist2, j4, A, B, P, HIST2 ? P2 : 0.0f, Sn, noise, seed, sid);
      if (KNOWN && renoise) {
        const f32x4 z = rn_noise ? *(const f32x4*)(rn_noise + j4 * 4) : philox_normal4(seed, rn_sid, (uint64_t)j4);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = o[e] * rn_a + z[e] * rn_b;
      }
    }
    if (mw != 0u) mix_known(mix, mw, c, y, xx, j4, seed, o);
    *(f32x4*)(x + j4 * 4) = o;
    *(f32x4*)(x0bar_out + j4 * 4) = xb;
  }
}
int launch_tiles_fuse_update(float* x, const float* hist, float* x0bar_out, const float* x0_tiles, const float* thr,
                             const int* tile_of, int N, int C, int S, int st, int ny, int nx, int ramp, float A, float B, float P,
                             float Sn, const float* noise, uint64_t seed, uint64_t stream_id, int renoise, float rn_a, float rn_b,
                             const float* rn_noise, uint64_t rn_sid, const TileMix& mix, hipStream_t s, const float* hist2,
                             float P2) {
  KD_REQUIRE(x && x0bar_out && x0_tiles && tile_of && (hist || P == 0.0f) && (hist2 || P2 == 0.0f), "tiles fuse: null argument");
  TileGeom g;
  if (tile_lattice("tiles fuse", N, C, S, st, ny, nx, ramp, &g)) return 1;
  KD_REQUIRE((((uintptr_t)x | (uintptr_t)hist | (uintptr_t)hist2 | (uintptr_t)x0bar_out | (uintptr_t)x0_tiles | (uintptr_t)noise |
               (uintptr_t)rn_noise) & 15) == 0,
             "tiles fuse: x, hist, x0bar_out, x0_tiles and the noise tensors must be 16-byte aligned");
  KD_REQUIRE(x != hist && x != hist2 && x != x0bar_out, "tiles fuse: x must not be the history or the estimate");
  MixArgs m;
  if (tile_mix("tiles fuse", mix, g.Hc, g.Wc, &m)) return 1;
  // nothing known and no re-noise: the lean instantiation, whichever entry the call came through
  // (a second history that is read - P2 != 0 - has its own pair, so the others carry no test for it)
  const bool known = renoise || m.on;
  const auto kernel = P2 != 0.0f ? (known ? tiles_fuse_update_kernel<true, true> : tiles_fuse_update_kernel<false, true>)
                                 : (known ? tiles_fuse_update_kernel<true, false> : tiles_fuse_update_kernel<false, false>);
  hipLaunchKernelGGL(kernel, canvas_grid(C, g.Hc, g.Wc), dim3(256), 0, s, x, hist, hist2, x0bar_out, x0_tiles, thr, tile_of, g, A, B,
                     P, P2, Sn, noise, seed, stream_id, renoise != 0, rn_a, rn_b, rn_noise, rn_sid, m);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- the end of a stage
// out[c, oy + y, ox + x] = (clamp(x[c, y, x], -1, 1) + 1) * 0.5 for every canvas pixel that a present tile covers; every
// other element of out [C, Ho, Wo] keeps its bits.  One pass, no host mask.  With PASTE: out = m ? kn : the same - the known
// value copied, not round-tripped.  kn may then be the window of `out` that is written (the host checks that an overlapping
// source is exactly that window): a thread reads and writes the same element, so `out` is not restrict.  Only the canvas
// rows y_lo <= y < y_hi are written (the whole canvas: 0, Hc): a shard of a canvas ends the rows it owns.
template <bool PASTE>
__global__ __launch_bounds__(256) void tiles_finalize_kernel(const float* __restrict__ x, const int* __restrict__ tile_of,
                                                             TileGeom g, float* out, int Ho, int Wo, int oy, int ox, ImgSrc kn,
                                                             MaskSrc mk, int y_lo, int y_hi) {
  const int W4 = g.Wc / 4;
  const int xq = blockIdx.x * 256 + threadIdx.x;
  if (xq >= W4) return;
  const int xx = 4 * xq;
  const int rows = g.C * g.Hc;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {
    const int c = row / g.Hc, y = row - c * g.Hc;
    if (y < y_lo || y >= y_hi || !tile_covered(tile_of, g, y, xx)) continue;
    const uint32_t mw = PASTE ? src_mask4(mk, y, xx) : 0u;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (!mask_all(mw)) {
      const f32x4 v = *(const f32x4*)(x + ((int64_t)row * W4 + xq) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float cl = v[e] < -1.0f ? -1.0f : (v[e] > 1.0f ? 1.0f : v[e]);
        o[e] = (cl + 1.0f) * 0.5f;
      }
    }
    if (mw != 0u) {
      const f32x4 kv = src_image4(kn, c, y, xx);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (mask_at(mw, e)) o[e] = kv[e];
    }
    *(f32x4*)(out + ((int64_t)c * Ho + oy + y) * Wo + ox + xx) = o;
  }
}
int launch_tiles_finalize(const float* x, const int* tile_of, int N, int C, int S, int st, int ny, int nx, float* out, int Ho,
                          int Wo, int oy, int ox, const TileImage* known, const TileMask* mask, int y_lo, int y_hi,
                          hipStream_t s) {
  KD_REQUIRE(x && tile_of && out, "tiles finalize: null argument");
  KD_REQUIRE((known != nullptr) == (mask != nullptr), "tiles finalize: the known image and the mask come together");
  TileGeom g;
  if (tile_lattice("tiles finalize", N, C, S, st, ny, nx, 0, &g)) return 1;
  const int64_t Wc = g.Wc;   // (oy + y_hi, ox + Wc: no overflow for any int offset)
  if (y_hi < 0) y_hi = g.Hc;   // the whole canvas
  KD_REQUIRE(y_lo >= 0 && y_lo < y_hi && y_hi <= g.Hc, "tiles finalize: the rows [y_lo, y_hi) must be a non-empty range of the canvas");
  KD_REQUIRE(Ho >= 1 && Wo >= 1 && Ho <= (1 << 20) && Wo <= (1 << 20) && Wo % 4 == 0 && ox % 4 == 0,
             "tiles finalize: needs an output with Wo % 4 == 0 and an offset ox % 4 == 0");
  // (oy < 0 with y_lo > 0: the output is a band that holds the rows written and not the ones above them)
  KD_REQUIRE((int64_t)oy + y_lo >= 0 && ox >= 0 && (int64_t)oy + y_hi <= Ho && ox + Wc <= Wo,
             "tiles finalize: the canvas at (oy, ox) lies outside the output");
  KD_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "tiles finalize: x and out must be 16-byte aligned");
  ImgSrc kn{};
  MaskSrc mk{};
  if (known) {
    if (tile_image("tiles finalize known image", known, g.Hc, g.Wc, &kn)) return 1;
    if (tile_source("tiles finalize known mask", mask, g.Hc, g.Wc, 0, 4, &mk)) return 1;
    // a source inside the output must be the window written: every thread then reads the element it writes, and no other
    const uintptr_t kn0 = (uintptr_t)known->d, out0 = (uintptr_t)out;
    const uintptr_t kn1 = kn0 + 4 * (uintptr_t)((int64_t)(C - 1) * known->plane + (int64_t)(known->H - 1) * known->row + known->W);
    if (kn0 < out0 + 4 * (uintptr_t)((int64_t)C * Ho * Wo) && kn1 > out0)
      KD_REQUIRE(known->d == out + (int64_t)oy * Wo + ox && known->H == g.Hc && known->W == g.Wc && known->row == Wo &&
                     (C == 1 || known->plane == (int64_t)Ho * Wo),
                 "tiles finalize: a known image inside the output must be the window at (oy, ox) that is written");
  }
  const auto kernel = known ? tiles_finalize_kernel<true> : tiles_finalize_kernel<false>;
  hipLaunchKernelGGL(kernel, canvas_grid(C, g.Hc, g.Wc), dim3(256), 0, s, x, tile_of, g, out, Ho, Wo, oy, ox, kn, mk, y_lo, y_hi);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------- row strips of tile estimates
// A canvas cut into shards by lattice rows: a shard fuses its band out of its own tiles' estimates and the overlap strips of
// its neighbours' boundary tiles.  One kernel moves them, dst tile d.dst[b] rows <- src tile d.src[b] rows, [C, rows, S] each,
// ROWS_CHUNK descriptors per launch as a kernel argument.  Either side is an array of tiles [., C, H, S]: H == S is a tile
// store, the strip lies at its rows row0 .. row0 + rows; H < S is a strip buffer, the strip lies at its top (rows <= H).  So
// the one kernel packs (store -> buffer), unpacks (buffer -> store) and copies store to store.  With thr_src the threshold
// of the tile travels too: thr_dst[d.dst[b]] = thr_src[d.src[b]].  Data movement only: 16-byte loads and stores, 64-bit
// offsets, every element written by one thread.
enum { ROWS_CHUNK = 32 };
struct RowStrips {
  int src[ROWS_CHUNK], dst[ROWS_CHUNK], row0[ROWS_CHUNK], rows[ROWS_CHUNK];
};
__global__ __launch_bounds__(256) void tiles_rows_copy_kernel(const float* __restrict__ src, int src_rows, float* __restrict__ dst,
                                                              int dst_rows, const float* __restrict__ thr_src,
                                                              float* __restrict__ thr_dst, int C, int S, RowStrips d) {
  const int b = blockIdx.y;
  const int S4 = S / 4, rows = d.rows[b];
  const int per4 = C * rows * S4;   // (< 2^31: checked by the host)
  const int sr0 = src_rows == S ? d.row0[b] : 0, dr0 = dst_rows == S ? d.row0[b] : 0;
  const float* from = src + (int64_t)d.src[b] * C * src_rows * S;
  float* to = dst + (int64_t)d.dst[b] * C * dst_rows * S;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < per4; j += gridDim.x * 256) {
    const int row = j / S4, xq = j - row * S4;   // row = c * rows + y
    const int c = row / rows, y = row - c * rows;
    *(f32x4*)(to + ((int64_t)c * dst_rows + dr0 + y) * S + 4 * xq) =
        *(const f32x4*)(from + ((int64_t)c * src_rows + sr0 + y) * S + 4 * xq);
  }
  if (thr_src && blockIdx.x == 0 && threadIdx.x == 0) thr_dst[d.dst[b]] = thr_src[d.src[b]];
}
int launch_tiles_rows_copy(const float* src, int src_tiles, int src_rows, float* dst, int dst_tiles, int dst_rows,
                           const float* thr_src, float* thr_dst, int n, int C, int S, const int* desc, hipStream_t s) {
  KD_REQUIRE(src && dst && desc && src != dst, "tiles rows copy: null argument, or src and dst are one buffer");
  KD_REQUIRE((thr_src != nullptr) == (thr_dst != nullptr), "tiles rows copy: the thresholds need a source and a destination");
  KD_REQUIRE(n >= 1 && C >= 1 && C <= 1024 && S >= 4 && S % 4 == 0 && (int64_t)C * S * S < (1ll << 31),
             "tiles rows copy: needs n, C >= 1 and a tile size S % 4 == 0 with C S S < 2^31");
  KD_REQUIRE(src_tiles >= 1 && dst_tiles >= 1 && src_rows >= 1 && src_rows <= S && dst_rows >= 1 && dst_rows <= S,
             "tiles rows copy: a side needs at least one tile and 1 <= rows per tile <= S");
  KD_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && (((uintptr_t)thr_src | (uintptr_t)thr_dst) & 3) == 0,
             "tiles rows copy: src and dst must be 16-byte aligned");
  for (int i = 0; i < n; ++i) {   // every descriptor before the first launch
    const int ts = desc[4 * i], td = desc[4 * i + 1], row0 = desc[4 * i + 2], rows = desc[4 * i + 3];
    KD_REQUIRE(ts >= 0 && ts < src_tiles && td >= 0 && td < dst_tiles, "tiles rows copy: a tile index lies outside its buffer");
    KD_REQUIRE(rows >= 0 && rows <= S && row0 >= 0 && row0 <= S - rows, "tiles rows copy: the rows of a strip must lie inside [0, S]");
    KD_REQUIRE((src_rows == S || rows <= src_rows) && (dst_rows == S || rows <= dst_rows),
               "tiles rows copy: a strip is taller than the strip buffer");
  }
  for (int i0 = 0; i0 < n; i0 += ROWS_CHUNK) {
    const int nb = std::min(n - i0, (int)ROWS_CHUNK);
    RowStrips d{};
    int most = 0;
    for (int i = 0; i < nb; ++i) {
      const int* e = desc + 4 * (i0 + i);
      d.src[i] = e[0], d.dst[i] = e[1], d.row0[i] = e[2], d.rows[i] = e[3];
      most = std::max(most, e[3]);
    }
    const int per4 = C * most * (S / 4);
    const int gx = std::max(1, std::min((per4 + 255) / 256, 8192 / nb));
    hipLaunchKernelGGL(tiles_rows_copy_kernel, dim3((unsigned)gx, (unsigned)nb), dim3(256), 0, s, src, src_rows, dst, dst_rows,
                       thr_src, thr_dst, C, S, d);
  }
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
