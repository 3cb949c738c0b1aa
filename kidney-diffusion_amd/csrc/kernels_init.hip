// The per-step share of the UNet's initial cross-embed convolution (CrossEmbedLayer, SURVEY A.1: three stride-1
// convs k = 3 / 7 / 15 over the network input, outputs dim/2 | dim/4 | dim/4 channels) in ONE kernel.
//
// Only x's 3 planes change between denoising steps (the cond / low-res planes' share is computed once per sampling
// call and enters as `res`, unet_build.inc), so per step this is a 3-input-channel convolution with up to 225
// taps: K = 27 / 147 / 675 against N = 64 / 32 / 32.  As three launches of the generic implicit-GEMM kernel it took
// 1.25 ms per step of the 64->256 UNet (0.31 + 0.23 + 0.72: a fourth channel of padding, K padded to 32, one
// pass over the output map and one over the residual per launch, the image packed to NHWC first).  Here:
//   * persistent workgroups (one per CU) keep ALL the weights in LDS for their whole life (dim 128: 113 KB);
//   * a workgroup takes 32 x 8 output pixels at a time: the (32+14) x (8+14) x 3 halo comes straight from the NCHW
//     planes (coalesced along x) into LDS as [row][pixel][channel], zero outside the image;
//   * for a fixed kernel row the K run (tap column, channel) is CONTIGUOUS in that layout, so the MFMA A operand
//     (v_mfma_f32_32x32x2_f32: one k per lane) is a ds_read_b32 at pixel base + immediate offset, no im2col, no
//     channel padding; runs are padded by one float to an even length (its weight is 0);
//   * wave w owns row w of the tile (32 pixels = one MFMA M tile) and all output channels: 15x23 + 7x11 + 2x3x5
//     = 452 MFMAs per tile, 3 LDS reads per MFMA; weight rows have an odd stride, pixels a stride of 3 floats:
//     both operand reads are free of bank conflicts;
//   * the epilogue adds bias or the step-invariant residual, stores NHWC (optionally into a channel slice of a
//     wider buffer) and leaves the GroupNorm partials of the output (SegSrc, common.h).
//
// Self-conditioned UNets (Unet(self_cond=True)) feed a second per-step image, the previous step's x0 estimate, whose
// 3 planes sit right after x's in the conv's input: the per-step share becomes a 6-plane conv (NP = 6), K = 54 / 294
// / 1350.  Its weights no longer fit LDS whole (dim 128: 219.5 KiB; the k = 15 group alone 169 KiB), so at NP = 6
// the k = 3 / 7 weights stay resident and the k = 15 weights STREAM through a two-slot LDS ring, one kernel row
// (32 rows x 90 values, 11.4 KiB) per slot: all eight waves run the k = 15 conv in lockstep, one barrier per kernel
// row, the next row's weights loaded into registers under the current row's MFMAs.
//
// Images of C = 1, 2 or 4 channels (Unet(channels=C)) give NP = C planes per step, 2 C with self-conditioning: the
// kernel is built for NP = 1, 2, 3, 4, 6, 8.  Resident weights or the ring is decided from the LDS bytes (ic_ring): every
// weight group is padded to at least 32 rows, so the resident form fits 160 KiB for NP <= 3 and for no NP >= 4 (NP = 4,
// 32 | 32 | 32 rows: 190 KiB; dim 128: 194 KiB resident, 97 KiB as a ring), and the ring form fits for all but NP = 8 at
// dim 128 (161.3 KiB: init_conv_fused_ok refuses it and the plan takes the generic three-conv path).  The pixel stride in
// the patch stays NP floats, so that the K run of a kernel row stays contiguous: an odd NP reads the A operand free of
// bank conflicts (ds_read_b32: 32 banks per 32-lane half), NP = 2 | 6 two-way, NP = 4 four-way, NP = 8 eight-way.
// Padding the stride to NP + 1 would buy the conflicts off with (NP + 1) / NP times the MFMAs (zero columns in every
// run); the cost of the conflicts at even NP is unmeasured.
#include "common.h"
#include "epilogue.h"

#include <stdlib.h>

namespace kd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int IC_TW = 32, IC_TH = 8;            // output tile
constexpr int IC_PW = IC_TW + 14, IC_PH = IC_TH + 14;   // halo patch (k = 15)
constexpr int IC_SCRATCH = 8 * 1024;             // floats: one 32 x 32 epilogue tile per wave
// floats of the halo patch of NP planes (+ zeroed tail: the padded last run reads one float past a row)
__host__ __device__ constexpr int ic_patch(int np) { return IC_PH * IC_PW * np + 8; }
// K run of one kernel row ((k | NP) values, padded to even) and the odd row stride of a resident weight group
__host__ __device__ constexpr int ic_run(int k, int np) { return (k * np + 1) / 2 * 2; }
__host__ __device__ constexpr int ic_ldk(int k, int np) { return k * ic_run(k, np) + 1; }
// ring form: the k = 15 weights as 15 kernel-row chunks [ky][32 rows][ic_ld15r] (odd stride); two chunks in LDS at a time
__host__ __device__ constexpr int ic_ld15r(int np) { return ic_run(15, np) + 1; }          // NP = 6: 91
__host__ __device__ constexpr int ic_chunk15(int np) { return 32 * ic_ld15r(np); }         // NP = 6: 2912 floats
constexpr int IC_LDS_BYTES = 160 * 1024;

// floats of LDS for the packed weights of (n3, n7, n15) output channels, each padded to a multiple of 32 rows
__host__ __device__ constexpr int ic_rows(int n) { return (n + 31) / 32 * 32; }
__host__ __device__ constexpr int ic_resident_floats(int r3, int r7, int r15, int np) {   // all three groups in LDS
  return r3 * ic_ldk(3, np) + r7 * ic_ldk(7, np) + r15 * ic_ldk(15, np);
}
// Resident weights or the k = 15 ring, from the LDS bytes: the kernel takes at most 64 | 32 | 32 and (rows are padded)
// at least 32 | 32 | 32 weight rows, and for every NP either the largest set fits resident or the smallest does not -
// so the form is a function of NP (the static_asserts below hold the argument)
__host__ __device__ constexpr bool ic_ring(int np) {
  return (ic_resident_floats(32, 32, 32, np) + ic_patch(np) + IC_SCRATCH) * (int)sizeof(float) > IC_LDS_BYTES;
}
template <int NP>
constexpr bool ic_form_decided() {
  return ic_ring(NP) || (ic_resident_floats(64, 32, 32, NP) + ic_patch(NP) + IC_SCRATCH) * (int)sizeof(float) <= IC_LDS_BYTES;
}
static_assert(ic_form_decided<1>() && ic_form_decided<2>() && ic_form_decided<3>() && ic_form_decided<4>() &&
                  ic_form_decided<6>() && ic_form_decided<8>(),
              "an NP whose resident weights fit for some widths only needs a kernel of either form");
static_assert(!ic_ring(3) && ic_ring(6), "3 planes: resident weights; 6 planes: the ring");
// whether ANY shape with 64 rows of k = 3 weights fits the LDS at np planes (else the two-tile kernel is not instantiated)
__host__ __device__ constexpr bool ic_two_tiles_fit(int np) {
  return !ic_ring(np) || (64 * ic_ldk(3, np) + 32 * ic_ldk(7, np) + 2 * ic_chunk15(np) + ic_patch(np) + IC_SCRATCH) *
                                 (int)sizeof(float) <= IC_LDS_BYTES;
}
static_assert(ic_two_tiles_fit(6) && !ic_two_tiles_fit(8), "6 planes run at dim 128, 8 planes up to dim 64");
static bool ic_np_ok(int np) { return np == 1 || np == 2 || np == 3 || np == 4 || np == 6 || np == 8; }
size_t init_conv_weight_floats(int n3, int n7, int n15, int np) {
  if (ic_ring(np))
    return (size_t)ic_rows(n3) * ic_ldk(3, np) + (size_t)ic_rows(n7) * ic_ldk(7, np) + (size_t)15 * ic_chunk15(np);
  return (size_t)ic_resident_floats(ic_rows(n3), ic_rows(n7), ic_rows(n15), np);
}
// LDS of the kernel: resident weights (ring form: k = 3 / 7 + the two ring slots) + patch + epilogue scratch
static size_t init_conv_lds_floats(int n3, int n7, int n15, int np) {
  const size_t w = ic_ring(np)
                       ? (size_t)ic_rows(n3) * ic_ldk(3, np) + (size_t)ic_rows(n7) * ic_ldk(7, np) + 2 * ic_chunk15(np)
                       : init_conv_weight_floats(n3, n7, n15, np);
  return w + ic_patch(np) + IC_SCRATCH;
}
bool init_conv_fused_ok(int S, int n3, int n7, int n15, int np) {
  if (!ic_np_ok(np) || n3 < 1 || n7 < 1 || n15 < 1) return false;
  const size_t lds = init_conv_lds_floats(n3, n7, n15, np) * sizeof(float);
  return S % IC_TW == 0 && S % IC_TH == 0 && lds <= (size_t)IC_LDS_BYTES && ic_rows(n3) <= 64 && ic_rows(n7) <= 32 &&
         ic_rows(n15) <= 32 && n3 % 4 == 0 && n7 % 4 == 0 && n15 % 4 == 0;
}

// OIHW [n][Itot][k][k] -> rows [n][ky][kx*np + c] over input channels c0..c0+np-1, runs padded to `run`, rows to `ldk`
// (zeros), n padded to a multiple of 32 rows (zeros).  chunked: [ky][n][r] with row stride ldk (the k = 15 ring)
__global__ void init_conv_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int n_real, int Itot, int c0,
                                      int np, int k, int run, int ldk, int rows, int chunked) {
  const int total = chunked ? k * rows * ldk : rows * ldk;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    int n, ky, r;
    if (chunked) {
      ky = idx / (rows * ldk);
      const int rem = idx - ky * rows * ldk;
      n = rem / ldk;
      r = rem - n * ldk;
    } else {
      n = idx / ldk;
      const int kk = idx - n * ldk;
      ky = kk / run;
      r = kk - ky * run;
    }
    float v = 0.f;
    if (n < n_real && ky < k && r < np * k) {
      const int kx = r / np, c = r - kx * np;
      v = w[(((int64_t)n * Itot + c0 + c) * k + ky) * k + kx];
    }
    out[idx] = v;
  }
}
int launch_init_conv_pack(const float* w3, const float* w7, const float* w15, float* out, int n3, int n7, int n15, int Itot,
                          int c0, int np, hipStream_t s) {
  KD_REQUIRE(ic_np_ok(np), "init conv pack: 1, 2, 3, 4, 6 or 8 planes");
  const int l3 = ic_ldk(3, np), l7 = ic_ldk(7, np);
  float* o3 = out;
  float* o7 = o3 + (size_t)ic_rows(n3) * l3;
  float* o15 = o7 + (size_t)ic_rows(n7) * l7;
  hipLaunchKernelGGL(init_conv_pack_kernel, dim3(64), dim3(256), 0, s, w3, o3, n3, Itot, c0, np, 3, ic_run(3, np), l3,
                     ic_rows(n3), 0);
  hipLaunchKernelGGL(init_conv_pack_kernel, dim3(64), dim3(256), 0, s, w7, o7, n7, Itot, c0, np, 7, ic_run(7, np), l7,
                     ic_rows(n7), 0);
  if (ic_ring(np))
    hipLaunchKernelGGL(init_conv_pack_kernel, dim3(64), dim3(256), 0, s, w15, o15, n15, Itot, c0, np, 15, ic_run(15, np),
                       ic_ld15r(np), 32, 1);
  else
    hipLaunchKernelGGL(init_conv_pack_kernel, dim3(64), dim3(256), 0, s, w15, o15, n15, Itot, c0, np, 15, ic_run(15, np),
                       ic_ldk(15, np), ic_rows(n15), 0);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

struct InitConvParams {
  const float* x;      // NCHW [B][cx][S][S]
  const float* wp;     // init_conv_weight_floats packed weights
  const float* bias;   // [n3 + n7 + n15] or nullptr (then `res` carries it)
  const float* res;    // dense NHWC [B][S][S][n3+n7+n15] step-invariant share, or nullptr
  float* y;            // NHWC, row stride ldy, first channel at y
  double* seg;         // GroupNorm partials [B][(n3+n7+n15)/16][S*S/32][2] or nullptr
  int B, S, ldy, n3, n7, n15;
  const float* sc;     // NP = 2 cx: the self-conditioning planes NCHW [B][cx][S][S] (nullptr: zeros)
  int cx;              // image channels: NP = cx (x) or 2 cx (x | self_cond)
};

template <int N3T, int NP>   // 32-row tiles of the k = 3 conv (1 or 2); input planes per step (C: x, 2 C: x | self_cond)
__global__ __launch_bounds__(512, 1) void init_conv_kernel(InitConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr bool RING = ic_ring(NP);   // k = 15 weights streamed through two LDS slots
  constexpr int IC_LD15R = ic_ld15r(NP), IC_CHUNK15 = ic_chunk15(NP);
  constexpr int RUN3 = ic_run(3, NP), RUN7 = ic_run(7, NP), RUN15 = ic_run(15, NP);
  constexpr int K3 = ic_ldk(3, NP), K7 = ic_ldk(7, NP), K15 = RING ? IC_LD15R : ic_ldk(15, NP);
  constexpr int PATCH = ic_patch(NP);
  const int r3 = N3T * 32, r7 = 32, r15 = 32;
  float* W3 = lds;
  float* W7 = W3 + r3 * K3;
  float* W15 = W7 + r7 * K7;   // RING: slot 0 | slot 1
  float* patch = W15 + (RING ? 2 * IC_CHUNK15 : r15 * K15);
  float* scratch = patch + PATCH + (threadIdx.x >> 6) * 1024;   // 4 KB per wave (epilogue.h)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // resident weights (RING: + the first kernel row of the k = 15 stream into slot 0)
  const int nw = RING ? r3 * K3 + r7 * K7 + IC_CHUNK15 : (r3 * K3 + r7 * K7 + r15 * K15);
  for (int i = tid; i < nw; i += 512) lds[i] = p.wp[i];
  for (int i = tid; i < 8; i += 512) patch[PATCH - 8 + i] = 0.f;
  // RING: chunk c of the stream (kernel row c % 15) lives at wp15 + (c % 15) * IC_CHUNK15; each thread carries its
  // share of the next chunk in registers (16-byte loads: a chunk is 728 float4 at NP = 6)
  const float* wp15 = p.wp + r3 * K3 + r7 * K7;
  constexpr int NRV = RING ? (IC_CHUNK15 / 4 + 511) / 512 : 1;
  f32x4 rv[NRV];
  auto ring_fetch = [&](int ky) {
#pragma unroll
    for (int q = 0; q < NRV; ++q) {
      const int i = tid + q * 512;
      if (i < IC_CHUNK15 / 4) rv[q] = *(const f32x4*)(wp15 + (size_t)ky * IC_CHUNK15 + 4 * i);
    }
  };
  auto ring_store = [&](float* slot) {
#pragma unroll
    for (int q = 0; q < NRV; ++q) {
      const int i = tid + q * 512;
      if (i < IC_CHUNK15 / 4) *(f32x4*)(slot + 4 * i) = rv[q];
    }
  };
  if (RING) ring_fetch(1);
  int gstep = 0;   // RING: k = 15 kernel rows consumed so far (slot = gstep & 1)

  const int S = p.S, tx_n = S / IC_TW, ty_n = S / IC_TH;
  const int ntiles = p.B * tx_n * ty_n;
  const int C = p.n3 + p.n7 + p.n15;
  const int frow = lane & 31, khalf = lane >> 5;
  const int64_t plane = (int64_t)S * S;
  // image channels: fixed by NP where only one channel count gives it (1, 3: x alone; 6, 8: x | self_cond)
  const int cx = (NP & 1) ? NP : NP == 6 ? 3 : NP == 8 ? 4 : p.cx;

  // halo loader: NP * 2 values per thread, fetched into registers one tile ahead (the loads fly during the MFMAs of
  // the current tile) and written to LDS behind the barrier that ends the current tile's reads
  constexpr int NPV = (IC_PH * IC_PW * NP + 511) / 512;
  float pv[NPV];
  auto fetch = [&](int tile) {
    const int b = tile / (tx_n * ty_n);
    const int rem = tile - b * tx_n * ty_n;
    const int y0 = (rem / tx_n) * IC_TH, x0 = (rem % tx_n) * IC_TW;
#pragma unroll
    for (int q = 0; q < NPV; ++q) {
      const int i = tid + q * 512;
      const int c = i / (IC_PH * IC_PW), r = i - c * (IC_PH * IC_PW);
      const int py = r / IC_PW, px = r - py * IC_PW;
      const int iy = y0 - 7 + py, ix = x0 - 7 + px;
      float v = 0.f;
      if (i < IC_PH * IC_PW * NP && iy >= 0 && iy < S && ix >= 0 && ix < S) {
        if ((NP & 1) || c < cx)
          v = p.x[((int64_t)b * cx + c) * plane + (int64_t)iy * S + ix];
        else if (p.sc)
          v = p.sc[((int64_t)b * cx + c - cx) * plane + (int64_t)iy * S + ix];
      }
      pv[q] = v;
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (tx_n * ty_n);
    const int rem = tile - b * tx_n * ty_n;
    const int y0 = (rem / tx_n) * IC_TH, x0 = (rem % tx_n) * IC_TW;
    __syncthreads();   // the previous tile's MFMA reads of the patch are done (and the weights have landed)
#pragma unroll
    for (int q = 0; q < NPV; ++q) {
      const int i = tid + q * 512;
      if (i < IC_PH * IC_PW * NP) {
        const int c = i / (IC_PH * IC_PW), r = i - c * (IC_PH * IC_PW);
        patch[r * NP + c] = pv[q];
      }
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) fetch(tile + gridDim.x);

    {   // wave w: row w of the tile (8 waves, two per SIMD); one conv after the other, each finished (stored) before
        // the next starts, so that only one set of accumulators is live
      const int row = wave;
      // epilogue: the wave turns its 32-pixel x 32-channel tile through its private LDS scratch and stores 16 B per
      // lane (epilogue.h): 4 stores + 4 residual loads per tile instead of 16 + 16
      const int64_t pix0 = ((int64_t)b * S + y0 + row) * S + x0;
      const int64_t chunk = ((int64_t)(y0 + row) * S + x0) >> 5;   // 32-pixel run index inside the image
      auto tile_of = [&](int ch0, int nreal) {   // channels ch0 + [0, 32) of the output
        WideEpilogue e;
        e.y = p.y + pix0 * p.ldy + ch0;
        e.ldy = p.ldy;
        e.bias = p.bias ? p.bias + ch0 : nullptr;
        e.res = p.res ? p.res + pix0 * C + ch0 : nullptr;
        e.ldres = C;
        e.gate_src = nullptr;
        e.ldgs = 0;
        e.gate = nullptr;
        e.rows = 32;
        e.cols = nreal < 32 ? nreal : 32;
        e.act = ACT_NONE;
        return e;
      };
      // the step-invariant share (residual) of all four tiles of this row, requested before the first MFMA: 64
      // registers that arrive under the convolutions instead of 4 dependent loads in front of every tile's stores
      ep_f32x4 rp15[4], rp7[4], rp3[N3T][4];
      wide_prefetch_res(tile_of(p.n3 + p.n7, p.n15), rp15);
      wide_prefetch_res(tile_of(p.n3, p.n7), rp7);
#pragma unroll
      for (int j = 0; j < N3T; ++j) wide_prefetch_res(tile_of(j * 32, p.n3 - j * 32), rp3[j]);
      auto finish = [&](const f32x16& acc, int ch0, int nreal, const ep_f32x4 (&rp)[4]) {
        const WideEpilogue e = tile_of(ch0, nreal);
        double s1, s2;
        if (p.seg) {   // wave-uniform
          store_tile32_wide_pre<true>(acc, scratch, e, rp, s1, s2);
          reduce_tile32_stats(s1, s2);
          const int n = ch0 + 4 * (lane & 7);   // lane 0: columns 0-15, lane 4: columns 16-31
          if ((lane & ~4) == 0 && 4 * (lane & 7) < nreal) {
            double* o = p.seg + (((int64_t)b * (C >> 4) + (n >> 4)) * (plane >> 5) + chunk) * 2;
            o[0] = s1;
            o[1] = s2;
          }
        } else {
          store_tile32_wide_pre<false>(acc, scratch, e, rp, s1, s2);
        }
      };
      // k = 15: window rows row .. row + 14, columns frow .. frow + 14.  Two accumulator chains (even / odd k pairs,
      // added at the end): hipcc sinks every operand read next to its MFMA, and with ONE chain each MFMA also
      // waits for its predecessor.  RING: every wave walks the kernel rows in step with the others - per row one
      // barrier (the slot written one row ago has landed; nobody reads the other slot any more), then that other
      // slot gets the registers' next row and the registers fetch the row after
      auto conv15 = [&]() {
        {
          const float* pa = patch + (row * IC_PW + frow) * NP + khalf;
          const float* pb = W15 + frow * K15 + khalf;
          f32x16 a15, b15;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            a15[r] = 0.f;
            b15[r] = 0.f;
          }
          for (int ky = 0; ky < 15; ++ky) {
            if (RING) {
              __syncthreads();
              ring_store(W15 + ((gstep + 1) & 1) * IC_CHUNK15);
              ring_fetch(ky + 2 < 15 ? ky + 2 : ky + 2 - 15);
              pb = W15 + (gstep & 1) * IC_CHUNK15 + frow * K15 + khalf;
              ++gstep;
            }
#pragma unroll
            for (int kk = 0; kk + 1 < RUN15 / 2; kk += 2) {
              a15 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * kk], pb[2 * kk], a15, 0, 0, 0);
              b15 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * kk + 2], pb[2 * kk + 2], b15, 0, 0, 0);
            }
            if ((RUN15 / 2) & 1)   // an odd number of k pairs (NP = 2, 3, 6): the last one
              a15 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[RUN15 - 2], pb[RUN15 - 2], a15, 0, 0, 0);
            pa += IC_PW * NP;
            if (!RING) pb += RUN15;
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) a15[r] += b15[r];
          finish(a15, p.n3 + p.n7, p.n15, rp15);
        }
      };
      // k = 7: the centred 7 x 7 window starts 4 rows / 4 columns into the 15 x 15 one
      auto conv7 = [&]() {
        {
          const float* pa = patch + ((row + 4) * IC_PW + frow + 4) * NP + khalf;
          const float* pb = W7 + frow * K7 + khalf;
          f32x16 a7;
#pragma unroll
          for (int r = 0; r < 16; ++r) a7[r] = 0.f;
          for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
            for (int kk = 0; kk < RUN7 / 2; ++kk)
              a7 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * kk], pb[2 * kk], a7, 0, 0, 0);
            pa += IC_PW * NP;
            pb += RUN7;
          }
          finish(a7, p.n3, p.n7, rp7);
        }
      };
      // k = 3: starts 6 rows / 6 columns in
      auto conv3 = [&]() {
#pragma unroll
        for (int j = 0; j < N3T; ++j) {
          const float* pa = patch + ((row + 6) * IC_PW + frow + 6) * NP + khalf;
          const float* pb = W3 + (j * 32 + frow) * K3 + khalf;
          f32x16 a3;
#pragma unroll
          for (int r = 0; r < 16; ++r) a3[r] = 0.f;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kk = 0; kk < RUN3 / 2; ++kk)
              a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[ky * IC_PW * NP + 2 * kk], pb[ky * RUN3 + 2 * kk], a3, 0, 0, 0);
          finish(a3, j * 32, p.n3 - j * 32, rp3[j]);
        }
      };
      // the two waves of a SIMD (w, w + 4) take the convs in opposite order: one's epilogues (LDS turn, residual
      // loads, stores, fp64 statistics) run under the other's long k = 15 MFMA chain instead of next to its epilogues.
      // RING: the k = 15 conv has barriers, so every wave runs it first
      if (RING || wave < 4) {
        conv15();
        conv7();
        conv3();
      } else {
        conv7();
        conv3();
        conv15();
      }
    }
  }
}

template <int NP>
static int launch_init_conv_np(const InitConvParams& p, int n3, size_t smem, int grid, hipStream_t s) {
  if (ic_rows(n3) == 64) {
    // (8 planes: no shape with two k = 3 tiles fits the LDS - init_conv_fused_ok - so that kernel is not built)
    if constexpr (ic_two_tiles_fit(NP)) {
      KD_HIP_CHECK(hipFuncSetAttribute((const void*)init_conv_kernel<2, NP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)smem));
      hipLaunchKernelGGL((init_conv_kernel<2, NP>), dim3(grid), dim3(512), smem, s, p);
    } else {
      KD_REQUIRE(false, "init conv kernel: two k = 3 tiles of this many planes do not fit LDS");
    }
  } else {
    KD_HIP_CHECK(hipFuncSetAttribute((const void*)init_conv_kernel<1, NP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)smem));
    hipLaunchKernelGGL((init_conv_kernel<1, NP>), dim3(grid), dim3(512), smem, s, p);
  }
  return 0;
}

int launch_init_conv(const float* x, const float* sc, int cx, int np, const float* wp, const float* bias, const float* res, float* y,
                     int ldy, double* seg, int B, int S, int n3, int n7, int n15, int cus, hipStream_t s) {
  KD_REQUIRE(cus > 0, "init conv kernel: CU count missing");
  KD_REQUIRE(init_conv_fused_ok(S, n3, n7, n15, np), "init conv kernel: image size % 32, weights must fit LDS");
  KD_REQUIRE(ldy % 4 == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)res & 15) == 0 && ((uintptr_t)bias & 15) == 0 &&
                 ((uintptr_t)wp & 15) == 0,
             "init conv kernel: 16-byte aligned output / residual / bias rows");
  KD_REQUIRE(!seg || ((n3 % 16) == 0 && (n7 % 16) == 0 && (n15 % 16) == 0), "init conv partials: 16-channel segments");
  KD_REQUIRE(cx >= 1 && (np == cx || np == 2 * cx), "init conv kernel: planes = channels (x) or 2 channels (x | self_cond)");
  InitConvParams p{x, wp, bias, res, y, seg, B, S, ldy, n3, n7, n15, np == 2 * cx ? sc : nullptr, cx};
  const size_t smem = init_conv_lds_floats(n3, n7, n15, np) * sizeof(float);
  const int ntiles = B * (S / IC_TW) * (S / IC_TH);
  const int grid = ntiles < cus ? ntiles : cus;   // persistent: one workgroup per CU keeps the weights in LDS
  int rc = 1;
  switch (np) {
    case 1: rc = launch_init_conv_np<1>(p, n3, smem, grid, s); break;
    case 2: rc = launch_init_conv_np<2>(p, n3, smem, grid, s); break;
    case 3: rc = launch_init_conv_np<3>(p, n3, smem, grid, s); break;
    case 4: rc = launch_init_conv_np<4>(p, n3, smem, grid, s); break;
    case 6: rc = launch_init_conv_np<6>(p, n3, smem, grid, s); break;
    case 8: rc = launch_init_conv_np<8>(p, n3, smem, grid, s); break;
  }
  if (rc) return 1;
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- Unet(init_cross_embed=False): the per-step share of ONE k x k conv (k = 3 | 5 | 7) of the NP per-step planes to all
// n <= 128 output channels, in the shape of init_conv_kernel: persistent workgroups with the packed weights [rows][ic_ldk(k, NP)]
// resident in LDS, 32 x 8 output pixels at a time from a (32 + k - 1) x (8 + k - 1) x NP halo patch read straight from the NCHW
// planes (fetched one tile ahead), K over whole kernel rows on v_mfma_f32_32x32x2_f32, wave w = row w of the tile and one
// 32-channel tile after the other, the same epilogue (bias | step-invariant residual, NHWC into a channel slice, 16-channel
// GroupNorm partials).  LDS: rows x ic_ldk floats + patch + 32 KiB of epilogue scratch within 160 KiB - dim 128 at k = 7:
// 128 x 155 floats (77.5 KiB) at NP = 3 fits, 128 x 295 (147.5 KiB) at NP = 6 does not (init_plain_ok; the plan then takes
// the generic conv).
__host__ __device__ constexpr int ip_patch(int k, int np) { return (IC_TH + k - 1) * (IC_TW + k - 1) * np + 8; }
static size_t init_plain_lds_floats(int n, int k, int np) {
  return (size_t)ic_rows(n) * ic_ldk(k, np) + ip_patch(k, np) + IC_SCRATCH;
}
size_t init_plain_weight_floats(int n, int k, int np) { return (size_t)ic_rows(n) * ic_ldk(k, np); }
bool init_plain_ok(int S, int n, int k, int np) {
  if (!ic_np_ok(np) || (k != 3 && k != 5 && k != 7) || n < 4 || n > 128 || n % 4) return false;
  return S >= IC_TW && S % IC_TW == 0 && S % IC_TH == 0 && init_plain_lds_floats(n, k, np) * sizeof(float) <= (size_t)IC_LDS_BYTES;
}
int launch_init_plain_pack(const float* w, float* out, int n, int Itot, int c0, int np, int k, hipStream_t s) {
  KD_REQUIRE(ic_np_ok(np) && (k == 3 || k == 5 || k == 7) && c0 >= 0 && c0 + np <= Itot,
             "plain init conv pack: 1, 2, 3, 4, 6 or 8 planes inside the weights, kernel size 3, 5 or 7");
  hipLaunchKernelGGL(init_conv_pack_kernel, dim3(64), dim3(256), 0, s, w, out, n, Itot, c0, np, k, ic_run(k, np), ic_ldk(k, np),
                     ic_rows(n), 0);
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

struct InitPlainParams {
  const float* x;      // NCHW [B][cx][S][S]
  const float* sc;     // NP = 2 cx: the self-conditioning planes NCHW [B][cx][S][S] (nullptr: zeros)
  const float* wp;     // init_plain_weight_floats packed weights
  const float* bias;   // [n] or nullptr
  const float* res;    // dense NHWC [B][S][S][n] step-invariant share, or nullptr
  float* y;            // NHWC, row stride ldy, first channel at y
  double* seg;         // GroupNorm partials [B][n/16][S*S/32][2] or nullptr
  int B, S, ldy, n, cx;
};

template <int KS, int NP>
__global__ __launch_bounds__(512, 1) void init_plain_kernel(InitPlainParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int RUN = ic_run(KS, NP), LDK = ic_ldk(KS, NP), PATCH = ip_patch(KS, NP);
  constexpr int PW = IC_TW + KS - 1, PH = IC_TH + KS - 1, PAD = KS / 2;
  const int rows = ic_rows(p.n);
  float* Wl = lds;
  float* patch = Wl + rows * LDK;
  float* scratch = patch + PATCH + (threadIdx.x >> 6) * 1024;   // 4 KB per wave (epilogue.h)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < rows * LDK; i += 512) lds[i] = p.wp[i];
  for (int i = tid; i < 8; i += 512) patch[PATCH - 8 + i] = 0.f;

  const int S = p.S, tx_n = S / IC_TW, ty_n = S / IC_TH;
  const int ntiles = p.B * tx_n * ty_n;
  const int C = p.n;
  const int frow = lane & 31, khalf = lane >> 5;
  const int64_t plane = (int64_t)S * S;
  const int cx = (NP & 1) ? NP : NP == 6 ? 3 : NP == 8 ? 4 : p.cx;

  constexpr int NPV = (PH * PW * NP + 511) / 512;
  float pv[NPV];
  auto fetch = [&](int tile) {
    const int b = tile / (tx_n * ty_n);
    const int rem = tile - b * tx_n * ty_n;
    const int y0 = (rem / tx_n) * IC_TH, x0 = (rem % tx_n) * IC_TW;
#pragma unroll
    for (int q = 0; q < NPV; ++q) {
      const int i = tid + q * 512;
      const int c = i / (PH * PW), r = i - c * (PH * PW);
      const int py = r / PW, px = r - py * PW;
      const int iy = y0 - PAD + py, ix = x0 - PAD + px;
      float v = 0.f;
      if (i < PH * PW * NP && iy >= 0 && iy < S && ix >= 0 && ix < S) {
        if ((NP & 1) || c < cx)
          v = p.x[((int64_t)b * cx + c) * plane + (int64_t)iy * S + ix];
        else if (p.sc)
          v = p.sc[((int64_t)b * cx + c - cx) * plane + (int64_t)iy * S + ix];
      }
      pv[q] = v;
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (tx_n * ty_n);
    const int rem = tile - b * tx_n * ty_n;
    const int y0 = (rem / tx_n) * IC_TH, x0 = (rem % tx_n) * IC_TW;
    __syncthreads();   // the previous tile's MFMA reads of the patch are done (and the weights have landed)
#pragma unroll
    for (int q = 0; q < NPV; ++q) {
      const int i = tid + q * 512;
      if (i < PH * PW * NP) {
        const int c = i / (PH * PW), r = i - c * (PH * PW);
        patch[r * NP + c] = pv[q];
      }
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) fetch(tile + gridDim.x);

    const int row = wave;
    const int64_t pix0 = ((int64_t)b * S + y0 + row) * S + x0;
    const int64_t chunk = ((int64_t)(y0 + row) * S + x0) >> 5;   // 32-pixel run index inside the image
    const float* pa = patch + (row * PW + frow) * NP + khalf;
    for (int j = 0; j * 32 < p.n; ++j) {   // one 32-channel tile after the other: one set of accumulators live
      const int ch0 = j * 32, nreal = p.n - ch0;
      WideEpilogue e;
      e.y = p.y + pix0 * p.ldy + ch0;
      e.ldy = p.ldy;
      e.bias = p.bias ? p.bias + ch0 : nullptr;
      e.res = p.res ? p.res + pix0 * C + ch0 : nullptr;
      e.ldres = C;
      e.gate_src = nullptr;
      e.ldgs = 0;
      e.gate = nullptr;
      e.rows = 32;
      e.cols = nreal < 32 ? nreal : 32;
      e.act = ACT_NONE;
      ep_f32x4 rp[4];
      wide_prefetch_res(e, rp);   // the step-invariant share arrives under the MFMAs
      const float* pb = Wl + (ch0 + frow) * LDK + khalf;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky)
#pragma unroll
        for (int kk = 0; kk < RUN / 2; ++kk)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[ky * PW * NP + 2 * kk], pb[ky * RUN + 2 * kk], acc, 0, 0, 0);
      double s1, s2;
      if (p.seg) {   // wave-uniform
        store_tile32_wide_pre<true>(acc, scratch, e, rp, s1, s2);
        reduce_tile32_stats(s1, s2);
        const int n = ch0 + 4 * (lane & 7);   // lane 0: columns 0-15, lane 4: columns 16-31
        if ((lane & ~4) == 0 && 4 * (lane & 7) < nreal) {
          double* o = p.seg + (((int64_t)b * (C >> 4) + (n >> 4)) * (plane >> 5) + chunk) * 2;
          o[0] = s1;
          o[1] = s2;
        }
      } else {
        store_tile32_wide_pre<false>(acc, scratch, e, rp, s1, s2);
      }
    }
  }
}

template <int KS, int NP>
static int launch_init_plain_knp(const InitPlainParams& p, size_t smem, int grid, hipStream_t s) {
  KD_HIP_CHECK(hipFuncSetAttribute((const void*)init_plain_kernel<KS, NP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL((init_plain_kernel<KS, NP>), dim3(grid), dim3(512), smem, s, p);
  return 0;
}
template <int KS>
static int launch_init_plain_k(const InitPlainParams& p, int np, size_t smem, int grid, hipStream_t s) {
  switch (np) {
    case 1: return launch_init_plain_knp<KS, 1>(p, smem, grid, s);
    case 2: return launch_init_plain_knp<KS, 2>(p, smem, grid, s);
    case 3: return launch_init_plain_knp<KS, 3>(p, smem, grid, s);
    case 4: return launch_init_plain_knp<KS, 4>(p, smem, grid, s);
    case 6: return launch_init_plain_knp<KS, 6>(p, smem, grid, s);
    case 8: return launch_init_plain_knp<KS, 8>(p, smem, grid, s);
  }
  return 1;
}

int launch_init_plain(const float* x, const float* sc, int cx, int np, const float* wp, const float* bias, const float* res, float* y,
                      int ldy, double* seg, int B, int S, int n, int k, int cus, hipStream_t s) {
  KD_REQUIRE(cus > 0, "plain init conv kernel: CU count missing");
  KD_REQUIRE(init_plain_ok(S, n, k, np), "plain init conv kernel: kernel size 3 | 5 | 7, image size % 32, weights must fit LDS");
  KD_REQUIRE(B >= 1 && (int64_t)B * (S / IC_TW) * (S / IC_TH) < 0x7fffffff, "plain init conv kernel: batch out of range");
  KD_REQUIRE(ldy % 4 == 0 && ldy >= n && ((uintptr_t)y & 15) == 0 && ((uintptr_t)res & 15) == 0 && ((uintptr_t)bias & 15) == 0 &&
                 ((uintptr_t)wp & 15) == 0,
             "plain init conv kernel: 16-byte aligned output / residual / bias rows");
  KD_REQUIRE(!seg || n % 16 == 0, "plain init conv partials: 16-channel segments");
  KD_REQUIRE(cx >= 1 && (np == cx || np == 2 * cx), "plain init conv kernel: planes = channels (x) or 2 channels (x | self_cond)");
  InitPlainParams p{x, np == 2 * cx ? sc : nullptr, wp, bias, res, y, seg, B, S, ldy, n, cx};
  const size_t smem = init_plain_lds_floats(n, k, np) * sizeof(float);
  const int ntiles = B * (S / IC_TW) * (S / IC_TH);
  const int grid = ntiles < cus ? ntiles : cus;   // persistent: one workgroup per CU keeps the weights in LDS
  int rc = 1;
  switch (k) {
    case 3: rc = launch_init_plain_k<3>(p, np, smem, grid, s); break;
    case 5: rc = launch_init_plain_k<5>(p, np, smem, grid, s); break;
    case 7: rc = launch_init_plain_k<7>(p, np, smem, grid, s); break;
  }
  if (rc) return 1;
  KD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace kd
