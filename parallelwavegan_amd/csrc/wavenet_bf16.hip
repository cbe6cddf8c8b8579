// wavenet_bf16.hip -- opt-in bf16-operand inference form of the one-launch Parallel WaveGAN layer (csrc/wavenet.hip):
//
//     z      = W_dil (*) bf16(x) + W_aux . bf16(c) + b_dil                 (128 rows; K = 3 * 64 + 80 = 272, padded to 288)
//     g      = bf16( tanh(z[:64]) * sigmoid(z[64:]) )                       (gate in fp32, hardware exp2 / rcp form)
//     skips' = (W_skip . g + b_skip + skips) * skip_mul
//     x'     = (W_out  . g + b_out  + x)     * out_mul
//
// Numerical definition (include/pwg_kernels.h, "bf16-operand inference", applied to each of the layer's four
// convolutions): W_dil, W_aux, W_skip, W_out are the effective weights (w * scale) rounded to bf16 once, by the packer;
// x and c are rounded to bf16 (nearest-even) while they are staged; products are accumulated in fp32 on the bf16 MFMA;
// biases, the gate, the residual x and the running skip sum are fp32.  The residual is re-read in fp32 from memory (it
// is L2-resident: the staging pass read it a moment earlier), never taken from the bf16 copy staged for the MFMA.
//
// A workgroup (4 waves) owns 64 columns of one item.  Staging: every operand row of those columns -- the three tap
// windows of x (x[n - d], x[n], x[n + d]: separate windows, so any dilation fits; at small d the overlapping bytes come
// from L2) and the 80 aux rows -- is loaded fp32 (16 B along t per lane and channel), converted in registers and
// stored as bf16 in [column][channel] order, 288 channels (36 octets; the last 16 are zero) per column, so that a
// lane's 8 consecutive reduction elements are one 16-B LDS read; the column stride is 37 x 16 B (odd).  Wave (h, n)
// computes rows [32 h, +32) of BOTH halves of z for columns [32 n, +32), so tanh * sigmoid is lane-local; g goes to a
// second LDS tile ([column][64 channels], bf16) and is the B operand of the two 1x1 convolutions (one K = 64
// contraction with 128 rows: skip rows then out rows).  A operands (weights) are 16-B fragments of a packed image
// [K / 8][128 rows][8] (phase 1, then phase 2), read straight from L2 through a 4-step register ring.  The kernel is
// latency-bound: everything a workgroup needs from memory is requested up front -- the staging loads,
// then the epilogue's fp32 residual and skip sum, then the first weight fragments -- and the biases sit in LDS.
// LDS: 47 KB, three workgroups per CU.  Both bf16 MFMA shapes (32x32x16, 16x16x32) are built at the same tiles;
// pwg_wavenet_bf16_layer_forward_cfg selects.  Deterministic: one workgroup owns its output tile over the whole
// reduction, no split-K, no atomics.
#include "common.h"
#include "wavenet_bf16.h"

#include <stdint.h>
#include <type_traits>

namespace pwg {
namespace {

constexpr int kDefaultMfmaShape = 32;  // by wall time at the PWG.v1 shapes

struct WbArgs {
  const float* x;       // (B, 64, T)
  const float* c;       // (B, 80, T)
  const float* skips;   // (B, 64, T) or NULL
  const bf16x8* w1;     // [36][128] fragments
  const bf16x8* w2;     // [8][128] fragments
  const float* b_dil;   // (128) or NULL
  const float* b_skip;  // (64) or NULL
  const float* b_out;   // (64) or NULL
  float* x_out;         // (B, 64, T)
  float* skips_out;     // (B, 64, T), may alias skips
  float* z_out;         // (B, 128, T) or NULL
  float* g_out;         // (B, 64, T) or NULL
  int T, dil;
  float out_mul, skip_mul;
};

// The ragged form (inference): item b ends at column E = min(frames[b] * rate, T); T stays the row stride.
struct WbRaggedArgs : WbArgs {
  const int* frames;  // (batch,) device table, frames per item
  int rate;           // columns per frame
};
template <bool RAGGED>
using WbArgsOf = typename std::conditional<RAGGED, WbRaggedArgs, WbArgs>::type;

// TILE: MFMA shape (32: 32x32x16, 16: 16x16x32).  A wave owns a 32 x 32 block of each half: TM x TN MFMA tiles.
// RAGGED: the sequence of item b is [0, E) inside a row of stride T.  Every read of x, c and the skip sum at a column
// >= E -- the staged windows and the fp32 residual and skip loads -- is replaced by zero, nothing at or past E is written,
// and a workgroup whose columns lie at or past E returns before any load.  The columns < E are bit for bit the plain
// kernel's on the item alone with T = E at the same TILE.  No z / g outputs.
template <int TILE, bool RAGGED>
__global__ __launch_bounds__(256, 2) void wavenet_bf16_layer_kernel(WbArgsOf<RAGGED> a) {
  constexpr int HL = 64 / TILE;      // lane groups along the reduction (2 / 4)
  constexpr int KSTEP = 8 * HL;      // reduction elements per MFMA (16 / 32)
  constexpr int NS1 = K1 / KSTEP;    // phase-1 steps (18 / 9)
  constexpr int NS2 = K2 / KSTEP;    // phase-2 steps (4 / 2)
  constexpr int TM = 32 / TILE, TN = 32 / TILE;
  constexpr int NREG = TILE * TILE / 64;
  constexpr int ITEMS = (OCT1 * BCOLS / 4 + 255) / 256;  // (column group of 4, channel octet) items per thread
  typedef typename Mfma<TILE>::acc_t acc_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);                 // [64 columns][RS]
  __bf16* gs = xs + BCOLS * RS;                                 // [64 columns][RG]
  float* bias = reinterpret_cast<float*>(gs + BCOLS * RG);      // b_dil (128), b_skip (64), b_out (64)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = wave >> 1, cn = wave & 1;
  const int r = lane % TILE, lg = lane / TILE;
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * BCOLS;
  const int T = a.T, dil = a.dil;
  int E = T;  // end of this item's sequence
  if constexpr (RAGGED) {
    const long end = (long)a.frames[b] * a.rate;  // (read once per workgroup)
    E = end < T ? (int)end : T;
    if (n0 >= E) return;
  }
  const float* xb = a.x + (long)b * BR * T;
  const float* cb = a.c + (long)b * BA * T;

  // accumulator element i of tile (mi, ni): row h * 32 + mi * TILE + rowin(i), column cn * 32 + ni * TILE + r
  auto rowin = [&](int i) { return mfma_acc_row<TILE>(0, i, lg); };

  {
    const float* src = tid < BG ? a.b_dil : (tid < BG + BS ? a.b_skip : a.b_out);
    const int k = tid < BG ? tid : (tid < BG + BS ? tid - BG : tid - BG - BS);
    bias[tid] = src ? src[k] : 0.f;
  }

  // ---- stage: item (grp, oct) = 4 columns x 8 channels.  Octets 0..23: tap windows of x (tap = oct / 8), 24..33:
  // the aux rows, 34..35: zero padding.  Interior workgroups (every window inside the sequence) load 16 B per channel;
  // the others check every sample (zeros outside = the zero padding).  The epilogue's fp32 residual and skip sum are
  // loaded right behind the staging loads (their latency hides under the whole matrix work).
  float xres[TM][TN][NREG], sres[TM][TN][NREG];
  {
    const bool interior = n0 - dil >= 0 && n0 + BCOLS + dil <= E;
    f32x4 st[ITEMS][8];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int idx = tid + it * 256, grp = idx & 15, oct = idx >> 4;
      const bool is_x = oct < 3 * 8;
      const float* src = is_x ? xb : cb;
      const int ch0 = is_x ? (oct & 7) * 8 : min(oct - 24, 9) * 8;
      const int f = n0 + 4 * grp + (is_x ? ((oct >> 3) - 1) * dil : 0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (oct < 34) {
          const float* p = src + (long)(ch0 + j) * T;
          if (interior) {
            const f4u u = *reinterpret_cast<const f4u*>(p + f);
            v = f32x4{u[0], u[1], u[2], u[3]};
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (f + e >= 0 && f + e < E) v[e] = p[f + e];
          }
        }
        st[it][j] = v;
      }
    }
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int n = n0 + cn * 32 + ni * TILE + r;
#pragma unroll
        for (int i = 0; i < NREG; ++i) {
          const long o = ((long)b * BR + h * 32 + mi * TILE + rowin(i)) * T + n;
          xres[mi][ni][i] = n < E ? a.x[o] : 0.f;
          sres[mi][ni][i] = (a.skips && n < E) ? a.skips[o] : 0.f;
        }
      }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int idx = tid + it * 256, grp = idx & 15, oct = idx >> 4;
      if (oct < OCT1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bf16x8 v;
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (__bf16)st[it][j][e];
          *reinterpret_cast<bf16x8*>(xs + (4 * grp + e) * RS + oct * 8) = v;
        }
      }
    }
  }

  acc_t acc[2][TM][TN];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int ni = 0; ni < TN; ++ni)
#pragma unroll
        for (int i = 0; i < NREG; ++i) acc[s][mi][ni][i] = 0.f;

  // ---- phase 1: z rows of both halves over K = 288 (A: image fragments from L2, RING-deep register ring whose first
  // loads are in flight during the staging barrier; B: LDS)
  {
    const bf16x8* wp = a.w1 + lg * BG + h * 32 + r;  // + (ks * HL) * 128 + half * 64 + mi * TILE
    bf16x8 A[RING][2][TM];
#pragma unroll
    for (int p = 0; p < RING - 1; ++p)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) A[p][s][mi] = wp[p * HL * BG + s * 64 + mi * TILE];
    __syncthreads();
    const __bf16* bl = xs + (cn * 32 + r) * RS + 8 * lg;
#pragma unroll
    for (int ks = 0; ks < NS1; ++ks) {
      if (ks + RING - 1 < NS1) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int mi = 0; mi < TM; ++mi)
            A[(ks + RING - 1) % RING][s][mi] = wp[(ks + RING - 1) * HL * BG + s * 64 + mi * TILE];
      }
      bf16x8 B[TN];
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) B[ni] = *reinterpret_cast<const bf16x8*>(bl + ni * TILE * RS + ks * KSTEP);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) acc[s][mi][ni] = Mfma<TILE>::run(A[ks % RING][s][mi], B[ni], acc[s][mi][ni]);
    }
  }

  // ---- gate in fp32, rounded to bf16 into the gate tile; z / g to memory for the stage tests
  {
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int col = cn * 32 + ni * TILE + r;
        const int n = n0 + col;
#pragma unroll
        for (int i4 = 0; i4 < NREG; i4 += 4) {
          bf16x4 gv;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int row = h * 32 + mi * TILE + rowin(i4 + e);
            const float zt = acc[0][mi][ni][i4 + e] + bias[row];
            const float zs = acc[1][mi][ni][i4 + e] + bias[BR + row];
            const __bf16 g = (__bf16)gate_fp32(zt, zs);
            gv[e] = g;
            if (!RAGGED && a.z_out && n < T) {
              a.z_out[((long)b * BG + row) * T + n] = zt;
              a.z_out[((long)b * BG + BR + row) * T + n] = zs;
              a.g_out[((long)b * BR + row) * T + n] = (float)g;
            }
          }
          // (4 consecutive rows = 4 consecutive channels of the column: one 8-B store)
          *reinterpret_cast<bf16x4*>(gs + col * RG + h * 32 + mi * TILE + rowin(i4)) = gv;
        }
#pragma unroll
        for (int i = 0; i < NREG; ++i) {
          acc[0][mi][ni][i] = 0.f;
          acc[1][mi][ni][i] = 0.f;
        }
      }
  }

  // ---- phase 2: skip rows [32 h, +32) (half 0) and out rows [32 h, +32) (half 1) over K = 64 rows of g
  {
    const bf16x8* wp = a.w2 + lg * BG + h * 32 + r;
    bf16x8 A[NS2][2][TM];
#pragma unroll
    for (int ks = 0; ks < NS2; ++ks)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) A[ks][s][mi] = wp[ks * HL * BG + s * 64 + mi * TILE];
    __syncthreads();
    const __bf16* bl = gs + (cn * 32 + r) * RG + 8 * lg;
#pragma unroll
    for (int ks = 0; ks < NS2; ++ks) {
      bf16x8 B[TN];
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) B[ni] = *reinterpret_cast<const bf16x8*>(bl + ni * TILE * RG + ks * KSTEP);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) acc[s][mi][ni] = Mfma<TILE>::run(A[ks][s][mi], B[ni], acc[s][mi][ni]);
    }
  }

  // ---- epilogue (fp32): the residual and the running skip sum are the fp32 values read from memory at the start
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      const int n = n0 + cn * 32 + ni * TILE + r;
      if (n >= E) continue;
#pragma unroll
      for (int i = 0; i < NREG; ++i) {
        const int row = h * 32 + mi * TILE + rowin(i);
        const long o = ((long)b * BR + row) * T + n;
        float sv = acc[0][mi][ni][i] + bias[BG + row];
        if (a.skips) sv += sres[mi][ni][i];
        if (a.skip_mul != 1.0f) sv *= a.skip_mul;
        const float xv = (acc[1][mi][ni][i] + bias[BG + BS + row] + xres[mi][ni][i]) * a.out_mul;
        a.skips_out[o] = sv;
        a.x_out[o] = xv;
      }
    }
}

// one thread per bf16 element of the image: phase 1 [36 octets][128 rows][8] over k = tap * 64 + ci (k < 192),
// 192 + aux channel (k < 272), zero (k < 288); phase 2 [8 octets][128 rows][8]: rows 0..63 = w_skip, 64..127 = w_out
__global__ __launch_bounds__(256) void wavenet_bf16_pack_kernel(const float* w_dil, const float* s_dil, const float* w_aux,
                                                                const float* s_aux, const float* w_skip, const float* s_skip,
                                                                const float* w_out, const float* s_out, __bf16* out) {
  const int n1 = K1 * BG, n2 = K2 * BG;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += gridDim.x * blockDim.x) {
    const bool p2 = i >= n1;
    const int e = p2 ? i - n1 : i;
    const int j = e & 7, row = (e >> 3) % BG, k = (e >> 3) / BG * 8 + j;
    float v = 0.f;
    if (!p2) {
      if (k < BK * BR) {
        const int tap = k / BR, ci = k % BR;
        v = w_dil[((long)row * BR + ci) * BK + tap] * (s_dil ? s_dil[row] : 1.f);
      } else if (k < BK * BR + BA) {
        v = w_aux[(long)row * BA + (k - BK * BR)] * (s_aux ? s_aux[row] : 1.f);
      }
    } else if (row < BS) {
      v = w_skip[(long)row * BR + k] * (s_skip ? s_skip[row] : 1.f);
    } else {
      v = w_out[(long)(row - BS) * BR + k] * (s_out ? s_out[row - BS] : 1.f);
    }
    out[i] = (__bf16)v;
  }
}

// the geometry of wavenet.hip's wavenet_ok, with the reason for a refusal in pwg_last_error
static int bf16_layer_check(const pwg_wavenet_desc* d) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "wavenet_bf16: NULL descriptor");
  PWG_REQUIRE(d->residual_channels == BR && d->gate_channels == BG && d->skip_channels == BS && d->kernel == BK,
              PWG_ERR_UNSUPPORTED,
              "wavenet_bf16: residual / gate / skip channels %d / %d / %d, kernel %d (built for 64 / 128 / 64, kernel 3)",
              d->residual_channels, d->gate_channels, d->skip_channels, d->kernel);
  PWG_REQUIRE(d->aux_channels == BA, PWG_ERR_UNSUPPORTED, "wavenet_bf16: aux_channels = %d (built for 80)",
              d->aux_channels);
  PWG_REQUIRE(!d->causal, PWG_ERR_UNSUPPORTED, "wavenet_bf16: causal layers are not built (symmetric padding only)");
  PWG_REQUIRE(d->batch >= 1 && d->batch <= 65535, PWG_ERR_UNSUPPORTED, "wavenet_bf16: batch = %d (1 .. 65535)", d->batch);
  PWG_REQUIRE(d->t >= 1 && d->dilation >= 1, PWG_ERR_BAD_SHAPE, "wavenet_bf16: t = %d, dilation = %d (>= 1)", d->t,
              d->dilation);
  PWG_REQUIRE((long)BG * d->t * 4 < (1L << 32), PWG_ERR_UNSUPPORTED, "wavenet_bf16: t = %d is too long", d->t);
  return PWG_OK;
}

// What the ragged forms ask beyond the plain ones (one rule for the fp32 and the bf16 layer: wavenet.hip's masked 16-B
// stores need an item to end on a multiple of 4 columns; pwg_wavenet_layer_ragged_supported)
static int bf16_ragged_check(const int32_t* frames, int rate) {
  PWG_REQUIRE(frames != nullptr, PWG_ERR_NULL, "wavenet_bf16_layer_forward_ragged: NULL frames table");
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 3u) == 0, PWG_ERR_BAD_SHAPE,
              "wavenet_bf16_layer_forward_ragged: the frames table must be 4-B aligned");
  PWG_REQUIRE(rate >= 4 && (rate & 3) == 0, PWG_ERR_UNSUPPORTED,
              "wavenet_bf16_layer_forward_ragged: rate = %d (a positive multiple of 4)", rate);
  return PWG_OK;
}

template <bool RAGGED>
static int bf16_layer_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                              const void* packed, const float* b_dil, const float* b_skip, const float* b_out, float* x_out,
                              float* skips_out, float* z_out, float* g_out, int mfma_shape, hipStream_t stream,
                              const int32_t* frames = nullptr, int rate = 0) {
  int rc = bf16_layer_check(d);
  if (rc != PWG_OK) return rc;
  if constexpr (RAGGED) {
    rc = bf16_ragged_check(frames, rate);
    if (rc != PWG_OK) return rc;
  }
  PWG_REQUIRE(x && c && packed && x_out && skips_out, PWG_ERR_NULL, "wavenet_bf16_layer_forward: NULL pointer");
  PWG_REQUIRE(x != x_out, PWG_ERR_BAD_SHAPE, "wavenet_bf16_layer_forward: x_out must not alias x (tiles read their neighbours' samples)");
  PWG_REQUIRE((z_out == nullptr) == (g_out == nullptr), PWG_ERR_BAD_SHAPE, "wavenet_bf16_layer_forward: z_out and g_out go together");
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(packed) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "wavenet_bf16_layer_forward: the weight image must be 16-B aligned");
  PWG_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(c)) & 3u) == 0, PWG_ERR_BAD_SHAPE,
              "wavenet_bf16_layer_forward: x and c must be 4-B aligned");
  PWG_REQUIRE(mfma_shape == 16 || mfma_shape == 32, PWG_ERR_BAD_SHAPE, "wavenet_bf16_layer_forward: mfma_shape = %d (16 or 32)",
              mfma_shape);
  WbArgsOf<RAGGED> a;
  a.x = x;
  a.c = c;
  a.skips = skips;
  a.w1 = static_cast<const bf16x8*>(packed);
  a.w2 = a.w1 + (size_t)OCT1 * BG;
  a.b_dil = b_dil;
  a.b_skip = b_skip;
  a.b_out = b_out;
  a.x_out = x_out;
  a.skips_out = skips_out;
  a.z_out = z_out;
  a.g_out = g_out;
  a.T = d->t;
  a.dil = d->dilation;
  a.out_mul = d->out_mul;
  a.skip_mul = d->skip_mul;
  if constexpr (RAGGED) a.frames = frames, a.rate = rate;
  // (the ragged form's figures are upper bounds: a tile past its item's end returns at once)
  const double samples = (double)d->batch * d->t;
  const double flops = 2.0 * samples * (BG * (double)(BK * BR + BA) + (double)(BS + BR) * BR);
  const double bytes = 4.0 * samples * (BR * 4 + BA + (skips ? BS : 0) + (z_out ? BG + BR : 0)) +
                       2.0 * (double)(K1 + K2) * BG;
  const dim3 grid(ceil_div(d->t, BCOLS), d->batch);
  maybe_poison_lds(stream);
  {
    ProfScope prof(stream, RAGGED ? "wavenet_bf16_layer_ragged_kernel" : "wavenet_bf16_layer_kernel", flops, bytes);
    if (mfma_shape == 32)
      hipLaunchKernelGGL((wavenet_bf16_layer_kernel<32, RAGGED>), grid, dim3(256), kLds, stream, a);
    else
      hipLaunchKernelGGL((wavenet_bf16_layer_kernel<16, RAGGED>), grid, dim3(256), kLds, stream, a);
  }
  PWG_CHECK_LAUNCH("wavenet_bf16_layer_forward");
  return PWG_OK;
}

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_wavenet_bf16_supported(const pwg_wavenet_desc* d) { return bf16_layer_check(d) == PWG_OK ? 1 : 0; }

extern "C" size_t pwg_wavenet_bf16_packed_weight_bytes(const pwg_wavenet_desc* d) {
  if (bf16_layer_check(d) != PWG_OK) return 0;
  return (size_t)(K1 + K2) * BG * sizeof(__bf16);
}

extern "C" int pwg_wavenet_bf16_pack_weights(const pwg_wavenet_desc* d, const float* w_dil, const float* scale_dil,
                                             const float* w_aux, const float* scale_aux, const float* w_skip,
                                             const float* scale_skip, const float* w_out, const float* scale_out,
                                             void* packed, void* stream) {
  int rc = bf16_layer_check(d);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(w_dil && w_aux && w_skip && w_out && packed, PWG_ERR_NULL, "wavenet_bf16_pack_weights: NULL pointer");
  const int total = (K1 + K2) * BG;
  hipLaunchKernelGGL(wavenet_bf16_pack_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, w_dil,
                     scale_dil, w_aux, scale_aux, w_skip, scale_skip, w_out, scale_out, static_cast<__bf16*>(packed));
  PWG_CHECK_LAUNCH("wavenet_bf16_pack_weights");
  return PWG_OK;
}

extern "C" int pwg_wavenet_bf16_layer_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                                              const void* packed, const float* b_dil, const float* b_skip,
                                              const float* b_out, float* x_out, float* skips_out, float* z_out,
                                              float* g_out, void* stream) {
  return bf16_layer_forward<false>(d, x, c, skips, packed, b_dil, b_skip, b_out, x_out, skips_out, z_out, g_out,
                                   kDefaultMfmaShape, (hipStream_t)stream);
}

extern "C" int pwg_wavenet_bf16_layer_forward_cfg(const pwg_wavenet_desc* d, const float* x, const float* c,
                                                  const float* skips, const void* packed, const float* b_dil,
                                                  const float* b_skip, const float* b_out, float* x_out, float* skips_out,
                                                  float* z_out, float* g_out, int32_t mfma_shape, void* stream) {
  return bf16_layer_forward<false>(d, x, c, skips, packed, b_dil, b_skip, b_out, x_out, skips_out, z_out, g_out,
                                   mfma_shape, (hipStream_t)stream);
}

extern "C" int pwg_wavenet_bf16_layer_forward_ragged(const pwg_wavenet_desc* d, const float* x, const float* c,
                                                     const float* skips, const void* packed, const float* b_dil,
                                                     const float* b_skip, const float* b_out, float* x_out,
                                                     float* skips_out, int32_t mfma_shape, const int32_t* frames,
                                                     int32_t rate, void* stream) {
  return bf16_layer_forward<true>(d, x, c, skips, packed, b_dil, b_skip, b_out, x_out, skips_out, nullptr, nullptr,
                                  mfma_shape == 0 ? kDefaultMfmaShape : mfma_shape, (hipStream_t)stream, frames, rate);
}
