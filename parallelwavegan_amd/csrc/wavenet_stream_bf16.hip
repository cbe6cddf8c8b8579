// wavenet_stream_bf16.hip -- the streaming forms of the gated Parallel WaveGAN layer (csrc/wavenet_stream.hip) with bf16
// operands: ONE launch per layer and chunk, computed the way wavenet_bf16_layer_kernel<32> (csrc/wavenet_bf16.hip)
// computes.  One kernel template over its argument struct, three instantiations:
//
//   causal   (WsbArgs)         X = concat(hist_in, x); taps X[n - 2d], X[n - d], X[n]; aux c[n]; residual x[n]
//   delayed  (WsbDelayedArgs)  the NON-causal layer of a look-ahead stream on a time axis shifted by d: the same taps,
//                              aux concat(c_line, c)[n - c_delay], residual X[n - d], skip addend
//                              concat(skip_line_in, skips)[n], zeros STORED outside [valid_lo, valid_hi)
//   slotted  (WsbSlotsArgs)    the delayed form with one position per item, read from the device table of
//                              stream_common.h (a pool of streams; csrc/wavenet_stream.hip)
//
//     z      = W_dil (*) bf16(X) + W_aux . bf16(C) + b_dil                 (128 rows; K = 3 * 64 + 80 = 272, padded to 288)
//     g      = bf16( tanh(z[:64]) * sigmoid(z[64:]) )                       (gate_fp32, then nearest-even)
//     skips' = (W_skip . g + b_skip + addend) * skip_mul
//     x'     = (W_out  . g + b_out  + residual) * out_mul
//
// Numerical definition: that of csrc/wavenet_bf16.hip, unchanged.  The image is that of pwg_wavenet_bf16_pack_weights
// (its K order tap 0, 1, 2, aux does not depend on causality); x and c windows are loaded as fp32 and rounded to bf16 on
// the way into LDS; accumulation, gate, biases, residual, skip addend, scales, tensors, history and lines are fp32.  The
// residual is the fp32 value re-read from memory (two-source in the delayed form), never the rounded copy.
//
// Staging: the register path of the whole-utterance kernel -- item (grp, oct) = 4 columns x 8 channels into the
// [column][channel] bf16 tile -- under the window rule of csrc/wavenet_stream.hip: tap window `tap` starts at
// chunk-relative column n0 + (tap - 2) d, the aux window at n0 - c_delay; columns < 0 come from the window's past source
// (hist_in[H + f], H = 2d; c_line[c_cols + f]; zeros where that is NULL), columns >= 0 from the chunk.  A group of 4
// columns wholly inside the chunk or wholly inside its past source is one 16-B load per channel at a 4-B aligned address;
// any other group goes per sample with range checks, zeros outside.  The fp32 value, hence the bf16 value, is the same
// through either path.  Everything a workgroup needs from memory is requested up front -- the staging loads, then the
// residual and the skip addend, then the first weight fragments -- and the biases sit in LDS.
//
// State: hist_out = the last H raw fp32 columns of X, skip_line_out = the last d raw columns of concat(skip_line_in,
// skips), both through stream_write_history<4> as in the fp32 kernel: the state a bf16 launch writes is bit for bit what
// the fp32 launch writes from the same inputs.
//
// Sum order: word for word that of wavenet_bf16_layer_kernel<32>.  One MFMA shape (32x32x16): the image's K order in one
// accumulator per output tile over 18 steps, then the K = 64 contraction over 4 steps, then
//     sv = acc + b_skip; sv += addend; sv *= skip_mul   (each step only when present)
//     xv = (acc + b_out + residual) * out_mul.
// One workgroup owns its 64 columns over the whole reduction: no split-K, no atomics.  The order is a function of the
// layer alone -- not of n, the batch, the chunk's position, c_delay or its alignment, or the staging path -- so any
// partition of a stream gives bit-identical results, and the delayed launch over a whole utterance gives the bits of the
// whole-utterance bf16 layer.  DESIGN.md s11.7.
#include "stream_common.h"
#include "wavenet_bf16.h"
#include "wavenet_stream.h"

#include <stdint.h>

#include <type_traits>

namespace pwg {
namespace {

struct WsbArgs {
  const float* x;        // (B, 64, n)
  const float* c;        // (B, 80, n)
  const float* skips;    // (B, 64, n) or NULL
  const float* hist_in;  // (B, 64, H) or NULL (start of stream)
  float* hist_out;       // (B, 64, H)
  const bf16x8* w1;      // [36][128] fragments
  const bf16x8* w2;      // [8][128] fragments
  const float* b_dil;    // (128) or NULL
  const float* b_skip;   // (64) or NULL
  const float* b_out;    // (64) or NULL
  float* x_out;          // (B, 64, n)
  float* skips_out;      // (B, 64, n) (causal form: may alias skips)
  float* z_out;          // (B, 128, n) or NULL
  float* g_out;          // (B, 64, n) or NULL
  int n, dil;
  float out_mul, skip_mul;
};

// What the delayed form adds (csrc/wavenet_stream.hip, WnDelayedArgs)
struct WsbDelayedArgs : WsbArgs {
  const float* c_line;        // (B, 80, c_cols) or NULL (zeros): the conditioning columns before this chunk
  const float* skip_line_in;  // (B, 64, d) or NULL (zeros)
  float* skip_line_out;       // (B, 64, d); unused without skips
  int c_cols, c_delay;        // 0 <= c_delay <= c_cols
  int valid_lo, valid_hi;     // output columns (chunk-relative)
};

// The slotted form (csrc/wavenet_stream.hip, WnSlotsArgs): one position per item, from the table
struct WsbSlotsArgs : WsbArgs {
  const float* c_line;        // (B, 80, c_cols) or NULL (zeros)
  const float* skip_line_in;  // (B, 64, d); required with skips
  float* skip_line_out;       // (B, 64, d); unused without skips
  int c_cols, c_delay;        // 0 <= c_delay <= c_cols
  const int32_t* slots;       // (B, kStreamSlotInts)
  int rate, out_delay;        // output columns per frame, delay of the output
};

template <class ARGS>
__global__ __launch_bounds__(256, 2) void wavenet_stream_bf16_kernel(ARGS a) {
  constexpr bool SLOTTED = std::is_same<ARGS, WsbSlotsArgs>::value;
  constexpr bool DELAYED = std::is_same<ARGS, WsbDelayedArgs>::value || SLOTTED;
  constexpr int TILE = 32;           // v_mfma_f32_32x32x16_bf16: a wave owns one 32 x 32 tile of each half
  constexpr int HL = 64 / TILE;      // lane groups along the reduction
  constexpr int KSTEP = 8 * HL;      // reduction elements per MFMA (16)
  constexpr int NS1 = K1 / KSTEP;    // phase-1 steps (18)
  constexpr int NS2 = K2 / KSTEP;    // phase-2 steps (4)
  constexpr int NREG = TILE * TILE / 64;
  constexpr int ITEMS = (OCT1 * BCOLS / 4 + 255) / 256;  // (column group of 4, channel octet) items per thread
  typedef Mfma<TILE>::acc_t acc_t;

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
  const int n = a.n, dil = a.dil;
  const int H = 2 * dil;
  const float* __restrict__ xb = a.x + (long)b * BR * n;
  const float* __restrict__ cb = a.c + (long)b * BA * n;
  // SLOTTED: what this item's table row resolves to -- fresh, paused and its own window
  [[maybe_unused]] StreamSlotItem item{};
  bool fresh = false;
  if constexpr (SLOTTED) {
    item = stream_slot_item(a.slots, b, a.rate, a.out_delay, n);
    fresh = item.fresh;
  }
  const float* __restrict__ hb = a.hist_in && !fresh ? a.hist_in + (long)b * BR * H : nullptr;
  // the aux window's past (delayed form): the conditioning line, L columns; the window starts c_delay columns early
  const float* __restrict__ lb = nullptr;
  // ... its skip line (all items'; NULL: zeros) and its valid window: the launch's, or the item's
  [[maybe_unused]] const float* __restrict__ sli = nullptr;
  [[maybe_unused]] int valid_lo = 0, valid_hi = 0;
  int L = 0, c_delay = 0;
  if constexpr (DELAYED) {
    L = a.c_cols;
    c_delay = a.c_delay;
    lb = a.c_line && !fresh ? a.c_line + (long)b * BA * L : nullptr;
    sli = fresh ? nullptr : a.skip_line_in;
    if constexpr (SLOTTED) {
      valid_lo = item.valid_lo;
      valid_hi = item.valid_hi;
    } else {
      valid_lo = a.valid_lo;
      valid_hi = a.valid_hi;
    }
  }
  if constexpr (SLOTTED) {
    if (item.paused) {  // (workgroup-uniform) state out = state in, zeros for both output tiles; in front of every barrier
      stream_write_history<4>(xb, hb, a.hist_out + (long)b * BR * H, BR, 0, H, false, blockIdx.x, gridDim.x);
      if (a.skips)
        stream_write_history<4>(a.skips + (long)b * BS * n, sli ? sli + (long)b * BS * dil : nullptr,
                                a.skip_line_out + (long)b * BS * dil, BS, 0, dil, false, blockIdx.x, gridDim.x);
      for (int e = tid; e < BR * BCOLS; e += 256) {
        const int row = e / BCOLS, j = n0 + (e - row * BCOLS);
        if (j >= n) continue;
        const long o = ((long)b * BR + row) * n + j;
        a.x_out[o] = 0.f;
        a.skips_out[o] = 0.f;
      }
      return;
    }
  }

  // accumulator element i: row h * 32 + rowin(i), column cn * 32 + r
  auto rowin = [&](int i) { return mfma_acc_row<TILE>(0, i, lg); };

  {
    const float* src = tid < BG ? a.b_dil : (tid < BG + BS ? a.b_skip : a.b_out);
    const int k = tid < BG ? tid : (tid < BG + BS ? tid - BG : tid - BG - BS);
    bias[tid] = src ? src[k] : 0.f;
  }

  // ---- stage: item (grp, oct) = 4 columns x 8 channels.  Octets 0..23: tap windows of X (tap = oct / 8), 24..33: the
  // aux rows, 34..35: zero padding.  The group's first column f is chunk-relative: f < 0 is the window's past source.
  // The epilogue's fp32 residual and skip addend are loaded right behind the staging loads (their latency hides under
  // the whole matrix work).
  const int col = cn * 32 + r;  // this lane's output column in the tile
  const int nc = n0 + col;      // ... and in the chunk
  float xres[NREG], sres[NREG];
  {
    f32x4 st[ITEMS][8];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
      const int idx = tid + it * 256, grp = idx & 15, oct = idx >> 4;
      // a wave's 64 items are 4 octets: the window's sources and its tap are wave-uniform (6 * 4 = the 24 octets of x),
      // and element offsets inside one item fit 32 bits (wavenet_stream_geometry)
      const int oct4 = __builtin_amdgcn_readfirstlane(idx >> 6);
      const bool is_x = oct4 < 6;
      const float* __restrict__ sb = is_x ? xb : cb;  // the chunk
      const float* __restrict__ pb = is_x ? hb : lb;  // the window's past source and its columns
      const int P = is_x ? H : L;
      const int ch0 = is_x ? (oct & 7) * 8 : min(oct - 24, 9) * 8;
      const int f = n0 + 4 * grp + (is_x ? ((oct4 >> 1) - 2) * dil : -c_delay);
      if (oct >= 34) {
#pragma unroll
        for (int j = 0; j < 8; ++j) st[it][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      } else if (f >= 0 && f + 4 <= n) {  // wholly inside the chunk
        const unsigned o = (unsigned)(ch0 * n + f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const f4u u = *reinterpret_cast<const f4u*>(sb + (o + (unsigned)(j * n)));
          st[it][j] = f32x4{u[0], u[1], u[2], u[3]};
        }
      } else if (pb != nullptr && f + 4 <= 0) {  // wholly inside the past source (f >= -P: no window starts before it)
        const unsigned o = (unsigned)(ch0 * P + P + f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const f4u u = *reinterpret_cast<const f4u*>(pb + (o + (unsigned)(j * P)));
          st[it][j] = f32x4{u[0], u[1], u[2], u[3]};
        }
      } else {
        // the group straddles past and chunk, leaves the chunk on the right, or is start-of-stream padding: per sample
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int fe = f + e;
            if (fe < 0) {
              if (pb) v[e] = pb[(unsigned)((ch0 + j) * P + P + fe)];
            } else if (fe < n) {
              v[e] = sb[(unsigned)((ch0 + j) * n + fe)];
            }
          }
          st[it][j] = v;
        }
      }
    }
    // This lane's column of the residual and of the skip addend; zeros where there is none.  Causal form: x[n] and
    // skips[n].  Delayed form, both two-source and d columns late: the middle tap concat(hist_in, x)[n - d], and
    // concat(skip_line_in, skips)[n] (the rule of stream_delayed_addend, stream_common.h).
#pragma unroll
    for (int i = 0; i < NREG; ++i) xres[i] = sres[i] = 0.f;
    if (nc < n) {
      const int row0 = h * 32;
      if constexpr (DELAYED) {
        const int j = nc - dil;
        if (j >= 0) {
          const float* __restrict__ kb = a.skips ? a.skips + (long)b * BS * n : nullptr;
#pragma unroll
          for (int i = 0; i < NREG; ++i) {
            const unsigned o = (unsigned)((row0 + rowin(i)) * n + j);
            xres[i] = xb[o];
            if (kb) sres[i] = kb[o];
          }
        } else {
          const float* __restrict__ kb = (a.skips && sli) ? sli + (long)b * BS * dil : nullptr;
#pragma unroll
          for (int i = 0; i < NREG; ++i) {
            const int row = row0 + rowin(i);
            if (hb) xres[i] = hb[(unsigned)(row * H + H + j)];
            if (kb) sres[i] = kb[(unsigned)(row * dil + nc)];
          }
        }
      } else {
        const float* __restrict__ kb = a.skips ? a.skips + (long)b * BS * n : nullptr;
#pragma unroll
        for (int i = 0; i < NREG; ++i) {
          const unsigned o = (unsigned)((row0 + rowin(i)) * n + nc);
          xres[i] = xb[o];
          if (kb) sres[i] = kb[o];
        }
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

  acc_t acc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < NREG; ++i) acc[s][i] = 0.f;

  // ---- phase 1: z rows of both halves over K = 288 (A: image fragments from L2, RING-deep register ring whose first
  // loads are in flight during the staging barrier; B: LDS)
  {
    const bf16x8* wp = a.w1 + lg * BG + h * 32 + r;  // + (ks * HL) * 128 + half * 64
    bf16x8 A[RING][2];
#pragma unroll
    for (int p = 0; p < RING - 1; ++p)
#pragma unroll
      for (int s = 0; s < 2; ++s) A[p][s] = wp[p * HL * BG + s * 64];
    __syncthreads();
    const __bf16* bl = xs + col * RS + 8 * lg;
#pragma unroll
    for (int ks = 0; ks < NS1; ++ks) {
      if (ks + RING - 1 < NS1) {
#pragma unroll
        for (int s = 0; s < 2; ++s) A[(ks + RING - 1) % RING][s] = wp[(ks + RING - 1) * HL * BG + s * 64];
      }
      const bf16x8 B = *reinterpret_cast<const bf16x8*>(bl + ks * KSTEP);
#pragma unroll
      for (int s = 0; s < 2; ++s) acc[s] = Mfma<TILE>::run(A[ks % RING][s], B, acc[s]);
    }
  }

  // ---- gate in fp32, rounded to bf16 into the gate tile; z / g to memory for the stage tests
  {
#pragma unroll
    for (int i4 = 0; i4 < NREG; i4 += 4) {
      bf16x4 gv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = h * 32 + rowin(i4 + e);
        const float zt = acc[0][i4 + e] + bias[row];
        const float zs = acc[1][i4 + e] + bias[BR + row];
        const __bf16 g = (__bf16)gate_fp32(zt, zs);
        gv[e] = g;
        if (a.z_out && nc < n) {
          a.z_out[((long)b * BG + row) * n + nc] = zt;
          a.z_out[((long)b * BG + BR + row) * n + nc] = zs;
          a.g_out[((long)b * BR + row) * n + nc] = (float)g;
        }
      }
      // (4 consecutive rows = 4 consecutive channels of the column: one 8-B store)
      *reinterpret_cast<bf16x4*>(gs + col * RG + h * 32 + rowin(i4)) = gv;
    }
#pragma unroll
    for (int i = 0; i < NREG; ++i) {
      acc[0][i] = 0.f;
      acc[1][i] = 0.f;
    }
  }

  // ---- phase 2: skip rows [32 h, +32) (half 0) and out rows [32 h, +32) (half 1) over K = 64 rows of g
  {
    const bf16x8* wp = a.w2 + lg * BG + h * 32 + r;
    bf16x8 A[NS2][2];
#pragma unroll
    for (int ks = 0; ks < NS2; ++ks)
#pragma unroll
      for (int s = 0; s < 2; ++s) A[ks][s] = wp[ks * HL * BG + s * 64];
    __syncthreads();
    const __bf16* bl = gs + col * RG + 8 * lg;
#pragma unroll
    for (int ks = 0; ks < NS2; ++ks) {
      const bf16x8 B = *reinterpret_cast<const bf16x8*>(bl + ks * KSTEP);
#pragma unroll
      for (int s = 0; s < 2; ++s) acc[s] = Mfma<TILE>::run(A[ks][s], B, acc[s]);
    }
  }

  // ---- epilogue (fp32): the residual and the skip addend are the fp32 values read from memory at the start; the
  // delayed form stores zeros outside the valid window
  if (nc < n) {
    bool valid = true;
    if constexpr (DELAYED) valid = nc >= valid_lo && nc < valid_hi;
#pragma unroll
    for (int i = 0; i < NREG; ++i) {
      const int row = h * 32 + rowin(i);
      const long o = ((long)b * BR + row) * n + nc;
      float sv = acc[0][i] + bias[BG + row];
      if (a.skips) sv += sres[i];
      if (a.skip_mul != 1.0f) sv *= a.skip_mul;
      const float xv = (acc[1][i] + bias[BG + BS + row] + xres[i]) * a.out_mul;
      a.skips_out[o] = valid ? sv : 0.f;
      a.x_out[o] = valid ? xv : 0.f;
    }
  }

  // ---- hist_out = last H columns of concat(hist_in, x), raw (start of stream: zeros)
  stream_write_history<4>(xb, hb, a.hist_out + (long)b * BR * H, BR, n, H, false, blockIdx.x, gridDim.x);
  // ---- delayed form: skip_line_out = last d columns of concat(skip_line_in, skips), raw
  if constexpr (DELAYED) {
    if (a.skips)
      stream_write_history<4>(a.skips + (long)b * BS * n, sli ? sli + (long)b * BS * dil : nullptr,
                              a.skip_line_out + (long)b * BS * dil, BS, n, dil, false, blockIdx.x, gridDim.x);
  }
}

// The argument fields the two forms share, behind the pointer rules of the fp32 forms
static int stream_bf16_fill(const char* name, WsbArgs* a, const pwg_wavenet_desc* d, const float* x, const float* c,
                            const float* skips, const float* hist_in, float* hist_out, const void* packed,
                            const float* b_dil, const float* b_skip, const float* b_out, float* x_out, float* skips_out,
                            float* z_out, float* g_out) {
  const int rc = wavenet_stream_pointers(name, x, c, hist_in, hist_out, packed, x_out, skips_out);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((z_out == nullptr) == (g_out == nullptr), PWG_ERR_BAD_SHAPE, "%s: z_out and g_out go together", name);
  a->x = x;
  a->c = c;
  a->skips = skips;
  a->hist_in = hist_in;
  a->hist_out = hist_out;
  a->w1 = static_cast<const bf16x8*>(packed);
  a->w2 = a->w1 + (size_t)OCT1 * BG;
  a->b_dil = b_dil;
  a->b_skip = b_skip;
  a->b_out = b_out;
  a->x_out = x_out;
  a->skips_out = skips_out;
  a->z_out = z_out;
  a->g_out = g_out;
  a->n = d->t;
  a->dil = d->dilation;
  a->out_mul = d->out_mul;
  a->skip_mul = d->skip_mul;
  return PWG_OK;
}

// state_floats: what the launch reads and writes besides the chunk (history; the delayed form's lines)
template <class ARGS>
static int stream_bf16_launch(const char* name, const char* kernel_name, const pwg_wavenet_desc* d, const ARGS& a,
                              double state_floats, hipStream_t stream) {
  const double samples = (double)d->batch * d->t;
  const double flops = 2.0 * samples * (BG * (double)(BK * BR + BA) + (double)(BS + BR) * BR);
  const double bytes = 4.0 * (samples * (BR * 4 + BA + (a.skips ? BS : 0) + (a.z_out ? BG + BR : 0)) + state_floats) +
                       2.0 * (double)(K1 + K2) * BG;
  maybe_poison_lds(stream);
  {
    ProfScope prof(stream, kernel_name, flops, bytes);
    hipLaunchKernelGGL(wavenet_stream_bf16_kernel<ARGS>, dim3(ceil_div(d->t, BCOLS), d->batch), dim3(256), kLds, stream, a);
  }
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_wavenet_stream_bf16_supported(const pwg_wavenet_desc* d) {
  return wavenet_stream_geometry(d) == PWG_OK ? 1 : 0;
}

extern "C" int pwg_wavenet_stream_bf16_forward(const pwg_wavenet_desc* d, const float* x, const float* c,
                                               const float* skips, const float* hist_in, float* hist_out,
                                               const void* packed, const float* b_dil, const float* b_skip,
                                               const float* b_out, float* x_out, float* skips_out, float* z_out,
                                               float* g_out, void* stream_) {
  const char* name = "wavenet_stream_bf16_forward";
  int rc = wavenet_stream_geometry(d);
  if (rc != PWG_OK) return rc;
  WsbArgs a;
  rc = stream_bf16_fill(name, &a, d, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, x_out, skips_out, z_out,
                        g_out);
  if (rc != PWG_OK) return rc;
  return stream_bf16_launch(name, "wavenet_stream_bf16_kernel", d, a, 2.0 * d->batch * BR * 2.0 * d->dilation,
                            (hipStream_t)stream_);
}

extern "C" int pwg_wavenet_stream_bf16_delayed_supported(const pwg_wavenet_desc* d, int32_t c_delay) {
  return wavenet_delayed_geometry(d, c_delay) == PWG_OK ? 1 : 0;
}

extern "C" int pwg_wavenet_stream_bf16_delayed_forward(const pwg_wavenet_desc* d, const float* x, const float* c,
                                                       const float* c_line, int32_t c_cols, int32_t c_delay,
                                                       const float* skips, const float* skip_line_in,
                                                       float* skip_line_out, const float* hist_in, float* hist_out,
                                                       const void* packed, const float* b_dil, const float* b_skip,
                                                       const float* b_out, int32_t valid_lo, int32_t valid_hi,
                                                       float* x_out, float* skips_out, float* z_out, float* g_out,
                                                       void* stream_) {
  const char* name = "wavenet_stream_bf16_delayed_forward";
  int rc = wavenet_delayed_geometry(d, c_delay);
  if (rc != PWG_OK) return rc;
  rc = wavenet_delayed_pointers(name, d, c_line, c_cols, c_delay, skips, skip_line_in, skip_line_out, skips_out);
  if (rc != PWG_OK) return rc;
  WsbDelayedArgs a;
  rc = stream_bf16_fill(name, &a, d, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, x_out, skips_out, z_out,
                        g_out);
  if (rc != PWG_OK) return rc;
  a.c_line = c_line;
  a.c_cols = c_line ? c_cols : 0;
  a.c_delay = c_delay;
  a.skip_line_in = skips ? skip_line_in : nullptr;
  a.skip_line_out = skips ? skip_line_out : nullptr;
  a.valid_lo = valid_lo;
  a.valid_hi = valid_hi;
  return stream_bf16_launch(name, "wavenet_stream_bf16_delayed_kernel", d, a,
                            (double)d->batch * (2.0 * BR * 2.0 * d->dilation + (skips ? 2.0 * BS * d->dilation : 0.0)),
                            (hipStream_t)stream_);
}

// The slotted form (pwg_wavenet_stream_slots_forward) under the numerical definition above; no z / g outputs
extern "C" int pwg_wavenet_stream_slots_forward_bf16(const pwg_wavenet_desc* d, const float* x, const float* c,
                                                     const float* c_line, int32_t c_cols, int32_t c_delay,
                                                     const float* skips, const float* skip_line_in, float* skip_line_out,
                                                     const float* hist_in, float* hist_out, const void* packed,
                                                     const float* b_dil, const float* b_skip, const float* b_out,
                                                     const int32_t* slots, int32_t rate, int32_t delay, float* x_out,
                                                     float* skips_out, void* stream_) {
  const char* name = "wavenet_stream_slots_forward_bf16";
  int rc = wavenet_delayed_geometry(d, c_delay);
  if (rc != PWG_OK) return rc;
  rc = wavenet_slots_pointers(name, d, c_delay, c_line, skips, skip_line_in, hist_in, slots, rate, delay);
  if (rc != PWG_OK) return rc;
  rc = wavenet_delayed_pointers(name, d, c_line, c_cols, c_delay, skips, skip_line_in, skip_line_out, skips_out);
  if (rc != PWG_OK) return rc;
  WsbSlotsArgs a;
  rc = stream_bf16_fill(name, &a, d, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, x_out, skips_out, nullptr,
                        nullptr);
  if (rc != PWG_OK) return rc;
  a.c_line = c_line;
  a.c_cols = c_line ? c_cols : 0;
  a.c_delay = c_delay;
  a.skip_line_in = skips ? skip_line_in : nullptr;
  a.skip_line_out = skips ? skip_line_out : nullptr;
  a.slots = slots;
  a.rate = rate;
  a.out_delay = delay;
  return stream_bf16_launch(name, "wavenet_stream_bf16_slots_kernel", d, a,
                            (double)d->batch * (2.0 * BR * 2.0 * d->dilation + (skips ? 2.0 * BS * d->dilation : 0.0)),
                            (hipStream_t)stream_);
}
