// resunit_split.hip -- one HiFi-GAN MRF residual unit as ONE launch on the gfx950 bf16 MFMA instructions, operands split
// three ways (inference, C = 32 / 64):
//
//     y = ( x + conv_{k,1}( lrelu( conv_{k,d}( lrelu(x) ) + b1 ) ) + b2  [+ add2] ) [/ out_div]
//
// and the single-convolution form y = ( x + conv_{k,d}(lrelu(x)) + b1 [+ add2] ) [/ out_div].  The structure is that of
// resunit.hip (all channels of a column tile and the intermediate h resident in LDS, 2 HBM passes), the arithmetic that
// of conv1d_split.hip, applied twice.
//
// Numerical definition (include/pwg_kernels.h, "split-operand residual unit"): lrelu(x) is formed in fp32 and split with
// split3 while the window is staged; the effective weights are split once by pwg_conv1d_split_pack_weight (the same
// image); per operand pair the products lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (weight part . input part) go, in
// this order, into one fp32 accumulator set (split_product of mfma_conv.h owns the order, for this kernel and for
// conv1d_split.hip); h = lrelu(acc + b1) is formed in fp32, is zero outside [0, T) and is split with split3; the
// residual is the raw fp32 x and the epilogue is acc + bias + x + add2, then / out_div.
// The accumulation order of an output element is the split kernel's: 32-channel chunk, tap, reduction step, product.  A
// unit is therefore bit-identical to two chained pwg_conv1d_split_forward_cfg launches at the same MFMA shape (conv1 with
// pre_act = post_act = leaky and bias b1; conv2 with bias b2, add1 = x, add2, out_div): that chain is the test oracle.
// Built without FMA contraction for the reason given in build.py for conv1d_split.hip.
//
// Tile: 4 waves, each 32 channels x 64 columns; C = 32: 256 h-columns per workgroup, C = 64: 128 (2 x 2 waves).  A tile
// of H h-columns yields (H - (k - 1)) & ~3 outputs (the halo is recomputed), H in the single form.
// LDS: three bf16 planes [column][C + 8] of the activated x window (rows of 80 B / 144 B: an odd number of 16-B slots);
// after phase 1 and a barrier the h planes take their place.  At k = 11, d = 5: 75 KB (C = 32) / 80 KB (C = 64), two
// workgroups per CU.
//   phase 1 (pair)   weight fragment first: a lane owns 4 consecutive channels of a column, each part of h is one 8-B
//                    LDS write per 4 accumulator registers
//   phase 2 / single x (h) fragment first: the transposed tile, a lane owns 4 consecutive samples of a channel and the
//                    epilogue reads x / add2 and writes y with 16-B accesses straight from the accumulators
// The operand order changes neither the products nor their summation order.  The residual x is read from global memory
// a second time (an fp32 copy in LDS would cost the second workgroup per CU), but behind the staging loads that fetch
// the same lines and into registers the two-wave occupancy leaves idle; add2 likewise ahead of the last contraction.
// Deterministic: one workgroup owns an output tile, no atomics.
// resblock_split_kernel, further down, chains up to three pair-form units in one launch from the same pieces.
#include "mfma_conv.h"

#include <stdlib.h>

#include <type_traits>

namespace pwg {
namespace {

constexpr size_t kRuSplitMaxLds = 80 * 1024;  // two workgroups per 160 KB CU

struct RuSplitArgs {
  const float* x;
  const bf16x8* w1;  // three-part image of pwg_conv1d_split_pack_weight
  const float* b1;
  const bf16x8* w2;  // nullptr: single convolution
  const float* b2;
  const float* add2;
  float* y;
  int T, k, d1;
  int bn_out;  // outputs per tile (multiple of 4)
  int hla;     // staged column of output slot 0 at the centre tap (left halo rounded up to a multiple of 4)
  int sh;      // hla - (true left halo)
  int p2;      // (k - 1) / 2 in pair mode, 0 otherwise
  int rows;    // staged columns = LDS rows of a plane (multiple of 4)
  int plane;   // bf16 elements per LDS plane
  long part_stride;  // bf16x8 elements per weight part image
  float slope1, slope2, out_div;
};

// The ragged form: item b ends at column Tv = min(frames[b] * rate, T); T stays the row stride.
struct RuSplitRaggedArgs : RuSplitArgs {
  const int* frames;  // (batch,) device table, frames per item
  int rate;           // columns per frame (a multiple of 4: Tv is one)
};
template <bool RAGGED>
using RuSplitArgsOf = typename std::conditional<RAGGED, RuSplitRaggedArgs, RuSplitArgs>::type;

template <int C>
struct RuSplitCfg {
  static constexpr int MB = C / KC;       // 32-row blocks = waves along the channels
  static constexpr int WAVES_N = 4 / MB;  // waves along the columns
  static constexpr int H = WAVES_N * 64;  // h-columns / output slots per workgroup
  static constexpr int ROW = C + 8;       // bf16 elements per LDS row
  static constexpr int OCTS = C / 8;
  static constexpr int CHUNKS = image_chunks(C), M_PAD = image_m_pad(C);  // the image of a C -> C convolution
};

// Stage the whole C-channel window: item = (group of 4 columns, channel octet), at most two per thread: 8 loads of 16 B
// (one per channel, along t), then per column 8 channels are activated, split and written as three 16-B LDS stores.
// T % 4 == 0 and the first staged column is a multiple of 4: a group lies inside the row or outside it.  CHECKED (first
// / last tiles of a row): a group outside [0, T) gives zeros = the zero padding of conv1: it reads a clamped, always
// valid address and is zeroed by a select (conv1d_split.hip, stage_window_vec).  behind() runs between the
// window's loads and its LDS stores: what it requests is in flight while the window is activated and split.
template <int C, bool CHECKED, typename Behind>
__device__ __forceinline__ void ru_stage_window(const RuSplitArgs& a, const float* __restrict__ xb, int base, __bf16* xs,
                                                int tid, Behind&& behind) {
  constexpr int OCTS = RuSplitCfg<C>::OCTS, ROW = RuSplitCfg<C>::ROW;
  const int nitems = (a.rows >> 2) * OCTS;
  const SplitActLeaky act{a.slope1};  // 0 < slope < 1 (ru_split_geometry)
  f32x4 st[2][8];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + it * 256, oct = idx % OCTS, grp = idx / OCTS;
    const int t = base + grp * 4;
    const bool in = idx < nitems && (!CHECKED || (t >= 0 && t < a.T));
    if (!CHECKED) {
      const float* __restrict__ src = xb + (size_t)(oct * 8) * a.T + t;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (in) v = *reinterpret_cast<const f32x4*>(src + (size_t)j * a.T);
        st[it][j] = v;
      }
    } else {
      const float* __restrict__ src = xb + (size_t)(oct * 8) * a.T + min(max(t, 0), a.T - 4);  // T % 4 == 0, T >= 4
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)j * a.T);
        st[it][j] = in ? v : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  behind();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + it * 256, oct = idx % OCTS, grp = idx / OCTS;
    if (idx < nitems) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = act(st[it][j][e]);
        split3_store<8>(v, xs + (grp * 4 + e) * ROW + oct * 8, a.plane);
        __builtin_amdgcn_sched_barrier(0);  // one column at a time (conv1d_split.hip, stage_window_vec)
      }
    }
  }
}

// acc += W (*) B over (chunk, tap, reduction step): the step sequence of conv1d_split_mfma_kernel around the streamed form
// of the step (split_step_streamed, mfma_conv.h: the product order the two kernels share); the weight fragments run a
// row tile ahead across taps and chunks.  w: the part-0 image; wrow: this lane's weight row; wf: row tile 0 of the first
// step, requested by the caller (ru_request) ahead of whatever it has to wait for; bl: plane 0 at this lane's column of
// tile 0, tap 0; tap_step: columns per tap.  XFIRST: the B fragment is the first MFMA operand (transposed tile).
template <int C, int TILE>
__device__ __forceinline__ void ru_request(bf16x8 (&wf)[3], const bf16x8* __restrict__ w, long part_stride, unsigned wrow,
                                           int h) {
  using Cfg = RuSplitCfg<C>;
  split_step_request(wf, w, part_stride, wrow + split_step_rows<TILE>(Cfg::CHUNKS, Cfg::M_PAD, SplitStepId{0, 0, 0}, h));
}
template <int C, int TILE, bool XFIRST>
__device__ __forceinline__ void ru_contract(bf16x8 (&wf)[3], const bf16x8* __restrict__ w, long part_stride, unsigned wrow,
                                            const __bf16* bl, int plane, int tap_step, int taps, int h,
                                            typename Mfma<TILE>::acc_t (&acc)[32 / TILE][64 / TILE]) {
  using Cfg = RuSplitCfg<C>;
  constexpr int HL = 64 / TILE, KSTEPS = KC / (8 * HL), TM = 32 / TILE, TN = 64 / TILE;
  SplitStepId step{0, 0, 0};
#pragma unroll 1
  for (int s = 0; s < Cfg::CHUNKS * taps * KSTEPS; ++s) {
    const SplitStepId next = split_step_successor(step, Cfg::CHUNKS, taps, KSTEPS);
    split_step_streamed<TILE, TM, TN, Cfg::ROW, XFIRST>(
        wf, w, part_stride, wrow + split_step_rows<TILE>(Cfg::CHUNKS, Cfg::M_PAD, step, h),
        wrow + split_step_rows<TILE>(Cfg::CHUNKS, Cfg::M_PAD, next, h), bl, step.tap * tap_step,
        step.chunk * KC + split_step_off<TILE>(step, h), plane, acc);
    step = next;
  }
}

// Output slot of value n (0 .. TN * NG - 1) of a lane of group h in the transposed tile of phase 2 / the single form
template <int TILE>
__device__ __forceinline__ int ru_out_slot(int wave_n, int h, int n) {
  constexpr int HL = 64 / TILE, NG = TILE * TILE / 256;
  return wave_n * 64 + (n / NG) * TILE + 4 * h + 4 * HL * (n % NG);
}

// RAGGED: x and add2 are zero at the columns >= Tv of their item (the invariant of a ragged forward), so the staging is
// the plain form's; h is zero outside [0, Tv), the values at columns in [Tv, T) are stored as zeros, and a workgroup
// whose tile lies at or beyond Tv stores its zeros and returns before it requests or stages anything.  The columns
// below Tv are formed by the plain form's operations on the plain form's operands: bit for bit the item run alone.
template <int C, int TILE, bool RAGGED>
__global__ __launch_bounds__(256, 2) void resunit_split_kernel(RuSplitArgsOf<RAGGED> a) {
  using Cfg = RuSplitCfg<C>;
  constexpr int WAVES_N = Cfg::WAVES_N, ROW = Cfg::ROW, H = Cfg::H;
  constexpr int HL = 64 / TILE, TM = 32 / TILE, TN = 64 / TILE, NREG = TILE * TILE / 64, NG = NREG / 4;
  typedef typename Mfma<TILE>::acc_t acc_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [part][column][ROW]: activated x, then h

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / WAVES_N, wave_n = wave % WAVES_N;
  const int r = lane & (TILE - 1), h = lane / TILE;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * a.bn_out;  // first output sample of this tile
  const int base = t0 - a.hla;           // sample of staged column 0 (a multiple of 4, also when negative)
  const int T = a.T;
  const bool pair = a.w2 != nullptr;
  const float* __restrict__ xb = a.x + (size_t)b * C * T;
  int Tv = T;  // end of the item: what h and the stored values are masked at
  if constexpr (RAGGED) {
    const long end = (long)a.frames[b] * a.rate;  // (read once per workgroup; wave-uniform)
    Tv = end < 0 ? 0 : end < T ? (int)end : T;
    if (t0 >= Tv) {
      const int quads = (T - t0 < a.bn_out ? T - t0 : a.bn_out) >> 2;  // t0 < T: the grid covers [0, T)
      for (int i = tid; i < C * quads; i += 256)
        *reinterpret_cast<f32x4*>(a.y + ((size_t)b * C + i / quads) * T + t0 + 4 * (i % quads)) = f32x4{0.f, 0.f, 0.f, 0.f};
      return;
    }
  }

  // the weight fragments run a row tile ahead of their MFMAs: the first ones of w1 are requested in front of the staging
  const unsigned wrow = wave_m * 32 + r;  // this lane's weight row of tile mi = 0
  bf16x8 wf[3];
  ru_request<C, TILE>(wf, a.w1, a.part_stride, wrow, h);

  // The epilogue's terms that no accumulator feeds -- the raw-x residual and add2 of the lane's own output values (the
  // transposed tile described at the epilogue) -- are requested ahead of the contractions and held in registers: LDS,
  // not registers, sets the two waves per SIMD.  The residual goes out behind the window's loads, which fetch the same
  // lines; add2 behind it in the single form, behind phase 1 in the pair form.  A value that is not stored reads the
  // tile's first samples (ok / t of the epilogue): no address outside the row.
  constexpr int NV = TN * NG;
  const bool has2 = a.add2 != nullptr;
  f32x4 res[TM][NV], ad2[TM][NV];
  auto request_values = [&](const float* __restrict__ src, f32x4 (&dst)[TM][NV]) {
    __builtin_amdgcn_sched_barrier(0);  // behind what was requested before, and not sunk to the epilogue
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      const float* __restrict__ rowp = src + ((size_t)b * C + wave_m * 32 + mi * TILE + r) * T;
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        const int slot = ru_out_slot<TILE>(wave_n, h, n);
        const bool ok = slot < a.bn_out && t0 + slot < T;
        dst[mi][n] = *reinterpret_cast<const f32x4*>(rowp + (ok ? t0 + slot : t0));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int n = 0; n < NV; ++n) ad2[mi][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the biases too: b1 of the lane's 4 consecutive channels per (mi, g) where h is formed, the epilogue's per row tile
  const float* __restrict__ bias_p = pair ? a.b2 : a.b1;
  const bool has_b1 = a.b1 != nullptr, has_bias = bias_p != nullptr;
  f32x4 bias_h[TM][NG];
  float bias_y[TM];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
    bias_y[mi] = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) bias_h[mi][g] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  auto behind_window = [&] {
    request_values(a.x, res);
    if (!pair && has2) request_values(a.add2, ad2);
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      if (has_bias) bias_y[mi] = bias_p[wave_m * 32 + mi * TILE + r];
      if (pair && has_b1) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) bias_h[mi][g][e] = a.b1[wave_m * 32 + mi * TILE + 4 * h + 4 * HL * g + e];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  if (base >= 0 && base + a.rows <= T)
    ru_stage_window<C, false>(a, xb, base, xs, tid, behind_window);
  else
    ru_stage_window<C, true>(a, xb, base, xs, tid, behind_window);

  acc_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < NREG; ++i) acc[mi][ni][i] = 0.f;
  __syncthreads();

  if (pair) {
    // ---- phase 1: conv_{k,d} over lrelu(x); h column m reads staged column m + sh + tap * d
    ru_contract<C, TILE, false>(wf, a.w1, a.part_stride, wrow, xs + (wave_n * 64 + r + a.sh) * ROW, a.plane, a.d1, a.k,
                                h, acc);
    ru_request<C, TILE>(wf, a.w2, a.part_stride, wrow, h);  // lands behind the forming of h and both barriers
    if (has2) request_values(a.add2, ad2);                  // (so does add2)
    __syncthreads();  // every wave has read its x columns: the h planes take their place
    // h = lrelu(acc + b1), zero outside [0, Tv) (conv2's zero padding; Tv = T in the plain form), split: a lane owns
    // channels c .. c + 3 of a column
    const SplitActLeaky act2{a.slope2};
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int c = wave_m * 32 + mi * TILE + 4 * h + 4 * HL * g;
        const f32x4 bias = bias_h[mi][g];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int m = wave_n * 64 + ni * TILE + r;
          const int th = t0 - a.p2 + m;
          const bool inside = th >= 0 && th < Tv;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = acc[mi][ni][4 * g + e];
            if (has_b1) v[e] += bias[e];
            v[e] = act2(v[e]);
            v[e] = inside ? v[e] : 0.f;
            acc[mi][ni][4 * g + e] = 0.f;
          }
          split3_store<4>(v, xs + m * ROW + c, a.plane);
        }
      }
    // h columns H .. H + k - 2 feed only the discarded output slots past bn_out: zeros, not what x left there
    for (int i = tid; i < (a.k - 1) * Cfg::OCTS; i += 256) {
      bf16x8 z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
      __bf16* dst = xs + (H + i / Cfg::OCTS) * ROW + (i % Cfg::OCTS) * 8;
      *reinterpret_cast<bf16x8*>(dst) = z;
      *reinterpret_cast<bf16x8*>(dst + a.plane) = z;
      *reinterpret_cast<bf16x8*>(dst + 2 * a.plane) = z;
    }
    __syncthreads();
    // ---- phase 2: conv_{k,1} over h; output slot n reads h column n + tap
    ru_contract<C, TILE, true>(wf, a.w2, a.part_stride, wrow, xs + (wave_n * 64 + r) * ROW, a.plane, 1, a.k, h,
                               acc);
  } else {
    ru_contract<C, TILE, true>(wf, a.w1, a.part_stride, wrow, xs + (wave_n * 64 + r + a.sh) * ROW, a.plane, a.d1, a.k,
                               h, acc);
  }

  // ---- epilogue (fp32, the order of split_epilogue: acc + bias + x + add2, then / out_div).  Transposed tile: a lane
  // owns channel c per mi and, per accumulator, NG values of 4 consecutive samples; value g of tile ni is output slot
  // wave_n * 64 + ni * TILE + 4 * h + 4 * HL * g.  bn_out, t0 and T are multiples of 4: a value is stored whole or not
  // at all; the loads of a value that is not stored read the tile's first samples instead.  x and add2 are the
  // registers requested ahead of the contractions (res, ad2): the epilogue waits for no memory.
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
    const int c = wave_m * 32 + mi * TILE + r;
    const size_t row = ((size_t)b * C + c) * T;
    int t[NV];
    bool ok[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int slot = ru_out_slot<TILE>(wave_n, h, n);
      ok[n] = slot < a.bn_out && t0 + slot < T;
      t[n] = ok[n] ? t0 + slot : t0;
    }
    const f32x4(&t1)[NV] = res[mi];
    const f32x4(&t2)[NV] = ad2[mi];
    f32x4 v[NV];
    const float bias = bias_y[mi];
#pragma unroll
    for (int n = 0; n < NV; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[n][e] = acc[mi][n / NG][(n % NG) * 4 + e];
    if (has_bias) {
#pragma unroll
      for (int n = 0; n < NV; ++n) v[n] += bias;
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) v[n] += t1[n];
    if (has2) {
#pragma unroll
      for (int n = 0; n < NV; ++n) v[n] += t2[n];
    }
    if (a.out_div != 1.0f) {
#pragma unroll
      for (int n = 0; n < NV; ++n) v[n] = v[n] / a.out_div;
    }
    if constexpr (RAGGED) {  // Tv is a multiple of 4 (or T): a value lies inside the item or outside it
#pragma unroll
      for (int n = 0; n < NV; ++n)
        if (t[n] >= Tv) v[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int n = 0; n < NV; ++n)
      if (ok[n]) *reinterpret_cast<f32x4*>(a.y + row + t[n]) = v[n];
  }
}

struct RuSplitGeom {
  int hla, sh, p2, bn_out, rows, tiles;
  size_t lds;
};

// Coverage: that of resunit_geometry (resunit.hip) plus what the planes need.  Pure host logic.
static int ru_split_geometry(const pwg_resunit_desc* d, RuSplitGeom* g) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "resunit_split: NULL descriptor");
  const int C = d->channels;
  PWG_REQUIRE(C == 32 || C == 64, PWG_ERR_UNSUPPORTED, "resunit_split: channels = %d (only 32 and 64)", C);
  PWG_REQUIRE(d->kernel >= 1 && (d->kernel & 1) == 1, PWG_ERR_UNSUPPORTED, "resunit_split: kernel = %d (only odd sizes)",
              d->kernel);
  PWG_REQUIRE(d->dilation >= 1, PWG_ERR_UNSUPPORTED, "resunit_split: dilation = %d", d->dilation);
  PWG_REQUIRE(d->batch >= 1 && d->batch <= 65535, PWG_ERR_UNSUPPORTED, "resunit_split: batch = %d (1 .. 65535)", d->batch);
  PWG_REQUIRE(d->t >= 4 && (d->t & 3) == 0, PWG_ERR_UNSUPPORTED, "resunit_split: t = %d (a positive multiple of 4)", d->t);
  PWG_REQUIRE(d->slope1 > 0.f && d->slope1 < 1.f, PWG_ERR_UNSUPPORTED, "resunit_split: slope1 = %g (0 < slope < 1)",
              (double)d->slope1);
  PWG_REQUIRE(!d->has_conv2 || (d->slope2 > 0.f && d->slope2 < 1.f), PWG_ERR_UNSUPPORTED,
              "resunit_split: slope2 = %g (0 < slope < 1)", (double)d->slope2);
  const int k = d->kernel, H = C == 32 ? RuSplitCfg<32>::H : RuSplitCfg<64>::H;
  PWG_REQUIRE((long)(k - 1) * d->dilation < (1 << 20), PWG_ERR_UNSUPPORTED, "resunit_split: receptive field too long");
  g->p2 = d->has_conv2 ? (k - 1) / 2 : 0;
  const int hl = (k - 1) / 2 * d->dilation + g->p2;
  g->hla = round_up(hl, 4);
  g->sh = g->hla - hl;
  g->bn_out = d->has_conv2 ? ((H - (k - 1)) & ~3) : H;
  PWG_REQUIRE(g->bn_out >= 64, PWG_ERR_UNSUPPORTED, "resunit_split: kernel = %d leaves %d outputs per tile", k, g->bn_out);
  g->rows = round_up(H + (k - 1) * d->dilation + g->sh, 4);
  g->lds = (size_t)3 * g->rows * (C + 8) * sizeof(__bf16);
  // (two staging items per thread cover every window that fits)
  PWG_REQUIRE(g->lds <= kRuSplitMaxLds && (g->rows / 4) * (C / 8) <= 512, PWG_ERR_UNSUPPORTED,
              "resunit_split: the window (kernel %d, dilation %d) needs %zu B of LDS", k, d->dilation, g->lds);
  g->tiles = ceil_div(d->t, g->bn_out);
  return PWG_OK;
}

template <bool RAGGED>
static int ru_split_forward(const pwg_resunit_desc* d, const float* x, const void* w1, const float* b1, const void* w2,
                            const float* b2, const float* add2, float* y, int mfma_shape, hipStream_t stream,
                            const int32_t* frames = nullptr, int rate = 0) {
  RuSplitGeom g;
  const int rc = ru_split_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(x && w1 && y, PWG_ERR_NULL, "resunit_split_forward: NULL pointer");
  PWG_REQUIRE(x != y, PWG_ERR_BAD_SHAPE, "resunit_split_forward: y must not alias x (tiles read their neighbours' halo)");
  PWG_REQUIRE((d->has_conv2 != 0) == (w2 != nullptr), PWG_ERR_BAD_SHAPE,
              "resunit_split_forward: has_conv2 = %d but w2_packed is %s", d->has_conv2, w2 ? "given" : "NULL");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  PWG_REQUIRE(al16(x) && al16(y) && al16(add2), PWG_ERR_BAD_SHAPE,
              "resunit_split_forward: x / y / add2 must be 16-B aligned");
  PWG_REQUIRE(al16(w1) && al16(w2), PWG_ERR_BAD_SHAPE, "resunit_split_forward: the weight images must be 16-B aligned");
  PWG_REQUIRE(mfma_shape == 16 || mfma_shape == 32, PWG_ERR_BAD_SHAPE, "resunit_split_forward: mfma_shape = %d (16 or 32)",
              mfma_shape);
  const int C = d->channels;
  RuSplitArgsOf<RAGGED> a;
  a.x = x;
  a.w1 = static_cast<const bf16x8*>(w1);
  a.b1 = b1;
  a.w2 = static_cast<const bf16x8*>(w2);
  a.b2 = b2;
  a.add2 = add2;
  a.y = y;
  a.T = d->t, a.k = d->kernel, a.d1 = d->dilation;
  a.bn_out = g.bn_out, a.hla = g.hla, a.sh = g.sh, a.p2 = g.p2, a.rows = g.rows;
  a.plane = g.rows * (C + 8);
  a.part_stride = image_elems(d->kernel, image_chunks(C), image_m_pad(C)) / 8;  // of the image RuSplitCfg<C> describes
  // (a window that fits LDS has a few hundred taps: the 32-bit fragment index of split_step_request always holds)
  PWG_REQUIRE(split_image_addressable(a.part_stride * 8), PWG_ERR_UNSUPPORTED, "resunit_split_forward: weight image too large");
  a.slope1 = d->slope1, a.slope2 = d->slope2, a.out_div = d->out_div;
  if constexpr (RAGGED) a.frames = frames, a.rate = rate;
  void (*kern)(RuSplitArgsOf<RAGGED>) =
      C == 32 ? (mfma_shape == 32 ? resunit_split_kernel<32, 32, RAGGED> : resunit_split_kernel<32, 16, RAGGED>)
              : (mfma_shape == 32 ? resunit_split_kernel<64, 32, RAGGED> : resunit_split_kernel<64, 16, RAGGED>);
  if (g.lds > kConvMaxLds && !lds_limit_is_set(reinterpret_cast<const void*>(kern), g.lds)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)g.lds);
    PWG_REQUIRE(e == hipSuccess, PWG_ERR_LAUNCH, "resunit_split_forward: cannot raise LDS limit to %zu: %s", g.lds,
                hipGetErrorString(e));
  }
  // the ALGORITHMIC flops and bytes of the unit (those of resunit_forward), whatever the number of part products
  const double elems = (double)d->batch * C * d->t;
  const double flops = 2.0 * elems * C * d->kernel * (d->has_conv2 ? 2 : 1);
  const double bytes = 4.0 * (elems * (2 + (add2 != nullptr)) + (d->has_conv2 ? 2 : 1) * (double)C * C * d->kernel);
  maybe_poison_lds(stream);
  {
    ProfScope prof(stream,
                   RAGGED ? prof_shape_name("resunit_split_ragged_kernel",
                                            "resunit_split_ragged_kernel B%d C%d T%d k%d d%d pair%d", d->batch, C, d->t,
                                            d->kernel, d->dilation, d->has_conv2)
                          : prof_shape_name("resunit_split_kernel", "resunit_split_kernel B%d C%d T%d k%d d%d pair%d",
                                            d->batch, C, d->t, d->kernel, d->dilation, d->has_conv2),
                   flops, bytes);
    hipLaunchKernelGGL(kern, dim3(g.tiles, d->batch), dim3(256), g.lds, stream, a);
  }
  PWG_CHECK_LAUNCH("resunit_split_forward");
  return PWG_OK;
}

// MFMA shape of pwg_resunit_split_forward
constexpr int kDefaultMfmaShape = 16;

// What the ragged form asks beyond the plain one: a value of four samples is stored whole or as zeros
static int ru_split_ragged_rate(int rate) {
  PWG_REQUIRE(rate > 0 && (rate & 3) == 0, PWG_ERR_UNSUPPORTED,
              "resunit_split_ragged: rate = %d (a positive multiple of 4: an item ends between two values of four samples)",
              rate);
  return PWG_OK;
}

// ---- A chain of N <= 3 pair-form units as ONE launch (resblock_split_kernel; DESIGN.md s9.2, "the chained block") ----
// Numerical definition: N chained pwg_resunit_split_forward_cfg launches at the same MFMA shape -- units 0 .. N - 2 with
// add2 = NULL and out_div = 1, the last with the block's; between units y_u = acc + b2 + x_u is formed in fp32 in that
// order, is zero outside [0, T), and is activated with the next unit's slope1 and split with split3, which is what the
// next launch would do to the stored tensor.  That chain is the test oracle, bit for bit.
// Fixed frame: every phase of every unit computes the same H absolute columns f0 .. f0 + H - 1; frame column m is plane
// row margin + m and a tap reads row margin + m + (tap - (k - 1) / 2) * d.  The margin rows ((k - 1) / 2 * max d on each
// side) are zeroed once and never written, so a column near the frame's edge is computed from a truncated window: it is
// wrong, finite or not, and it is never an input of a column that is stored -- validity shrinks by (k - 1) / 2 * (d_u + 1)
// columns per unit and side, the frame's `edge` is the sum over the units (rounded up to a multiple of 4: f0 = t0 - edge
// stays 16-B aligned and the staging needs no halo loads), and only the central bn_out = H - 2 * edge columns are stored.
// Registers: output slot -> absolute column is the same map in every unit (ru_out_slot), so the residual of unit u + 1 is
// the y_u this lane just formed: it stays in `res`.  x is read once for the planes and once for `res`, add2 once (behind
// the last unit's phase 1), y is written once.
// LDS: lrelu(y_u) goes from the transposed tile of phase 2 (a lane owns 4 consecutive samples of a channel) to the
// [column][channel] planes as 2-byte writes, 3 parts x 4 samples per value.
constexpr int kRbMaxUnits = 3;

struct RbSplitArgs {
  RuSplitArgs u;  // x, add2, y, T, k, plane, part_stride, bn_out, out_div; rows = H, slope1 = unit 0's: what the staging reads
  const bf16x8* w1[kRbMaxUnits];
  const bf16x8* w2[kRbMaxUnits];
  const float* b1[kRbMaxUnits];
  const float* b2[kRbMaxUnits];
  int d[kRbMaxUnits];
  float slope1[kRbMaxUnits], slope2[kRbMaxUnits];
  int n_units;
  int margin;  // zero rows on each side of a plane
  int edge;    // frame columns in front of output slot 0 (a multiple of 4)
};

template <int C, int TILE>
__global__ __launch_bounds__(256, 2) void resblock_split_kernel(RbSplitArgs a) {
  using Cfg = RuSplitCfg<C>;
  constexpr int WAVES_N = Cfg::WAVES_N, ROW = Cfg::ROW, H = Cfg::H;
  constexpr int HL = 64 / TILE, TM = 32 / TILE, TN = 64 / TILE, NREG = TILE * TILE / 64, NG = NREG / 4;
  typedef typename Mfma<TILE>::acc_t acc_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [part][margin + frame column + margin][ROW]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave_m = wave / WAVES_N, wave_n = wave % WAVES_N;
  const int r = lane & (TILE - 1), h = lane / TILE;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * a.u.bn_out;  // first output sample of this tile
  const int f0 = t0 - a.edge;              // sample of frame column 0 (a multiple of 4, also when negative)
  const int T = a.u.T, k = a.u.k, p = (k - 1) / 2, plane = a.u.plane, margin = a.margin;
  const long part_stride = a.u.part_stride;
  const float* __restrict__ xb = a.u.x + (size_t)b * C * T;
  __bf16* fr = xs + margin * ROW;  // plane 0 at frame column 0

  const unsigned wrow = wave_m * 32 + r;
  bf16x8 wf[3];
  ru_request<C, TILE>(wf, a.w1[0], part_stride, wrow, h);

  // the margins: zero, once
  for (int i = tid; i < 2 * margin * Cfg::OCTS; i += 256) {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
    const int row = i / Cfg::OCTS;
    __bf16* dst = xs + (row < margin ? row : H + row) * ROW + (i % Cfg::OCTS) * 8;
    *reinterpret_cast<bf16x8*>(dst) = z;
    *reinterpret_cast<bf16x8*>(dst + plane) = z;
    *reinterpret_cast<bf16x8*>(dst + 2 * plane) = z;
  }

  // The residual of unit 0 is the raw x at the lane's own frame columns (every column of the frame inside [0, T): the
  // columns in front of the stored ones are inputs of the next unit); add2 is needed at the stored columns only.  A value
  // that is not needed reads the tile's first samples: no address outside the row.
  constexpr int NV = TN * NG;
  const bool has2 = a.u.add2 != nullptr;
  f32x4 res[TM][NV], ad2[TM][NV];
  auto request_values = [&](const float* __restrict__ src, f32x4 (&dst)[TM][NV], bool stored_only) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      const float* __restrict__ rowp = src + ((size_t)b * C + wave_m * 32 + mi * TILE + r) * T;
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        const int slot = ru_out_slot<TILE>(wave_n, h, n), t = f0 + slot;
        const bool ok = t >= 0 && t < T && (!stored_only || (slot >= a.edge && slot < a.edge + a.u.bn_out));
        dst[mi][n] = *reinterpret_cast<const f32x4*>(rowp + (ok ? t : t0));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int n = 0; n < NV; ++n) ad2[mi][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto behind_window = [&] { request_values(a.u.x, res, false); };
  if (f0 >= 0 && f0 + H <= T)
    ru_stage_window<C, false>(a.u, xb, f0, fr, tid, behind_window);
  else
    ru_stage_window<C, true>(a.u, xb, f0, fr, tid, behind_window);

  acc_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < NREG; ++i) acc[mi][ni][i] = 0.f;

#pragma unroll 1
  for (int u = 0; u < a.n_units; ++u) {
    const bool last = u + 1 == a.n_units;
    const int d1 = a.d[u];
    const float* __restrict__ b1p = a.b1[u];
    const float* __restrict__ b2p = a.b2[u];
    const bool has_b1 = b1p != nullptr, has_b2 = b2p != nullptr;
    // the unit's biases: b1 of the lane's 4 consecutive channels per (mi, g) where h is formed, b2 per row tile
    f32x4 bias_h[TM][NG];
    float bias_y[TM];
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      bias_y[mi] = has_b2 ? b2p[wave_m * 32 + mi * TILE + r] : 0.f;
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          bias_h[mi][g][e] = has_b1 ? b1p[wave_m * 32 + mi * TILE + 4 * h + 4 * HL * g + e] : 0.f;
    }
    __syncthreads();  // the planes hold lrelu(x_u), split (and, for u = 0, the zeroed margins)

    // ---- phase 1: conv_{k,d} over lrelu(x_u); frame column m reads row margin + m + (tap - p) * d
    ru_contract<C, TILE, false>(wf, a.w1[u], part_stride, wrow, fr + (wave_n * 64 + r - p * d1) * ROW, plane, d1, k, h,
                                acc);
    ru_request<C, TILE>(wf, a.w2[u], part_stride, wrow, h);  // lands behind the forming of h and both barriers
    if (last && has2) request_values(a.u.add2, ad2, true);   // (so does add2)
    __syncthreads();  // every wave has read its x columns: the h planes take their place
    // h = lrelu(acc + b1), zero outside [0, T), split: a lane owns channels c .. c + 3 of a column
    const SplitActLeaky act2{a.slope2[u]};
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int c = wave_m * 32 + mi * TILE + 4 * h + 4 * HL * g;
        const f32x4 bias = bias_h[mi][g];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int m = wave_n * 64 + ni * TILE + r;
          const int th = f0 + m;
          const bool inside = th >= 0 && th < T;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = acc[mi][ni][4 * g + e];
            if (has_b1) v[e] += bias[e];
            v[e] = act2(v[e]);
            v[e] = inside ? v[e] : 0.f;
            acc[mi][ni][4 * g + e] = 0.f;
          }
          split3_store<4>(v, fr + m * ROW + c, plane);
        }
      }
    __syncthreads();
    // ---- phase 2: conv_{k,1} over h; frame column m reads row margin + m + tap - p
    ru_contract<C, TILE, true>(wf, a.w2[u], part_stride, wrow, fr + (wave_n * 64 + r - p) * ROW, plane, 1, k, h, acc);
    if (last) break;

    // ---- between units: y_u = acc + b2 + x_u (the epilogue's order), zero outside [0, T); it is the next unit's
    // residual, and lrelu(y_u) with the next unit's slope1, split, is the next unit's window
    ru_request<C, TILE>(wf, a.w1[u + 1], part_stride, wrow, h);
    const SplitActLeaky act1{a.slope1[u + 1]};
    __syncthreads();  // every wave has read its h columns
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
      const int c = wave_m * 32 + mi * TILE + r;
      const float bias = bias_y[mi];
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        const int slot = ru_out_slot<TILE>(wave_n, h, n), t = f0 + slot;
        const bool inside = t >= 0 && t < T;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[mi][n / NG][(n % NG) * 4 + e];
          acc[mi][n / NG][(n % NG) * 4 + e] = 0.f;
        }
        if (has_b2) v += bias;
        v += res[mi][n];
        if (!inside) v = f32x4{0.f, 0.f, 0.f, 0.f};
        res[mi][n] = v;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {  // two samples per split3_pair; a sample is a column: 2-byte writes
          unsigned part[3];
          split3_pair(act1(v[e]), act1(v[e + 1]), part[0], part[1], part[2]);
          unsigned short* dst = reinterpret_cast<unsigned short*>(fr + (slot + e) * ROW + c);
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            dst[q * plane] = (unsigned short)part[q];
            dst[q * plane + ROW] = (unsigned short)(part[q] >> 16);
          }
        }
      }
    }
  }

  // ---- epilogue of the last unit: that of resunit_split_kernel (acc + bias + x + add2, then / out_div) on the stored
  // slots edge .. edge + bn_out - 1
  const float* __restrict__ b2l = a.b2[a.n_units - 1];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
    const int c = wave_m * 32 + mi * TILE + r;
    const size_t row = ((size_t)b * C + c) * T;
    f32x4 v[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[n][e] = acc[mi][n / NG][(n % NG) * 4 + e];
    if (b2l != nullptr) {
      const float bias = b2l[c];
#pragma unroll
      for (int n = 0; n < NV; ++n) v[n] += bias;
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) v[n] += res[mi][n];
    if (has2) {
#pragma unroll
      for (int n = 0; n < NV; ++n) v[n] += ad2[mi][n];
    }
    if (a.u.out_div != 1.0f) {
#pragma unroll
      for (int n = 0; n < NV; ++n) v[n] = v[n] / a.u.out_div;
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int slot = ru_out_slot<TILE>(wave_n, h, n), t = f0 + slot;
      if (slot >= a.edge && slot < a.edge + a.u.bn_out && t < T) *reinterpret_cast<f32x4*>(a.u.y + row + t) = v[n];
    }
  }
}

struct RbSplitGeom {
  int H, edge, margin, bn_out, rows, tiles;
  size_t lds;
};

// Coverage of the chained block: every unit's own (ru_split_geometry), the pair form, and a frame that keeps at least
// half of its columns.  Pure host logic.
static int rb_split_geometry(const pwg_resunit_desc* d, int n_units, const int32_t* dilations, RbSplitGeom* g) {
  PWG_REQUIRE(d != nullptr && dilations != nullptr, PWG_ERR_NULL, "resblock_split: NULL descriptor or dilations");
  PWG_REQUIRE(n_units >= 1 && n_units <= kRbMaxUnits, PWG_ERR_UNSUPPORTED, "resblock_split: n_units = %d (1 .. %d)",
              n_units, kRbMaxUnits);
  PWG_REQUIRE(d->has_conv2, PWG_ERR_UNSUPPORTED, "resblock_split: single-convolution units are not chained");
  int dmax = 1, sum = 0;
  for (int u = 0; u < n_units; ++u) {
    pwg_resunit_desc du = *d;
    du.dilation = dilations[u];
    RuSplitGeom gu;
    const int rc = ru_split_geometry(&du, &gu);
    if (rc != PWG_OK) return rc;
    dmax = dilations[u] > dmax ? dilations[u] : dmax;
    sum += (d->kernel - 1) / 2 * (dilations[u] + 1);
  }
  const int C = d->channels;
  g->H = C == 32 ? RuSplitCfg<32>::H : RuSplitCfg<64>::H;
  g->edge = round_up(sum, 4);
  g->margin = (d->kernel - 1) / 2 * dmax;
  g->bn_out = g->H - 2 * g->edge;
  PWG_REQUIRE(g->bn_out >= g->H / 2, PWG_ERR_UNSUPPORTED,
              "resblock_split: kernel = %d over %d units leaves %d outputs per frame of %d columns", d->kernel, n_units,
              g->bn_out, g->H);
  g->rows = g->H + 2 * g->margin;
  g->lds = (size_t)3 * g->rows * (C + 8) * sizeof(__bf16);
  PWG_REQUIRE(g->lds <= kRuSplitMaxLds, PWG_ERR_UNSUPPORTED, "resblock_split: the planes (kernel %d) need %zu B of LDS",
              d->kernel, g->lds);
  g->tiles = ceil_div(d->t, g->bn_out);
  return PWG_OK;
}

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_resblock_split_supported(const pwg_resunit_desc* d, int32_t n_units, const int32_t* dilations) {
  RbSplitGeom g;
  return rb_split_geometry(d, n_units, dilations, &g) == PWG_OK ? 1 : 0;
}

extern "C" int pwg_resblock_split_frame(const pwg_resunit_desc* d, int32_t n_units, const int32_t* dilations,
                                        int32_t* out) {
  RbSplitGeom g;
  const int rc = rb_split_geometry(d, n_units, dilations, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(out != nullptr, PWG_ERR_NULL, "resblock_split_frame: NULL out");
  out[0] = g.H, out[1] = g.bn_out, out[2] = g.edge, out[3] = g.margin, out[4] = (int32_t)g.lds, out[5] = g.tiles;
  return PWG_OK;
}

extern "C" int pwg_resblock_split_forward_cfg(const pwg_resunit_desc* d, int32_t n_units, const int32_t* dilations,
                                              const float* slopes1, const float* slopes2, const float* x,
                                              const void* const* w1_split, const float* const* b1,
                                              const void* const* w2_split, const float* const* b2, const float* add2,
                                              float* y, int32_t mfma_shape, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RbSplitGeom g;
  const int rc = rb_split_geometry(d, n_units, dilations, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(x && y && w1_split && w2_split && b1 && b2 && slopes1 && slopes2, PWG_ERR_NULL,
              "resblock_split_forward: NULL pointer");
  PWG_REQUIRE(x != y, PWG_ERR_BAD_SHAPE, "resblock_split_forward: y must not alias x (frames read their neighbours' columns)");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  PWG_REQUIRE(al16(x) && al16(y) && al16(add2), PWG_ERR_BAD_SHAPE,
              "resblock_split_forward: x / y / add2 must be 16-B aligned");
  PWG_REQUIRE(mfma_shape == 16 || mfma_shape == 32, PWG_ERR_BAD_SHAPE, "resblock_split_forward: mfma_shape = %d (16 or 32)",
              mfma_shape);
  const int C = d->channels;
  RbSplitArgs a = {};
  for (int u = 0; u < n_units; ++u) {
    PWG_REQUIRE(w1_split[u] && w2_split[u], PWG_ERR_NULL, "resblock_split_forward: NULL weight image of unit %d", u);
    PWG_REQUIRE(al16(w1_split[u]) && al16(w2_split[u]), PWG_ERR_BAD_SHAPE,
                "resblock_split_forward: the weight images must be 16-B aligned");
    PWG_REQUIRE(slopes1[u] > 0.f && slopes1[u] < 1.f && slopes2[u] > 0.f && slopes2[u] < 1.f, PWG_ERR_UNSUPPORTED,
                "resblock_split_forward: slopes of unit %d = %g, %g (0 < slope < 1)", u, (double)slopes1[u],
                (double)slopes2[u]);
    a.w1[u] = static_cast<const bf16x8*>(w1_split[u]);
    a.w2[u] = static_cast<const bf16x8*>(w2_split[u]);
    a.b1[u] = b1[u], a.b2[u] = b2[u];
    a.d[u] = dilations[u];
    a.slope1[u] = slopes1[u], a.slope2[u] = slopes2[u];
  }
  a.n_units = n_units, a.margin = g.margin, a.edge = g.edge;
  a.u.x = x, a.u.add2 = add2, a.u.y = y;
  a.u.T = d->t, a.u.k = d->kernel, a.u.d1 = dilations[0];
  a.u.bn_out = g.bn_out, a.u.rows = g.H;
  a.u.plane = g.rows * (C + 8);
  a.u.part_stride = image_elems(d->kernel, image_chunks(C), image_m_pad(C)) / 8;
  PWG_REQUIRE(split_image_addressable(a.u.part_stride * 8), PWG_ERR_UNSUPPORTED,
              "resblock_split_forward: weight image too large");
  a.u.slope1 = slopes1[0], a.u.slope2 = slopes2[0], a.u.out_div = d->out_div;
  void (*kern)(RbSplitArgs) = C == 32 ? (mfma_shape == 32 ? resblock_split_kernel<32, 32> : resblock_split_kernel<32, 16>)
                                      : (mfma_shape == 32 ? resblock_split_kernel<64, 32> : resblock_split_kernel<64, 16>);
  if (g.lds > kConvMaxLds && !lds_limit_is_set(reinterpret_cast<const void*>(kern), g.lds)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)g.lds);
    PWG_REQUIRE(e == hipSuccess, PWG_ERR_LAUNCH, "resblock_split_forward: cannot raise LDS limit to %zu: %s", g.lds,
                hipGetErrorString(e));
  }
  // the ALGORITHMIC flops and bytes of the N units the launch stands for
  const double elems = (double)d->batch * C * d->t;
  const double flops = 2.0 * elems * C * d->kernel * 2 * n_units;
  const double bytes = 4.0 * (elems * (2 * n_units + (add2 != nullptr)) + 2.0 * n_units * C * C * d->kernel);
  maybe_poison_lds(stream);
  {
    ProfScope prof(stream,
                   prof_shape_name("resblock_split_kernel", "resblock_split_kernel B%d C%d T%d k%d n%d", d->batch, C, d->t,
                                   d->kernel, n_units),
                   flops, bytes);
    hipLaunchKernelGGL(kern, dim3(g.tiles, d->batch), dim3(256), g.lds, stream, a);
  }
  PWG_CHECK_LAUNCH("resblock_split_forward");
  return PWG_OK;
}

extern "C" int pwg_resunit_split_supported(const pwg_resunit_desc* d) {
  RuSplitGeom g;
  return ru_split_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" int pwg_resunit_split_forward(const pwg_resunit_desc* d, const float* x, const void* w1_split, const float* b1,
                                         const void* w2_split, const float* b2, const float* add2, float* y,
                                         void* stream) {
  return ru_split_forward<false>(d, x, w1_split, b1, w2_split, b2, add2, y, kDefaultMfmaShape, (hipStream_t)stream);
}

extern "C" int pwg_resunit_split_forward_cfg(const pwg_resunit_desc* d, const float* x, const void* w1_split,
                                             const float* b1, const void* w2_split, const float* b2, const float* add2,
                                             float* y, int32_t mfma_shape, void* stream) {
  return ru_split_forward<false>(d, x, w1_split, b1, w2_split, b2, add2, y, mfma_shape, (hipStream_t)stream);
}

extern "C" int pwg_resunit_split_ragged_supported(const pwg_resunit_desc* d, int32_t rate) {
  RuSplitGeom g;
  return ru_split_geometry(d, &g) == PWG_OK && ru_split_ragged_rate(rate) == PWG_OK ? 1 : 0;
}

extern "C" int pwg_resunit_split_forward_ragged(const pwg_resunit_desc* d, const float* x, const void* w1_split,
                                                const float* b1, const void* w2_split, const float* b2,
                                                const float* add2, float* y, int32_t mfma_shape, const int32_t* frames,
                                                int32_t rate, void* stream) {
  PWG_REQUIRE(frames != nullptr, PWG_ERR_NULL, "resunit_split_forward_ragged: NULL frames table");
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 3u) == 0, PWG_ERR_BAD_SHAPE,
              "resunit_split_forward_ragged: the frames table must be 4-B aligned");
  const int rc = ru_split_ragged_rate(rate);
  if (rc != PWG_OK) return rc;
  return ru_split_forward<true>(d, x, w1_split, b1, w2_split, b2, add2, y, mfma_shape, (hipStream_t)stream, frames, rate);
}
