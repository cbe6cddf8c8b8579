// conv1d_split.hip -- fp32-accurate inference convolution on the gfx950 bf16 MFMA instructions: both operands are split
// into three bf16 parts and six of the nine part products are accumulated in fp32.
//
// Numerical definition (include/pwg_kernels.h, "split-operand inference"): an fp32 value v is split exactly as
//   hi = bf16_rne(v),  r = v - float(hi),  mid = bf16_rne(r),  lo = bf16_rne(r - float(mid))        (v == hi + mid + lo)
// for finite v whose low parts are not subnormal.  The fused pre-activation is applied to the fp32 input in fp32, then the
// activated input is split while it is staged; the effective fp32 weight (w * scale) is split once when the weight image
// is packed.  Per operand pair the products lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (weight part . input part) are
// issued in this order -- small terms first; split_product of mfma_conv.h owns it, for this kernel and for
// resunit_split.hip -- into ONE fp32 accumulator set; each of the three dropped products
// (mid.lo, lo.mid, lo.lo) is <= 2^-24 of the full product in the worst case (|mid| <= 2^-8 |v|, |lo| <= 2^-16 |v|) and
// about 2^-28 of it on average.  A bf16 x bf16 product is exact in fp32, so what is left is
// the fp32 accumulation of the MFMA.  bias / add1 / add2 / out_mul / out_div / post-activation / the stored result are
// fp32, in the order of the fp32 kernel.
// Non-finite inputs give non-finite outputs, but not necessarily the same ones: hi(inf) = inf and r = inf - inf = NaN, so
// an inf comes out as NaN.  There is no branch for it.
//
// Scope: stride-1 Conv1d, groups 1, width 1, zero padding, forward only (conv1d_split_mfma_kernel); and, under the same
// definition, ConvTranspose1d with kernel == 2 * stride (convtr1d_split_mfma_kernel, further down).
// Contraction, coverage, weight image, tiles and launch plan are those of csrc/mfma_conv.h, with three parts: A operand =
// three weight images read from global memory (L2-resident), B operand = three bf16 planes of the x window in LDS, staged
// per 32-channel chunk.  A wave holds all A and B fragments of a reduction step (3 x TM + 3 x TN) and issues 6 x TM x TN
// MFMAs on them: six times the MFMA work of the bf16 kernel behind the same global loads and barriers.  A window whose
// three planes do not fit 64 KB of LDS at the full-size column tile runs on the half-size tiles (32 rows, k = 11 at
// dilation 5).
// Deterministic: one workgroup owns an output tile, no split reduction, no atomics; the accumulation order of an element
// (chunk, tap, reduction step, product) does not depend on the tile or the grid.
#include "mfma_conv.h"

namespace pwg {
namespace {

constexpr int PARTS = 3;

struct SplitArgs : MfmaConvArgs {
  int plane;          // bf16 elements per LDS plane
  long part_stride;   // bf16x8 elements per weight part image
  float pre_mul;      // pre-activation: SplitActMasked{pre_mul, pre_mask} for none / leaky / relu, or, where pre_leaky is
  unsigned pre_mask;  // set (leaky with 0 < slope < 1), SplitActLeaky{pre_mul}; split_staged picks the form of a launch
  int pre_leaky;
  int wide_out;  // y / add1 / add2 are 16-B aligned and t_out % 4 == 0: 16-B accesses in the epilogue
};

static int split_geometry(const pwg_conv1d_desc* d, MfmaConvGeom* g) {
  return mfma_conv_geometry("conv1d_split", PARTS, false, d, g);
}

// Run a staging site with the activation form of the launch (mfma_conv.h): wave-uniform, one branch around the site
template <typename Site>
__device__ __forceinline__ void split_staged(const SplitArgs& a, Site&& site) {
  if (a.pre_leaky)
    site(SplitActLeaky{a.pre_mul});
  else
    site(SplitActMasked{a.pre_mul, a.pre_mask});
}

// Vector staging of one 32-channel chunk of the x window (xc: channel 0 of the chunk, c_left channels are left).
// item = (group of 4 columns, channel octet): 8 loads of 16 B (one per channel, lanes walk t), then per column 8 channels
// are activated, split and written as three 16-B LDS stores (one per plane).  CHECKED (edge tiles): a load whose group
// of columns lies outside the row or whose channel is past the end gives zeros.  It reads a clamped address that is
// always valid (the group clamped into the row, the channel to the last one) and the value is zeroed by a select, so
// the 8 loads of an item are in flight together as in the interior copy, not one round trip each behind its own branch.
template <int NT, bool CHECKED, typename Act>
__device__ __forceinline__ void stage_window_vec(const SplitArgs& a, const float* __restrict__ xc, int c_left, int base,
                                                 int ngroups, __bf16* xs, int tid, Act act) {
  constexpr int ITEMS = window_items(NT);
  f32x4 st[ITEMS][8];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int idx = tid + it * 256, oct = idx & 3, grp = idx >> 2;
    const int t = base + grp * 4;
    const float* __restrict__ src = xc + (size_t)(oct * 8) * a.t_in + t;
    if (!CHECKED) {
      if (grp < ngroups) {
#pragma unroll
        for (int j = 0; j < 8; ++j) st[it][j] = *reinterpret_cast<const f32x4*>(src + (size_t)j * a.t_in);
      }
    } else {
      const bool tin = grp < ngroups && t >= 0 && t < a.t_in;
      const float* __restrict__ srcc = xc + min(max(t, 0), a.t_in - 4);  // t_in % 4 == 0, t_in >= 4
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(srcc + (size_t)min(oct * 8 + j, c_left - 1) * a.t_in);
        st[it][j] = tin && oct * 8 + j < c_left ? v : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int idx = tid + it * 256, oct = idx & 3, grp = idx >> 2;
    if (grp < ngroups) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = act(st[it][j][e]);
        split3_store<8>(v, xs + (grp * 4 + e) * kConvRow + oct * 8, a.plane);
        // one column at a time: the scheduler otherwise interleaves all 32 splits and spills the accumulators
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
}

// The epilogue of one wave (fp32, the operation order of the fp32 kernel: acc + bias + add1 + add2, * out_mul, / out_div,
// post-activation).  The kernel issues its MFMAs with the x fragment as the first operand, so the accumulators hold the
// TRANSPOSED tile: a lane owns ONE output row per mi (row0 + mi * TILE) and, per accumulator, NREG / 4 "values" of 4
// consecutive samples (value g of tile ni starts at col0 + ni * TILE + 4 * (64 / TILE) * g; col0 includes 4 * lane_group).
// Every switch of the descriptor is wave-uniform and is taken once per batch of values, around straight-line code; the
// loads of a batch are issued together and waited for once, and no store is waited for.
// WIDE: 16-B accesses (y / add1 / add2 16-B aligned, t_out % 4 == 0: a value is inside a row or outside it), a batch is
// the TN * NREG / 4 values of one mi.  Otherwise 4-B accesses and batches of one value (an address per sample: larger
// batches would cost the kernel a wave per SIMD).  FULL: the tile has no padded row and no column past the end; otherwise
// a load of a missing sample reads the last row / the last samples of the row instead, and its store is masked.
// add1 / add2 may be y itself (same element, same lane), not a shifted view of it.
template <int TILE, int TM, int TN, bool WIDE, bool FULL>
__device__ __forceinline__ void split_epilogue(const SplitArgs& a, const typename Mfma<TILE>::acc_t (&acc)[TM][TN],
                                               int row0, int col0, size_t out_base) {
  constexpr int HL = 64 / TILE, NG = TILE * TILE / 64 / 4, NV = TN * NG;
  constexpr int NB = WIDE ? NV : 1, BATCHES = TM * NV / NB;
  const bool has_bias = a.bias != nullptr, has1 = a.add1 != nullptr, has2 = a.add2 != nullptr;
#pragma unroll
  for (int bi = 0; bi < BATCHES; ++bi) {
    const int mi = bi * NB / NV;
    const int m = row0 + mi * TILE, mc = FULL ? m : min(m, a.m - 1);
    const size_t row = out_base + (size_t)mc * a.t_out;
    int q[NB];  // first sample of value k
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int n = (bi * NB + k) % NV;
      q[k] = col0 + (n / NG) * TILE + (n % NG) * (4 * HL);
    }
    auto load = [&](const float* __restrict__ src, f32x4 (&t)[NB]) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        if (WIDE) {
          t[k] = *reinterpret_cast<const f32x4*>(src + row + (FULL ? q[k] : min(q[k], a.nq - 4)));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) t[k][e] = src[row + min(q[k] + e, a.nq - 1)];
        }
      }
    };
    f32x4 t1[NB], t2[NB], v[NB];
    float bias = 0.f;
    if (has_bias) bias = a.bias[mc];
    if (has1) load(a.add1, t1);
    if (has2) load(a.add2, t2);
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int n = (bi * NB + k) % NV;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = acc[mi][n / NG][(n % NG) * 4 + e];
    }
    if (has_bias) {
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] += bias;
    }
    if (has1) {
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] += t1[k];
    }
    if (has2) {
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] += t2[k];
    }
    if (a.out_mul != 1.0f) {
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] *= a.out_mul;
    }
    if (a.out_div != 1.0f) {
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] = v[k] / a.out_div;
    }
    if (a.post_act == PWG_ACT_LEAKY_RELU) {
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = v[k][e] > 0.f ? v[k][e] : v[k][e] * a.post_slope;
    } else if (a.post_act == PWG_ACT_RELU) {
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = v[k][e] > 0.f ? v[k][e] : 0.f;
    } else if (a.post_act == PWG_ACT_TANH) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = tanhf(v[k][e]);
        __builtin_amdgcn_sched_barrier(0);  // one value's tanhf at a time: interleaved, their temporaries cost a wave
      }
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (WIDE) {
        if (FULL || (m < a.m && q[k] < a.nq)) *reinterpret_cast<f32x4*>(a.y + row + q[k]) = v[k];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m < a.m && q[k] + e < a.nq) a.y[row + q[k] + e] = v[k][e];
      }
    }
  }
}

// One 32-channel chunk of the x window into the three LDS planes: the staging of every kernel of this file
template <int NT, bool VEC, typename Act>
__device__ __forceinline__ void stage_chunk(const SplitArgs& a, const MfmaConvTile& c, int chunk, __bf16* xs, Act act) {
  if (VEC) {
    const int ngroups = (c.wcols + 3) >> 2, c_left = a.c_in - chunk * KC;
    const float* __restrict__ xc = c.xb + (size_t)chunk * KC * a.t_in;
    // an interior tile (decided once per workgroup and chunk: every staged column inside the row, a whole chunk of
    // channels) takes unconditional loads; an edge tile checks every load
    if (c.base >= 0 && c.base + 4 * ngroups <= a.t_in && c_left >= KC)
      stage_window_vec<NT, false>(a, xc, c_left, c.base, ngroups, xs, c.tid, act);
    else
      stage_window_vec<NT, true>(a, xc, c_left, c.base, ngroups, xs, c.tid, act);
  } else {
    // wave `wave` stages channel octet `wave` of the chunk: lanes walk the columns (coalesced fp32 rows)
    const int c_base = chunk * KC + c.wave * 8;
    const bool interior = c.base >= 0 && c.base + c.wcols <= a.t_in && c_base + 8 <= a.c_in;  // per wave and chunk
    for (int col = c.lane; col < c.wcols; col += 64) {
      const int t = c.base + col;
      float f[8];
      if (interior) {
        const float* __restrict__ src = c.xb + (size_t)c_base * a.t_in + t;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = src[(size_t)j * a.t_in];
      } else {
        // as the CHECKED vector copy: a clamped, always valid address and a select, the 8 loads in flight together
        const bool tin = t >= 0 && t < a.t_in;
        const float* __restrict__ srcc = c.xb + min(max(t, 0), a.t_in - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = srcc[(size_t)min(c_base + j, a.c_in - 1) * a.t_in];
          f[j] = tin && c_base + j < a.c_in ? v : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = act(f[j]);
      split3_store<8>(f, xs + col * kConvRow + c.wave * 8, a.plane);
    }
  }
}

// TILE, WM, WN, WAVES_M: the tile ladder of mfma_conv.h.  VEC: the x window is staged with 16-B loads along t (rows 16-B
// aligned, t_in % 4 == 0, window <= 2 * NT columns) and transposed in registers.
// The second launch bound (waves per SIMD) is the occupancy that the main loop's registers allow: without it the register
// allocator copies every accumulator out of the AGPRs at the head of the epilogue and the kernel loses a wave.
template <int TILE, int WM, int WN, int WAVES_M, bool VEC>
__global__ __launch_bounds__(256, WM * WN == 4 ? (TILE == 16 ? 3 : 2) : (WM * WN == 2 ? 3 : 4)) void
conv1d_split_mfma_kernel(SplitArgs a) {
  constexpr int HL = 64 / TILE;
  constexpr int KSTEPS = KC / (8 * HL);
  constexpr int TM = WM * 32 / TILE, TN = WN * 32 / TILE;
  constexpr int NREG = TILE * TILE / 64;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int MT = WAVES_M * WM * 32, NT = WAVES_N * WN * 32;
  typedef typename Mfma<TILE>::acc_t acc_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [part][column][ROW]

  const MfmaConvTile c = mfma_conv_tile<TILE, MT, NT, WAVES_M, VEC>(a);

  acc_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < NREG; ++i) acc[mi][ni][i] = 0.f;

  for (int chunk = 0; chunk < a.cin_chunks; ++chunk) {
    if (chunk) __syncthreads();
    split_staged(a, [&](auto act) { stage_chunk<NT, VEC>(a, c, chunk, xs, act); });
    __syncthreads();
    for (int tap = 0; tap < a.taps; ++tap) {
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const int oct = ks * HL + c.h;
        const bf16x8* __restrict__ wp =
            image_rows(a.w, a.cin_chunks, a.m_pad, tap, chunk, oct) + c.m0 + c.wave_m * (WM * 32) + c.r;
        // the x fragment goes first: the transposed tile, a lane gets 4 consecutive samples of a row (split_epilogue)
        split_step<TILE, TM, TN, kConvRow, true>(wp, a.part_stride, xs, c.sh + c.wave_n * (WN * 32) + c.r + tap * a.dil,
                                                 oct * 8, a.plane, acc);
      }
    }
  }

  const size_t out_base = (size_t)c.b * a.c_out * a.t_out;
  const int row0 = c.m0 + c.wave_m * (WM * 32) + c.r, col0 = c.q0 + c.wave_n * (WN * 32) + 4 * c.h;
  const bool full = c.m0 + MT <= a.m && c.q0 + NT <= a.nq;  // no padded row and no column past the end in this tile
  if (!a.wide_out)
    split_epilogue<TILE, TM, TN, false, false>(a, acc, row0, col0, out_base);
  else if (full)
    split_epilogue<TILE, TM, TN, true, true>(a, acc, row0, col0, out_base);
  else
    split_epilogue<TILE, TM, TN, true, false>(a, acc, row0, col0, out_base);
}

// conv1d_split_mfma_kernel with the STREAMED form of the reduction step (split_step_streamed, as resunit_split_kernel runs
// it) in place of the resident one: tap and k-step are one flat sequence of steps (split_step_successor), the weight
// fragments run a row tile ahead of their MFMAs across taps and chunks -- those of a chunk's first step are in flight
// while the chunk is staged -- and the very first request goes out in front of the first chunk's staging.  Staging,
// tiles, launch bounds and epilogue are the resident kernel's, and an accumulator receives its products in the same
// order (chunk, tap, step, product): the same bits.  split_step_form (below) chooses the kernel per launch.
template <int TILE, int WM, int WN, int WAVES_M, bool VEC>
__global__ __launch_bounds__(256, WM * WN == 4 ? (TILE == 16 ? 3 : 2) : (WM * WN == 2 ? 3 : 4)) void
conv1d_split_streamed_mfma_kernel(SplitArgs a) {
  constexpr int HL = 64 / TILE;
  constexpr int KSTEPS = KC / (8 * HL);
  constexpr int TM = WM * 32 / TILE, TN = WN * 32 / TILE;
  constexpr int NREG = TILE * TILE / 64;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int MT = WAVES_M * WM * 32, NT = WAVES_N * WN * 32;
  typedef typename Mfma<TILE>::acc_t acc_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [part][column][ROW]

  const MfmaConvTile c = mfma_conv_tile<TILE, MT, NT, WAVES_M, VEC>(a);

  // this lane's weight row of tile mi = 0; the fragments of row tile 0 of the step to come; that step
  const unsigned wrow = c.m0 + c.wave_m * (WM * 32) + c.r;
  bf16x8 wf[3];
  SplitStepId step{0, 0, 0};
  split_step_request(wf, a.w, a.part_stride, wrow + split_step_rows<TILE>(a.cin_chunks, a.m_pad, step, c.h));

  acc_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < NREG; ++i) acc[mi][ni][i] = 0.f;

  for (int chunk = 0; chunk < a.cin_chunks; ++chunk) {
    if (chunk) __syncthreads();
    split_staged(a, [&](auto act) { stage_chunk<NT, VEC>(a, c, chunk, xs, act); });
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < a.taps * KSTEPS; ++s) {  // the steps of this chunk: the planes hold one chunk
      const SplitStepId next = split_step_successor(step, a.cin_chunks, a.taps, KSTEPS);
      // the x fragment goes first: the transposed tile of split_epilogue
      split_step_streamed<TILE, TM, TN, kConvRow, true>(
          wf, a.w, a.part_stride, wrow + split_step_rows<TILE>(a.cin_chunks, a.m_pad, step, c.h),
          wrow + split_step_rows<TILE>(a.cin_chunks, a.m_pad, next, c.h), xs,
          c.sh + c.wave_n * (WN * 32) + c.r + step.tap * a.dil, split_step_off<TILE>(step, c.h), a.plane, acc);
      step = next;
    }
  }

  const size_t out_base = (size_t)c.b * a.c_out * a.t_out;
  const int row0 = c.m0 + c.wave_m * (WM * 32) + c.r, col0 = c.q0 + c.wave_n * (WN * 32) + 4 * c.h;
  const bool full = c.m0 + MT <= a.m && c.q0 + NT <= a.nq;  // no padded row and no column past the end in this tile
  if (!a.wide_out)
    split_epilogue<TILE, TM, TN, false, false>(a, acc, row0, col0, out_base);
  else if (full)
    split_epilogue<TILE, TM, TN, true, true>(a, acc, row0, col0, out_base);
  else
    split_epilogue<TILE, TM, TN, true, false>(a, acc, row0, col0, out_base);
}

// ---- the PREFETCHED window ("The prefetched window").  Beside the three planes LDS holds the RAW fp32
// window of one chunk: per wave a region of its own, [8 channels][ngroups] groups of 4 columns (16 B each), wave w
// holding channel octet w of the chunk.  The region is filled by LDS-DMA (global_load_lds_dwordx4: 64 consecutive
// 16-B elements of the region per wave instruction, the source address per lane) and holds exactly the values that the
// 16-B loads of stage_window_vec<NT, false> deliver.
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// bytes of the raw regions of a workgroup whose planes have `rows` LDS rows: KC channels x rows columns of fp32
static inline size_t split_raw_bytes(int rows) { return (size_t)KC * rows * sizeof(float); }

// Request the wave's raw region of one chunk.  xw: column `base` of the wave's first channel (8 * wave of the chunk);
// element e = j * ngroups + grp of the region is columns base + 4 * grp .. + 3 of channel j.  The caller guarantees an
// interior window (base >= 0, base + 4 * ngroups <= t_in) and 8 whole channels, so every requested byte is inside the
// row; lanes past the last element of the region are masked and write nothing.
__device__ __forceinline__ void request_raw_window(const float* __restrict__ xw, int t_in, int ngroups, float* raww,
                                                   int lane) {
  const int total = 8 * ngroups;
  const int dq = 64 / ngroups, dr = 64 - dq * ngroups;
  int j = lane / ngroups, g = lane - j * ngroups;
  for (int e0 = 0; e0 < total; e0 += 64) {
    if (e0 + lane < total)
      __builtin_amdgcn_global_load_lds(xw + (size_t)j * t_in + 4 * g, (lds_ptr_t)(raww + e0 * 4), 16, 0, 0);
    j += dq, g += dr;
    if (g >= ngroups) g -= ngroups, ++j;
  }
}

// Activate, split and write the wave's raw region to the planes: item = (group of 4 columns, the wave's channel octet),
// lanes walk the groups -- the values, the arithmetic and the plane addresses of stage_window_vec, with the items of a
// window dealt evenly over the four waves (there: item = thread index, which leaves wave 3 idle on a short window).
// Measured and not kept (profiles/split_window.txt): lanes that walk the COLUMNS (8 values per lane and pass, plane rows
// 80 B apart instead of 320 B, which halves the LDS bank conflicts of this form) -- a VGPR spill in the flagship
// instantiation, 0.97 x of the staged kernel at 16 x 800 frames where this form has 0.96 x, 0.94 x at 1 x 800.
template <typename Act>
__device__ __forceinline__ void split_raw_window(const SplitArgs& a, const float* raww, int ngroups, __bf16* xs, int wave,
                                                 int lane, Act act) {
  for (int grp = lane; grp < ngroups; grp += 64) {
    f32x4 st[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) st[j] = *reinterpret_cast<const f32x4*>(raww + (j * ngroups + grp) * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = act(st[j][e]);
      split3_store<8>(v, xs + (grp * 4 + e) * kConvRow + wave * 8, a.plane);
      __builtin_amdgcn_sched_barrier(0);  // one column at a time, as in stage_window_vec
    }
  }
}

// conv1d_split_mfma_kernel (16-B staging, resident step) with the raw window of chunk n + 1 requested in front of the tap
// loop of chunk n and consumed behind it.  Only a chunk that passes the interior test of the staged kernel (every staged
// column inside the row, 32 whole channels) is prefetched; an edge tile, or the channel tail of an interior tile, is
// staged by stage_chunk as before, in this kernel: the decision is workgroup-uniform.  The planes receive the same
// values at the same addresses and the tap loop and the epilogue are the staged kernel's: the same bits.
template <int TILE, int WM, int WN, int WAVES_M>
__global__ __launch_bounds__(256, WM * WN == 4 ? (TILE == 16 ? 3 : 2) : (WM * WN == 2 ? 3 : 4)) void
conv1d_split_window_mfma_kernel(SplitArgs a) {
  constexpr int HL = 64 / TILE;
  constexpr int KSTEPS = KC / (8 * HL);
  constexpr int TM = WM * 32 / TILE, TN = WN * 32 / TILE;
  constexpr int NREG = TILE * TILE / 64;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int MT = WAVES_M * WM * 32, NT = WAVES_N * WN * 32;
  typedef typename Mfma<TILE>::acc_t acc_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [part][column][ROW]

  const MfmaConvTile c = mfma_conv_tile<TILE, MT, NT, WAVES_M, true>(a);
  const int ngroups = (c.wcols + 3) >> 2;
  // the wave's raw region, behind the planes: 8 channels x the plane's rows (>= 4 * ngroups columns)
  float* raww = reinterpret_cast<float*>(xs + PARTS * a.plane) + c.wave * (8 * (a.plane / kConvRow));
  const bool interior = c.base >= 0 && c.base + 4 * ngroups <= a.t_in;  // per workgroup
  const float* __restrict__ xw = c.xb + (size_t)(c.wave * 8) * a.t_in + c.base;
  auto prefetched = [&](int chunk) { return interior && a.c_in - chunk * KC >= KC; };

  if (prefetched(0)) request_raw_window(xw, a.t_in, ngroups, raww, c.lane);

  acc_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < NREG; ++i) acc[mi][ni][i] = 0.f;

  // Synchronisation.  A raw region is PRIVATE to its wave: the wave that requests it is the only one that reads it.  A
  // ds_read is ordered behind a pending LDS-DMA only by the issuing wave's own vmcnt wait, and here that wave is the
  // reader, so its vmcnt(0) in front of the reads suffices and no barrier guards the raw data.  The count is drained
  // there completely: besides the DMA only the weight fragments of the resident step use vmcnt, and every one of them
  // was waited for by the MFMA that consumed it before the tap loop ended, so nothing else is in flight.  The region of
  // chunk n is overwritten by the request for chunk n + 1, which the same wave issues after its split of chunk n has
  // used every value it read (the reads have returned) and behind barrier 2.  The two barriers per chunk are the
  // staged kernel's and guard the planes alone: barrier 1, every wave has finished the taps of chunk n - 1, the planes
  // may be overwritten; barrier 2, the planes of chunk n are written, every wave may read them.
  for (int chunk = 0; chunk < a.cin_chunks; ++chunk) {
    if (chunk) __syncthreads();
    if (prefetched(chunk)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      split_staged(a, [&](auto act) { split_raw_window(a, raww, ngroups, xs, c.wave, c.lane, act); });
    } else {
      split_staged(a, [&](auto act) { stage_chunk<NT, true>(a, c, chunk, xs, act); });
    }
    __syncthreads();
    if (chunk + 1 < a.cin_chunks && prefetched(chunk + 1))
      request_raw_window(xw + (size_t)(chunk + 1) * KC * a.t_in, a.t_in, ngroups, raww, c.lane);
    for (int tap = 0; tap < a.taps; ++tap) {
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const int oct = ks * HL + c.h;
        const bf16x8* __restrict__ wp =
            image_rows(a.w, a.cin_chunks, a.m_pad, tap, chunk, oct) + c.m0 + c.wave_m * (WM * 32) + c.r;
        // the x fragment goes first: the transposed tile of split_epilogue
        split_step<TILE, TM, TN, kConvRow, true>(wp, a.part_stride, xs, c.sh + c.wave_n * (WN * 32) + c.r + tap * a.dil,
                                                 oct * 8, a.plane, acc);
      }
    }
  }

  const size_t out_base = (size_t)c.b * a.c_out * a.t_out;
  const int row0 = c.m0 + c.wave_m * (WM * 32) + c.r, col0 = c.q0 + c.wave_n * (WN * 32) + 4 * c.h;
  const bool full = c.m0 + MT <= a.m && c.q0 + NT <= a.nq;  // no padded row and no column past the end in this tile
  if (!a.wide_out)
    split_epilogue<TILE, TM, TN, false, false>(a, acc, row0, col0, out_base);
  else if (full)
    split_epilogue<TILE, TM, TN, true, true>(a, acc, row0, col0, out_base);
  else
    split_epilogue<TILE, TM, TN, true, false>(a, acc, row0, col0, out_base);
}

struct WindowFamily {
  template <int TILE, int WM, int WN, int WAVES_M>
  struct K {
    static constexpr auto fn = conv1d_split_window_mfma_kernel<TILE, WM, WN, WAVES_M>;
  };
};

template <bool VEC, bool STREAMED>
struct Family {
  template <int TILE, int WM, int WN, int WAVES_M>
  struct K {
    static constexpr auto fn = STREAMED ? conv1d_split_streamed_mfma_kernel<TILE, WM, WN, WAVES_M, VEC>
                                        : conv1d_split_mfma_kernel<TILE, WM, WN, WAVES_M, VEC>;
  };
};

// what the stride-1 and the transposed launch fill alike.  wide_out here is the stride-1 rule (a value = 4 consecutive
// samples of an output row); the transposed launch adds its own conditions
static void split_fill_args(SplitArgs* a, const pwg_conv1d_desc* d, const MfmaConvGeom& g, const MfmaConvPlan& p,
                            const float* x, const void* w_packed, const float* bias, const float* add1, const float* add2,
                            float* y) {
  mfma_conv_fill_args(a, d, g, x, w_packed, bias, add1, add2, y);
  a->plane = p.plane;
  a->part_stride = image_elems(g) / 8;
  a->pre_mul = d->pre_act == PWG_ACT_LEAKY_RELU ? d->pre_slope : (d->pre_act == PWG_ACT_RELU ? 0.0f : 1.0f);
  a->pre_mask = d->pre_act == PWG_ACT_RELU ? 0u : ~0u;
  a->pre_leaky = split_act_is_leaky(d->pre_act, d->pre_slope);
  a->wide_out = d->t_out % 4 == 0 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(add1) |
                                       reinterpret_cast<uintptr_t>(add2)) & 15u) == 0;
}

// The form of the reduction step of a launch (kStepResident / kStepStreamed), chosen where its plan is made, from the
// launch's class: input channels (chunks) and taps.  Admitted to the streamed form is what the isolated A/B of the two
// forms (tools/bench_conv_split_forms.py; DESIGN.md s9.1, profiles/split_early_loads.txt) measured: every run at
// 16 x 800 frames disjointly faster than every resident run, and no shorter launch (1 x 800, 1 x 100; full-size and
// half-size tiles) disjointly slower.  That held for every class measured -- 64, 128 and 256 input channels at 7 and 11
// taps -- so the rule is their hull; classes nobody measured (fewer taps, a single chunk, the transposed kernel's two
// taps) stay resident, and so does a part image that the 32-bit fragment index of the streamed form cannot address.
// Pure host logic.
constexpr int kStepPlanDecides = 0, kStepResident = 1, kStepStreamed = 2;
constexpr int kStreamedMinTaps = 7, kStreamedMinChunks = 2;
static int split_step_form(const MfmaConvGeom& g) {
  if (!split_image_addressable(image_elems(g))) return kStepResident;
  return g.taps >= kStreamedMinTaps && g.cin_chunks >= kStreamedMinChunks ? kStepStreamed : kStepResident;
}

// The form of the window staging of a launch (kWindowStaged / kWindowPrefetched): a second axis beside the step form.
// The prefetched kernel covers a launch with 16-B staging (plan.vec) whose planes and raw regions fit the LDS of a CU;
// split_window_lds is that size.  The plan CHOOSES it by the keep rule of the step form, read off the isolated A/B of the
// two window forms (tools/bench_conv_split_window.py; DESIGN.md s9.1, profiles/split_window.txt): a class is admitted when
// every run at 16 x 800 frames is disjointly faster than every staged run and no shorter launch is disjointly slower,
// and the rule is the hull of the admitted classes.  A launch the streamed step is chosen for keeps the staged window
// (the prefetched kernel has the resident step), and so does one whose planes and raw regions would not leave three
// workgroups to a CU (kWindowLdsShare).  Pure host logic.
constexpr int kWindowPlanDecides = 0, kWindowStaged = 1, kWindowPrefetched = 2;
constexpr size_t kLdsPerCu = 160 * 1024, kWindowLdsShare = kLdsPerCu / 3;
constexpr int kWindowMaxTaps = 0;  // taps up to which the A/B admitted the prefetched window (0: no class)
static size_t split_window_lds(const MfmaConvPlan& p) { return p.lds + split_raw_bytes(p.plane / kConvRow); }
static bool split_window_covers(const MfmaConvPlan& p) { return p.vec && split_window_lds(p) <= kLdsPerCu; }
static int split_window_form(const MfmaConvGeom& g, const MfmaConvPlan& p) {
  if (!split_window_covers(p) || split_step_form(g) == kStepStreamed) return kWindowStaged;
  return g.taps <= kWindowMaxTaps && g.cin_chunks >= 2 && split_window_lds(p) <= kWindowLdsShare ? kWindowPrefetched
                                                                                                   : kWindowStaged;
}

static int split_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                         const float* add1, const float* add2, float* y, int mfma_shape, int tile_mode, int step_form,
                         int window_form, hipStream_t stream) {
  MfmaConvGeom g;
  int rc = split_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(step_form >= kStepPlanDecides && step_form <= kStepStreamed, PWG_ERR_BAD_SHAPE,
              "conv1d_split: step_form = %d (0 = the plan decides, 1 = resident, 2 = streamed)", step_form);
  PWG_REQUIRE(window_form >= kWindowPlanDecides && window_form <= kWindowPrefetched, PWG_ERR_BAD_SHAPE,
              "conv1d_split: window_form = %d (0 = the plan decides, 1 = staged, 2 = prefetched)", window_form);
  rc = mfma_conv_check_forward("conv1d_split", d, x, w_packed, y, mfma_shape, tile_mode);
  if (rc != PWG_OK) return rc;
  const MfmaConvPlan p = mfma_conv_plan(d, g, PARTS, tile_mode, x, add1, add2);
  PWG_REQUIRE(step_form != kStepStreamed || split_image_addressable(image_elems(g)), PWG_ERR_UNSUPPORTED,
              "conv1d_split: weight image too large for the streamed step");
  // the prefetched window has the resident step: it is the plan's choice only where the plan's step is resident, and a
  // caller that names it gets it unless they also name the streamed step
  PWG_REQUIRE(window_form != kWindowPrefetched || step_form != kStepStreamed, PWG_ERR_UNSUPPORTED,
              "conv1d_split: the prefetched window (window_form = 2) has no streamed step (step_form = 2)");
  PWG_REQUIRE(window_form != kWindowPrefetched || p.vec, PWG_ERR_UNSUPPORTED,
              "conv1d_split: the prefetched window (window_form = 2) needs 16-B staging: t_in %% 4 == 0, x 16-B aligned, "
              "a window of at most %d columns", 2 * p.nt);
  PWG_REQUIRE(window_form != kWindowPrefetched || split_window_covers(p), PWG_ERR_UNSUPPORTED,
              "conv1d_split: the prefetched window (window_form = 2) needs %zu B of LDS (> %zu)", split_window_lds(p),
              kLdsPerCu);
  const bool prefetched = window_form == kWindowPrefetched ||
                          (window_form == kWindowPlanDecides && step_form == kStepPlanDecides &&
                           split_window_form(g, p) == kWindowPrefetched);
  const bool streamed = !prefetched && (step_form == kStepPlanDecides ? split_step_form(g) : step_form) == kStepStreamed;
  SplitArgs a;
  split_fill_args(&a, d, g, p, x, w_packed, bias, add1, add2, y);
  if (prefetched) {
    const size_t lds = split_window_lds(p);
    void (*kern)(SplitArgs) = mfma_shape == 32 ? mfma_conv_tile_kernel<WindowFamily::K, 32, SplitArgs>(p)
                                               : mfma_conv_tile_kernel<WindowFamily::K, 16, SplitArgs>(p);
    if (lds > kConvMaxLds && !lds_limit_is_set(reinterpret_cast<const void*>(kern), lds)) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds);
      PWG_REQUIRE(e == hipSuccess, PWG_ERR_LAUNCH, "conv1d_split: cannot raise LDS limit to %zu: %s", lds,
                  hipGetErrorString(e));
    }
    maybe_poison_lds(stream);
    ProfScope prof(stream, "conv1d_split_mfma_kernel", p.flops, p.bytes);
    hipLaunchKernelGGL(kern, p.grid, dim3(256), lds, stream, a);
    PWG_CHECK_LAUNCH("conv1d_split");
    return PWG_OK;
  }
  maybe_poison_lds(stream);
  ProfScope prof(stream, "conv1d_split_mfma_kernel", p.flops, p.bytes);
  if (p.vec) {
    if (streamed)
      mfma_conv_launch<Family<true, true>::K>(p, mfma_shape, a, stream);
    else
      mfma_conv_launch<Family<true, false>::K>(p, mfma_shape, a, stream);
  } else {
    if (streamed)
      mfma_conv_launch<Family<false, true>::K>(p, mfma_shape, a, stream);
    else
      mfma_conv_launch<Family<false, false>::K>(p, mfma_shape, a, stream);
  }
  PWG_CHECK_LAUNCH("conv1d_split");
  return PWG_OK;
}

// ---- ConvTranspose1d with kernel == 2 * stride: the polyphase contraction of mfma_conv.h -- rows
// m = co * s + phase, two taps (x[q - 1], x[q]), sample o = q * s + phase - padding -- under the numerical definition
// above, word for word: the same staging, the same split_step, the same six products in the same order.  What is its own
// is the operand order and the epilogue: the WEIGHT fragment is the first MFMA operand, so a lane owns 4 consecutive rows
// of one column q (mfma_acc_row), which are 4 consecutive samples of one output channel when s % 4 == 0.
struct ConvtrArgs : SplitArgs {
  int phases, out_off;  // stride and padding; wide_out additionally needs phases % 4 == 0 and out_off % 4 == 0
};

static int convtr_geometry(const pwg_conv1d_desc* d, MfmaConvGeom* g) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "convtr1d_split: NULL descriptor");
  PWG_REQUIRE(d->transposed, PWG_ERR_UNSUPPORTED,
              "convtr1d_split: not a transposed convolution (a stride-1 Conv1d runs on conv1d_split)");
  return mfma_conv_geometry("convtr1d_split", PARTS, true, d, g);
}

// The fp32 tail of a batch of N values of 4 samples, in the fp32 kernel's order (acc + bias + add1 + add2, * out_mul,
// / out_div, post-activation); bias: per sample (the 4 samples of a value may lie in different channels).  Every switch
// is wave-uniform and taken once per batch.  The four scalars come by value: read through a reference to the argument
// struct, 16 of the 20 instantiations kept a piece of it in 24 B of scratch (profiles/convtr_split_resources.txt).
template <int N>
__device__ __forceinline__ void convtr_finish(float out_mul, float out_div, int post_act, float post_slope, f32x4 (&v)[N],
                                              const f32x4& bias, bool has_bias, bool has1, bool has2,
                                              const f32x4 (&t1)[N], const f32x4 (&t2)[N]) {
  if (has_bias) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += bias;
  }
  if (has1) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += t1[k];
  }
  if (has2) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += t2[k];
  }
  if (out_mul != 1.0f) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] *= out_mul;
  }
  if (out_div != 1.0f) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = v[k] / out_div;
  }
  if (post_act == PWG_ACT_LEAKY_RELU) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = v[k][e] > 0.f ? v[k][e] : v[k][e] * post_slope;
  } else if (post_act == PWG_ACT_RELU) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = v[k][e] > 0.f ? v[k][e] : 0.f;
  } else if (post_act == PWG_ACT_TANH) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[k][e] = tanhf(v[k][e]);
      __builtin_amdgcn_sched_barrier(0);  // one value's tanhf at a time, as in split_epilogue
    }
  }
}

// The epilogue of one wave.  Accumulator registers 4 g .. 4 g + 3 of tile (mi, ni) are rows m4 .. m4 + 3
// (m4 = row0 + mi * TILE + 4 * (64 / TILE) * g, row0 includes 4 * lane_group) of column col0 + ni * TILE: one "value".
// The structure is split_epilogue's: wave-uniform switches once per batch around straight-line code, the add1 / add2
// loads of a batch issued together and waited for once, no store waited for.
// WIDE (s % 4 == 0, padding % 4 == 0, t_out % 4 == 0, y / add1 / add2 16-B aligned): the 4 rows are phases ph .. ph + 3
// of ONE channel, the value is the 4 samples from o = q * s + ph - padding, 16-B aligned and wholly inside [0, t_out) or
// wholly outside it; a batch is the TN values of one (mi, g); a 16-lane group covers 16 columns of a row.  FULL: the
// tile has no padded row and no sample outside [0, t_out); otherwise a load of a missing value reads a clamped address
// and its store is masked.
// Otherwise 4-B accesses, a (channel, phase) per sample and batches of one value: s == 2 (two channels x two phases, the
// pair of a channel starting at the odd sample 2 q - 1), odd strides (rows straddle channels), ragged or unaligned rows.
// Samples with o < 0 or o >= t_out (first and last q) and padded rows are never written.
template <int TILE, int TM, int TN, bool WIDE, bool FULL>
__device__ __forceinline__ void convtr_epilogue(const ConvtrArgs& a, const typename Mfma<TILE>::acc_t (&acc)[TM][TN],
                                                int row0, int col0, size_t out_base) {
  constexpr int HL = 64 / TILE, NG = TILE * TILE / 64 / 4;
  const bool has_bias = a.bias != nullptr, has1 = a.add1 != nullptr, has2 = a.add2 != nullptr;
  const int s = a.phases, post_act = a.post_act;
  const float out_mul = a.out_mul, out_div = a.out_div, post_slope = a.post_slope;
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int m4 = row0 + mi * TILE + 4 * HL * g;
      if (WIDE) {
        const int mc = FULL ? m4 : min(m4, a.m - 4);  // a.m = c_out * s is a multiple of 4
        const int co = mc / s, ph = mc - co * s;
        const size_t row = out_base + (size_t)co * a.t_out;
        int o[TN];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) o[ni] = (col0 + ni * TILE) * s + ph - a.out_off;
        auto load = [&](const float* __restrict__ src, f32x4 (&t)[TN]) {
#pragma unroll
          for (int ni = 0; ni < TN; ++ni)
            t[ni] = *reinterpret_cast<const f32x4*>(src + row + (FULL ? o[ni] : min(max(o[ni], 0), a.t_out - 4)));
        };
        f32x4 t1[TN], t2[TN], v[TN];
        float b = 0.f;
        if (has_bias) b = a.bias[co];
        if (has1) load(a.add1, t1);
        if (has2) load(a.add2, t2);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[ni][e] = acc[mi][ni][g * 4 + e];
        const f32x4 bias = {b, b, b, b};
        convtr_finish<TN>(out_mul, out_div, post_act, post_slope, v, bias, has_bias, has1, has2, t1, t2);
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
          if (FULL || (m4 < a.m && o[ni] >= 0 && o[ni] < a.t_out)) *reinterpret_cast<f32x4*>(a.y + row + o[ni]) = v[ni];
      } else {
        // (channel, phase) of the 4 rows: one division per (mi, g), then counted up
        int co = m4 / s, ph = m4 - co * s;
        size_t row[4];
        int phr[4];
        f32x4 bias = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int cc = min(co, a.c_out - 1);
          row[e] = out_base + (size_t)cc * a.t_out;
          phr[e] = ph - a.out_off;
          if (has_bias) bias[e] = a.bias[cc];
          if (++ph == s) ph = 0, ++co;
        }
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int qs = (col0 + ni * TILE) * s;
          f32x4 t1[1], t2[1], v[1];
          if (has1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) t1[0][e] = a.add1[row[e] + min(max(qs + phr[e], 0), a.t_out - 1)];
          }
          if (has2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) t2[0][e] = a.add2[row[e] + min(max(qs + phr[e], 0), a.t_out - 1)];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[0][e] = acc[mi][ni][g * 4 + e];
          convtr_finish<1>(out_mul, out_div, post_act, post_slope, v, bias, has_bias, has1, has2, t1, t2);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int o = qs + phr[e];
            if (m4 + e < a.m && o >= 0 && o < a.t_out) a.y[row[e] + o] = v[0][e];
          }
        }
      }
    }
  }
}

// The tile ladder, VEC and the second launch bound are those of conv1d_split_mfma_kernel.
template <int TILE, int WM, int WN, int WAVES_M, bool VEC>
__global__ __launch_bounds__(256, WM * WN == 4 ? (TILE == 16 ? 3 : 2) : (WM * WN == 2 ? 3 : 4)) void
convtr1d_split_mfma_kernel(ConvtrArgs a) {
  constexpr int HL = 64 / TILE;
  constexpr int KSTEPS = KC / (8 * HL);
  constexpr int TM = WM * 32 / TILE, TN = WN * 32 / TILE;
  constexpr int NREG = TILE * TILE / 64;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int MT = WAVES_M * WM * 32, NT = WAVES_N * WN * 32;
  typedef typename Mfma<TILE>::acc_t acc_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [part][column][ROW]

  const MfmaConvTile c = mfma_conv_tile<TILE, MT, NT, WAVES_M, VEC>(a);

  acc_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < NREG; ++i) acc[mi][ni][i] = 0.f;

  for (int chunk = 0; chunk < a.cin_chunks; ++chunk) {
    if (chunk) __syncthreads();
    split_staged(a, [&](auto act) { stage_chunk<NT, VEC>(a, c, chunk, xs, act); });
    __syncthreads();
    for (int tap = 0; tap < a.taps; ++tap) {
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const int oct = ks * HL + c.h;
        const bf16x8* __restrict__ wp =
            image_rows(a.w, a.cin_chunks, a.m_pad, tap, chunk, oct) + c.m0 + c.wave_m * (WM * 32) + c.r;
        // the weight fragment goes first: a lane gets 4 consecutive rows (phases) of a column (convtr_epilogue)
        split_step<TILE, TM, TN, kConvRow, false>(wp, a.part_stride, xs, c.sh + c.wave_n * (WN * 32) + c.r + tap * a.dil,
                                                  oct * 8, a.plane, acc);
      }
    }
  }

  const size_t out_base = (size_t)c.b * a.c_out * a.t_out;
  const int row0 = c.m0 + c.wave_m * (WM * 32) + 4 * c.h, col0 = c.q0 + c.wave_n * (WN * 32) + c.r;
  // no padded row, and every sample of the tile's columns inside the output row
  const bool full = c.m0 + MT <= a.m && c.q0 * a.phases >= a.out_off && (c.q0 + NT) * a.phases - a.out_off <= a.t_out;
  if (!a.wide_out)
    convtr_epilogue<TILE, TM, TN, false, false>(a, acc, row0, col0, out_base);
  else if (full)
    convtr_epilogue<TILE, TM, TN, true, true>(a, acc, row0, col0, out_base);
  else
    convtr_epilogue<TILE, TM, TN, true, false>(a, acc, row0, col0, out_base);
}

template <bool VEC>
struct ConvtrFamily {
  template <int TILE, int WM, int WN, int WAVES_M>
  struct K {
    static constexpr auto fn = convtr1d_split_mfma_kernel<TILE, WM, WN, WAVES_M, VEC>;
  };
};

static int convtr_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                          const float* add1, const float* add2, float* y, int mfma_shape, int tile_mode,
                          hipStream_t stream) {
  MfmaConvGeom g;
  int rc = convtr_geometry(d, &g);
  if (rc == PWG_OK) rc = mfma_conv_check_forward("convtr1d_split", d, x, w_packed, y, mfma_shape, tile_mode);
  if (rc != PWG_OK) return rc;
  // 32-bit sample index q * s + phase - padding of a column past the end of the last tile
  PWG_REQUIRE((long)(g.nq + 256) * g.phases < (1L << 31), PWG_ERR_UNSUPPORTED, "convtr1d_split: output row too long");
  const MfmaConvPlan p = mfma_conv_plan(d, g, PARTS, tile_mode, x, add1, add2);
  ConvtrArgs a;
  split_fill_args(&a, d, g, p, x, w_packed, bias, add1, add2, y);
  a.phases = g.phases;
  a.out_off = g.out_off;
  a.wide_out = a.wide_out && g.phases % 4 == 0 && g.out_off % 4 == 0;
  maybe_poison_lds(stream);
  ProfScope prof(stream, "convtr1d_split_mfma_kernel", p.flops, p.bytes);
  if (p.vec)
    mfma_conv_launch<ConvtrFamily<true>::K>(p, mfma_shape, a, stream);
  else
    mfma_conv_launch<ConvtrFamily<false>::K>(p, mfma_shape, a, stream);
  PWG_CHECK_LAUNCH("convtr1d_split");
  return PWG_OK;
}

// MFMA shape of pwg_conv1d_split_forward and pwg_convtr1d_split_forward (both are built at the same tiles)
constexpr int kDefaultMfmaShape = 16;

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_conv1d_split_supported(const pwg_conv1d_desc* d) {
  MfmaConvGeom g;
  return split_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_conv1d_split_packed_weight_bytes(const pwg_conv1d_desc* d) {
  MfmaConvGeom g;
  if (split_geometry(d, &g) != PWG_OK) return 0;
  return (size_t)PARTS * image_elems(g) * sizeof(__bf16);
}

extern "C" int pwg_conv1d_split_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                            void* stream) {
  MfmaConvGeom g;
  int rc = split_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(w && w_packed, PWG_ERR_NULL, "conv1d_split_pack_weight: NULL pointer");
  mfma_conv_pack<PARTS>(d, g, w, scale, w_packed, (hipStream_t)stream);
  PWG_CHECK_LAUNCH("conv1d_split_pack_weight");
  return PWG_OK;
}

extern "C" int pwg_conv1d_split_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                        const float* add1, const float* add2, float* y, float* workspace,
                                        size_t workspace_floats, void* stream) {
  (void)workspace;  // no split reduction: one workgroup owns an output tile
  (void)workspace_floats;
  return split_forward(d, x, w_packed, bias, add1, add2, y, kDefaultMfmaShape, 0, kStepPlanDecides, kWindowPlanDecides,
                       (hipStream_t)stream);
}

extern "C" int pwg_conv1d_split_forward_cfg(const pwg_conv1d_desc* d, const float* x, const void* w_packed,
                                            const float* bias, const float* add1, const float* add2, float* y,
                                            int32_t mfma_shape, int32_t tile_mode, void* stream) {
  return split_forward(d, x, w_packed, bias, add1, add2, y, mfma_shape, tile_mode, kStepPlanDecides, kWindowPlanDecides,
                       (hipStream_t)stream);
}

extern "C" int pwg_conv1d_split_forward_step(const pwg_conv1d_desc* d, const float* x, const void* w_packed,
                                             const float* bias, const float* add1, const float* add2, float* y,
                                             int32_t mfma_shape, int32_t tile_mode, int32_t step_form, void* stream) {
  return split_forward(d, x, w_packed, bias, add1, add2, y, mfma_shape, tile_mode, step_form, kWindowPlanDecides,
                       (hipStream_t)stream);
}

extern "C" int pwg_conv1d_split_forward_window(const pwg_conv1d_desc* d, const float* x, const void* w_packed,
                                               const float* bias, const float* add1, const float* add2, float* y,
                                               int32_t mfma_shape, int32_t tile_mode, int32_t step_form,
                                               int32_t window_form, void* stream) {
  return split_forward(d, x, w_packed, bias, add1, add2, y, mfma_shape, tile_mode, step_form, window_form,
                       (hipStream_t)stream);
}

// the plan of the default launch (small-grid rule, aligned pointers)
extern "C" int pwg_conv1d_split_window_form(const pwg_conv1d_desc* d) {
  MfmaConvGeom g;
  if (split_geometry(d, &g) != PWG_OK) return 0;
  return split_window_form(g, mfma_conv_plan(d, g, PARTS, 0, nullptr, nullptr, nullptr));
}

extern "C" int pwg_conv1d_split_step_form(const pwg_conv1d_desc* d) {
  MfmaConvGeom g;
  if (split_geometry(d, &g) != PWG_OK) return 0;
  return split_step_form(g);
}

extern "C" int pwg_convtr1d_split_supported(const pwg_conv1d_desc* d) {
  MfmaConvGeom g;
  return convtr_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_convtr1d_split_packed_weight_bytes(const pwg_conv1d_desc* d) {
  MfmaConvGeom g;
  if (convtr_geometry(d, &g) != PWG_OK) return 0;
  return (size_t)PARTS * image_elems(g) * sizeof(__bf16);
}

extern "C" int pwg_convtr1d_split_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                              void* stream) {
  MfmaConvGeom g;
  int rc = convtr_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(w && w_packed, PWG_ERR_NULL, "convtr1d_split_pack_weight: NULL pointer");
  mfma_conv_pack<PARTS>(d, g, w, scale, w_packed, (hipStream_t)stream);
  PWG_CHECK_LAUNCH("convtr1d_split_pack_weight");
  return PWG_OK;
}

extern "C" int pwg_convtr1d_split_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                          const float* add1, const float* add2, float* y, float* workspace,
                                          size_t workspace_floats, void* stream) {
  (void)workspace;  // no split reduction: one workgroup owns an output tile
  (void)workspace_floats;
  return convtr_forward(d, x, w_packed, bias, add1, add2, y, kDefaultMfmaShape, 0, (hipStream_t)stream);
}

extern "C" int pwg_convtr1d_split_forward_cfg(const pwg_conv1d_desc* d, const float* x, const void* w_packed,
                                              const float* bias, const float* add1, const float* add2, float* y,
                                              int32_t mfma_shape, int32_t tile_mode, void* stream) {
  return convtr_forward(d, x, w_packed, bias, add1, add2, y, mfma_shape, tile_mode, (hipStream_t)stream);
}
