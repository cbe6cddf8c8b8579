// conv1d_split.hip -- fp32-accurate inference convolution on the gfx950 bf16 MFMA instructions: both operands are split
// into three bf16 parts and six of the nine part products are accumulated in fp32.
//
// Numerical definition (include/pwg_kernels.h, "split-operand inference"): an fp32 value v is split exactly as
//   hi = bf16_rne(v),  r = v - float(hi),  mid = bf16_rne(r),  lo = bf16_rne(r - float(mid))        (v == hi + mid + lo)
// for finite v whose low parts are not subnormal.  The fused pre-activation is applied to the fp32 input in fp32, then the
// activated input is split while it is staged; the effective fp32 weight (w * scale) is split once when the weight image
// is packed.  Per operand pair the products lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (weight part . input part) are
// issued in this order -- small terms first -- into ONE fp32 accumulator set; each of the three dropped products
// (mid.lo, lo.mid, lo.lo) is <= 2^-24 of the full product in the worst case (|mid| <= 2^-8 |v|, |lo| <= 2^-16 |v|) and
// about 2^-28 of it on average.  A bf16 x bf16 product is exact in fp32, so what is left is
// the fp32 accumulation of the MFMA.  bias / add1 / add2 / out_mul / out_div / post-activation / the stored result are
// fp32, in the order of the fp32 kernel.
// Non-finite inputs give non-finite outputs, but not necessarily the same ones: hi(inf) = inf and r = inf - inf = NaN, so
// an inf comes out as NaN.  There is no branch for it.
//
// Scope: stride-1 Conv1d, groups 1, width 1, zero padding, forward only.
// Layout and tiles are those of csrc/conv1d_bf16.hip: A operand = three weight images [part][tap][ci / 8][m_pad][8] read
// from global memory (L2-resident), B operand = three bf16 planes of the x window in LDS, rows of 80 B, staged per
// 32-channel chunk.  A wave holds all A and B fragments of a reduction step (3 x TM + 3 x TN) and issues 6 x TM x TN
// MFMAs on them: six times the MFMA work of the bf16 kernel behind the same global loads and barriers.
// Tiles (rows x columns, 4 waves): 128 x 128 above 64 rows, 64 x 128 for 33 .. 64 rows, 32 x 256 up to 32 rows; launches of
// fewer than 256 such workgroups run on 64 x 64 / 32 x 128 tiles, and so does a window whose three planes do not fit 64 KB
// of LDS at the full-size column tile (32 rows, k = 11 at dilation 5).
// Deterministic: one workgroup owns an output tile, no split reduction, no atomics; the accumulation order of an element
// (chunk, tap, reduction step, product) does not depend on the tile or the grid.
#include "common.h"
#include "bf16_mfma.h"

namespace pwg {
namespace {

constexpr int KC = 32;       // input channels per staged chunk
constexpr int ROW = KC + 8;  // bf16 elements per LDS row (80 B)
constexpr int PARTS = 3;
constexpr size_t kMaxLds = 64 * 1024;
constexpr int kSmallGridWorkgroups = 256;  // one per CU

// LDS rows of one plane of a column tile (as in conv1d_bf16.hip): nt + halo columns, up to 3 in front for the 16-B
// aligned start of the vector staging, rounded up to whole groups of 4 columns
static inline int plane_rows(int nt, int halo) { return round_up(nt + halo + 3, 4); }
static inline size_t lds_bytes(int nt, int halo) { return (size_t)PARTS * plane_rows(nt, halo) * ROW * sizeof(__bf16); }

struct SplitGeom {
  int taps, dil, x_off;
  int m, m_pad, mt, nt;
  int nq, cin_chunks;
  bool half_only;  // three planes of the full-size column tile do not fit LDS: half-size tiles whatever the grid
};

struct SplitArgs {
  const float* x;
  const bf16x8* w;
  const float* bias;
  const float* add1;
  const float* add2;
  float* y;
  int c_in, c_out, t_in, t_out;
  int m, m_pad, cin_chunks, taps, dil, x_off, nq;
  int plane;         // bf16 elements per LDS plane
  long part_stride;  // bf16x8 elements per weight part image
  float pre_mul;      // pre-activation, one branch-free form for none / leaky / relu (pre_activate)
  unsigned pre_mask;
  int post_act;
  float post_slope, out_mul, out_div;
  int wide_out;  // y / add1 / add2 are 16-B aligned and t_out % 4 == 0: 16-B accesses in the epilogue
};

static int split_geometry(const pwg_conv1d_desc* d, SplitGeom* g) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "conv1d_split: NULL descriptor");
  PWG_REQUIRE(d->batch > 0 && d->c_in > 0 && d->c_out > 0 && d->t_in > 0 && d->t_out > 0 && d->kernel > 0 &&
                  d->stride > 0 && d->dilation > 0 && d->groups > 0 && d->width > 0 && d->pad_left >= 0,
              PWG_ERR_BAD_SHAPE, "conv1d_split: non-positive size in descriptor");
  PWG_REQUIRE(d->groups == 1, PWG_ERR_UNSUPPORTED, "conv1d_split: groups = %d (only groups == 1)", d->groups);
  PWG_REQUIRE(d->width == 1, PWG_ERR_UNSUPPORTED, "conv1d_split: width = %d (only width == 1)", d->width);
  PWG_REQUIRE(d->pad_mode == PWG_PAD_ZERO, PWG_ERR_UNSUPPORTED, "conv1d_split: only zero padding (pad_mode = %d)",
              d->pad_mode);
  PWG_REQUIRE(!d->transposed, PWG_ERR_UNSUPPORTED, "conv1d_split: transposed convolutions are not covered");
  PWG_REQUIRE(d->stride == 1, PWG_ERR_UNSUPPORTED, "conv1d_split: stride = %d (only stride 1)", d->stride);
  PWG_REQUIRE(d->pre_act == PWG_ACT_NONE || d->pre_act == PWG_ACT_LEAKY_RELU || d->pre_act == PWG_ACT_RELU,
              PWG_ERR_UNSUPPORTED, "conv1d_split: pre_act = %d", d->pre_act);
  PWG_REQUIRE(d->batch <= 65535, PWG_ERR_UNSUPPORTED, "conv1d_split: batch = %d (> 65535)", d->batch);
  g->taps = d->kernel;
  g->dil = d->dilation;
  g->x_off = -d->pad_left;
  g->m = d->c_out;
  g->nq = d->t_out;
  g->mt = g->m <= 32 ? 32 : (g->m <= 64 ? 64 : 128);
  g->nt = g->m <= 32 ? 256 : 128;
  g->m_pad = round_up(g->m, g->mt);
  g->cin_chunks = ceil_div(d->c_in, KC);
  PWG_REQUIRE((long)(g->taps - 1) * g->dil < (1 << 20), PWG_ERR_UNSUPPORTED, "conv1d_split: receptive field too long");
  g->half_only = lds_bytes(g->nt, (g->taps - 1) * g->dil) > kMaxLds;
  const size_t lds = lds_bytes(g->half_only ? g->nt / 2 : g->nt, (g->taps - 1) * g->dil);
  PWG_REQUIRE(lds <= kMaxLds, PWG_ERR_UNSUPPORTED, "conv1d_split: receptive field (%d taps, dilation %d) needs %zu B of LDS",
              g->taps, g->dil, lds);
  PWG_REQUIRE(ceil_div(g->m_pad, g->mt) <= 65535, PWG_ERR_UNSUPPORTED, "conv1d_split: too many row blocks");
  return PWG_OK;
}

// the exact 3-way split of the header comment
__device__ __forceinline__ void split3(float v, __bf16& hi, __bf16& mid, __bf16& lo) {
  hi = (__bf16)v;
  const float r = v - (float)hi;
  mid = (__bf16)r;
  lo = (__bf16)(r - (float)mid);
}

// The pre-activation without control flow: v > 0 ? v : bits(v * mul) & mask, with (mul, mask) = (1, ~0) for none,
// (slope, ~0) for leaky and (0, 0) for relu.  For finite v these are the bits of apply_act(): v * 1 is v, v * slope is
// the same rounded product, and the relu's negative side is +0.0 (the mask clears the sign of v * 0).
__device__ __forceinline__ float pre_activate(float v, float mul, unsigned mask) {
  const float n = __uint_as_float(__float_as_uint(v * mul) & mask);
  return v > 0.f ? v : n;
}

// one thread per element of ONE part image [tap][ci / 8][m_pad][8], writing that element of all three parts; padding
// rows / channels are zero
__global__ __launch_bounds__(256) void pack_weight_split_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                                __bf16* __restrict__ wp, int c_in, int kernel, int cin_pad,
                                                                int m, int m_pad) {
  const long total = (long)kernel * cin_pad * m_pad;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const int j = (int)(i & 7);
    long rest = i >> 3;
    const int row = (int)(rest % m_pad);
    rest /= m_pad;
    const int oct = (int)(rest % (cin_pad / 8));
    const int tap = (int)(rest / (cin_pad / 8));
    const int ci = oct * 8 + j;
    float v = 0.f;
    if (ci < c_in && row < m) {
      v = w[((long)row * c_in + ci) * kernel + tap];
      if (scale) v *= scale[row];
    }
    __bf16 hi, mid, lo;
    split3(v, hi, mid, lo);
    wp[i] = hi;
    wp[total + i] = mid;
    wp[2 * total + i] = lo;
  }
}

// Vector staging of one 32-channel chunk of the x window (xc: channel 0 of the chunk, c_left channels are left).
// item = (group of 4 columns, channel octet): 8 loads of 16 B (one per channel, lanes walk t), then per column 8 channels
// are activated, split and written as three 16-B LDS stores (one per plane).  CHECKED (edge tiles): a load whose group
// of columns lies outside the row or whose channel is past the end gives zeros.
template <int NT, bool CHECKED>
__device__ __forceinline__ void stage_window_vec(const SplitArgs& a, const float* __restrict__ xc, int c_left, int base,
                                                 int ngroups, __bf16* xs, int tid) {
  constexpr int ITEMS = NT >= 128 ? NT / 128 : 1;
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
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (tin && oct * 8 + j < c_left) v = *reinterpret_cast<const f32x4*>(src + (size_t)j * a.t_in);
        st[it][j] = v;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const int idx = tid + it * 256, oct = idx & 3, grp = idx >> 2;
    if (grp < ngroups) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bf16x8 vh, vm, vl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          __bf16 hi, mid, lo;
          split3(pre_activate(st[it][j][e], a.pre_mul, a.pre_mask), hi, mid, lo);
          vh[j] = hi;
          vm[j] = mid;
          vl[j] = lo;
        }
        __bf16* dst = xs + (grp * 4 + e) * ROW + oct * 8;
        *reinterpret_cast<bf16x8*>(dst) = vh;
        *reinterpret_cast<bf16x8*>(dst + a.plane) = vm;
        *reinterpret_cast<bf16x8*>(dst + 2 * a.plane) = vl;
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

// Template parameters as in conv1d_bf16.hip.  TILE: MFMA shape (32: 32x32x16, 16: 16x16x32).  A wave computes (WM * 32)
// rows x (WN * 32) columns; the 4 waves of a workgroup are arranged WAVES_M x (4 / WAVES_M).  VEC: the x window is staged
// with 16-B loads along t (rows 16-B aligned, t_in % 4 == 0, window <= 2 * NT columns) and transposed in registers.
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

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_m = wave % WAVES_M, wave_n = wave / WAVES_M;
  const int r = lane & (TILE - 1), h = lane / TILE;
  const int q0 = blockIdx.x * NT, m0 = blockIdx.y * MT, b = blockIdx.z;
  const int start = q0 + a.x_off;               // input column of (local column 0, tap 0)
  const int base = VEC ? (start & ~3) : start;  // first staged input column (VEC: 16-B aligned, also when negative)
  const int sh = start - base;                  // 0 .. 3
  const int wcols = NT + (a.taps - 1) * a.dil + sh;
  const float* __restrict__ xb = a.x + (size_t)b * a.c_in * a.t_in;

  acc_t acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < NREG; ++i) acc[mi][ni][i] = 0.f;

  for (int chunk = 0; chunk < a.cin_chunks; ++chunk) {
    if (chunk) __syncthreads();
    if (VEC) {
      // an interior tile (decided once per workgroup and chunk: every staged column inside the row, a whole chunk of
      // channels) takes unconditional loads; an edge tile checks every load
      const int ngroups = (wcols + 3) >> 2, c_left = a.c_in - chunk * KC;
      const float* __restrict__ xc = xb + (size_t)chunk * KC * a.t_in;
      if (base >= 0 && base + 4 * ngroups <= a.t_in && c_left >= KC)
        stage_window_vec<NT, false>(a, xc, c_left, base, ngroups, xs, tid);
      else
        stage_window_vec<NT, true>(a, xc, c_left, base, ngroups, xs, tid);
    } else {
      // wave `wave` stages channel octet `wave` of the chunk: lanes walk the columns (coalesced fp32 rows)
      const int c_base = chunk * KC + wave * 8;
      const bool interior = base >= 0 && base + wcols <= a.t_in && c_base + 8 <= a.c_in;  // per wave and chunk
      for (int col = lane; col < wcols; col += 64) {
        const int t = base + col;
        const float* __restrict__ src = xb + (size_t)c_base * a.t_in + t;
        float f[8];
        if (interior) {
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = src[(size_t)j * a.t_in];
        } else {
          const bool tin = t >= 0 && t < a.t_in;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            f[j] = 0.f;
            if (tin && c_base + j < a.c_in) f[j] = src[(size_t)j * a.t_in];
          }
        }
        bf16x8 vh, vm, vl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          __bf16 hi, mid, lo;
          split3(pre_activate(f[j], a.pre_mul, a.pre_mask), hi, mid, lo);
          vh[j] = hi;
          vm[j] = mid;
          vl[j] = lo;
        }
        __bf16* dst = xs + col * ROW + wave * 8;
        *reinterpret_cast<bf16x8*>(dst) = vh;
        *reinterpret_cast<bf16x8*>(dst + a.plane) = vm;
        *reinterpret_cast<bf16x8*>(dst + 2 * a.plane) = vl;
      }
    }
    __syncthreads();
    for (int tap = 0; tap < a.taps; ++tap) {
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const int oct = ks * HL + h;
        const bf16x8* __restrict__ wp =
            a.w + ((size_t)(tap * a.cin_chunks + chunk) * (KC / 8) + oct) * a.m_pad + m0 + wave_m * (WM * 32) + r;
        bf16x8 af[PARTS][TM], bfr[PARTS][TN];  // [0] hi, [1] mid, [2] lo
#pragma unroll
        for (int p = 0; p < PARTS; ++p)
#pragma unroll
          for (int mi = 0; mi < TM; ++mi) af[p][mi] = wp[p * a.part_stride + mi * TILE];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int col = sh + wave_n * (WN * 32) + ni * TILE + r + tap * a.dil;
          const __bf16* src = xs + col * ROW + oct * 8;
#pragma unroll
          for (int p = 0; p < PARTS; ++p) bfr[p][ni] = *reinterpret_cast<const bf16x8*>(src + p * a.plane);
        }
        // (weight part, input part), small terms first.  The x fragment goes first: the same products summed in the
        // same order, the tile transposed (a lane gets 4 consecutive samples of a row, split_epilogue)
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
        constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = Mfma<TILE>::run(bfr[PB[p]][ni], af[PA[p]][mi], acc[mi][ni]);
      }
    }
  }

  const size_t out_base = (size_t)b * a.c_out * a.t_out;
  const int row0 = m0 + wave_m * (WM * 32) + r, col0 = q0 + wave_n * (WN * 32) + 4 * h;
  const bool full = m0 + MT <= a.m && q0 + NT <= a.nq;  // no padded row and no column past the end in this tile
  if (!a.wide_out)
    split_epilogue<TILE, TM, TN, false, false>(a, acc, row0, col0, out_base);
  else if (full)
    split_epilogue<TILE, TM, TN, true, true>(a, acc, row0, col0, out_base);
  else
    split_epilogue<TILE, TM, TN, true, false>(a, acc, row0, col0, out_base);
}

template <int TILE, bool VEC>
static void launch_tile(const SplitGeom& g, const SplitArgs& a, int batch, bool small, size_t lds, hipStream_t stream) {
  const int mt = small ? (g.mt > 32 ? 64 : 32) : g.mt, nt = small ? g.nt / 2 : g.nt;
  const dim3 grid(ceil_div(g.nq, nt), g.m_pad / mt, batch);
  if (small && mt == 32)  // 32 x 128
    hipLaunchKernelGGL((conv1d_split_mfma_kernel<TILE, 1, 1, 1, VEC>), grid, dim3(256), lds, stream, a);
  else if (small)  // 64 x 64
    hipLaunchKernelGGL((conv1d_split_mfma_kernel<TILE, 1, 1, 2, VEC>), grid, dim3(256), lds, stream, a);
  else if (g.mt == 32)  // 32 x 256
    hipLaunchKernelGGL((conv1d_split_mfma_kernel<TILE, 1, 2, 1, VEC>), grid, dim3(256), lds, stream, a);
  else if (g.mt == 64)  // 64 x 128
    hipLaunchKernelGGL((conv1d_split_mfma_kernel<TILE, 1, 2, 2, VEC>), grid, dim3(256), lds, stream, a);
  else  // 128 x 128
    hipLaunchKernelGGL((conv1d_split_mfma_kernel<TILE, 2, 2, 2, VEC>), grid, dim3(256), lds, stream, a);
}

// tile_mode: 0 = the small-grid rule decides, 1 = full-size tiles (where their three planes fit LDS), 2 = half-size tiles
static int split_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                         const float* add1, const float* add2, float* y, int mfma_shape, int tile_mode,
                         hipStream_t stream) {
  SplitGeom g;
  int rc = split_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(x && w_packed && y, PWG_ERR_NULL, "conv1d_split: NULL pointer");
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_split: the weight image must be 16-B aligned");
  PWG_REQUIRE(mfma_shape == 16 || mfma_shape == 32, PWG_ERR_BAD_SHAPE, "conv1d_split: mfma_shape = %d (16 or 32)",
              mfma_shape);
  PWG_REQUIRE(tile_mode >= 0 && tile_mode <= 2, PWG_ERR_BAD_SHAPE, "conv1d_split: tile_mode = %d (0, 1 or 2)", tile_mode);
  PWG_REQUIRE(d->post_act >= PWG_ACT_NONE && d->post_act <= PWG_ACT_RELU, PWG_ERR_BAD_SHAPE, "conv1d_split: post_act = %d",
              d->post_act);
  const int halo = (g.taps - 1) * g.dil;
  // short inputs: a launch that would not give every CU a workgroup runs on half-size tiles (the weight image is the
  // same); the accumulation order of an output element does not depend on the tile
  const bool small = g.half_only || (tile_mode == 0 ? (long)ceil_div(g.nq, g.nt) * (g.m_pad / g.mt) * d->batch <
                                                          kSmallGridWorkgroups
                                                    : tile_mode == 2);
  const int nt = small ? g.nt / 2 : g.nt;
  SplitArgs a;
  a.x = x;
  a.w = static_cast<const bf16x8*>(w_packed);
  a.bias = bias;
  a.add1 = add1;
  a.add2 = add2;
  a.y = y;
  a.c_in = d->c_in;
  a.c_out = d->c_out;
  a.t_in = d->t_in;
  a.t_out = d->t_out;
  a.m = g.m;
  a.m_pad = g.m_pad;
  a.cin_chunks = g.cin_chunks;
  a.taps = g.taps;
  a.dil = g.dil;
  a.x_off = g.x_off;
  a.nq = g.nq;
  a.plane = plane_rows(nt, halo) * ROW;
  a.part_stride = (long)g.taps * g.cin_chunks * (KC / 8) * g.m_pad;
  a.pre_mul = d->pre_act == PWG_ACT_LEAKY_RELU ? d->pre_slope : (d->pre_act == PWG_ACT_RELU ? 0.0f : 1.0f);
  a.pre_mask = d->pre_act == PWG_ACT_RELU ? 0u : ~0u;
  a.post_act = d->post_act;
  a.post_slope = d->post_slope;
  a.out_mul = d->out_mul;
  a.out_div = d->out_div;
  a.wide_out = d->t_out % 4 == 0 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(add1) |
                                      reinterpret_cast<uintptr_t>(add2)) & 15u) == 0;
  const size_t lds = lds_bytes(nt, halo);
  // vector staging: 16-B loads along t need aligned rows, and the window must fit the per-thread register items
  const bool vec = d->t_in % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0 &&
                   nt + halo + 3 <= (nt >= 128 ? 2 * nt : 256);
  const double out_elems = (double)d->batch * d->c_out * d->t_out;
  const double in_elems = (double)d->batch * d->c_in * d->t_in;
  // the ALGORITHMIC flops of the convolution, not the six products that are executed
  const double flops = 2.0 * (double)d->batch * g.m * g.nq * g.taps * d->c_in;
  const double bytes = 4.0 * (in_elems + out_elems * (1 + (add1 ? 1 : 0) + (add2 ? 1 : 0))) +
                       2.0 * PARTS * (double)g.taps * g.cin_chunks * KC * g.m_pad;
  maybe_poison_lds(stream);
  ProfScope prof(stream, "conv1d_split_mfma_kernel", flops, bytes);
  if (mfma_shape == 32) {
    if (vec)
      launch_tile<32, true>(g, a, d->batch, small, lds, stream);
    else
      launch_tile<32, false>(g, a, d->batch, small, lds, stream);
  } else {
    if (vec)
      launch_tile<16, true>(g, a, d->batch, small, lds, stream);
    else
      launch_tile<16, false>(g, a, d->batch, small, lds, stream);
  }
  PWG_CHECK_LAUNCH("conv1d_split");
  return PWG_OK;
}

// MFMA shape of pwg_conv1d_split_forward (both are built at the same tiles)
constexpr int kDefaultMfmaShape = 16;

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_conv1d_split_supported(const pwg_conv1d_desc* d) {
  SplitGeom g;
  return split_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_conv1d_split_packed_weight_bytes(const pwg_conv1d_desc* d) {
  SplitGeom g;
  if (split_geometry(d, &g) != PWG_OK) return 0;
  return (size_t)PARTS * g.taps * g.cin_chunks * KC * g.m_pad * sizeof(__bf16);
}

extern "C" int pwg_conv1d_split_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                            void* stream) {
  SplitGeom g;
  int rc = split_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(w && w_packed, PWG_ERR_NULL, "conv1d_split_pack_weight: NULL pointer");
  const long total = (long)g.taps * g.cin_chunks * KC * g.m_pad;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_weight_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, scale,
                     static_cast<__bf16*>(w_packed), d->c_in, d->kernel, g.cin_chunks * KC, g.m, g.m_pad);
  PWG_CHECK_LAUNCH("conv1d_split_pack_weight");
  return PWG_OK;
}

extern "C" int pwg_conv1d_split_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                        const float* add1, const float* add2, float* y, float* workspace,
                                        size_t workspace_floats, void* stream) {
  (void)workspace;  // no split reduction: one workgroup owns an output tile
  (void)workspace_floats;
  return split_forward(d, x, w_packed, bias, add1, add2, y, kDefaultMfmaShape, 0, (hipStream_t)stream);
}

extern "C" int pwg_conv1d_split_forward_cfg(const pwg_conv1d_desc* d, const float* x, const void* w_packed,
                                            const float* bias, const float* add1, const float* add2, float* y,
                                            int32_t mfma_shape, int32_t tile_mode, void* stream) {
  return split_forward(d, x, w_packed, bias, add1, add2, y, mfma_shape, tile_mode, (hipStream_t)stream);
}
