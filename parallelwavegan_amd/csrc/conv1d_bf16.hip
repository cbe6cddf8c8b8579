// conv1d_bf16.hip -- opt-in bf16-operand inference convolution (implicit GEMM on the gfx950 bf16 MFMA instructions).
//
// Numerical definition (include/pwg_kernels.h, "bf16-operand inference"): the fused pre-activation is applied to the fp32
// input in fp32, the activated input is rounded to bf16 (round-to-nearest-even, a plain C++ cast) while it is staged, the
// effective fp32 weight is rounded to bf16 once when the weight image is packed, products are accumulated in fp32 by the
// MFMA, and bias / add1 / add2 / out_mul / out_div / post-activation / the stored result are fp32.
//
// Contraction: Y[m][q] = sum_{tap, ci} W[m][tap][ci] * X[ci][q + x_off + tap * dil]
//   Conv1d (stride 1):           m = output channel, q = output column, taps = kernel, x_off = -pad_left
//   ConvTranspose1d with k = 2s: polyphase -- m = co * s + phase, q = (o + padding) / s, two taps (x[q - 1] with
//                                w[.., phase + s], x[q] with w[.., phase]); the epilogue scatters to o = q * s + phase - p
// A operand = weights, read straight from the pre-packed global image [tap][ci / 8][m_pad][8] (one 16-B fragment per lane,
// 512 B contiguous per half wave; the image of a layer is L2-resident).  B operand = x window, staged per 32-channel
// chunk into LDS as bf16 in [column][channel] order so that a lane's 8 consecutive reduction elements are one
// ds_read_b128; rows are 80 B (5 slots of 16 B, odd) so that consecutive columns fall on different bank groups.
// Staging reads fp32 rows (16 B along t per lane where the rows are 16-B aligned, else 4 B), applies the activation,
// converts, and writes 16 B (8 channels of one column) per LDS store.
// Tiles (rows x columns, 4 waves): 128 x 128 above 64 rows, 64 x 128 for 33 .. 64 rows, 32 x 256 up to 32 rows; launches of
// fewer than 256 such workgroups run on 64 x 64 / 32 x 128 tiles.  Rows are zero-padded in the weight image, columns are
// masked.  Both bf16 MFMA shapes are built at the same tiles.
// Deterministic: one workgroup owns an output tile, no split reduction, no atomics.
// What bounds it and what was measured on the way: DESIGN.md s9, profiles/bf16_infer.json, bf16_infer_variants.txt.
#include "common.h"
#include "bf16_mfma.h"

namespace pwg {
namespace {

constexpr int KC = 32;       // input channels per staged chunk
constexpr int ROW = KC + 8;  // bf16 elements per LDS row (80 B)
constexpr size_t kMaxLds = 64 * 1024;
constexpr int kSmallGridWorkgroups = 256;  // one per CU

// LDS rows of a column tile: the window of nt + halo columns, plus up to 3 columns in front when the staging starts at a
// 16-B aligned input column (vector path), rounded up to whole groups of 4 columns
static inline size_t lds_bytes(int nt, int halo) { return (size_t)round_up(nt + halo + 3, 4) * ROW * sizeof(__bf16); }

struct Bf16Geom {
  int taps, dil, x_off;  // reduction taps, their spacing, input column of (q = 0, tap 0)
  int m, m_pad, mt;      // GEMM rows, padded to the row tile mt
  int phases, out_off;   // transposed: stride and padding (o = q * phases + phase - out_off)
  int nq;                // GEMM columns
  int cin_chunks;        // ceil(c_in / KC)
  int nt;                // column tile of the configuration
};

struct Bf16Args {
  const float* x;
  const bf16x8* w;
  const float* bias;
  const float* add1;
  const float* add2;
  float* y;
  int c_in, c_out, t_in, t_out;
  int m, m_pad, cin_chunks, taps, dil, x_off, phases, out_off, nq;
  int pre_act, post_act;
  float pre_slope, post_slope, out_mul, out_div;
};

static int bf16_geometry(const pwg_conv1d_desc* d, Bf16Geom* g) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "conv1d_bf16: NULL descriptor");
  PWG_REQUIRE(d->batch > 0 && d->c_in > 0 && d->c_out > 0 && d->t_in > 0 && d->t_out > 0 && d->kernel > 0 &&
                  d->stride > 0 && d->dilation > 0 && d->groups > 0 && d->width > 0 && d->pad_left >= 0,
              PWG_ERR_BAD_SHAPE, "conv1d_bf16: non-positive size in descriptor");
  PWG_REQUIRE(d->groups == 1, PWG_ERR_UNSUPPORTED, "conv1d_bf16: groups = %d (only groups == 1)", d->groups);
  PWG_REQUIRE(d->width == 1, PWG_ERR_UNSUPPORTED, "conv1d_bf16: width = %d (only width == 1)", d->width);
  PWG_REQUIRE(d->pad_mode == PWG_PAD_ZERO, PWG_ERR_UNSUPPORTED, "conv1d_bf16: only zero padding (pad_mode = %d)",
              d->pad_mode);
  PWG_REQUIRE(d->pre_act == PWG_ACT_NONE || d->pre_act == PWG_ACT_LEAKY_RELU || d->pre_act == PWG_ACT_RELU,
              PWG_ERR_UNSUPPORTED, "conv1d_bf16: pre_act = %d", d->pre_act);
  PWG_REQUIRE(d->batch <= 65535, PWG_ERR_UNSUPPORTED, "conv1d_bf16: batch = %d (> 65535)", d->batch);
  if (d->transposed) {
    PWG_REQUIRE(d->kernel == 2 * d->stride && d->dilation == 1, PWG_ERR_UNSUPPORTED,
                "conv1d_bf16: transposed convolution with kernel = %d, stride = %d (only kernel == 2 * stride)", d->kernel,
                d->stride);
    g->taps = 2;
    g->dil = 1;
    g->x_off = -1;
    g->m = d->c_out * d->stride;
    g->phases = d->stride;
    g->out_off = d->pad_left;
    g->nq = ceil_div(d->t_out + d->pad_left, d->stride);
  } else {
    PWG_REQUIRE(d->stride == 1, PWG_ERR_UNSUPPORTED, "conv1d_bf16: stride = %d (only stride 1)", d->stride);
    g->taps = d->kernel;
    g->dil = d->dilation;
    g->x_off = -d->pad_left;
    g->m = d->c_out;
    g->phases = 1;
    g->out_off = 0;
    g->nq = d->t_out;
  }
  g->mt = g->m <= 32 ? 32 : (g->m <= 64 ? 64 : 128);
  g->nt = g->m <= 32 ? 256 : 128;
  g->m_pad = round_up(g->m, g->mt);
  g->cin_chunks = ceil_div(d->c_in, KC);
  const size_t lds = lds_bytes(g->nt, (g->taps - 1) * g->dil);
  PWG_REQUIRE(lds <= kMaxLds, PWG_ERR_UNSUPPORTED, "conv1d_bf16: receptive field (%d taps, dilation %d) needs %zu B of LDS",
              g->taps, g->dil, lds);
  PWG_REQUIRE(ceil_div(g->m_pad, g->mt) <= 65535, PWG_ERR_UNSUPPORTED, "conv1d_bf16: too many row blocks");
  return PWG_OK;
}

// one thread per bf16 element of the image [tap][ci / 8][m_pad][8]; padding rows / channels are zero
__global__ __launch_bounds__(256) void pack_weight_bf16_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                               __bf16* __restrict__ wp, int c_in, int c_out, int kernel,
                                                               int taps, int cin_pad, int m, int m_pad, int phases,
                                                               int transposed) {
  const long total = (long)taps * cin_pad * m_pad;
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
      if (transposed) {
        const int co = row / phases, ph = row - co * phases;
        const int kk = tap == 0 ? ph + phases : ph;
        v = w[((long)ci * c_out + co) * kernel + kk];
        if (scale) v *= scale[ci];
      } else {
        v = w[((long)row * c_in + ci) * kernel + tap];
        if (scale) v *= scale[row];
      }
    }
    wp[i] = (__bf16)v;
  }
}

// TILE: MFMA shape (32: 32x32x16, 16: 16x16x32).  A wave computes (WM * 32) rows x (WN * 32) columns; the 4 waves of a
// workgroup are arranged WAVES_M x (4 / WAVES_M).  TRANSPOSED: polyphase epilogue scatter.  VEC: the x window is staged
// with 16-B loads along t (rows 16-B aligned, t_in % 4 == 0, window <= 2 * NT columns) and transposed in registers.
template <int TILE, int WM, int WN, int WAVES_M, bool TRANSPOSED, bool VEC>
__global__ __launch_bounds__(256) void conv1d_bf16_mfma_kernel(Bf16Args a) {
  constexpr int HL = 64 / TILE;             // lane groups along the reduction (2 / 4)
  constexpr int KSTEPS = KC / (8 * HL);     // MFMA reduction steps per chunk (2 / 1)
  constexpr int TM = WM * 32 / TILE, TN = WN * 32 / TILE;
  constexpr int NREG = TILE * TILE / 64;
  constexpr int WAVES_N = 4 / WAVES_M;
  constexpr int MT = WAVES_M * WM * 32, NT = WAVES_N * WN * 32;
  typedef typename Mfma<TILE>::acc_t acc_t;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_m = wave % WAVES_M, wave_n = wave / WAVES_M;
  const int r = lane & (TILE - 1), h = lane / TILE;
  const int q0 = blockIdx.x * NT, m0 = blockIdx.y * MT, b = blockIdx.z;
  const int start = q0 + a.x_off;                // input column of (local column 0, tap 0)
  const int base = VEC ? (start & ~3) : start;   // first staged input column (VEC: 16-B aligned, also when negative)
  const int sh = start - base;                   // 0 .. 3
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
      // item = (group of 4 columns, channel octet): 8 loads of 16 B (one per channel, lanes walk t: coalesced), then
      // per column 8 channels are activated, rounded and written as one 16-B LDS store.  All loads of a thread are
      // issued before the first conversion (ITEMS * 8 loads in flight per lane).
      constexpr int ITEMS = NT >= 128 ? NT / 128 : 1;  // ITEMS * 256 columns / 4 per group * 4 octets / 256 threads
      const int ngroups = (wcols + 3) >> 2;
      f32x4 st[ITEMS][8];
#pragma unroll
      for (int it = 0; it < ITEMS; ++it) {
        const int idx = tid + it * 256, oct = idx & 3, grp = idx >> 2;
        const int t = base + grp * 4;
        const bool tin = grp < ngroups && t >= 0 && t < a.t_in;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ci = chunk * KC + oct * 8 + j;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (tin && ci < a.c_in) v = *reinterpret_cast<const f32x4*>(xb + (size_t)ci * a.t_in + t);
          st[it][j] = v;
        }
      }
#pragma unroll
      for (int it = 0; it < ITEMS; ++it) {
        const int idx = tid + it * 256, oct = idx & 3, grp = idx >> 2;
        if (grp < ngroups) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (__bf16)apply_act(st[it][j][e], a.pre_act, a.pre_slope);
            *reinterpret_cast<bf16x8*>(xs + (grp * 4 + e) * ROW + oct * 8) = v;
          }
        }
      }
    } else {
      // wave `wave` stages channel octet `wave` of the chunk: lanes walk the columns (coalesced fp32 rows), 8 channels are
      // activated, rounded and written as one 16-B LDS store
      const int c_base = chunk * KC + wave * 8;
      for (int col = lane; col < wcols; col += 64) {
        const int t = base + col;
        const bool tin = t >= 0 && t < a.t_in;
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ci = c_base + j;
          float f = 0.f;
          if (tin && ci < a.c_in) f = xb[(size_t)ci * a.t_in + t];
          f = apply_act(f, a.pre_act, a.pre_slope);
          v[j] = (__bf16)f;
        }
        *reinterpret_cast<bf16x8*>(xs + col * ROW + wave * 8) = v;
      }
    }
    __syncthreads();
    for (int tap = 0; tap < a.taps; ++tap) {
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const int oct = ks * HL + h;
        const bf16x8* __restrict__ wp =
            a.w + ((size_t)(tap * a.cin_chunks + chunk) * (KC / 8) + oct) * a.m_pad + m0 + wave_m * (WM * 32) + r;
        bf16x8 af[TM], bfr[TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) af[mi] = wp[mi * TILE];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int col = sh + wave_n * (WN * 32) + ni * TILE + r + tap * a.dil;
          bfr[ni] = *reinterpret_cast<const bf16x8*>(xs + col * ROW + oct * 8);
        }
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = Mfma<TILE>::run(af[mi], bfr[ni], acc[mi][ni]);
      }
    }
  }

  // epilogue (fp32): C layout col = lane % TILE, row = mfma_acc_row (bf16_mfma.h)
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
    for (int i = 0; i < NREG; ++i) {
      const int m = mfma_acc_row<TILE>(m0 + wave_m * (WM * 32) + mi * TILE, i, h);
      if (m >= a.m) continue;
      int co = m, ph = 0;
      if (TRANSPOSED) {
        co = m / a.phases;
        ph = m - co * a.phases;
      }
      const float bias = a.bias ? a.bias[co] : 0.f;
      const size_t rowbase = ((size_t)b * a.c_out + co) * a.t_out;
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int q = q0 + wave_n * (WN * 32) + ni * TILE + r;
        if (q >= a.nq) continue;
        const int o = TRANSPOSED ? q * a.phases + ph - a.out_off : q;
        if (o < 0 || o >= a.t_out) continue;
        const size_t idx = rowbase + o;
        float v = acc[mi][ni][i];
        if (a.bias) v += bias;
        if (a.add1) v += a.add1[idx];
        if (a.add2) v += a.add2[idx];
        if (a.out_mul != 1.0f) v *= a.out_mul;
        if (a.out_div != 1.0f) v = v / a.out_div;
        v = apply_act(v, a.post_act, a.post_slope);
        a.y[idx] = v;
      }
    }
  }
}

template <int TILE, bool TRANSPOSED, bool VEC>
static void launch_tile(const Bf16Geom& g, const Bf16Args& a, int batch, bool small, size_t lds, hipStream_t stream) {
  const int mt = small ? (g.mt > 32 ? 64 : 32) : g.mt, nt = small ? g.nt / 2 : g.nt;
  const dim3 grid(ceil_div(g.nq, nt), g.m_pad / mt, batch);
  if (small && mt == 32)  // 32 x 128
    hipLaunchKernelGGL((conv1d_bf16_mfma_kernel<TILE, 1, 1, 1, TRANSPOSED, VEC>), grid, dim3(256), lds, stream, a);
  else if (small)  // 64 x 64
    hipLaunchKernelGGL((conv1d_bf16_mfma_kernel<TILE, 1, 1, 2, TRANSPOSED, VEC>), grid, dim3(256), lds, stream, a);
  else if (g.mt == 32)  // 32 x 256
    hipLaunchKernelGGL((conv1d_bf16_mfma_kernel<TILE, 1, 2, 1, TRANSPOSED, VEC>), grid, dim3(256), lds, stream, a);
  else if (g.mt == 64)  // 64 x 128
    hipLaunchKernelGGL((conv1d_bf16_mfma_kernel<TILE, 1, 2, 2, TRANSPOSED, VEC>), grid, dim3(256), lds, stream, a);
  else  // 128 x 128
    hipLaunchKernelGGL((conv1d_bf16_mfma_kernel<TILE, 2, 2, 2, TRANSPOSED, VEC>), grid, dim3(256), lds, stream, a);
}

template <int TILE>
static void launch_cfg(const Bf16Geom& g, const Bf16Args& a, int batch, bool transposed, bool vec, bool small, size_t lds,
                       hipStream_t stream) {
  if (transposed) {
    if (vec)
      launch_tile<TILE, true, true>(g, a, batch, small, lds, stream);
    else
      launch_tile<TILE, true, false>(g, a, batch, small, lds, stream);
  } else {
    if (vec)
      launch_tile<TILE, false, true>(g, a, batch, small, lds, stream);
    else
      launch_tile<TILE, false, false>(g, a, batch, small, lds, stream);
  }
}

static int bf16_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias, const float* add1,
                        const float* add2, float* y, int mfma_shape, hipStream_t stream) {
  Bf16Geom g;
  int rc = bf16_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(x && w_packed && y, PWG_ERR_NULL, "conv1d_bf16: NULL pointer");
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_bf16: the weight image must be 16-B aligned");
  PWG_REQUIRE(mfma_shape == 16 || mfma_shape == 32, PWG_ERR_BAD_SHAPE, "conv1d_bf16: mfma_shape = %d (16 or 32)", mfma_shape);
  PWG_REQUIRE(d->post_act >= PWG_ACT_NONE && d->post_act <= PWG_ACT_RELU, PWG_ERR_BAD_SHAPE, "conv1d_bf16: post_act = %d",
              d->post_act);
  Bf16Args a;
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
  a.phases = g.phases;
  a.out_off = g.out_off;
  a.nq = g.nq;
  a.pre_act = d->pre_act;
  a.post_act = d->post_act;
  a.pre_slope = d->pre_slope;
  a.post_slope = d->post_slope;
  a.out_mul = d->out_mul;
  a.out_div = d->out_div;
  const int halo = (g.taps - 1) * g.dil;
  // short inputs: a launch that would not give every CU a workgroup runs on half-size tiles (64 x 64 / 32 x 128; the
  // weight image is the same).  The accumulation order of an output element does not depend on the tile.
  const bool small = (long)ceil_div(g.nq, g.nt) * (g.m_pad / g.mt) * d->batch < kSmallGridWorkgroups;
  const int nt = small ? g.nt / 2 : g.nt;
  const size_t lds = lds_bytes(nt, halo);
  // vector staging: 16-B loads along t need aligned rows, and the window must fit the per-thread register items
  const bool vec = d->t_in % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0 &&
                   nt + halo + 3 <= (nt >= 128 ? 2 * nt : 256);
  const double out_elems = (double)d->batch * d->c_out * d->t_out;
  const double in_elems = (double)d->batch * d->c_in * d->t_in;
  const double flops = 2.0 * (double)d->batch * g.m * g.nq * g.taps * d->c_in;
  const double bytes = 4.0 * (in_elems + out_elems * (1 + (add1 ? 1 : 0) + (add2 ? 1 : 0))) +
                       2.0 * (double)g.taps * g.cin_chunks * KC * g.m_pad;
  maybe_poison_lds(stream);
  ProfScope prof(stream, "conv1d_bf16_mfma_kernel", flops, bytes);
  if (mfma_shape == 32)
    launch_cfg<32>(g, a, d->batch, d->transposed != 0, vec, small, lds, stream);
  else
    launch_cfg<16>(g, a, d->batch, d->transposed != 0, vec, small, lds, stream);
  PWG_CHECK_LAUNCH("conv1d_bf16");
  return PWG_OK;
}

// MFMA shape of pwg_conv1d_bf16_forward: both shapes are built at the same output tiles; 16x16x32 is the faster one by
// wall time on random data on every layer class of HiFi-GAN V1 (profiles/bf16_infer.json)
constexpr int kDefaultMfmaShape = 16;

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_conv1d_bf16_supported(const pwg_conv1d_desc* d) {
  Bf16Geom g;
  return bf16_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_conv1d_bf16_packed_weight_bytes(const pwg_conv1d_desc* d) {
  Bf16Geom g;
  if (bf16_geometry(d, &g) != PWG_OK) return 0;
  return (size_t)g.taps * g.cin_chunks * KC * g.m_pad * sizeof(__bf16);
}

extern "C" int pwg_conv1d_bf16_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                           void* stream) {
  Bf16Geom g;
  int rc = bf16_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(w && w_packed, PWG_ERR_NULL, "conv1d_bf16_pack_weight: NULL pointer");
  const long total = (long)g.taps * g.cin_chunks * KC * g.m_pad;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_weight_bf16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, scale,
                     static_cast<__bf16*>(w_packed), d->c_in, d->c_out, d->kernel, g.taps, g.cin_chunks * KC, g.m, g.m_pad,
                     g.phases, d->transposed);
  PWG_CHECK_LAUNCH("conv1d_bf16_pack_weight");
  return PWG_OK;
}

extern "C" int pwg_conv1d_bf16_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                       const float* add1, const float* add2, float* y, float* workspace,
                                       size_t workspace_floats, void* stream) {
  (void)workspace;  // no split reduction: one workgroup owns an output tile
  (void)workspace_floats;
  return bf16_forward(d, x, w_packed, bias, add1, add2, y, kDefaultMfmaShape, (hipStream_t)stream);
}

extern "C" int pwg_conv1d_bf16_forward_cfg(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias,
                                           const float* add1, const float* add2, float* y, int32_t mfma_shape,
                                           void* stream) {
  return bf16_forward(d, x, w_packed, bias, add1, add2, y, mfma_shape, (hipStream_t)stream);
}
