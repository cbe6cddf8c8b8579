// conv1d_bf16.hip -- opt-in bf16-operand inference convolution (implicit GEMM on the gfx950 bf16 MFMA instructions).
//
// Numerical definition (include/pwg_kernels.h, "bf16-operand inference"): the fused pre-activation is applied to the fp32
// input in fp32, the activated input is rounded to bf16 (round-to-nearest-even, a plain C++ cast) while it is staged, the
// effective fp32 weight is rounded to bf16 once when the weight image is packed, products are accumulated in fp32 by the
// MFMA, and bias / add1 / add2 / out_mul / out_div / post-activation / the stored result are fp32.
//
// Contraction, coverage, weight image, tiles and launch plan are those of csrc/mfma_conv.h (a transposed layer's rows are
// m = co * s + phase; the epilogue scatters column q to o = q * s + phase - padding).
// A operand = weights, read straight from the pre-packed global image (one 16-B fragment per lane; the image of a layer
// is L2-resident).  B operand = x window, staged per 32-channel chunk into LDS as bf16 in [column][channel] order so that
// a lane's 8 consecutive reduction elements are one ds_read_b128; the odd number of 16-B slots per row puts consecutive
// columns on different bank groups.
// Staging reads fp32 rows (16 B along t per lane where the rows are 16-B aligned, else 4 B), applies the activation,
// converts, and writes 16 B (8 channels of one column) per LDS store.  Both bf16 MFMA shapes are built at the same tiles.
// Deterministic: one workgroup owns an output tile, no split reduction, no atomics.
// What bounds it and what was measured on the way: DESIGN.md s9, profiles/bf16_infer.json, bf16_infer_variants.txt.
#include "mfma_conv.h"

namespace pwg {
namespace {

struct Bf16Args : MfmaConvArgs {
  int phases, out_off, pre_act;
  float pre_slope;
};

static int bf16_geometry(const pwg_conv1d_desc* d, MfmaConvGeom* g) {
  return mfma_conv_geometry("conv1d_bf16", 1, true, d, g);
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

  const MfmaConvTile c = mfma_conv_tile<TILE, MT, NT, WAVES_M, VEC>(a);
  const float* __restrict__ xb = c.xb;

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
      constexpr int ITEMS = window_items(NT);
      const int ngroups = (c.wcols + 3) >> 2;
      f32x4 st[ITEMS][8];
#pragma unroll
      for (int it = 0; it < ITEMS; ++it) {
        const int idx = c.tid + it * 256, oct = idx & 3, grp = idx >> 2;
        const int t = c.base + grp * 4;
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
        const int idx = c.tid + it * 256, oct = idx & 3, grp = idx >> 2;
        if (grp < ngroups) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (__bf16)apply_act(st[it][j][e], a.pre_act, a.pre_slope);
            *reinterpret_cast<bf16x8*>(xs + (grp * 4 + e) * kConvRow + oct * 8) = v;
          }
        }
      }
    } else {
      // wave `wave` stages channel octet `wave` of the chunk: lanes walk the columns (coalesced fp32 rows), 8 channels are
      // activated, rounded and written as one 16-B LDS store
      const int c_base = chunk * KC + c.wave * 8;
      for (int col = c.lane; col < c.wcols; col += 64) {
        const int t = c.base + col;
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
        *reinterpret_cast<bf16x8*>(xs + col * kConvRow + c.wave * 8) = v;
      }
    }
    __syncthreads();
    for (int tap = 0; tap < a.taps; ++tap) {
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const int oct = ks * HL + c.h;
        const bf16x8* __restrict__ wp =
            image_rows(a.w, a.cin_chunks, a.m_pad, tap, chunk, oct) + c.m0 + c.wave_m * (WM * 32) + c.r;
        bf16x8 af[TM], bfr[TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) af[mi] = wp[mi * TILE];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
          const int col = c.sh + c.wave_n * (WN * 32) + ni * TILE + c.r + tap * a.dil;
          bfr[ni] = *reinterpret_cast<const bf16x8*>(xs + col * kConvRow + oct * 8);
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
      const int m = mfma_acc_row<TILE>(c.m0 + c.wave_m * (WM * 32) + mi * TILE, i, c.h);
      if (m >= a.m) continue;
      int co = m, ph = 0;
      if (TRANSPOSED) {
        co = m / a.phases;
        ph = m - co * a.phases;
      }
      const float bias = a.bias ? a.bias[co] : 0.f;
      const size_t rowbase = ((size_t)c.b * a.c_out + co) * a.t_out;
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) {
        const int q = c.q0 + c.wave_n * (WN * 32) + ni * TILE + c.r;
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

template <bool TRANSPOSED, bool VEC>
struct Family {
  template <int TILE, int WM, int WN, int WAVES_M>
  struct K {
    static constexpr auto fn = conv1d_bf16_mfma_kernel<TILE, WM, WN, WAVES_M, TRANSPOSED, VEC>;
  };
};

static int bf16_forward(const pwg_conv1d_desc* d, const float* x, const void* w_packed, const float* bias, const float* add1,
                        const float* add2, float* y, int mfma_shape, hipStream_t stream) {
  MfmaConvGeom g;
  int rc = bf16_geometry(d, &g);
  if (rc == PWG_OK) rc = mfma_conv_check_forward("conv1d_bf16", d, x, w_packed, y, mfma_shape, 0);
  if (rc != PWG_OK) return rc;
  Bf16Args a;
  mfma_conv_fill_args(&a, d, g, x, w_packed, bias, add1, add2, y);
  a.phases = g.phases;
  a.out_off = g.out_off;
  a.pre_act = d->pre_act;
  a.pre_slope = d->pre_slope;
  const MfmaConvPlan p = mfma_conv_plan(d, g, 1, 0, x, add1, add2);
  maybe_poison_lds(stream);
  ProfScope prof(stream, "conv1d_bf16_mfma_kernel", p.flops, p.bytes);
  if (d->transposed) {
    if (p.vec)
      mfma_conv_launch<Family<true, true>::K>(p, mfma_shape, a, stream);
    else
      mfma_conv_launch<Family<true, false>::K>(p, mfma_shape, a, stream);
  } else {
    if (p.vec)
      mfma_conv_launch<Family<false, true>::K>(p, mfma_shape, a, stream);
    else
      mfma_conv_launch<Family<false, false>::K>(p, mfma_shape, a, stream);
  }
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
  MfmaConvGeom g;
  return bf16_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_conv1d_bf16_packed_weight_bytes(const pwg_conv1d_desc* d) {
  MfmaConvGeom g;
  if (bf16_geometry(d, &g) != PWG_OK) return 0;
  return (size_t)image_elems(g) * sizeof(__bf16);
}

extern "C" int pwg_conv1d_bf16_pack_weight(const pwg_conv1d_desc* d, const float* w, const float* scale, void* w_packed,
                                           void* stream) {
  MfmaConvGeom g;
  int rc = bf16_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(w && w_packed, PWG_ERR_NULL, "conv1d_bf16_pack_weight: NULL pointer");
  mfma_conv_pack<1>(d, g, w, scale, w_packed, (hipStream_t)stream);
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
