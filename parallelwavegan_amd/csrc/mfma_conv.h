// What the whole-utterance MFMA convolutions share (conv1d_bf16.hip, conv1d_split.hip; for the weight image also
// conv1d_stream_bf16.hip; for the split image and the split arithmetic also resunit_split.hip): everything that has to
// agree between the kernels is stated here, once.
//   chunk, LDS row        KC, kConvRow, plane_rows   32 channels per staged chunk; rows of 80 B; rows of a column tile
//   coverage, tile rule   mfma_conv_geometry         128 / 64 / 32 rows x 128 / 128 / 256 columns from the GEMM rows
//   weight image          image_chunks, image_m_pad, image_elems, image_decode, image_rows, mfma_conv_pack
//                                                    [tap][ci / 8][m_pad][8] per part
//   split arithmetic      SplitActLeaky, SplitActMasked   the activation of a value in front of its split: max(v, v * slope)
//                                                    for leaky with 0 < slope < 1, (mul, mask) for every other kind
//                         split3, split3_pair, split3_store, split_product   the 3-way split of a value, of two values
//                                                    as packed words; N values split and stored, a
//                                                    vector per plane; one of the six part products of a row tile.
//                                                    split_product OWNS the product order of conv1d_split.hip and
//                                                    resunit_split.hip, which must agree to the bit
//   reduction step        split_step                 resident form (conv1d_split.hip): all fragments of a step loaded,
//                                                    then its MFMAs
//                         split_step_streamed, SplitStepId, split_step_successor, split_step_rows, split_step_request
//                                                    streamed form (resunit_split.hip): the weight fragments a row
//                                                    tile ahead of their MFMAs; the numbering of the steps and the one
//                                                    rule for the step that follows
//   launch plan           mfma_conv_plan             half-size tiles for short inputs, grid, LDS, vector staging
//   tile ladder           mfma_conv_launch           the five tiles x two MFMA shapes of a kernel family
//   arguments             MfmaConvArgs, mfma_conv_fill_args, mfma_conv_check_forward
//   tile coordinates      MfmaConvTile               thread, wave and window coordinates of a workgroup
// Internal to csrc/.  What stays with the kernels, on purpose: the bf16 kernel's contraction (one product, its own
// operand pipeline); every kernel's chunk / tap / k-step loops, barriers and staging loads (shared forms of the loads
// changed the VGPR counts, profiles/refactor_mfma_conv_resources.txt); the epilogues (the unit masks slot < bn_out and
// clamps to t0, the conv clamps to nq - 4 and has a FULL form: different loads).  conv1d_bf16.hip instantiates none of the
// split arithmetic.  The stream kernel reads the bf16 image with its own tiles and LDS row (conv1d_stream_bf16.hip).
#pragma once
#include "common.h"

#include "bf16_mfma.h"  // after common.h: it needs the HIP runtime header

#include <stdint.h>

namespace pwg {

constexpr int KC = 32;                     // input channels per chunk of the image and per staged chunk
constexpr int kConvRow = KC + 8;           // bf16 elements per LDS row: 80 B, 5 slots of 16 B (odd)
constexpr size_t kConvMaxLds = 64 * 1024;  // what a workgroup gets without raising the kernel's limit
constexpr int kConvFillWorkgroups = 256;   // one per CU

// LDS rows of one plane of a column tile: the window of nt + halo columns, plus up to 3 columns in front when the
// staging starts at a 16-B aligned input column (vector path), rounded up to whole groups of 4 columns
static inline int plane_rows(int nt, int halo) { return round_up(nt + halo + 3, 4); }
static inline size_t conv_lds_bytes(int parts, int nt, int halo) {
  return (size_t)parts * plane_rows(nt, halo) * kConvRow * sizeof(__bf16);
}

// The row tile of a configuration and what the weight image pads to: rows to the row tile, channels to whole chunks.
// constexpr: resunit_split.hip reads the image of a C -> C convolution with C a template parameter.
constexpr int conv_row_tile(int m) { return m <= 32 ? 32 : (m <= 64 ? 64 : 128); }
constexpr int image_m_pad(int m) { return (m + conv_row_tile(m) - 1) / conv_row_tile(m) * conv_row_tile(m); }
constexpr int image_chunks(int c_in) { return (c_in + KC - 1) / KC; }

// ---- coverage and tile rule.  Contraction: Y[m][q] = sum_{tap, ci} W[m][tap][ci] * X[ci][q + x_off + tap * dil]
//   Conv1d (stride 1):           m = output channel, q = output column, taps = kernel, x_off = -pad_left
//   ConvTranspose1d with k = 2s: polyphase -- m = co * s + phase, q = (o + padding) / s, two taps (x[q - 1] with
//                                w[.., phase + s], x[q] with w[.., phase]); output column o = q * s + phase - padding
// Tiles (rows x columns, 4 waves): 128 x 128 above 64 rows, 64 x 128 for 33 .. 64 rows, 32 x 256 up to 32 rows.  Rows are
// zero-padded in the weight image, columns are masked.
struct MfmaConvGeom {
  int taps, dil, x_off;  // reduction taps, their spacing, input column of (q = 0, tap 0)
  int m, m_pad, mt;      // GEMM rows, padded to the row tile mt
  int phases, out_off;   // transposed: stride and padding (o = q * phases + phase - out_off), else 1 and 0
  int nq;                // GEMM columns
  int cin_chunks;        // ceil(c_in / KC)
  int nt;                // column tile of the configuration
  bool half_only;        // the planes of the full-size column tile do not fit LDS: half-size tiles whatever the grid
};

// parts: operand parts = LDS planes and weight images (1: bf16 operands, 3: split operands).  The refusals are worded
// and ordered as each kernel has always reported them.
static inline int mfma_conv_geometry(const char* name, int parts, bool allow_transposed, const pwg_conv1d_desc* d,
                                     MfmaConvGeom* g) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "%s: NULL descriptor", name);
  PWG_REQUIRE(d->batch > 0 && d->c_in > 0 && d->c_out > 0 && d->t_in > 0 && d->t_out > 0 && d->kernel > 0 &&
                  d->stride > 0 && d->dilation > 0 && d->groups > 0 && d->width > 0 && d->pad_left >= 0,
              PWG_ERR_BAD_SHAPE, "%s: non-positive size in descriptor", name);
  PWG_REQUIRE(d->groups == 1, PWG_ERR_UNSUPPORTED, "%s: groups = %d (only groups == 1)", name, d->groups);
  PWG_REQUIRE(d->width == 1, PWG_ERR_UNSUPPORTED, "%s: width = %d (only width == 1)", name, d->width);
  PWG_REQUIRE(d->pad_mode == PWG_PAD_ZERO, PWG_ERR_UNSUPPORTED, "%s: only zero padding (pad_mode = %d)", name, d->pad_mode);
  if (!allow_transposed) {
    PWG_REQUIRE(!d->transposed, PWG_ERR_UNSUPPORTED, "%s: transposed convolutions are not covered", name);
    PWG_REQUIRE(d->stride == 1, PWG_ERR_UNSUPPORTED, "%s: stride = %d (only stride 1)", name, d->stride);
  }
  PWG_REQUIRE(d->pre_act == PWG_ACT_NONE || d->pre_act == PWG_ACT_LEAKY_RELU || d->pre_act == PWG_ACT_RELU,
              PWG_ERR_UNSUPPORTED, "%s: pre_act = %d", name, d->pre_act);
  PWG_REQUIRE(d->batch <= 65535, PWG_ERR_UNSUPPORTED, "%s: batch = %d (> 65535)", name, d->batch);
  if (d->transposed) {
    PWG_REQUIRE(d->kernel == 2 * d->stride && d->dilation == 1, PWG_ERR_UNSUPPORTED,
                "%s: transposed convolution with kernel = %d, stride = %d (only kernel == 2 * stride)", name, d->kernel,
                d->stride);
    *g = MfmaConvGeom{2, 1, -1, d->c_out * d->stride, 0, 0, d->stride, d->pad_left,
                      ceil_div(d->t_out + d->pad_left, d->stride)};
  } else {
    PWG_REQUIRE(d->stride == 1, PWG_ERR_UNSUPPORTED, "%s: stride = %d (only stride 1)", name, d->stride);
    *g = MfmaConvGeom{d->kernel, d->dilation, -d->pad_left, d->c_out, 0, 0, 1, 0, d->t_out};
  }
  g->mt = conv_row_tile(g->m);
  g->nt = g->m <= 32 ? 256 : 128;
  g->m_pad = image_m_pad(g->m);
  g->cin_chunks = image_chunks(d->c_in);
  // Only the split kernel bounds the window before it sizes it, and only it falls back to half-size tiles for LDS alone
  // (the bf16 kernel refuses such a window; admitting it there would be a new rule)
  PWG_REQUIRE(parts == 1 || (long)(g->taps - 1) * g->dil < (1 << 20), PWG_ERR_UNSUPPORTED, "%s: receptive field too long",
              name);
  const int halo = (g->taps - 1) * g->dil;
  g->half_only = parts > 1 && conv_lds_bytes(parts, g->nt, halo) > kConvMaxLds;
  const size_t lds = conv_lds_bytes(parts, g->half_only ? g->nt / 2 : g->nt, halo);
  PWG_REQUIRE(lds <= kConvMaxLds, PWG_ERR_UNSUPPORTED, "%s: receptive field (%d taps, dilation %d) needs %zu B of LDS", name,
              g->taps, g->dil, lds);
  PWG_REQUIRE(ceil_div(g->m_pad, g->mt) <= 65535, PWG_ERR_UNSUPPORTED, "%s: too many row blocks", name);
  return PWG_OK;
}

// ---- weight image.  One part is [tap][ci / 8][m_pad][8] bf16: rows padded to the row tile (g.m_pad), channels to whole
// chunks, padding zero; a lane's A fragment is 16 B and a half wave reads 512 B contiguous.  The split kernel's image is
// three parts (hi, mid, lo) of image_elems() each, one after the other.
constexpr long image_elems(int taps, int cin_chunks, int m_pad) { return (long)taps * cin_chunks * KC * m_pad; }
static inline long image_elems(const MfmaConvGeom& g) { return image_elems(g.taps, g.cin_chunks, g.m_pad); }

struct ImageIndex {
  int tap, ci, row;
};
__device__ __forceinline__ ImageIndex image_decode(long i, int cin_pad, int m_pad) {
  const int j = (int)(i & 7);
  long rest = i >> 3;
  const int row = (int)(rest % m_pad);
  rest /= m_pad;
  const int oct = (int)(rest % (cin_pad / 8));
  return ImageIndex{(int)(rest / (cin_pad / 8)), oct * 8 + j, row};
}

// the A fragments (8 channels from channel 8 * oct of chunk `chunk`, one fragment per row) at tap `tap`
__device__ __forceinline__ const bf16x8* image_rows(const bf16x8* w, int cin_chunks, int m_pad, int tap, int chunk, int oct) {
  return w + ((size_t)(tap * cin_chunks + chunk) * (KC / 8) + oct) * m_pad;
}

// ---- split-operand arithmetic (numerical definition: conv1d_split.hip; a translation unit that uses it is built
// without FMA contraction).  The exact 3-way split of an fp32 value:
__device__ __forceinline__ void split3(float v, __bf16& hi, __bf16& mid, __bf16& lo) {
  hi = (__bf16)v;
  const float r = v - (float)hi;
  mid = (__bf16)r;
  lo = (__bf16)(r - (float)mid);
}

// The activation of a value in front of its split ("activate and split" has one owner: every staging and forming site of
// conv1d_split.hip and resunit_split.hip applies one of the two forms below and then split3 / split3_store).  The kind is
// fixed at launch and wave-uniform: a site is instantiated once per form and the launch's form is chosen around it.
//
// SplitActMasked: none / leaky / relu without control flow: v > 0 ? v : bits(v * mul) & mask, with (mul, mask) = (1, ~0)
// for none, (slope, ~0) for leaky and (0, 0) for relu.  For finite v these are the bits of apply_act(): v * 1 is v,
// v * slope is the same rounded product, and the relu's negative side is +0.0 (the mask clears the sign of v * 0).
struct SplitActMasked {
  float mul;
  unsigned mask;
  __device__ __forceinline__ float operator()(float v) const {
    const float n = __uint_as_float(__float_as_uint(v * mul) & mask);
    return v > 0.f ? v : n;
  }
};
// SplitActLeaky: leaky with 0 < slope < 1 (split_act_is_leaky) as max(v, v * slope), two instructions a value.  The same
// bits as the select for every finite v: a positive v is above its product, a negative v below the same rounded product,
// and +-0 * slope = +-0.  The max is v_med3_f32 against FLT_MAX: under IEEE mode fmaxf grows a canonicalising v_max per
// input that was loaded, not computed; the median of three takes the operands as they are.
struct SplitActLeaky {
  float slope;
  __device__ __forceinline__ float operator()(float v) const {
    return __builtin_amdgcn_fmed3f(v, v * slope, 3.40282347e+38f);
  }
};
static inline bool split_act_is_leaky(int act, float slope) {
  return act == PWG_ACT_LEAKY_RELU && slope > 0.f && slope < 1.f;
}

// Split N (8 or 4) fp32 values and write one N-wide vector per plane: hi at dst, mid at dst + plane, lo at
// dst + 2 * plane.  The values are final: the caller has applied its activation.
// The values go two at a time (split3_pair): one packed conversion per part serves both, and the arithmetic between the
// conversions stays scalar.
//
// split3 of a and b, as the words (b's part << 16 | a's part): the bits of split3 -- float(hi) is hi's bits << 16 -- at
// 11 VALU instructions a pair (3 v_cvt_pk_bf16_f32, 2 x (v_perm + v_and), 4 v_sub_f32).  a's part moves up by a byte
// permute, not a shift: a shift is folded through the pack into a second conversion of a alone.  The subtractions stay
// scalar because the translation units that use this are built without the SLP vectoriser (build.py): paired into
// v_pk_add_f32 they cost more beside another workgroup's MFMAs than the two scalar ones (profiles/split_staging.txt).
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned split_pack2(float a, float b) {
  const bf16x2 p = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, p);
}
__device__ __forceinline__ float split_low_part(unsigned w) {  // bytes {w1, w0, 0, 0}
  return __uint_as_float(__builtin_amdgcn_perm(w, w, 0x01000c0cu));
}
__device__ __forceinline__ void split3_pair(float a, float b, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = split_pack2(a, b);
  const float ra = a - split_low_part(hi), rb = b - __uint_as_float(hi & 0xffff0000u);
  mid = split_pack2(ra, rb);
  const float la = ra - split_low_part(mid), lb = rb - __uint_as_float(mid & 0xffff0000u);
  lo = split_pack2(la, lb);
}
template <int N>
__device__ __forceinline__ void split3_store(const float (&v)[N], __bf16* dst, int plane) {
  typedef unsigned vec_t __attribute__((ext_vector_type(N / 2)));
  vec_t vh, vm, vl;
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    unsigned hi, mid, lo;
    split3_pair(v[2 * j], v[2 * j + 1], hi, mid, lo);
    vh[j] = hi;
    vm[j] = mid;
    vl[j] = lo;
  }
  *reinterpret_cast<vec_t*>(dst) = vh;
  *reinterpret_cast<vec_t*>(dst + plane) = vm;
  *reinterpret_cast<vec_t*>(dst + 2 * plane) = vl;
}

// Product p (0 .. 5) of one row tile of a reduction step: the ONE statement of the product order -- (weight part, input
// part) = lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi, small terms first -- that conv1d_split_mfma_kernel and
// resunit_split_kernel share, so that a unit equals two chained convolutions bit for bit by construction.  Per
// accumulator the products arrive in the order (chunk, tap, step, product) in both forms of the step below.
//   wf, bfr   the weight fragments of the row tile and the plane fragments of the step, [0] hi, [1] mid, [2] lo
// XFIRST: the plane fragment is the first MFMA operand: the same products summed in the same order, the tile transposed
// (a lane gets 4 consecutive samples of a row instead of 4 consecutive rows of a column).
constexpr int kSplitWeightPart[6] = {2, 0, 1, 1, 0, 0};
constexpr int kSplitInputPart[6] = {0, 2, 1, 0, 1, 0};
template <int TILE, int TN, bool XFIRST>
__device__ __forceinline__ void split_product(int p, const bf16x8 (&wf)[3], const bf16x8 (&bfr)[3][TN],
                                              typename Mfma<TILE>::acc_t (&acc)[TN]) {
#pragma unroll
  for (int ni = 0; ni < TN; ++ni)
    acc[ni] = XFIRST ? Mfma<TILE>::run(bfr[kSplitInputPart[p]][ni], wf[kSplitWeightPart[p]], acc[ni])
                     : Mfma<TILE>::run(wf[kSplitWeightPart[p]], bfr[kSplitInputPart[p]][ni], acc[ni]);
}

// the 3 x TN plane fragments of a step.  xs, col, off: plane 0 (hi), the lane's column of tile ni = 0 at this tap (a
// caller may have folded part of it into xs), element offset of its 8 channels in an LDS row of ROW elements; plane:
// elements per plane
template <int TILE, int TN, int ROW>
__device__ __forceinline__ void split_plane_fragments(bf16x8 (&bfr)[3][TN], const __bf16* xs, int col, int off, int plane) {
#pragma unroll
  for (int ni = 0; ni < TN; ++ni) {
    const __bf16* src = xs + (col + ni * TILE) * ROW + off;
#pragma unroll
    for (int p = 0; p < 3; ++p) bfr[p][ni] = *reinterpret_cast<const bf16x8*>(src + p * plane);
  }
}

// One reduction step (the lane's 8 channels of one tap), RESIDENT form (conv1d_split_mfma_kernel): loads the 3 x TM
// weight fragments and the 3 x TN plane fragments and issues the 6 x TM x TN MFMAs, product by product.
//   wp, part_stride  the lane's row of tile mi = 0 in the part-0 (hi) image at this tap / chunk / octet (image_rows),
//                    bf16x8 elements per part image
template <int TILE, int TM, int TN, int ROW, bool XFIRST>
__device__ __forceinline__ void split_step(const bf16x8* __restrict__ wp, long part_stride, const __bf16* xs, int col,
                                           int off, int plane, typename Mfma<TILE>::acc_t (&acc)[TM][TN]) {
  bf16x8 af[TM][3], bfr[3][TN];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) af[mi][p] = wp[p * part_stride + mi * TILE];
  split_plane_fragments<TILE, TN, ROW>(bfr, xs, col, off, plane);
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) split_product<TILE, TN, XFIRST>(p, af[mi], bfr, acc[mi]);
}

// ---- STREAMED form of the step (resunit_split_kernel): the plane fragments stay resident for a step and the weight
// fragments run one ROW TILE ahead of their MFMAs, across tap, k-step and chunk boundaries.
// The steps of a contraction are numbered (chunk, tap, k-step), k-step fastest: a step is the lane's 8 channels (octet
// ks * (64 / TILE) + lane group) of one tap of one 32-channel chunk.  split_step_successor is the ONE rule for "which
// step follows this one".  After the last step of the last chunk the successor is that step itself: a valid fragment of
// the same image, so the last request needs no branch and reads no address past the image.
struct SplitStepId {
  int chunk, tap, ks;
};
__host__ __device__ __forceinline__ constexpr SplitStepId split_step_successor(SplitStepId s, int chunks, int taps,
                                                                               int ksteps) {
  if (s.ks + 1 < ksteps) return SplitStepId{s.chunk, s.tap, s.ks + 1};
  if (s.tap + 1 < taps) return SplitStepId{s.chunk, s.tap + 1, 0};
  if (s.chunk + 1 < chunks) return SplitStepId{s.chunk + 1, 0, 0};
  return s;
}
constexpr bool split_step_is(SplitStepId s, int chunk, int tap, int ks) {
  return s.chunk == chunk && s.tap == tap && s.ks == ks;
}
// k-step, then tap; the last step of an inner chunk -> step 0 of the next chunk; the last of the last -> clamped
static_assert(split_step_is(split_step_successor({0, 0, 0}, 2, 3, 2), 0, 0, 1), "k-step advances first");
static_assert(split_step_is(split_step_successor({0, 0, 1}, 2, 3, 2), 0, 1, 0), "then the tap");
static_assert(split_step_is(split_step_successor({0, 2, 1}, 2, 3, 2), 1, 0, 0), "last step of an inner chunk");
static_assert(split_step_is(split_step_successor({1, 2, 1}, 2, 3, 2), 1, 2, 1), "last step of the last chunk: clamped");
static_assert(split_step_is(split_step_successor({0, 0, 0}, 2, 3, 1), 0, 1, 0), "KSTEPS = 1: every step is a tap");
static_assert(split_step_is(split_step_successor({0, 2, 0}, 2, 3, 1), 1, 0, 0), "KSTEPS = 1: chunk crossing");
static_assert(split_step_is(split_step_successor({1, 2, 0}, 2, 3, 1), 1, 2, 0), "KSTEPS = 1: clamped");
static_assert(split_step_is(split_step_successor({0, 0, 0}, 1, 1, 1), 0, 0, 0), "one step in total: clamped at once");
static_assert(split_step_is(split_step_successor({0, 0, 0}, 3, 1, 1), 1, 0, 0), "k = 1: a chunk crossing every step");

// Where the weight fragments of step s start, for a lane of group h: the bf16x8 index of row 0 in a part image (the lane
// adds its row), and the element offset of the step's 8 channels inside a staged chunk.  A fragment is addressed as
// (part image, 32-bit index): a part image is below 4 GiB (split_image_addressable, checked by the host), and one index
// register serves all three parts.
constexpr bool split_image_addressable(long elems_per_part) { return elems_per_part * (long)sizeof(__bf16) < (1L << 32); }
template <int TILE>
__device__ __forceinline__ unsigned split_step_rows(int cin_chunks, int m_pad, SplitStepId s, int h) {
  return (unsigned)(((s.tap * cin_chunks + s.chunk) * (KC / 8) + s.ks * (64 / TILE) + h) * m_pad);
}
template <int TILE>
__device__ __forceinline__ int split_step_off(SplitStepId s, int h) {
  return (s.ks * (64 / TILE) + h) * 8;
}

// Request weight fragment `part` (0 hi, 1 mid, 2 lo) at index `row` of its part image (w: part 0), or all three.  A
// contraction calls split_step_request once, for row tile 0 of its first step, as early as it can (before the window is
// staged); split_step_streamed requests every later fragment.
__device__ __forceinline__ bf16x8 split_part_request(const bf16x8* __restrict__ w, long part_stride, unsigned row, int part) {
  return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(w + part * part_stride) +
                                          (size_t)(row * (unsigned)sizeof(bf16x8)));
}
__device__ __forceinline__ void split_step_request(bf16x8 (&wf)[3], const bf16x8* __restrict__ w, long part_stride,
                                                   unsigned row) {
#pragma unroll
  for (int p = 0; p < 3; ++p) wf[p] = split_part_request(w, part_stride, row, p);
}

// One reduction step, streamed: loads the 3 x TN plane fragments; before the 6 x TN MFMAs of row tile mi are issued, row
// tile mi + 1 is requested, and after the last row tile, row tile 0 of the NEXT step.  So a weight fragment is requested
// 5 x TN (lo) or 6 x TN MFMAs ahead of its first use, and the step holds 3 x TN + 5 fragments.
//   wf               in: the fragments of row tile 0 of this step (split_step_request, or the step before);
//                    out: those of row tile 0 of the next step
//   w, part_stride   the part-0 (hi) image; bf16x8 elements per part image
//   row, row_next    the lane's row of tile mi = 0 at this step and at its successor (its row in the image +
//                    split_step_rows of the step / of split_step_successor)
//   xs, col, off, plane   as split_plane_fragments
template <int TILE, int TM, int TN, int ROW, bool XFIRST>
__device__ __forceinline__ void split_step_streamed(bf16x8 (&wf)[3], const bf16x8* __restrict__ w, long part_stride,
                                                    unsigned row, unsigned row_next, const __bf16* xs, int col, int off,
                                                    int plane, typename Mfma<TILE>::acc_t (&acc)[TM][TN]) {
  bf16x8 bfr[3][TN];
  split_plane_fragments<TILE, TN, ROW>(bfr, xs, col, off, plane);
  // only the first product reads the weight's lo part: its successor is requested behind that product, into the
  // registers it frees (20 instead of 24 fragment registers for the two row tiles in flight)
  static_assert(kSplitWeightPart[0] == 2 && kSplitWeightPart[1] != 2 && kSplitWeightPart[2] != 2 &&
                    kSplitWeightPart[3] != 2 && kSplitWeightPart[4] != 2 && kSplitWeightPart[5] != 2,
                "lo is read by the first product only");
#pragma unroll
  for (int mi = 0; mi < TM; ++mi) {
    const unsigned rn = mi + 1 < TM ? row + (mi + 1) * TILE : row_next;
    bf16x8 nx[3];
    nx[0] = split_part_request(w, part_stride, rn, 0);
    nx[1] = split_part_request(w, part_stride, rn, 1);
    // the requests go out in front of this row tile's MFMAs: the scheduler otherwise sinks them to their first use
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      split_product<TILE, TN, XFIRST>(p, wf, bfr, acc[mi]);
      if (p == 0) {
        __builtin_amdgcn_sched_barrier(0);
        nx[2] = split_part_request(w, part_stride, rn, 2);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) wf[p] = nx[p];
    // a row tile at a time: the scheduler otherwise gathers the requests of all row tiles in front of the first MFMA
    __builtin_amdgcn_sched_barrier(0);
  }
}

// One thread per element of ONE part image.  PARTS == 1 stores the rounded effective weight w * scale, PARTS == 3 its
// split3 parts at i, total + i and 2 * total + i.  Instantiated in each translation unit, under that unit's flags.
template <int PARTS>
static __global__ __launch_bounds__(256) void mfma_conv_pack_kernel(const float* __restrict__ w,
                                                                    const float* __restrict__ scale,
                                                                    __bf16* __restrict__ wp, int c_in, int c_out, int kernel,
                                                                    int taps, int cin_pad, int m, int m_pad, int phases,
                                                                    int transposed) {
  const long total = (long)taps * cin_pad * m_pad;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const ImageIndex e = image_decode(i, cin_pad, m_pad);
    float v = 0.f;
    if (e.ci < c_in && e.row < m) {
      if (transposed) {
        const int co = e.row / phases, ph = e.row - co * phases;
        const int kk = e.tap == 0 ? ph + phases : ph;
        v = w[((long)e.ci * c_out + co) * kernel + kk];
        if (scale) v *= scale[e.ci];
      } else {
        v = w[((long)e.row * c_in + e.ci) * kernel + e.tap];
        if (scale) v *= scale[e.row];
      }
    }
    if (PARTS == 1) {
      wp[i] = (__bf16)v;
    } else {
      __bf16 hi, mid, lo;
      split3(v, hi, mid, lo);
      wp[i] = hi;
      wp[total + i] = mid;
      wp[2 * total + i] = lo;
    }
  }
}

template <int PARTS>
static inline void mfma_conv_pack(const pwg_conv1d_desc* d, const MfmaConvGeom& g, const float* w, const float* scale,
                                  void* w_packed, hipStream_t stream) {
  int blocks = (int)((image_elems(g) + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mfma_conv_pack_kernel<PARTS>, dim3(blocks), dim3(256), 0, stream, w, scale,
                     static_cast<__bf16*>(w_packed), d->c_in, d->c_out, d->kernel, g.taps, g.cin_chunks * KC, g.m, g.m_pad,
                     g.phases, d->transposed);
}

// ---- launch plan.  The vector staging deals its items = (group of 4 columns, channel octet) of a chunk over the 256
// threads: window_items(nt) per thread, nt / 4 groups * 4 octets / 256, so a window of up to that many * 256 columns
constexpr int window_items(int nt) { return nt >= 128 ? nt / 128 : 1; }

struct MfmaConvPlan {
  bool small, vec;  // half-size tiles; 16-B staging loads
  int mt, nt;       // the launch's tile
  int plane;        // bf16 elements of one LDS plane
  dim3 grid;
  size_t lds;
  double flops, bytes;  // the ALGORITHMIC flops of the convolution, whatever the number of part products
};

// tile_mode: 0 = the small-grid rule decides, 1 = full-size tiles (where their planes fit LDS), 2 = half-size tiles
static inline MfmaConvPlan mfma_conv_plan(const pwg_conv1d_desc* d, const MfmaConvGeom& g, int parts, int tile_mode,
                                          const float* x, const float* add1, const float* add2) {
  MfmaConvPlan p;
  const int halo = (g.taps - 1) * g.dil;
  // short inputs: a launch that would not give every CU a workgroup runs on half-size tiles (64 x 64 / 32 x 128; the
  // weight image is the same).  The accumulation order of an output element does not depend on the tile.
  const bool few = (long)ceil_div(g.nq, g.nt) * (g.m_pad / g.mt) * d->batch < kConvFillWorkgroups;
  p.small = g.half_only || (tile_mode == 0 ? few : tile_mode == 2);
  p.mt = p.small ? (g.mt > 32 ? 64 : 32) : g.mt;
  p.nt = p.small ? g.nt / 2 : g.nt;
  p.plane = plane_rows(p.nt, halo) * kConvRow;
  p.grid = dim3(ceil_div(g.nq, p.nt), g.m_pad / p.mt, d->batch);
  p.lds = conv_lds_bytes(parts, p.nt, halo);
  // vector staging: 16-B loads along t need aligned rows, and the window must fit the per-thread register items
  p.vec = d->t_in % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0 &&
          p.nt + halo + 3 <= window_items(p.nt) * 256;
  const double out_elems = (double)d->batch * d->c_out * d->t_out;
  const double in_elems = (double)d->batch * d->c_in * d->t_in;
  p.flops = 2.0 * (double)d->batch * g.m * g.nq * g.taps * d->c_in;
  p.bytes = 4.0 * (in_elems + out_elems * (1 + (add1 ? 1 : 0) + (add2 ? 1 : 0))) + 2.0 * parts * (double)image_elems(g);
  return p;
}

// The tile ladder of a kernel family, handed over as K<TILE, WM, WN, WAVES_M>::fn.  TILE: MFMA shape (32: 32x32x16,
// 16: 16x16x32; both are built at the same tiles).  A wave computes (WM * 32) rows x (WN * 32) columns; the 4 waves of a
// workgroup are arranged WAVES_M x (4 / WAVES_M).
template <template <int, int, int, int> class K, int TILE, class Args>
static inline auto mfma_conv_tile_kernel(const MfmaConvPlan& p) -> void (*)(Args) {
  if (p.small && p.mt == 32) return K<TILE, 1, 1, 1>::fn;  // 32 x 128
  if (p.small) return K<TILE, 1, 1, 2>::fn;                // 64 x 64
  if (p.mt == 32) return K<TILE, 1, 2, 1>::fn;             // 32 x 256
  if (p.mt == 64) return K<TILE, 1, 2, 2>::fn;             // 64 x 128
  return K<TILE, 2, 2, 2>::fn;                             // 128 x 128
}
template <template <int, int, int, int> class K, class Args>
static inline void mfma_conv_launch(const MfmaConvPlan& p, int mfma_shape, const Args& a, hipStream_t stream) {
  void (*kern)(Args) = mfma_shape == 32 ? mfma_conv_tile_kernel<K, 32, Args>(p) : mfma_conv_tile_kernel<K, 16, Args>(p);
  hipLaunchKernelGGL(kern, p.grid, dim3(256), p.lds, stream, a);
}

// ---- the arguments both kernels' structs share
struct MfmaConvArgs {
  const float* x;
  const bf16x8* w;
  const float* bias;
  const float* add1;
  const float* add2;
  float* y;
  int c_in, c_out, t_in, t_out;
  int m, m_pad, cin_chunks, taps, dil, x_off, nq;
  int post_act;
  float post_slope, out_mul, out_div;
};

static inline void mfma_conv_fill_args(MfmaConvArgs* a, const pwg_conv1d_desc* d, const MfmaConvGeom& g, const float* x,
                                       const void* w_packed, const float* bias, const float* add1, const float* add2,
                                       float* y) {
  *a = MfmaConvArgs{x, static_cast<const bf16x8*>(w_packed), bias, add1, add2, y, d->c_in, d->c_out, d->t_in, d->t_out,
                    g.m, g.m_pad, g.cin_chunks, g.taps, g.dil, g.x_off, g.nq, d->post_act, d->post_slope, d->out_mul,
                    d->out_div};
}

// what a forward call checks after the geometry (the bf16 kernel has no tile_mode and passes 0)
static inline int mfma_conv_check_forward(const char* name, const pwg_conv1d_desc* d, const void* x, const void* w_packed,
                                          const void* y, int mfma_shape, int tile_mode) {
  PWG_REQUIRE(x && w_packed && y, PWG_ERR_NULL, "%s: NULL pointer", name);
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "%s: the weight image must be 16-B aligned", name);
  PWG_REQUIRE(mfma_shape == 16 || mfma_shape == 32, PWG_ERR_BAD_SHAPE, "%s: mfma_shape = %d (16 or 32)", name, mfma_shape);
  PWG_REQUIRE(tile_mode >= 0 && tile_mode <= 2, PWG_ERR_BAD_SHAPE, "%s: tile_mode = %d (0, 1 or 2)", name, tile_mode);
  PWG_REQUIRE(d->post_act >= PWG_ACT_NONE && d->post_act <= PWG_ACT_RELU, PWG_ERR_BAD_SHAPE, "%s: post_act = %d", name,
              d->post_act);
  return PWG_OK;
}

// ---- device side.  Coordinates of a thread in its workgroup's MT x NT tile, and of the tile's x window
struct MfmaConvTile {
  int tid, lane, wave, wave_m, wave_n;
  int r, h;         // lane % TILE, lane / TILE: row / column inside an MFMA tile, lane group along the reduction
  int q0, m0, b;    // first column, first row, batch item
  int base;         // first staged input column (VEC: 16-B aligned, also when negative)
  int sh;           // local column 0 at tap 0 is staged column sh (0 .. 3)
  int wcols;        // staged columns
  const float* xb;  // the item's input
};
template <int TILE, int MT, int NT, int WAVES_M, bool VEC>
__device__ __forceinline__ MfmaConvTile mfma_conv_tile(const MfmaConvArgs& a) {
  MfmaConvTile c;
  c.tid = threadIdx.x, c.lane = c.tid & 63, c.wave = c.tid >> 6;
  c.wave_m = c.wave % WAVES_M, c.wave_n = c.wave / WAVES_M;
  c.r = c.lane & (TILE - 1), c.h = c.lane / TILE;
  c.q0 = blockIdx.x * NT, c.m0 = blockIdx.y * MT, c.b = blockIdx.z;
  const int start = c.q0 + a.x_off;  // input column of (local column 0, tap 0)
  c.base = VEC ? (start & ~3) : start;
  c.sh = start - c.base;
  c.wcols = NT + (a.taps - 1) * a.dil + c.sh;
  c.xb = a.x + (size_t)c.b * a.c_in * a.t_in;
  return c;
}

}  // namespace pwg
