// What the stream kernels share (conv1d_stream.hip, conv1d_stream_bf16.hip and, for the history writer,
// wavenet_stream.hip): every rule of a stream that has to agree bit for bit between the kernels is stated here, once.
//   history rule          stream_write_history   hist_out = the last H RAW columns of concat(hist_in, x)
//   start-of-stream rule  StreamWindow::at       which source window column t comes from (history, chunk, padding)
//   sum order, epilogue   stream_reduce_epilogue ((p0 + p1) + p2) + p3, then the fp32 epilogue
//   delayed form          StreamDelay            addends read through a delay line, zeros stored outside a valid window
//   window rule           stream_slot_window     the valid columns of a launch from a push-relative position
//   slotted form          StreamSlots            the delayed form with one position per item, read from a device table
//                         stream_slot_item       ... the row reader, shared with the slotted kernels that are no convolution
//                         StreamSlots::mirrored_at ... with the input edges of a reflect-padded layer (slotted-mirrored form)
//   mirror rule           StreamMirrorWindow::at the reflect-padded layer of a look-ahead stream: mirror, then resolve
//   tile rule             stream_tile            column tile from n; 32-row blocks only at 2 x 256 or more workgroups
//   coverage              stream_geometry        defined in conv1d_stream.hip; both precisions admit the same layers
//                         delayed_geometry       ... and the same delays (what the delayed form adds; defined there too)
//   host path             stream_run             pointer checks, common arguments, accounting (stream_work), launch
// Internal to csrc/; the staging loops and contractions of the kernels differ on purpose and stay with them.
#pragma once
#include "common.h"

#include "bf16_mfma.h"  // f32x4 (after common.h: it needs the HIP runtime header)

#include <stdint.h>

#include <type_traits>

namespace pwg {

constexpr int kStreamMaxNt = 64;            // widest column tile
constexpr int kStreamMaxHist = 144;         // history columns stream_geometry() admits; each kernel asserts its window fits LDS
constexpr int kStreamLdsBytes = 64 * 1024;  // what a workgroup gets without raising the kernel's limit
constexpr int kStreamFillWorkgroups = 256;  // one per CU

// ---- history rule.  hist_out = last H columns of concat(hist_in, x), raw, also when n < H (part of hist_in carries
// over); hb == NULL is the start of a stream: the replicated first column, or zeros.  xb / hb / ho are one item's
// (c, n) / (c, H) / (c, H); its c * H elements are dealt over the item's nwg workgroups, this one being number wg.
// UNROLL: the wavenet kernel's long copy (64 * 2d elements) is unrolled by 4; the conv kernels pass 1, which compiles
// to the instruction stream of the loop without a pragma.
template <int UNROLL>
__device__ __forceinline__ void stream_write_history(const float* __restrict__ xb, const float* __restrict__ hb,
                                                     float* __restrict__ ho, int c, int n, int H, bool replicate, int wg,
                                                     int nwg) {
  const int total = c * H;
#pragma unroll UNROLL
  for (int i = wg * 256 + (int)threadIdx.x; i < total; i += nwg * 256) {
    const int ci = i / H, h = i - ci * H;
    const int t = n - H + h;
    float v = 0.f;
    if (t >= 0)
      v = xb[(size_t)ci * n + t];
    else if (hb)
      v = hb[(size_t)ci * H + n + h];
    else if (replicate)
      v = xb[(size_t)ci * n];
    ho[i] = v;
  }
}

// ---- start-of-stream rule.  The window of one item: chunk-relative column t >= 0 is x[t]; t < 0 is hist_in[H + t],
// or at the start of a stream (hb == NULL) what pad_mode synthesises: reflect x[-t], replicate x[0], zero nothing.
struct StreamWindow {
  const float* xb;  // (c_in, n)
  const float* hb;  // (c_in, H) or NULL
  int n, H, pad_mode;

  // Column t: `live` if it holds data (else zero: zero padding, a mirror image past the chunk, or past the chunk's
  // end); it is column `col` of the history if `hist`, else of the chunk.  A staging loop forms the address from the
  // buffer that `hist` names (never from a NULL history), selects a safe one where the column is not live, and always
  // loads.
  struct Column {
    bool live, hist;
    int col;
  };
  __device__ __forceinline__ Column at(int t) const {
    const bool replicate = pad_mode == PWG_PAD_REPLICATE, reflect = pad_mode == PWG_PAD_REFLECT;
    const bool has_hist = hb != nullptr;
    const bool in_chunk = t >= 0;
    const int tt = in_chunk ? t : (reflect ? -t : 0);  // column of x: the chunk's own, the mirrored one, or the first
    Column c;
    c.live = in_chunk ? t < n : (has_hist || replicate || (reflect && tt < n));
    c.hist = !in_chunk && has_hist;
    c.col = c.hist ? H + t : tt;
    return c;
  }
};

// ---- mirror rule (the mirrored form: a REFLECT-padded layer of a non-causal network in a look-ahead stream, DESIGN.md
// s11.8).  The layer's input is valid on [in_lo, in_hi) (chunk-relative, in_lo < 0: the left edge lies in the history);
// outside it the raw history and chunk hold stored zeros (or the flush's dummy columns), not mirror images, and keep
// holding them.  So a window column t is first mapped to the column reflection reads -- t < in_lo: 2 * in_lo - t;
// t >= in_hi: 2 * (in_hi - 1) - t; at most one applies to a column a valid output reads (pad < T) -- and the mapped
// column is then resolved by the start-of-stream rule above with zero padding.  A mapped column outside [-H, n) is not
// live (it reads as zero through the staging loop's safe address): only outputs outside the valid window can depend on
// one, and those are stored as zeros.  The host saturates in_lo / in_hi to [-H, n + kStreamMaxNt] (mirror_bound), which
// changes no mapped column inside [-H, n) and keeps the arithmetic far from overflow; the slotted-mirrored form does the
// same per item on the device (StreamSlots::mirrored_at).
struct StreamMirrorWindow {
  StreamWindow raw;  // pad_mode == PWG_PAD_ZERO
  int in_lo, in_hi;

  __device__ __forceinline__ StreamWindow::Column at(int t) const {
    const int m = t < in_lo ? 2 * in_lo - t : (t >= in_hi ? 2 * (in_hi - 1) - t : t);
    StreamWindow::Column c = raw.at(m);
    c.live = c.live && m >= -raw.H;
    c.col = c.live ? c.col : 0;  // (the staging loop selects its safe address anyway; this one stays in range too)
    return c;
  }
};

// An edge of the mirrored form's input window, saturated for the kernel (StreamMirrorWindow): every window column t lies
// in [-H, n + kStreamMaxNt), so an edge at or below -H, or at or above n + kStreamMaxNt, acts as that bound does.  One
// statement for the host (the mirrored entry's scalar edges) and the device (the slotted-mirrored form's per-item ones).
__host__ __device__ static inline int mirror_bound(long edge, int H, int n) {
  const long lo = -(long)H, hi = (long)n + kStreamMaxNt;
  return (int)(edge < lo ? lo : (edge > hi ? hi : edge));
}

// ---- the fp32 epilogue of an output tile; both argument structs embed it
struct StreamEpilogue {
  const float* bias;
  const float* add1;
  const float* add2;
  float* y;
  int c_out, n, t_out, m, phases;
  int post_act;
  float post_slope, out_mul, out_div;
};

// ---- the delayed form of the epilogue (the look-ahead stream of a non-causal network).  Addend i is
// read through a delay line of delay[i] columns: output column j takes concat(hist_in[i], add_i)[j], i.e. hist_in[i][j]
// for j < delay[i] (zero when hist_in[i] is NULL: start of stream) and add_i[j - delay[i]] afterwards; hist_out[i] = the
// last delay[i] columns of that concatenation, written by the history rule above.  Output columns outside
// [valid_lo, valid_hi) are STORED as 0.0f: the next layer then sees the whole-utterance zero padding there.  The value
// of a valid column is formed by the same operations in the same order as without a delay.
struct StreamLines {
  const float* hist_in[2];  // (B, c_out, delay[i]) or NULL
  float* hist_out[2];       // (B, c_out, delay[i]); NULL where delay[i] == 0
  int delay[2];
};
struct StreamDelay : StreamLines {
  int valid_lo, valid_hi;   // output columns (chunk-relative, of t_out)
};
struct StreamNoDelay {};

// ---- window rule (layers.causal_conv.lookahead_window, stated for a position that is relative to the push): a launch
// whose output is `delay` columns late at `rate` columns per frame, on a push of t_out columns that `before` frames
// went before; `left` = frames of the utterance from this push's first frame on (negative once the stream is past its
// end), if `left_known`.  The valid columns are [max(delay - before * rate, 0), delay + left * rate), clamped to
// [0, t_out].  64-bit throughout: no position overflows, however long the stream.
struct StreamValid {
  int lo, hi;
};
__host__ __device__ static inline StreamValid stream_slot_window(int delay, int rate, int t_out, int before, int left,
                                                                 bool left_known) {
  const long long lo = (long long)delay - (long long)before * rate;
  const long long hi = left_known ? (long long)delay + (long long)left * rate : (long long)t_out;
  StreamValid v;
  v.lo = (int)(lo < 0 ? 0 : (lo > t_out ? t_out : lo));
  v.hi = (int)(hi < 0 ? 0 : (hi > t_out ? t_out : hi));
  return v;
}

// ---- the slotted form of the delayed epilogue (utils.StreamPool): every item of the batch sits at
// its own point of its own utterance.  The launch carries the delay lines, its `rate` and output `delay`, and a device
// table with one row of kStreamSlotInts int32 per item b = blockIdx.z:
//   row[0]  frames that went before this push (the host saturates it once it is past every delay of the plan);
//           0: the item is FRESH -- history and both delay lines read as zeros whatever the buffers hold
//   row[1]  frames of the utterance from this push's first frame on, if row[2] says it is known
//   row[2]  kStreamSlotPaused: the item takes no frames in this launch; kStreamSlotLeftKnown: row[1] holds
//   row[3]  not read by the kernel: the host's own (utils.StreamPool keeps the push's count of real frames there)
// at(b) resolves the row, delayed(item) gives the item's StreamDelay: a running item IS a delayed launch with its window.
constexpr int kStreamSlotInts = 4;
constexpr int kStreamSlotPaused = 1, kStreamSlotLeftKnown = 2;

struct StreamSlots : StreamLines {
  const int32_t* slots;  // (B, kStreamSlotInts)
  int rate, out_delay;

  // What a kernel keeps of its item's row across its main loop: four scalars, and the two saturated input edges of a
  // reflect-padded layer (mirrored_at; 0 and never read in every other kernel)
  struct Item {
    int valid_lo, valid_hi;
    bool fresh, paused;
    int in_lo, in_hi;
  };
  // The row reader: workgroup-uniform; a table value reaches addressing only through the clamped window and the flags
  __device__ __forceinline__ Item at(int b, int t_out) const {
    const int32_t* __restrict__ row = slots + (size_t)b * kStreamSlotInts;
    const int before = __builtin_amdgcn_readfirstlane(row[0]), left = __builtin_amdgcn_readfirstlane(row[1]);
    const int flags = __builtin_amdgcn_readfirstlane(row[2]);
    const StreamValid v = stream_slot_window(out_delay, rate, t_out, before, left, (flags & kStreamSlotLeftKnown) != 0);
    return Item{v.lo, v.hi, before == 0, (flags & kStreamSlotPaused) != 0, 0, 0};
  }
  // The row reader of the slotted-mirrored form (a reflect-padded stride-1 layer of history H = 2 * pad on a chunk of n
  // columns).  Its input is out_delay - pad columns late, so the item's input is valid on
  // [in_delay - before * rate, in_delay + left * rate), the right edge unbounded while the length is unknown: formed in
  // 64 bits and saturated by mirror_bound, as the host does for the mirrored entry.  The valid window of the output is
  // the input's shifted by pad and clamped -- the window rule's, since saturation moves an edge only outside [0, n].
  // Workgroup-uniform like at(): a table value reaches addressing only through the saturated edges and the flags.
  __device__ __forceinline__ Item mirrored_at(int b, int H, int n) const {
    const int32_t* __restrict__ row = slots + (size_t)b * kStreamSlotInts;
    const int before = __builtin_amdgcn_readfirstlane(row[0]), left = __builtin_amdgcn_readfirstlane(row[1]);
    const int flags = __builtin_amdgcn_readfirstlane(row[2]);
    const int pad = H / 2;
    const long in_delay = (long)out_delay - pad;
    const int in_lo = mirror_bound(in_delay - (long)before * rate, H, n);
    const int in_hi = (flags & kStreamSlotLeftKnown) != 0 ? mirror_bound(in_delay + (long)left * rate, H, n)
                                                          : n + kStreamMaxNt;
    const int lo = in_lo + pad, hi = in_hi + pad;
    return Item{lo < 0 ? 0 : (lo > n ? n : lo), hi < 0 ? 0 : (hi > n ? n : hi), before == 0,
                (flags & kStreamSlotPaused) != 0, in_lo, in_hi};
  }
  // The item's delayed form, built where it is used (the launch's fields come from the kernel arguments again): the
  // launch's lines -- their inputs NULL for a fresh item -- and the item's window
  __device__ __forceinline__ StreamDelay delayed(const Item& it) const {
    StreamDelay dl;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      dl.hist_in[i] = it.fresh ? nullptr : hist_in[i];
      dl.hist_out[i] = hist_out[i];
      dl.delay[i] = delay[i];
    }
    dl.valid_lo = it.valid_lo;
    dl.valid_hi = it.valid_hi;
    return dl;
  }
};

// The same row reader for the slotted kernels that are no convolution and carry no StreamLines (the gated layer, the
// stretch stage, the delay line and the seeding kernel of a Parallel WaveGAN pool): item b's row for a
// launch `out_delay` columns late at `rate` columns per frame on t_out output columns
typedef StreamSlots::Item StreamSlotItem;
__device__ __forceinline__ StreamSlotItem stream_slot_item(const int32_t* slots, int b, int rate, int out_delay,
                                                           int t_out) {
  StreamSlots sl;
  sl.slots = slots;
  sl.rate = rate;
  sl.out_delay = out_delay;
  return sl.at(b, t_out);
}

__device__ __forceinline__ float stream_delayed_addend(const float* __restrict__ add, const float* __restrict__ hist,
                                                       int delay, size_t row, int t_out, int j) {
  if (j >= delay) return add[row * t_out + (j - delay)];
  return hist ? hist[row * delay + j] : 0.f;
}

// Row order of a transposed layer's image: row m = phase * C_out + co (fp32 image) or co * s + phase (bf16 image)
enum class StreamRows { PhaseMajor, ChannelMajor };

// Sum order and epilogue.  The four waves' partial tiles (D layout of the 16 x 16 MFMA forms: column = lane % 16,
// row = 4 * (lane / 16) + register) go through LDS -- every wave writes its tile, zeros where it contracted nothing --
// and one thread per output element adds them in wave order, ((p0 + p1) + p2) + p3, then bias, add1, add2, out_mul,
// out_div and the post-activation.  `red` is the workgroup's LDS ([4][MT][NT + 1] floats, reusing the window's).
template <int MT, int NT, bool TRANSPOSED, StreamRows ROWS, class DELAY = StreamNoDelay>
__device__ __forceinline__ void stream_reduce_epilogue(float* red, const f32x4 (&acc)[MT / 16][NT / 16],
                                                       const StreamEpilogue& a, int m0, int q0, int b,
                                                       const DELAY& dl = DELAY()) {
  constexpr bool DELAYED = !std::is_same<DELAY, StreamNoDelay>::value;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  constexpr int RS = NT + 1;
  __syncthreads();
#pragma unroll
  for (int mi = 0; mi < MT / 16; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT / 16; ++ni)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[(wave * MT + mi * 16 + 4 * lq + i) * RS + ni * 16 + l15] = acc[mi][ni][i];
  __syncthreads();

  for (int e = tid; e < MT * NT; e += 256) {
    const int row = e / NT, col = e - row * NT;
    const int m = m0 + row, j = q0 + col;
    if (m >= a.m || j >= a.n) continue;
    // (stream_store_zeros below walks the same elements to the same addresses)
    float v = red[row * RS + col];
    v += red[(MT + row) * RS + col];
    v += red[(2 * MT + row) * RS + col];
    v += red[(3 * MT + row) * RS + col];
    int co = m, ph = 0;
    if (TRANSPOSED) {
      if (ROWS == StreamRows::PhaseMajor) {
        ph = m / a.c_out;
        co = m - ph * a.c_out;
      } else {
        co = m / a.phases;
        ph = m - co * a.phases;
      }
    }
    const size_t o = ((size_t)b * a.c_out + co) * a.t_out + (TRANSPOSED ? j * a.phases + ph : j);
    if constexpr (DELAYED) {
      const int jo = TRANSPOSED ? j * a.phases + ph : j;  // output column
      if (jo < dl.valid_lo || jo >= dl.valid_hi) {
        a.y[o] = 0.f;
        continue;
      }
      const size_t orow = (size_t)b * a.c_out + co;
      if (a.bias) v += a.bias[co];
      if (a.add1) v += stream_delayed_addend(a.add1, dl.hist_in[0], dl.delay[0], orow, a.t_out, jo);
      if (a.add2) v += stream_delayed_addend(a.add2, dl.hist_in[1], dl.delay[1], orow, a.t_out, jo);
    } else {
      if (a.bias) v += a.bias[co];
      if (a.add1) v += a.add1[o];
      if (a.add2) v += a.add2[o];
    }
    if (a.out_mul != 1.0f) v *= a.out_mul;
    if (a.out_div != 1.0f) v = v / a.out_div;
    v = apply_act(v, a.post_act, a.post_slope);
    a.y[o] = v;
  }
}

// The addends' delay lines of one item: the history rule on (c_out, t_out) rows, zero start.  `t_out`: the output columns
// this launch gives the item -- 0 for a paused one, whose lines are then copied through (zeros if it is fresh).
__device__ __forceinline__ void stream_write_lines(const StreamLines& dl, const StreamEpilogue& a, int b, int t_out,
                                                   int wg, int nwg) {
  const float* adds[2] = {a.add1, a.add2};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int D = dl.delay[i];
    if (D == 0) continue;
    const size_t rows = (size_t)b * a.c_out;
    stream_write_history<1>(adds[i] + rows * a.t_out, dl.hist_in[i] ? dl.hist_in[i] + rows * D : nullptr,
                            dl.hist_out[i] + rows * D, a.c_out, t_out, D, false, wg, nwg);
  }
}

// What a paused item of a slotted launch stores for its output tile: exact zeros, at the elements and addresses of
// stream_reduce_epilogue.  No LDS, no barrier.
template <int MT, int NT, bool TRANSPOSED, StreamRows ROWS>
__device__ __forceinline__ void stream_store_zeros(const StreamEpilogue& a, int m0, int q0, int b) {
  for (int e = threadIdx.x; e < MT * NT; e += 256) {
    const int row = e / NT, col = e - row * NT;
    const int m = m0 + row, j = q0 + col;
    if (m >= a.m || j >= a.n) continue;
    int co = m, ph = 0;
    if (TRANSPOSED) {
      if (ROWS == StreamRows::PhaseMajor) {
        ph = m / a.c_out;
        co = m - ph * a.c_out;
      } else {
        co = m / a.phases;
        ph = m - co * a.phases;
      }
    }
    a.y[((size_t)b * a.c_out + co) * a.t_out + (TRANSPOSED ? j * a.phases + ph : j)] = 0.f;
  }
}

// ---- host side

struct StreamGeom {
  int taps, dil, hist;  // reduction taps, their spacing, history columns H
  int m, m_pad, cin_pad;  // m_pad, cin_pad: of the fp32 packed image
  int phases;           // transposed: stride (output column j * phases + phase), else 1
};

// What a stream launch covers, in either precision (conv1d_stream.hip); the reason for a refusal is pwg_last_error.
// Shared between two translation units but not exported from the library.
__attribute__((visibility("hidden"))) int stream_geometry(const pwg_conv1d_desc* d, StreamGeom* g);

// What the delayed form adds to it, in either precision (conv1d_stream.hip): zero padding only, delays >= 0 and no
// longer than a history.
__attribute__((visibility("hidden"))) int delayed_geometry(const pwg_conv1d_desc* d, int32_t delay1, int32_t delay2,
                                                           StreamGeom* g);

// What the mirrored form admits (conv1d_stream.hip): a stride-1, non-transposed, ungrouped PWG_PAD_REFLECT layer whose
// history (k - 1) * d is even (symmetric padding) and fits the window.
__attribute__((visibility("hidden"))) int mirrored_geometry(const pwg_conv1d_desc* d, StreamGeom* g);

// The slotted-mirrored launch (conv1d_stream.hip, where the kernel family is), behind the entry point of
// csrc/conv1d_stream_slots_mirrored.hip: the checks, the arguments and the launch of
// pwg_conv1d_stream_slots_mirrored_forward.
__attribute__((visibility("hidden"))) int stream_slots_mirrored_forward(const pwg_conv1d_desc* d, const float* x,
                                                                        const float* hist_in, float* hist_out,
                                                                        const float* w_packed, const float* bias,
                                                                        const int32_t* slots, int32_t rate, int32_t delay,
                                                                        float* y, void* stream);

// The fields both kernels' argument structs share
struct StreamCommonArgs {
  const float* x;
  const float* hist_in;
  float* hist_out;
  int c_in, hist, taps, dil;
  int step_q, step_w;  // 256 / W and 256 % W for the staged window of W = tile columns + hist columns
  int pad_mode, pre_act;
  float pre_slope;
  StreamEpilogue ep;
};

// ---- tile rule: 16 / 32 / 64 columns for chunks of up to 16 / 32 / more; 32-row blocks only when they still give
// every CU two workgroups (the order of an element's sum is the same)
struct StreamTile {
  int tn, tm, col_tiles;
};
static inline StreamTile stream_tile(int n, int m, int batch) {
  StreamTile t;
  t.tn = n <= 16 ? 1 : (n <= 32 ? 2 : 4);
  t.col_tiles = ceil_div(n, 16 * t.tn);
  t.tm = (t.tn == 4 && (long)ceil_div(m, 32) * t.col_tiles * batch >= 2 * kStreamFillWorkgroups) ? 2 : 1;
  return t;
}

// The grid of a launch: column tiles x row blocks x items (what pwg_conv1d_stream_plan reports)
static inline dim3 stream_grid(const StreamTile& t, int m, int batch) {
  return dim3(t.col_tiles, ceil_div(m, 16 * t.tm), batch);
}

// LDS of a launch: the window, or the partial tiles that reuse it
static inline size_t stream_lds_bytes(size_t window_bytes, const StreamTile& t) {
  const size_t red = (size_t)4 * (16 * t.tm) * (16 * t.tn + 1) * sizeof(float);
  return window_bytes > red ? window_bytes : red;
}

static inline int stream_check_pointers(const char* name, const pwg_conv1d_desc* d, const StreamGeom& g, const void* x,
                                        const void* w, const void* y, const float* hist_in, const float* hist_out) {
  PWG_REQUIRE(x && w && y, PWG_ERR_NULL, "%s: NULL pointer", name);
  PWG_REQUIRE(hist_out || g.hist == 0, PWG_ERR_NULL, "%s: hist_out is NULL (the layer keeps %d columns)", name, g.hist);
  PWG_REQUIRE(g.hist == 0 || hist_in != hist_out, PWG_ERR_BAD_SHAPE,
              "%s: hist_in and hist_out must be distinct buffers (other workgroups read the history)", name);
  PWG_REQUIRE(hist_in || d->pad_mode != PWG_PAD_REFLECT || d->t_in > g.hist, PWG_ERR_BAD_SHAPE,
              "%s: a reflect-padded stream starts with at least %d columns (got %d)", name, g.hist + 1, d->t_in);
  return PWG_OK;
}

// The delay lines of a delayed launch: a delayed addend needs its tensor and a hist_out distinct from its hist_in;
// the pointers of an addend that is not delayed are ignored
static inline int stream_lines(const char* name, const float* add1, const float* add1_hist_in, float* add1_hist_out,
                               int delay1, const float* add2, const float* add2_hist_in, float* add2_hist_out,
                               int delay2, StreamLines* dl) {
  const float* adds[2] = {add1, add2};
  const float* hin[2] = {add1_hist_in, add2_hist_in};
  float* hout[2] = {add1_hist_out, add2_hist_out};
  const int delays[2] = {delay1, delay2};
  for (int i = 0; i < 2; ++i) {
    if (delays[i]) {
      PWG_REQUIRE(adds[i] && hout[i], PWG_ERR_NULL, "%s: delay%d = %d needs add%d and add%d_hist_out", name, i + 1,
                  delays[i], i + 1, i + 1);
      PWG_REQUIRE(hin[i] != hout[i], PWG_ERR_BAD_SHAPE, "%s: add%d_hist_in and add%d_hist_out must be distinct buffers",
                  name, i + 1, i + 1);
    }
    dl->hist_in[i] = delays[i] ? hin[i] : nullptr;
    dl->hist_out[i] = delays[i] ? hout[i] : nullptr;
    dl->delay[i] = delays[i];
  }
  return PWG_OK;
}

// ... of a delayed launch, with its valid window
static inline int stream_delay_lines(const char* name, const float* add1, const float* add1_hist_in, float* add1_hist_out,
                                     int delay1, const float* add2, const float* add2_hist_in, float* add2_hist_out,
                                     int delay2, int valid_lo, int valid_hi, StreamDelay* dl) {
  dl->valid_lo = valid_lo;
  dl->valid_hi = valid_hi;
  return stream_lines(name, add1, add1_hist_in, add1_hist_out, delay1, add2, add2_hist_in, add2_hist_out, delay2, dl);
}

// ... of a slotted launch, with its table: every state buffer is there from the first launch on (a fresh item does not
// read its inputs, a launch-wide NULL would), so a delayed addend needs its hist_in too
static inline int stream_slot_lines(const char* name, const float* add1, const float* add1_hist_in, float* add1_hist_out,
                                    int delay1, const float* add2, const float* add2_hist_in, float* add2_hist_out,
                                    int delay2, const int32_t* slots, int rate, int delay, StreamSlots* sl) {
  PWG_REQUIRE(slots != nullptr, PWG_ERR_NULL, "%s: slots is NULL", name);
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(slots) & 3u) == 0, PWG_ERR_BAD_SHAPE, "%s: unaligned slot table", name);
  PWG_REQUIRE(rate >= 1 && delay >= 0, PWG_ERR_BAD_SHAPE, "%s: rate = %d, delay = %d (needs rate >= 1, delay >= 0)", name,
              rate, delay);
  PWG_REQUIRE((!delay1 || add1_hist_in) && (!delay2 || add2_hist_in), PWG_ERR_NULL,
              "%s: a delayed addend needs its add_hist_in (a fresh item does not read it)", name);
  sl->slots = slots;
  sl->rate = rate;
  sl->out_delay = delay;
  return stream_lines(name, add1, add1_hist_in, add1_hist_out, delay1, add2, add2_hist_in, add2_hist_out, delay2, sl);
}

static inline void stream_fill_args(StreamCommonArgs* a, const pwg_conv1d_desc* d, const StreamGeom& g, const StreamTile& t,
                                    const float* x, const float* hist_in, float* hist_out, const float* bias,
                                    const float* add1, const float* add2, float* y) {
  a->x = x;
  a->hist_in = g.hist ? hist_in : nullptr;
  a->hist_out = hist_out;
  a->c_in = d->c_in;
  a->hist = g.hist;
  a->taps = g.taps;
  a->dil = g.dil;
  a->step_q = 256 / (16 * t.tn + g.hist);
  a->step_w = 256 % (16 * t.tn + g.hist);
  a->pad_mode = d->pad_mode;
  a->pre_act = d->pre_act;
  a->pre_slope = d->pre_slope;
  a->ep = StreamEpilogue{bias, add1, add2, y, d->c_out, d->t_in, d->t_out, g.m, g.phases,
                         d->post_act, d->post_slope, d->out_mul, d->out_div};
}

// The four tile configurations of a kernel template, handed over as K<TM, TN, TRANSPOSED>::fn
template <template <int, int, bool> class K, class Args>
static inline void stream_launch(const StreamTile& t, bool transposed, const Args& a, int m, int batch, size_t lds,
                                 hipStream_t stream) {
  void (*kern)(Args);
  if (t.tn == 1)
    kern = transposed ? K<1, 1, true>::fn : K<1, 1, false>::fn;
  else if (t.tn == 2)
    kern = transposed ? K<1, 2, true>::fn : K<1, 2, false>::fn;
  else if (t.tm == 1)
    kern = transposed ? K<1, 4, true>::fn : K<1, 4, false>::fn;
  else
    kern = transposed ? K<2, 4, true>::fn : K<2, 4, false>::fn;
  hipLaunchKernelGGL(kern, stream_grid(t, m, batch), dim3(256), lds, stream, a);
}

// What a launch is accounted with (ProfScope): the contraction, and the bytes of the chunk and both histories, of the
// output and its addends, of `line_floats` delay-line elements read and as many written, and of the weight image
struct StreamWork {
  double flops, bytes;
};
static inline StreamWork stream_work(const pwg_conv1d_desc* d, const StreamGeom& g, int addends, double line_floats,
                                     double image_bytes) {
  const double n = d->t_in, out_elems = (double)d->batch * d->c_out * d->t_out;
  return StreamWork{2.0 * (double)d->batch * g.m * n * g.taps * d->c_in,
                    4.0 * ((double)d->batch * d->c_in * (n + 2.0 * g.hist) + out_elems * (1 + addends) + 2.0 * line_floats) +
                        image_bytes};
}

// The host path the conv stream entry points share, from the pointer checks to the launch.  The entry point has done
// what is its own: the geometry `g` of `d`, the tile, its image and alignment line, the delay lines and every field of
// `a` beyond StreamCommonArgs.  `name` heads an error text, `scope` names the ProfScope, K is the kernel family
// (stream_launch), `window_bytes` the LDS of the staged window under `tile`.
template <template <int, int, bool> class K, class Args>
static inline int stream_run(const char* name, const char* scope, const pwg_conv1d_desc* d, const StreamGeom& g,
                             const StreamTile& tile, Args* a, const float* x, const float* hist_in, float* hist_out,
                             const void* w, const float* bias, const float* add1, const float* add2, float* y,
                             size_t window_bytes, double line_floats, double image_bytes, hipStream_t stream) {
  const int rc = stream_check_pointers(name, d, g, x, w, y, hist_in, hist_out);
  if (rc != PWG_OK) return rc;
  stream_fill_args(a, d, g, tile, x, hist_in, hist_out, bias, add1, add2, y);
  const StreamWork work = stream_work(d, g, (add1 ? 1 : 0) + (add2 ? 1 : 0), line_floats, image_bytes);
  maybe_poison_lds(stream);
  ProfScope prof(stream, scope, work.flops, work.bytes);
  stream_launch<K>(tile, d->transposed != 0, *a, g.m, d->batch, stream_lds_bytes(window_bytes, tile), stream);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

}  // namespace pwg
