// conv1d_stream.hip -- stateful (streaming) form of the causal convolutions, fp32 on the exact-fp32 MFMA.
//
// A causal stride-1 convolution (left-only padding (k-1)*d, t_out = t_in) needs only its last H = (k-1)*d input columns
// from the past; the causal k = 2s transposed convolution (polyphase, two taps) needs one.  One launch takes the new chunk
// x (B, C_in, n) and the history hist_in (B, C_in, H), writes y (B, C_out, n) -- n*s for the transposed form -- and
// hist_out = the last H columns of concat(hist_in, x), also when n < H (part of hist_in carries over).  hist_in and
// hist_out are distinct buffers: other workgroups of the launch read hist_in while this one writes hist_out.
//
// Numerical definition.  History holds the RAW input; the fused pre-activation is applied while the window is staged,
// to both sources alike (pad and an element-wise activation commute).  hist_in == NULL is the start of a stream: the
// left context is synthesised from pad_mode exactly as the whole-utterance kernels pad implicitly (zero; reflect:
// column -j is x[j]; replicate: x[0]; the transposed form replicates the first column or pads zero).
//   Y[m][j] = sum_{group, tap, ci in group} W[tap][ci][m] * act(X[ci][j - H + tap * dil])       X[t < 0] = history
//   Conv1d:          m = output channel, taps = k, dil = dilation
//   ConvTranspose1d: m = phase * C_out + co, taps = 2 (x[j - 1] with w[phase + s], x[j] with w[phase]), output column
//                    j * s + phase -- the row order and tap order of the fp32 packed image (csrc/conv1d.hip)
// The A operand is read straight from that image ([tap][ci pad 16][m pad 128], no second image); the B operand is the
// window of NT + H columns, staged per 64 input channels into LDS.  A kernel-1 convolution is the case H = 0 (no history
// buffers): the 1 x 1 layers of a streamed network run here too, because the bit-for-bit rule below holds for a network
// only if it holds for every one of its convolutions.
//
// Contraction: v_mfma_f32_16x16x4_f32 only, whatever the tile.  An output element is the sum of four partial sums,
// ((p0 + p1) + p2) + p3, where p_w runs over the 16-channel groups g with g % 4 == w in the order (group ascending, tap
// ascending, 4 channels per MFMA step; an fmaf chain).  That order depends neither on n, nor on the batch, nor on where
// the chunk sits in the stream, nor on the tile a launch picks: two partitions of the same frames give bit-identical results.  One
// workgroup owns an output tile over the whole reduction: no split across workgroups, no workspace, no atomics.
//
// Tiles: 16 rows x 16 / 32 / 64 columns for chunks of up to 16 / 32 / more columns, 32 x 64 when that still gives every
// CU two workgroups.  Chunks are short and the layers wide (8 columns x 512 rows at the top of HiFi-GAN V1): a launch is a
// pass over the layer's weights for a handful of columns, so what counts is how many waves pull weights at once.  The
// 16-column MFMA wastes half a tile at 8 columns where the 32-column shape would waste three quarters; 16-row blocks
// give 32 workgroups for 512 rows; and inside a workgroup the four waves split the REDUCTION (each takes every fourth
// 16-channel group) instead of the rows, with the next four taps' weights in flight while the current ones are contracted.
// DESIGN.md s11.
//
// Delayed form (pwg_conv1d_stream_delayed_forward): the same launch for a layer of a NON-causal
// network streamed with a fixed look-ahead.  The layer runs in its causal form on a shifted time axis, so its addends
// (the residual input, the MRF running sum) arrive earlier than its output and are read through delay lines kept like
// the history, and output columns outside the utterance's valid window are stored as zeros (StreamDelay,
// stream_common.h).  Operand pipeline, contraction and sum order are those of the plain form: only the history writer
// and the epilogue differ, and the plain instantiations are the code they were.
//
// Slotted form (pwg_conv1d_stream_slots_forward): the delayed form with one position per item.  Item
// b reads its row of a device table (StreamSlots, stream_common.h): how many frames went before and how many remain give
// its valid window by the window rule; a fresh item (nothing went before) reads history and delay lines as zeros whatever
// the buffers hold; a paused item copies its state through, stores zeros for y and returns in front of every barrier.
// A running item's columns are the delayed form's with the same window, bit for bit: one launch serves items at
// different points of different utterances, and one captured graph covers start, steady state and tail.
//
// Slotted-mirrored form (pwg_conv1d_stream_slots_mirrored_forward): the mirrored form with one
// position per item, for a pool of reflect-padded (MelGAN) streams.  The item's row gives the two edges of its INPUT
// window (StreamSlots::mirrored_at: formed in 64 bits, saturated by mirror_bound as the host does for the mirrored
// entry); a running item then builds the StreamMirrorWindow and StreamDelay a batch-1 mirrored launch gets, and from
// there on the code is shared; fresh and paused items are the slotted form's.  The right-hand mirror is never needed
// before the table knows the length: while it is unknown a chunk's columns stop pad short of the utterance's end.
#include "stream_common.h"

namespace pwg {

int stream_geometry(const pwg_conv1d_desc* d, StreamGeom* g) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "conv1d_stream: NULL descriptor");
  PWG_REQUIRE(d->batch > 0 && d->c_in > 0 && d->c_out > 0 && d->t_in > 0 && d->t_out > 0 && d->kernel > 0 &&
                  d->stride > 0 && d->dilation > 0 && d->groups > 0 && d->width > 0 && d->pad_left >= 0,
              PWG_ERR_BAD_SHAPE, "conv1d_stream: non-positive size in descriptor");
  PWG_REQUIRE(d->groups == 1, PWG_ERR_UNSUPPORTED, "conv1d_stream: groups = %d (only groups == 1)", d->groups);
  PWG_REQUIRE(d->width == 1, PWG_ERR_UNSUPPORTED, "conv1d_stream: width = %d (only width == 1)", d->width);
  PWG_REQUIRE(d->pad_mode == PWG_PAD_ZERO || d->pad_mode == PWG_PAD_REFLECT || d->pad_mode == PWG_PAD_REPLICATE,
              PWG_ERR_UNSUPPORTED, "conv1d_stream: pad_mode = %d", d->pad_mode);
  PWG_REQUIRE(d->pre_act == PWG_ACT_NONE || d->pre_act == PWG_ACT_LEAKY_RELU || d->pre_act == PWG_ACT_RELU,
              PWG_ERR_UNSUPPORTED, "conv1d_stream: pre_act = %d", d->pre_act);
  PWG_REQUIRE(d->post_act >= PWG_ACT_NONE && d->post_act <= PWG_ACT_RELU, PWG_ERR_UNSUPPORTED,
              "conv1d_stream: post_act = %d", d->post_act);
  PWG_REQUIRE(d->batch <= 65535, PWG_ERR_UNSUPPORTED, "conv1d_stream: batch = %d (> 65535)", d->batch);
  if (d->transposed) {
    PWG_REQUIRE(d->kernel == 2 * d->stride && d->dilation == 1, PWG_ERR_UNSUPPORTED,
                "conv1d_stream: transposed convolution with kernel = %d, stride = %d, dilation = %d (only kernel == 2 * "
                "stride, dilation 1)", d->kernel, d->stride, d->dilation);
    PWG_REQUIRE(d->pad_left == d->stride, PWG_ERR_UNSUPPORTED,
                "conv1d_stream: transposed convolution with padding = %d (the causal form has padding == stride = %d)",
                d->pad_left, d->stride);
    PWG_REQUIRE((long)d->t_out == (long)d->t_in * d->stride, PWG_ERR_BAD_SHAPE,
                "conv1d_stream: transposed t_out = %d must be t_in * stride = %d * %d", d->t_out, d->t_in, d->stride);
    PWG_REQUIRE(d->pad_mode != PWG_PAD_REFLECT, PWG_ERR_UNSUPPORTED,
                "conv1d_stream: the transposed form starts a stream from a replicated or zero column, not a reflected one");
    g->taps = 2;
    g->dil = 1;
    g->hist = 1;
    g->m = d->c_out * d->stride;
    g->phases = d->stride;
  } else {
    PWG_REQUIRE(d->stride == 1, PWG_ERR_UNSUPPORTED, "conv1d_stream: stride = %d (only stride 1)", d->stride);
    PWG_REQUIRE((long)d->pad_left == (long)(d->kernel - 1) * d->dilation && d->t_out == d->t_in, PWG_ERR_UNSUPPORTED,
                "conv1d_stream: not a causal convolution (pad_left = %d, t_in = %d, t_out = %d; needs left-only padding "
                "(k - 1) * d = %ld and t_out == t_in)", d->pad_left, d->t_in, d->t_out, (long)(d->kernel - 1) * d->dilation);
    g->taps = d->kernel;
    g->dil = d->dilation;
    g->hist = d->pad_left;
    g->m = d->c_out;
    g->phases = 1;
  }
  PWG_REQUIRE(g->hist <= kStreamMaxHist, PWG_ERR_UNSUPPORTED,
              "conv1d_stream: history of %d columns (%d taps, dilation %d) does not fit the LDS window", g->hist, g->taps,
              g->dil);
  PWG_REQUIRE(ceil_div(g->m, 16) <= 65535, PWG_ERR_UNSUPPORTED, "conv1d_stream: too many row blocks");
  g->m_pad = round_up(g->m, 128);   // the fp32 packed image's row extent (csrc/conv1d.hip make_geometry)
  g->cin_pad = round_up(d->c_in, 16);
  return PWG_OK;
}

// What the delayed form adds to stream_geometry(): zero padding only (the shifted time axis starts from the
// whole-utterance zero padding) and delay lines no longer than a history
int delayed_geometry(const pwg_conv1d_desc* d, int32_t delay1, int32_t delay2, StreamGeom* g) {
  const int rc = stream_geometry(d, g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(d->pad_mode == PWG_PAD_ZERO, PWG_ERR_UNSUPPORTED,
              "conv1d_stream_delayed: pad_mode = %d (the delayed form starts a stream from zeros only)", d->pad_mode);
  PWG_REQUIRE(delay1 >= 0 && delay2 >= 0, PWG_ERR_BAD_SHAPE, "conv1d_stream_delayed: negative delay (%d, %d)", delay1,
              delay2);
  PWG_REQUIRE(delay1 <= kStreamMaxHist && delay2 <= kStreamMaxHist, PWG_ERR_UNSUPPORTED,
              "conv1d_stream_delayed: addend delay of %d columns (at most %d)", delay1 > delay2 ? delay1 : delay2,
              kStreamMaxHist);
  return PWG_OK;
}

// What the mirrored form admits: the reflect-padded stride-1 layer of stream_geometry() with a symmetric reach.  The
// refusals that name the form come first, so that a transposed or zero-padded layer is told why THIS entry turns it down
int mirrored_geometry(const pwg_conv1d_desc* d, StreamGeom* g) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "conv1d_stream_mirrored: NULL descriptor");
  PWG_REQUIRE(!d->transposed, PWG_ERR_UNSUPPORTED,
              "conv1d_stream_mirrored: a transposed convolution is not reflect-padded (it streams through the delayed form)");
  PWG_REQUIRE(d->pad_mode == PWG_PAD_REFLECT, PWG_ERR_UNSUPPORTED,
              "conv1d_stream_mirrored: pad_mode = %d (the mirrored form is the reflect-padded layer's; a zero-padded one "
              "streams through the delayed form)", d->pad_mode);
  const int rc = stream_geometry(d, g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(g->hist % 2 == 0, PWG_ERR_UNSUPPORTED,
              "conv1d_stream_mirrored: history of %d columns is odd (symmetric padding needs an even (k - 1) * d)", g->hist);
  PWG_REQUIRE(d->t_in <= (1 << 28), PWG_ERR_UNSUPPORTED, "conv1d_stream_mirrored: chunk of %d columns", d->t_in);
  return PWG_OK;
}

namespace {

constexpr int SC = 64;  // input channels staged per LDS block (four 16-channel groups of the image)

// LDS row stride for a window of w columns: >= w and == 16 (mod 64), so that the four channel rows one MFMA step reads
// (16 lanes each, consecutive columns) fall on four different groups of 16 banks
constexpr int xs_stride(int w) { return (((w > 16 ? w - 16 : 0) + 63) / 64) * 64 + 16; }
static_assert(SC * xs_stride(kStreamMaxNt + kStreamMaxHist) * sizeof(float) <= kStreamLdsBytes,
              "the widest fp32 window does not fit LDS");

struct StreamArgs : StreamCommonArgs {
  const float* w;
  int cin_pad, m_pad, xs;
};

struct StreamDelayedArgs : StreamArgs {
  StreamDelay dl;
};

// One workgroup (4 waves) owns MT = 16 * TM rows x NT = 16 * TN columns.  The reduction is dealt over the four waves:
// wave w takes the w-th 16-channel group of every staged block of 64 channels, and the four partial tiles are summed
// through LDS in wave order, ((p0 + p1) + p2) + p3 -- the same in every configuration.
// MIRRORED (with DELAYED): the window is read through the mirror rule (StreamMirrorWindow); everything else is the
// delayed form.
struct StreamMirroredArgs : StreamDelayedArgs {
  int in_lo, in_hi;  // the input's valid window, saturated (mirror_bound)
};

// SLOTTED (with DELAYED): the item's position comes from the launch's table (StreamSlots); a running item is from there
// on the delayed form with its own window, a fresh one reads no state, a paused one copies its state through, stores
// zeros and returns.  With MIRRORED the row also gives the input's edges, which stand where a.in_lo / a.in_hi do; the
// arguments are the slotted ones (a reflect-padded layer has no addends: both delay lines are zero).
struct StreamSlotsArgs : StreamArgs {
  StreamSlots sl;
};

template <bool DELAYED, bool MIRRORED, bool SLOTTED>
using stream_args_t = std::conditional_t<
    SLOTTED, StreamSlotsArgs,
    std::conditional_t<MIRRORED, StreamMirroredArgs, std::conditional_t<DELAYED, StreamDelayedArgs, StreamArgs>>>;

template <int TM, int TN, bool TRANSPOSED, bool DELAYED = false, bool MIRRORED = false, bool SLOTTED = false>
__global__ __launch_bounds__(256) void conv1d_stream_kernel(stream_args_t<DELAYED, MIRRORED, SLOTTED> a) {
  static_assert(!MIRRORED || (DELAYED && !TRANSPOSED), "the mirrored form is a delayed stride-1 convolution");
  static_assert(!SLOTTED || DELAYED, "the slotted form is a delayed launch with a position per item");
  constexpr int MT = 16 * TM, NT = 16 * TN;
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [SC][a.xs]; afterwards the partial tiles [4][MT][NT]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int q0 = blockIdx.x * NT, m0 = blockIdx.y * MT, b = blockIdx.z;
  const int H = a.hist, n = a.ep.n, XS = a.xs;
  const int W = NT + H;  // window column w holds stream column q0 - H + w (chunk-relative; < 0: history)
  const int wg = blockIdx.y * gridDim.x + blockIdx.x, nwg = gridDim.x * gridDim.y;
  const float* __restrict__ xb = a.x + (size_t)b * a.c_in * n;

  // SLOTTED: what this item's table row resolves to -- fresh, paused and its own window (a.sl.delayed(item) stands
  // where a.dl does)
  [[maybe_unused]] std::conditional_t<SLOTTED, StreamSlots::Item, StreamNoDelay> item;
  bool fresh = false;
  if constexpr (SLOTTED) {
    if constexpr (MIRRORED)
      item = a.sl.mirrored_at(b, H, n);
    else
      item = a.sl.at(b, a.ep.t_out);
    fresh = item.fresh;
  }
  const float* __restrict__ hb = a.hist_in && !fresh ? a.hist_in + (size_t)b * a.c_in * H : nullptr;

  if constexpr (SLOTTED) {
    if (item.paused) {  // (workgroup-uniform) the history rule with n = 0, zeros for y; in front of every barrier
      stream_write_history<1>(xb, hb, a.hist_out + (size_t)b * a.c_in * H, a.c_in, 0, H, false, wg, nwg);
      stream_write_lines(a.sl.delayed(item), a.ep, b, 0, wg, nwg);
      stream_store_zeros<MT, NT, TRANSPOSED, StreamRows::PhaseMajor>(a.ep, m0, q0, b);
      return;
    }
  }
  stream_write_history<1>(xb, hb, a.hist_out + (size_t)b * a.c_in * H, a.c_in, n, H, a.pad_mode == PWG_PAD_REPLICATE, wg,
                          nwg);
  if constexpr (SLOTTED)
    stream_write_lines(a.sl.delayed(item), a.ep, b, a.ep.t_out, wg, nwg);
  else if constexpr (DELAYED)
    stream_write_lines(a.dl, a.ep, b, a.ep.t_out, wg, nwg);

  f32x4 acc[TM][TN];
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A operands straight from the packed image: per (16-channel group, tap) 4 MFMA steps x TM row tiles, one float per
  // lane each (row m0 + mi * 16 + lane % 16, channel group base + 4 * step + lane / 16).  They are fetched in batches
  // of up to TB taps, the next batch in flight while the current one is contracted (and across the staging of the next
  // block): a launch is mostly a pass over the weights, few waves are resident, so loads in flight per wave are what
  // bounds it.
  constexpr int TB = 4;
  typedef float abuf_t[TB][4][TM];
  const float* __restrict__ wlane = a.w + (size_t)(wave * 16 + lq) * a.m_pad + m0 + l15;
  auto load_batch = [&](abuf_t& av, int c0, int tap0) {
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      if (tap0 + u < a.taps) {
        const float* __restrict__ wp = wlane + ((size_t)(tap0 + u) * a.cin_pad + c0) * a.m_pad;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int mi = 0; mi < TM; ++mi) av[u][kk][mi] = wp[(size_t)kk * 4 * a.m_pad + mi * 16];
      }
    }
  };
  auto contract = [&](const abuf_t& av, int tap0, const float* xt) {
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      if (tap0 + u < a.taps) {
        float bv[4][TN];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) bv[kk][ni] = xt[kk * 4 * XS + (tap0 + u) * a.dil + ni * 16];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][kk][mi], bv[kk][ni], acc[mi][ni], 0, 0, 0);
      }
    }
  };
  abuf_t buf0, buf1;
  int parity = 0;
  if (wave * 16 < a.cin_pad) load_batch(buf0, 0, 0);

  // window elements come from the history, the chunk or the start-of-stream padding; the pre-activation is applied on
  // the way into LDS.  The load phase is branch-free: the source address is selected (a safe one where the element is
  // zero padding or past the chunk) and always loaded, so that the loads of a staging batch are issued back to back
  const StreamWindow raw_win = {xb, hb, n, H, a.pad_mode};
  const auto win = [&] {
    if constexpr (MIRRORED && SLOTTED)
      return StreamMirrorWindow{raw_win, item.in_lo, item.in_hi};  // (the item's own edges, saturated on the device)
    else if constexpr (MIRRORED)
      return StreamMirrorWindow{raw_win, a.in_lo, a.in_hi};  // (the launch passes pad_mode zero: history reads raw)
    else
      return raw_win;
  }();
  const int r_first = tid / W, w_first = tid - r_first * W;

  for (int c0 = 0; c0 < a.cin_pad; c0 += SC) {
    if (c0) __syncthreads();
    // ---- stage the block's channels (up to SC; none past the image) x W columns, 8 loads in flight per thread.
    // Element tid + 256 * i is (row, column) = (r, w); stepping by 256 adds (a.step_q, a.step_w) with one carry, so
    // the only division is the one per thread in front of the block loop
    const int rows = a.cin_pad - c0 < SC ? a.cin_pad - c0 : SC;
    for (int r = r_first, w = w_first; r < rows;) {
      float v[8];
      bool ok[8];
      int off[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool live = r < rows;
        off[u] = live ? r * XS + w : -1;
        const int ci = c0 + r;
        const StreamWindow::Column col = win.at(q0 - H + w);
        ok[u] = live && ci < a.c_in && col.live;
        const float* src = col.hist ? hb + ((size_t)ci * H + col.col) : xb + ((size_t)ci * n + col.col);
        v[u] = *(ok[u] ? src : xb);
        r += a.step_q;
        w += a.step_w;
        if (w >= W) {
          w -= W;
          ++r;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float f = ok[u] ? v[u] : 0.f;
        const float neg = a.pre_act == PWG_ACT_LEAKY_RELU ? f * a.pre_slope : (a.pre_act == PWG_ACT_RELU ? 0.f : f);
        f = f > 0.f ? f : neg;
        if (off[u] >= 0) xs[off[u]] = f;
      }
    }
    __syncthreads();
    if (c0 + wave * 16 >= a.cin_pad) continue;  // this wave's group of the block lies past the image (wave-uniform)
    const bool more_blocks = c0 + SC + wave * 16 < a.cin_pad;
    const float* xt = xs + (wave * 16 + lq) * XS + l15;
    for (int tap0 = 0; tap0 < a.taps; tap0 += TB) {
      const bool in_block = tap0 + TB < a.taps;
      const bool has_next = in_block || more_blocks;
      const int nc0 = in_block ? c0 : c0 + SC, ntap0 = in_block ? tap0 + TB : 0;
      if (parity == 0) {
        if (has_next) load_batch(buf1, nc0, ntap0);
        contract(buf0, tap0, xt);
      } else {
        if (has_next) load_batch(buf0, nc0, ntap0);
        contract(buf1, tap0, xt);
      }
      parity ^= 1;
    }
  }

  if constexpr (SLOTTED)
    stream_reduce_epilogue<MT, NT, TRANSPOSED, StreamRows::PhaseMajor>(xs, acc, a.ep, m0, q0, b, a.sl.delayed(item));
  else if constexpr (DELAYED)
    stream_reduce_epilogue<MT, NT, TRANSPOSED, StreamRows::PhaseMajor>(xs, acc, a.ep, m0, q0, b, a.dl);
  else
    stream_reduce_epilogue<MT, NT, TRANSPOSED, StreamRows::PhaseMajor>(xs, acc, a.ep, m0, q0, b);
}

template <int TM, int TN, bool TRANSPOSED>
struct Kernel {
  static constexpr auto fn = conv1d_stream_kernel<TM, TN, TRANSPOSED>;
};

template <int TM, int TN, bool TRANSPOSED>
struct DelayedKernel {
  static constexpr auto fn = conv1d_stream_kernel<TM, TN, TRANSPOSED, true>;
};

template <int TM, int TN, bool TRANSPOSED>
struct SlotsKernel {
  static constexpr auto fn = conv1d_stream_kernel<TM, TN, TRANSPOSED, true, false, true>;
};

// (mirrored_geometry() admits no transposed layer: that slot of stream_launch names the same kernel, never launched)
template <int TM, int TN, bool TRANSPOSED>
struct MirroredKernel {
  static constexpr auto fn = conv1d_stream_kernel<TM, TN, false, true, true>;
};

template <int TM, int TN, bool TRANSPOSED>
struct SlotsMirroredKernel {
  static constexpr auto fn = conv1d_stream_kernel<TM, TN, false, true, true, true>;
};

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_conv1d_stream_supported(const pwg_conv1d_desc* d) {
  StreamGeom g;
  return stream_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_conv1d_stream_hist_floats(const pwg_conv1d_desc* d) {
  StreamGeom g;
  if (stream_geometry(d, &g) != PWG_OK) return 0;
  return (size_t)d->batch * d->c_in * g.hist;
}

// Diagnostics, host only: the tile and grid every conv stream launch of `d` takes, in either precision and every form
// (they all call stream_geometry + stream_tile as below and launch on stream_grid).  Launches nothing.
extern "C" int pwg_conv1d_stream_plan(const pwg_conv1d_desc* d, int32_t* out) {
  StreamGeom g;
  const int rc = stream_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(out != nullptr, PWG_ERR_NULL, "conv1d_stream_plan: NULL out");
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  const dim3 grid = stream_grid(tile, g.m, d->batch);
  out[0] = 16 * tile.tm;
  out[1] = 16 * tile.tn;
  out[2] = (int32_t)grid.x;
  out[3] = (int32_t)grid.y;
  out[4] = (int32_t)grid.z;
  return PWG_OK;
}

// The fields of the argument struct that come from the fp32 packed image -> the LDS bytes of the staged window
static size_t fill_image_args(StreamArgs* a, const float* w_packed, const StreamGeom& g, const StreamTile& tile) {
  a->w = w_packed;
  a->cin_pad = g.cin_pad;
  a->m_pad = g.m_pad;
  a->xs = xs_stride(16 * tile.tn + g.hist);
  return (size_t)SC * a->xs * sizeof(float);
}

static double image_bytes(const StreamGeom& g) { return 4.0 * (double)g.taps * g.cin_pad * g.m_pad; }

extern "C" int pwg_conv1d_stream_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                                         const float* w_packed, const float* bias, const float* add1, const float* add2,
                                         float* y, void* stream_) {
  StreamGeom g;
  const int rc = stream_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 3u) == 0, PWG_ERR_BAD_SHAPE, "conv1d_stream: unaligned weight image");
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  StreamArgs a;
  const size_t window = fill_image_args(&a, w_packed, g, tile);
  return stream_run<Kernel>("conv1d_stream", "conv1d_stream_kernel", d, g, tile, &a, x, hist_in, hist_out, w_packed, bias,
                            add1, add2, y, window, 0.0, image_bytes(g), (hipStream_t)stream_);
}

extern "C" int pwg_conv1d_stream_delayed_supported(const pwg_conv1d_desc* d, int32_t delay1, int32_t delay2) {
  StreamGeom g;
  return delayed_geometry(d, delay1, delay2, &g) == PWG_OK ? 1 : 0;
}

extern "C" int pwg_conv1d_stream_delayed_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                                 float* hist_out, const float* w_packed, const float* bias,
                                                 const float* add1, const float* add1_hist_in, float* add1_hist_out,
                                                 int32_t delay1, const float* add2, const float* add2_hist_in,
                                                 float* add2_hist_out, int32_t delay2, int32_t valid_lo, int32_t valid_hi,
                                                 float* y, void* stream_) {
  StreamGeom g;
  int rc = delayed_geometry(d, delay1, delay2, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 3u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_delayed: unaligned weight image");
  StreamDelayedArgs a;
  rc = stream_delay_lines("conv1d_stream_delayed", add1, add1_hist_in, add1_hist_out, delay1, add2, add2_hist_in,
                          add2_hist_out, delay2, valid_lo, valid_hi, &a.dl);
  if (rc != PWG_OK) return rc;
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  const size_t window = fill_image_args(&a, w_packed, g, tile);
  return stream_run<DelayedKernel>("conv1d_stream_delayed", "conv1d_stream_delayed_kernel", d, g, tile, &a, x, hist_in,
                                   hist_out, w_packed, bias, add1, add2, y, window,
                                   (double)d->batch * d->c_out * (delay1 + delay2), image_bytes(g), (hipStream_t)stream_);
}

extern "C" int pwg_conv1d_stream_slots_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                               float* hist_out, const float* w_packed, const float* bias,
                                               const float* add1, const float* add1_hist_in, float* add1_hist_out,
                                               int32_t delay1, const float* add2, const float* add2_hist_in,
                                               float* add2_hist_out, int32_t delay2, const int32_t* slots, int32_t rate,
                                               int32_t delay, float* y, void* stream_) {
  StreamGeom g;
  int rc = delayed_geometry(d, delay1, delay2, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 3u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_slots: unaligned weight image");
  PWG_REQUIRE(hist_in || g.hist == 0, PWG_ERR_NULL,
              "conv1d_stream_slots: hist_in is NULL (the start of a stream is an item's, in the table)");
  StreamSlotsArgs a;
  rc = stream_slot_lines("conv1d_stream_slots", add1, add1_hist_in, add1_hist_out, delay1, add2, add2_hist_in,
                         add2_hist_out, delay2, slots, rate, delay, &a.sl);
  if (rc != PWG_OK) return rc;
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  const size_t window = fill_image_args(&a, w_packed, g, tile);
  return stream_run<SlotsKernel>("conv1d_stream_slots", "conv1d_stream_slots_kernel", d, g, tile, &a, x, hist_in, hist_out,
                                 w_packed, bias, add1, add2, y, window,
                                 (double)d->batch * d->c_out * (delay1 + delay2), image_bytes(g), (hipStream_t)stream_);
}

extern "C" int pwg_conv1d_stream_mirrored_supported(const pwg_conv1d_desc* d) {
  StreamGeom g;
  return mirrored_geometry(d, &g) == PWG_OK ? 1 : 0;
}

extern "C" int pwg_conv1d_stream_mirrored_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                                  float* hist_out, const float* w_packed, const float* bias, float* y,
                                                  int32_t in_lo, int32_t in_hi, int32_t valid_lo, int32_t valid_hi,
                                                  void* stream_) {
  StreamGeom g;
  int rc = mirrored_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 3u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_mirrored: unaligned weight image");
  StreamMirroredArgs a;
  rc = stream_delay_lines("conv1d_stream_mirrored", nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, valid_lo,
                          valid_hi, &a.dl);
  if (rc != PWG_OK) return rc;
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  const size_t window = fill_image_args(&a, w_packed, g, tile);
  a.in_lo = mirror_bound(in_lo, g.hist, d->t_in);
  a.in_hi = mirror_bound(in_hi, g.hist, d->t_in);
  // history and chunk are read raw (zeros before the stream, stored zeros around the utterance): the launch itself is
  // a zero-padded one, the reflection lives in the window's mirror rule alone
  pwg_conv1d_desc raw = *d;
  raw.pad_mode = PWG_PAD_ZERO;
  return stream_run<MirroredKernel>("conv1d_stream_mirrored", "conv1d_stream_mirrored_kernel", &raw, g, tile, &a, x, hist_in,
                                    hist_out, w_packed, bias, nullptr, nullptr, y, window, 0.0, image_bytes(g),
                                    (hipStream_t)stream_);
}

// The slotted-mirrored launch: what pwg_conv1d_stream_slots_mirrored_forward (csrc/conv1d_stream_slots_mirrored.hip) is.
// The kernel family lives here; the entry point has its own translation unit and its own tests
// (tests/test_stream_melgan_pool_gpu.py).
int pwg::stream_slots_mirrored_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in, float* hist_out,
                                       const float* w_packed, const float* bias, const int32_t* slots, int32_t rate,
                                       int32_t delay, float* y, void* stream_) {
  StreamGeom g;
  int rc = mirrored_geometry(d, &g);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 3u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_slots_mirrored: unaligned weight image");
  PWG_REQUIRE(hist_in || g.hist == 0, PWG_ERR_NULL,
              "conv1d_stream_slots_mirrored: hist_in is NULL (the start of a stream is an item's, in the table)");
  StreamSlotsArgs a;
  rc = stream_slot_lines("conv1d_stream_slots_mirrored", nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, slots,
                         rate, delay, &a.sl);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(delay >= g.hist / 2, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_slots_mirrored: delay = %d is less than the layer's padding %d (the input would be early)",
              delay, g.hist / 2);
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  const size_t window = fill_image_args(&a, w_packed, g, tile);
  // as in the mirrored entry: the launch itself is a zero-padded one, the reflection lives in the window's mirror rule
  pwg_conv1d_desc raw = *d;
  raw.pad_mode = PWG_PAD_ZERO;
  return stream_run<SlotsMirroredKernel>("conv1d_stream_slots_mirrored", "conv1d_stream_slots_mirrored_kernel", &raw, g, tile,
                                         &a, x, hist_in, hist_out, w_packed, bias, nullptr, nullptr, y, window, 0.0,
                                         image_bytes(g), (hipStream_t)stream_);
}
