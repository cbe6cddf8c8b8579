// conv1d_stream_bf16.hip -- the stream launch of conv1d_stream.hip under the numerical definition of conv1d_bf16.hip.
//
// One launch takes the new chunk x (B, C_in, n) and the history hist_in (B, C_in, H), writes y (B, C_out, n) -- n * s for
// the causal k = 2s transposed form -- and hist_out = the last H RAW fp32 columns of concat(hist_in, x): the state of a
// stream does not depend on its precision, and hist_out is bit-identical to what the fp32 stream launch writes.
//
// Numerical definition.  The window is concat(hist_in, x) (hist_in == NULL: the start-of-stream context of pad_mode, as
// in conv1d_stream.hip); the fused pre-activation is applied in fp32 while the window is staged, to history, chunk and
// padding alike; the activated value is rounded to bf16 (round-to-nearest-even, a plain cast) on the way into LDS; the
// weights are the layer's bf16 image (rounded once, when it is packed); products accumulate in fp32 on the bf16 MFMA;
// bias / add1 / add2 / out_mul / out_div / post-activation / the stored result are fp32.
//   Y[m][j] = sum_{tap, ci} W[m][tap][ci] * bf16(act(X[ci][j - H + tap * dil]))        X[t < 0] = history
//   Conv1d:          m = output channel, taps = k, dil = dilation
//   ConvTranspose1d: m = co * s + phase, taps = 2 (x[j - 1] with w[phase + s], x[j] with w[phase]), output column
//                    j * s + phase -- the row order of the bf16 image (csrc/mfma_conv.h), NOT the phase-major order
//                    of the fp32 one
// The A operand is read straight from that image (layout and row padding: csrc/mfma_conv.h; rows come in whole tiles of 32:
// a 16-row block never leaves it; no second image).  The B operand is the window of NT + H columns, staged per block of
// 128 input channels into LDS as bf16 in [column][channel] order: a lane's 8 reduction elements are one ds_read_b128,
// and a row is 17 slots of 16 B (odd), so that the 16 columns an MFMA reads start on 16 different slots of the bank row.
// A kernel-1 convolution is the case H = 0 (no history buffers).
//
// Contraction and sum order (the contract): v_mfma_f32_16x16x32_bf16 only, whatever the tile.  Number the (32-channel
// chunk, tap) pairs of the layer item = chunk * taps + tap.  An output element is ((p0 + p1) + p2) + p3, where p_w is the
// MFMA accumulation over the items with item % 4 == w in ascending order.  That depends on the layer alone -- not on n,
// the batch, the chunk's position in the stream, the tile, or whether a window column came from history, chunk or
// padding.  One workgroup owns an output tile over the whole reduction: no split across workgroups, no workspace, no
// atomics.  (Dealing items instead of whole chunks keeps all four waves busy on the 32- and 64-channel layers at the
// bottom of a generator, which have one or two chunks but 3 .. 11 taps -- "wave w takes chunk w" would leave three or
// two waves idle there -- and costs the wide layers nothing: a full block is 4 * taps items, taps per wave either way.
// A block starts at a multiple of 4 items, so item % 4 is also the item's number inside its block.)
//
// Tiles: as the fp32 stream kernel -- 16 rows x 16 / 32 / 64 columns for chunks of up to 16 / 32 / more columns, 32 x 64
// when that still gives every CU two workgroups; the four waves deal the REDUCTION, and the A fragments of the next four
// items (one 16-B load per lane and item) are in flight while the current four are contracted.  DESIGN.md s11.2.
//
// Delayed form (pwg_conv1d_stream_bf16_delayed_forward): the delayed form of conv1d_stream.hip under
// the numerical definition above, for a layer of a NON-causal network streamed with a fixed look-ahead.  The addends
// are read through delay lines kept like the history (raw fp32, bit-identical to what the fp32 delayed launch writes)
// and output columns outside the valid window are stored as 0.0f (StreamDelay, stream_common.h): bf16(act(0)) = 0, so
// the next layer sees the whole-utterance zero padding.  Staging, item dealing, A-fragment prefetch, contraction and
// sum order are those of the plain form: only the history writer and the epilogue differ, and the plain instantiations
// are the code they were.
//
// Slotted form (pwg_conv1d_stream_slots_forward_bf16): the slotted form of conv1d_stream.hip under
// the numerical definition above -- a position per item from a device table, fresh and paused items, and a running
// item's columns bit for bit the delayed form's with the same window.
#include "mfma_conv.h"
#include "stream_common.h"

namespace pwg {
namespace {

constexpr int SC = 4 * KC;        // input channels staged per LDS block (KC, a chunk of the image: one MFMA reduction step)
constexpr int ROW = SC + 8;       // bf16 elements per LDS row: 17 slots of 16 B
static_assert((kStreamMaxNt + kStreamMaxHist) * ROW * sizeof(__bf16) <= kStreamLdsBytes,
              "the widest bf16 window does not fit LDS");

struct StreamBf16Args : StreamCommonArgs {
  const bf16x8* w;
  int cin_chunks, m_pad;
  int q4, r4;  // 4 / taps and 4 % taps: a wave's next item is 4 items on
};

struct StreamBf16DelayedArgs : StreamBf16Args {
  StreamDelay dl;
};

struct StreamBf16SlotsArgs : StreamBf16Args {
  StreamSlots sl;
};

// (chunk of the staged block, tap) of an item; wave-uniform
struct Item {
  int cl, tap;
};

// One workgroup (4 waves) owns MT = 16 * TM rows x NT = 16 * TN columns; wave w contracts the items with item % 4 == w
// and the four partial tiles are summed through LDS in wave order, ((p0 + p1) + p2) + p3 -- the same in every configuration.
// SLOTTED (with DELAYED): as in conv1d_stream.hip -- the item's position comes from the launch's table (StreamSlots).
template <int TM, int TN, bool TRANSPOSED, bool DELAYED = false, bool SLOTTED = false>
__global__ __launch_bounds__(256) void conv1d_stream_bf16_kernel(
    std::conditional_t<SLOTTED, StreamBf16SlotsArgs, std::conditional_t<DELAYED, StreamBf16DelayedArgs, StreamBf16Args>> a) {
  static_assert(!SLOTTED || DELAYED, "the slotted form is a delayed launch with a position per item");
  constexpr int MT = 16 * TM, NT = 16 * TN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [W][ROW]; afterwards the partial tiles [4][MT][NT + 1] fp32

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int q0 = blockIdx.x * NT, m0 = blockIdx.y * MT, b = blockIdx.z;
  const int H = a.hist, n = a.ep.n;
  const int W = NT + H;  // window column w holds stream column q0 - H + w (chunk-relative; < 0: history)
  const int wg = blockIdx.y * gridDim.x + blockIdx.x, nwg = gridDim.x * gridDim.y;
  const float* __restrict__ xb = a.x + (size_t)b * a.c_in * n;

  // SLOTTED: what this item's table row resolves to -- fresh, paused and its own window (a.sl.delayed(item) stands
  // where a.dl does)
  [[maybe_unused]] std::conditional_t<SLOTTED, StreamSlots::Item, StreamNoDelay> item;
  bool fresh = false;
  if constexpr (SLOTTED) {
    item = a.sl.at(b, a.ep.t_out);
    fresh = item.fresh;
  }
  const float* __restrict__ hb = a.hist_in && !fresh ? a.hist_in + (size_t)b * a.c_in * H : nullptr;

  if constexpr (SLOTTED) {
    if (item.paused) {  // (workgroup-uniform) the history rule with n = 0, zeros for y; in front of every barrier
      stream_write_history<1>(xb, hb, a.hist_out + (size_t)b * a.c_in * H, a.c_in, 0, H, false, wg, nwg);
      stream_write_lines(a.sl.delayed(item), a.ep, b, 0, wg, nwg);
      stream_store_zeros<MT, NT, TRANSPOSED, StreamRows::ChannelMajor>(a.ep, m0, q0, b);
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

  // this wave's first item of a block is item `wave` of it; the following ones are 4 items apart
  Item first = {0, wave};
  while (first.tap >= a.taps) {
    first.tap -= a.taps;
    ++first.cl;
  }
  auto advance = [&](Item& it) {
    it.tap += a.r4;
    it.cl += a.q4;
    if (it.tap >= a.taps) {
      it.tap -= a.taps;
      ++it.cl;
    }
  };
  auto chunks_of = [&](int blk) {  // chunks of the image in staged block blk (<= 0 past the last one)
    const int left = a.cin_chunks - 4 * blk;
    return left < 4 ? left : 4;
  };

  // A operands straight from the image: per item and row tile one 16-B fragment per lane (row m0 + mi * 16 + lane % 16,
  // channels 8 * (lane / 16) .. + 7 of the chunk).  They are fetched in batches of up to TB items, the next batch in
  // flight while the current one is contracted (and across the staging of the next block).
  constexpr int TB = 4;
  typedef bf16x8 abuf_t[TB][TM];
  const bf16x8* __restrict__ wlane = a.w + (size_t)lq * a.m_pad + m0 + l15;
  auto load_batch = [&](abuf_t& av, int blk, Item& it) {
    const int nch = chunks_of(blk);
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      if (it.cl < nch) {
        const bf16x8* __restrict__ wp = wlane + ((size_t)it.tap * a.cin_chunks + blk * 4 + it.cl) * 4 * a.m_pad;
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) av[u][mi] = wp[mi * 16];
      }
      advance(it);
    }
  };
  auto contract = [&](const abuf_t& av, int nch, Item& it) {
#pragma unroll
    for (int u = 0; u < TB; ++u) {
      if (it.cl < nch) {
        const __bf16* xt = xs + (size_t)(l15 + it.tap * a.dil) * ROW + (it.cl * 4 + lq) * 8;
        bf16x8 bv[TN];
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) bv[ni] = *reinterpret_cast<const bf16x8*>(xt + ni * 16 * ROW);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
          for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = Mfma<16>::run(av[u][mi], bv[ni], acc[mi][ni]);
      }
      advance(it);
    }
  };
  abuf_t buf0, buf1;
  int parity = 0;
  int lblk = 0;        // block and item the next batch of loads starts at
  Item lit = first;
  load_batch(buf0, 0, lit);

  // window elements come from the history, the chunk or the start-of-stream padding; the pre-activation and the
  // rounding are applied on the way into LDS.  The load phase is branch-free: the source address is selected (a safe
  // one where the element is zero padding, past the chunk or past c_in) and always loaded
  const StreamWindow win = {xb, hb, n, H, a.pad_mode};
  const int o_first = tid / W, w_first = tid - o_first * W;
  const int nblocks = (a.cin_chunks + 3) >> 2;

  for (int blk = 0; blk < nblocks; ++blk) {
    if (blk) __syncthreads();
    // ---- stage the block's chunks (all 32 channels of each: zeros past c_in) x W columns.  Item tid + 256 * i is
    // (channel octet, column) = (o, w): lanes walk the columns (coalesced fp32 rows), 8 channels are activated, rounded
    // and written as one 16-B LDS store; 16 loads in flight per thread.  Stepping by 256 adds (a.step_q, a.step_w)
    // with one carry, so the only division is the one per thread in front of the block loop
    const int c0 = blk * SC, nch = chunks_of(blk), octs = nch * 4;
    for (int o = o_first, w = w_first; o < octs;) {
      constexpr int U = 2;
      float v[U][8];
      bool ok[U][8];
      int off[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool live = o < octs;
        off[u] = live ? w * ROW + o * 8 : -1;
        const StreamWindow::Column col = win.at(q0 - H + w);
        const bool okc = live && col.live;
        const float* src = (col.hist ? hb : xb) + col.col;
        const size_t rs = col.hist ? H : n;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ci = c0 + o * 8 + j;
          ok[u][j] = okc && ci < a.c_in;
          v[u][j] = *(ok[u][j] ? src + (size_t)ci * rs : xb);
        }
        o += a.step_q;
        w += a.step_w;
        if (w >= W) {
          w -= W;
          ++o;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bf16x8 p;
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = (__bf16)apply_act(ok[u][j] ? v[u][j] : 0.f, a.pre_act, a.pre_slope);
        if (off[u] >= 0) *reinterpret_cast<bf16x8*>(xs + off[u]) = p;
      }
    }
    __syncthreads();
    Item cit = first;
    while (cit.cl < nch) {  // (wave-uniform)
      if (lblk == blk && lit.cl >= nch) {  // the batch in hand is this wave's last of the block
        lblk = blk + 1;
        lit = first;
      }
      const bool has_next = lit.cl < chunks_of(lblk);
      if (parity == 0) {
        if (has_next) load_batch(buf1, lblk, lit);
        contract(buf0, nch, cit);
      } else {
        if (has_next) load_batch(buf0, lblk, lit);
        contract(buf1, nch, cit);
      }
      parity ^= 1;
    }
  }

  if constexpr (SLOTTED)
    stream_reduce_epilogue<MT, NT, TRANSPOSED, StreamRows::ChannelMajor>(reinterpret_cast<float*>(smem), acc, a.ep, m0, q0, b,
                                                                         a.sl.delayed(item));
  else if constexpr (DELAYED)
    stream_reduce_epilogue<MT, NT, TRANSPOSED, StreamRows::ChannelMajor>(reinterpret_cast<float*>(smem), acc, a.ep, m0, q0, b,
                                                                         a.dl);
  else
    stream_reduce_epilogue<MT, NT, TRANSPOSED, StreamRows::ChannelMajor>(reinterpret_cast<float*>(smem), acc, a.ep, m0, q0, b);
}

template <int TM, int TN, bool TRANSPOSED>
struct Kernel {
  static constexpr auto fn = conv1d_stream_bf16_kernel<TM, TN, TRANSPOSED>;
};

template <int TM, int TN, bool TRANSPOSED>
struct DelayedKernel {
  static constexpr auto fn = conv1d_stream_bf16_kernel<TM, TN, TRANSPOSED, true>;
};

template <int TM, int TN, bool TRANSPOSED>
struct SlotsKernel {
  static constexpr auto fn = conv1d_stream_bf16_kernel<TM, TN, TRANSPOSED, true, true>;
};

// The image of the layer (csrc/mfma_conv.h) and the fields of the argument struct that come from it.  The image does
// not depend on padding, which its owner's geometry admits only as zero.
int bf16_image(const char* name, const pwg_conv1d_desc* d, MfmaConvGeom* image) {
  pwg_conv1d_desc dz = *d;
  dz.pad_mode = PWG_PAD_ZERO;
  PWG_REQUIRE(mfma_conv_geometry("conv1d_bf16", 1, true, &dz, image) == PWG_OK, PWG_ERR_UNSUPPORTED,
              "%s: the layer has no bf16 weight image", name);
  return PWG_OK;
}

void fill_image_args(StreamBf16Args* a, const void* w_packed_bf16, const MfmaConvGeom& image, const StreamGeom& g) {
  a->w = static_cast<const bf16x8*>(w_packed_bf16);
  a->cin_chunks = image.cin_chunks;
  a->m_pad = image.m_pad;  // of the bf16 image, not g.m_pad
  a->q4 = 4 / g.taps;
  a->r4 = 4 % g.taps;
}

}  // namespace
}  // namespace pwg

using namespace pwg;

// Coverage is that of the fp32 stream kernel by construction: a layer that streams in fp32 streams in bf16.
extern "C" int pwg_conv1d_stream_bf16_supported(const pwg_conv1d_desc* d) { return pwg_conv1d_stream_supported(d); }

// LDS bytes of the staged window
static size_t window_bytes(const StreamGeom& g, const StreamTile& tile) {
  return (size_t)(16 * tile.tn + g.hist) * ROW * sizeof(__bf16);
}

extern "C" int pwg_conv1d_stream_bf16_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                              float* hist_out, const void* w_packed_bf16, const float* bias,
                                              const float* add1, const float* add2, float* y, void* stream_) {
  StreamGeom g;
  if (stream_geometry(d, &g) != PWG_OK) return PWG_ERR_UNSUPPORTED;  // (pwg_last_error holds the reason)
  MfmaConvGeom image;
  const int rc = bf16_image("conv1d_stream_bf16", d, &image);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed_bf16) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_bf16: the weight image must be 16-B aligned");
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  StreamBf16Args a;
  fill_image_args(&a, w_packed_bf16, image, g);
  return stream_run<Kernel>("conv1d_stream_bf16", "conv1d_stream_bf16_kernel", d, g, tile, &a, x, hist_in, hist_out,
                            w_packed_bf16, bias, add1, add2, y, window_bytes(g, tile), 0.0,
                            2.0 * (double)image_elems(image), (hipStream_t)stream_);
}

// Coverage is that of the fp32 delayed form by construction: both go through delayed_geometry().
extern "C" int pwg_conv1d_stream_bf16_delayed_supported(const pwg_conv1d_desc* d, int32_t delay1, int32_t delay2) {
  return pwg_conv1d_stream_delayed_supported(d, delay1, delay2);
}

extern "C" int pwg_conv1d_stream_bf16_delayed_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                                      float* hist_out, const void* w_packed_bf16, const float* bias,
                                                      const float* add1, const float* add1_hist_in, float* add1_hist_out,
                                                      int32_t delay1, const float* add2, const float* add2_hist_in,
                                                      float* add2_hist_out, int32_t delay2, int32_t valid_lo,
                                                      int32_t valid_hi, float* y, void* stream_) {
  StreamGeom g;
  int rc = delayed_geometry(d, delay1, delay2, &g);
  if (rc != PWG_OK) return rc;
  MfmaConvGeom image;
  rc = bf16_image("conv1d_stream_bf16_delayed", d, &image);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed_bf16) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_bf16_delayed: the weight image must be 16-B aligned");
  StreamBf16DelayedArgs a;
  rc = stream_delay_lines("conv1d_stream_bf16_delayed", add1, add1_hist_in, add1_hist_out, delay1, add2, add2_hist_in,
                          add2_hist_out, delay2, valid_lo, valid_hi, &a.dl);
  if (rc != PWG_OK) return rc;
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  fill_image_args(&a, w_packed_bf16, image, g);
  return stream_run<DelayedKernel>("conv1d_stream_bf16_delayed", "conv1d_stream_bf16_delayed_kernel", d, g, tile, &a, x,
                                   hist_in, hist_out, w_packed_bf16, bias, add1, add2, y, window_bytes(g, tile),
                                   (double)d->batch * d->c_out * (delay1 + delay2), 2.0 * (double)image_elems(image),
                                   (hipStream_t)stream_);
}

// The slotted form (conv1d_stream.hip) under the numerical definition above; coverage is that of the delayed forms.
extern "C" int pwg_conv1d_stream_slots_forward_bf16(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                                    float* hist_out, const void* w_packed_bf16, const float* bias,
                                                    const float* add1, const float* add1_hist_in, float* add1_hist_out,
                                                    int32_t delay1, const float* add2, const float* add2_hist_in,
                                                    float* add2_hist_out, int32_t delay2, const int32_t* slots,
                                                    int32_t rate, int32_t delay, float* y, void* stream_) {
  StreamGeom g;
  int rc = delayed_geometry(d, delay1, delay2, &g);
  if (rc != PWG_OK) return rc;
  MfmaConvGeom image;
  rc = bf16_image("conv1d_stream_slots_bf16", d, &image);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed_bf16) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_slots_bf16: the weight image must be 16-B aligned");
  PWG_REQUIRE(hist_in || g.hist == 0, PWG_ERR_NULL,
              "conv1d_stream_slots_bf16: hist_in is NULL (the start of a stream is an item's, in the table)");
  StreamBf16SlotsArgs a;
  rc = stream_slot_lines("conv1d_stream_slots_bf16", add1, add1_hist_in, add1_hist_out, delay1, add2, add2_hist_in,
                         add2_hist_out, delay2, slots, rate, delay, &a.sl);
  if (rc != PWG_OK) return rc;
  const StreamTile tile = stream_tile(d->t_in, g.m, d->batch);
  fill_image_args(&a, w_packed_bf16, image, g);
  return stream_run<SlotsKernel>("conv1d_stream_slots_bf16", "conv1d_stream_bf16_slots_kernel", d, g, tile, &a, x, hist_in,
                                 hist_out, w_packed_bf16, bias, add1, add2, y, window_bytes(g, tile),
                                 (double)d->batch * d->c_out * (delay1 + delay2), 2.0 * (double)image_elems(image),
                                 (hipStream_t)stream_);
}
