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
//                    j * s + phase -- the row order of the bf16 image (csrc/conv1d_bf16.hip), NOT the phase-major order
//                    of the fp32 one
// The A operand is read straight from that image ([tap][ci / 8][m_pad][8], rows padded to 32 / 64 / 128, channels to 32:
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
#include "common.h"
#include "bf16_mfma.h"

namespace pwg {
namespace {

constexpr int KC = 32;            // input channels per chunk of the image = one MFMA reduction step
constexpr int SC = 4 * KC;        // input channels staged per LDS block
constexpr int ROW = SC + 8;       // bf16 elements per LDS row: 17 slots of 16 B
constexpr int kMaxNt = 64;        // widest column tile
constexpr int kMaxHist = 144;     // what pwg_conv1d_stream_supported admits: (64 + 144) * 272 B = 56.6 KB of LDS
constexpr int kFillWorkgroups = 256;  // one per CU

struct StreamBf16Args {
  const float* x;
  const float* hist_in;
  float* hist_out;
  const bf16x8* w;
  const float* bias;
  const float* add1;
  const float* add2;
  float* y;
  int c_in, c_out, n, t_out, hist;
  int taps, dil, cin_chunks, m, m_pad, phases;
  int q4, r4;          // 4 / taps and 4 % taps: a wave's next item is 4 items on
  int step_o, step_w;  // 256 / W and 256 % W for the staged window of W = tile columns + hist columns
  int pad_mode, pre_act, post_act;
  float pre_slope, post_slope, out_mul, out_div;
};

// (chunk of the staged block, tap) of an item; wave-uniform
struct Item {
  int cl, tap;
};

// One workgroup (4 waves) owns MT = 16 * TM rows x NT = 16 * TN columns; wave w contracts the items with item % 4 == w
// and the four partial tiles are summed through LDS in wave order, ((p0 + p1) + p2) + p3 -- the same in every configuration.
template <int TM, int TN, bool TRANSPOSED>
__global__ __launch_bounds__(256) void conv1d_stream_bf16_kernel(StreamBf16Args a) {
  constexpr int MT = 16 * TM, NT = 16 * TN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);  // [W][ROW]; afterwards the partial tiles [4][MT][NT + 1] fp32

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, lq = lane >> 4;
  const int q0 = blockIdx.x * NT, m0 = blockIdx.y * MT, b = blockIdx.z;
  const int H = a.hist, n = a.n;
  const int W = NT + H;  // window column w holds stream column q0 - H + w (chunk-relative; < 0: history)
  const float* __restrict__ xb = a.x + (size_t)b * a.c_in * n;
  const float* __restrict__ hb = a.hist_in ? a.hist_in + (size_t)b * a.c_in * H : nullptr;

  // ---- hist_out = last H columns of concat(hist_in, x), raw fp32; the elements are dealt over the workgroups of the item
  {
    const int total = a.c_in * H;
    const int wg = blockIdx.y * gridDim.x + blockIdx.x, nwg = gridDim.x * gridDim.y;
    float* __restrict__ ho = a.hist_out + (size_t)b * a.c_in * H;
    for (int i = wg * 256 + tid; i < total; i += nwg * 256) {
      const int ci = i / H, h = i - ci * H;
      const int t = n - H + h;
      float v = 0.f;
      if (t >= 0)
        v = xb[(size_t)ci * n + t];
      else if (hb)
        v = hb[(size_t)ci * H + n + h];
      else if (a.pad_mode == PWG_PAD_REPLICATE)
        v = xb[(size_t)ci * n];
      ho[i] = v;
    }
  }

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
  const bool replicate = a.pad_mode == PWG_PAD_REPLICATE, reflect = a.pad_mode == PWG_PAD_REFLECT;
  const bool has_hist = hb != nullptr;
  const int o_first = tid / W, w_first = tid - o_first * W;
  const int nblocks = (a.cin_chunks + 3) >> 2;

  for (int blk = 0; blk < nblocks; ++blk) {
    if (blk) __syncthreads();
    // ---- stage the block's chunks (all 32 channels of each: zeros past c_in) x W columns.  Item tid + 256 * i is
    // (channel octet, column) = (o, w): lanes walk the columns (coalesced fp32 rows), 8 channels are activated, rounded
    // and written as one 16-B LDS store; 16 loads in flight per thread.  Stepping by 256 adds (a.step_o, a.step_w)
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
        const int t = q0 - H + w;
        const bool in_chunk = t >= 0;
        const int tt = in_chunk ? t : (reflect ? -t : 0);  // column of x: the chunk's own, the mirrored one, or the first
        const bool okc = live && (in_chunk ? t < n : (has_hist || replicate || (reflect && tt < n)));
        const bool from_hist = !in_chunk && has_hist;
        const float* src = from_hist ? hb + (H + t) : xb + tt;
        const size_t rs = from_hist ? H : n;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int ci = c0 + o * 8 + j;
          ok[u][j] = okc && ci < a.c_in;
          v[u][j] = *(ok[u][j] ? src + (size_t)ci * rs : xb);
        }
        o += a.step_o;
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

  // ---- the four waves' partial tiles through LDS (D layout of the 16 x 16 forms: column = lane % 16,
  // row = 4 * (lane / 16) + register); every wave writes its tile, zeros where it had no item
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);  // [4][MT][NT + 1]
  constexpr int RS = NT + 1;
#pragma unroll
  for (int mi = 0; mi < TM; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[(wave * MT + mi * 16 + 4 * lq + i) * RS + ni * 16 + l15] = acc[mi][ni][i];
  __syncthreads();

  // ---- epilogue (fp32): one thread per output element, partial sums added in wave order
  for (int e = tid; e < MT * NT; e += 256) {
    const int row = e / NT, col = e - row * NT;
    const int m = m0 + row, j = q0 + col;
    if (m >= a.m || j >= n) continue;
    float v = red[row * RS + col];
    v += red[(MT + row) * RS + col];
    v += red[(2 * MT + row) * RS + col];
    v += red[(3 * MT + row) * RS + col];
    int co = m, ph = 0;
    if (TRANSPOSED) {
      co = m / a.phases;
      ph = m - co * a.phases;
    }
    const size_t o = ((size_t)b * a.c_out + co) * a.t_out + (TRANSPOSED ? j * a.phases + ph : j);
    if (a.bias) v += a.bias[co];
    if (a.add1) v += a.add1[o];
    if (a.add2) v += a.add2[o];
    if (a.out_mul != 1.0f) v *= a.out_mul;
    if (a.out_div != 1.0f) v = v / a.out_div;
    v = apply_act(v, a.post_act, a.post_slope);
    a.y[o] = v;
  }
}

template <int TM, int TN>
static void launch_tile(const StreamBf16Args& a, bool transposed, dim3 grid, size_t lds, hipStream_t stream) {
  if (transposed)
    hipLaunchKernelGGL((conv1d_stream_bf16_kernel<TM, TN, true>), grid, dim3(256), lds, stream, a);
  else
    hipLaunchKernelGGL((conv1d_stream_bf16_kernel<TM, TN, false>), grid, dim3(256), lds, stream, a);
}

}  // namespace
}  // namespace pwg

using namespace pwg;

// Coverage is that of the fp32 stream kernel by construction: a layer that streams in fp32 streams in bf16.
extern "C" int pwg_conv1d_stream_bf16_supported(const pwg_conv1d_desc* d) { return pwg_conv1d_stream_supported(d); }

extern "C" int pwg_conv1d_stream_bf16_forward(const pwg_conv1d_desc* d, const float* x, const float* hist_in,
                                              float* hist_out, const void* w_packed_bf16, const float* bias,
                                              const float* add1, const float* add2, float* y, void* stream_) {
  if (!pwg_conv1d_stream_supported(d)) return PWG_ERR_UNSUPPORTED;  // (pwg_last_error holds the reason)
  hipStream_t stream = (hipStream_t)stream_;
  const bool transposed = d->transposed != 0;
  const int taps = transposed ? 2 : d->kernel, dil = transposed ? 1 : d->dilation;
  const int hist = transposed ? 1 : d->pad_left;
  const int m = transposed ? d->c_out * d->stride : d->c_out, phases = transposed ? d->stride : 1;
  const int cin_chunks = ceil_div(d->c_in, KC);
  // the row extent of the image comes from its owner (csrc/conv1d_bf16.hip); the image does not depend on padding,
  // which the packer's geometry check admits only as zero
  pwg_conv1d_desc dz = *d;
  dz.pad_mode = PWG_PAD_ZERO;
  const size_t image_bytes = pwg_conv1d_bf16_packed_weight_bytes(&dz);
  PWG_REQUIRE(image_bytes != 0, PWG_ERR_UNSUPPORTED, "conv1d_stream_bf16: the layer has no bf16 weight image");
  const size_t row_bytes = (size_t)taps * cin_chunks * KC * sizeof(__bf16);
  const int m_pad = (int)(image_bytes / row_bytes);
  PWG_REQUIRE((size_t)m_pad * row_bytes == image_bytes && m_pad % 32 == 0 && m_pad >= m, PWG_ERR_UNSUPPORTED,
              "conv1d_stream_bf16: unexpected bf16 weight image of %zu B for %d rows", image_bytes, m);
  PWG_REQUIRE(hist <= kMaxHist, PWG_ERR_UNSUPPORTED, "conv1d_stream_bf16: history of %d columns does not fit the LDS window",
              hist);
  PWG_REQUIRE(x && w_packed_bf16 && y, PWG_ERR_NULL, "conv1d_stream_bf16: NULL pointer");
  PWG_REQUIRE(hist_out || hist == 0, PWG_ERR_NULL, "conv1d_stream_bf16: hist_out is NULL (the layer keeps %d columns)", hist);
  PWG_REQUIRE(hist == 0 || hist_in != hist_out, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_bf16: hist_in and hist_out must be distinct buffers (other workgroups read the history)");
  PWG_REQUIRE(hist_in || d->pad_mode != PWG_PAD_REFLECT || d->t_in > hist, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_bf16: a reflect-padded stream starts with at least %d columns (got %d)", hist + 1, d->t_in);
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(w_packed_bf16) & 15u) == 0, PWG_ERR_BAD_SHAPE,
              "conv1d_stream_bf16: the weight image must be 16-B aligned");
  const int n = d->t_in;
  const int tn = n <= 16 ? 1 : (n <= 32 ? 2 : 4);
  const int nt = 16 * tn;
  const int col_tiles = ceil_div(n, nt);
  // 32-row blocks only when they still give every CU two workgroups (the order of an element's sum is the same)
  const int tm = (tn == 4 && (long)ceil_div(m, 32) * col_tiles * d->batch >= 2 * kFillWorkgroups) ? 2 : 1;
  const size_t win = (size_t)(nt + hist) * ROW * sizeof(__bf16);
  const size_t red = (size_t)4 * (16 * tm) * (nt + 1) * sizeof(float);  // the partial tiles reuse the window's LDS
  const size_t lds = win > red ? win : red;

  StreamBf16Args a;
  a.x = x;
  a.hist_in = hist ? hist_in : nullptr;
  a.hist_out = hist_out;
  a.w = static_cast<const bf16x8*>(w_packed_bf16);
  a.bias = bias;
  a.add1 = add1;
  a.add2 = add2;
  a.y = y;
  a.c_in = d->c_in;
  a.c_out = d->c_out;
  a.n = n;
  a.t_out = d->t_out;
  a.hist = hist;
  a.taps = taps;
  a.dil = dil;
  a.cin_chunks = cin_chunks;
  a.m = m;
  a.m_pad = m_pad;
  a.phases = phases;
  a.q4 = 4 / taps;
  a.r4 = 4 % taps;
  a.step_o = 256 / (nt + hist);
  a.step_w = 256 % (nt + hist);
  a.pad_mode = d->pad_mode;
  a.pre_act = d->pre_act;
  a.post_act = d->post_act;
  a.pre_slope = d->pre_slope;
  a.post_slope = d->post_slope;
  a.out_mul = d->out_mul;
  a.out_div = d->out_div;

  const dim3 grid(col_tiles, ceil_div(m, 16 * tm), d->batch);
  const double out_elems = (double)d->batch * d->c_out * d->t_out;
  const double flops = 2.0 * (double)d->batch * m * n * taps * d->c_in;
  const double bytes = 4.0 * ((double)d->batch * d->c_in * (n + 2.0 * hist) +
                              out_elems * (1 + (add1 ? 1 : 0) + (add2 ? 1 : 0))) + (double)image_bytes;
  maybe_poison_lds(stream);
  ProfScope prof(stream, "conv1d_stream_bf16_kernel", flops, bytes);
  if (tn == 1)
    launch_tile<1, 1>(a, transposed, grid, lds, stream);
  else if (tn == 2)
    launch_tile<1, 2>(a, transposed, grid, lds, stream);
  else if (tm == 1)
    launch_tile<1, 4>(a, transposed, grid, lds, stream);
  else
    launch_tile<2, 4>(a, transposed, grid, lds, stream);
  PWG_CHECK_LAUNCH("conv1d_stream_bf16");
  return PWG_OK;
}
