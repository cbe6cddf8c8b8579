// elementwise_slots.hip -- the slotted forms of the Parallel WaveGAN look-ahead stream's launches that are no
// convolution and no gated layer (utils.PWGStreamPool): the upsampler stage
// (stretch_conv_stream_kernel<true> of csrc/elementwise.hip), the delay line (delay_line_kernel, there) and the kernel
// that seeds conv_in's history with an utterance's first frame.  Each is the lock-step kernel with one position per
// item, read from the device table of stream_common.h by the conv stream kernels' own row reader.
//
// Item = blockIdx.y (its `channels` rows); the item's elements are dealt over gridDim.x workgroups, so the row is read
// workgroup-uniform.  A running item is the lock-step launch of its rows with its own window -- the stage's fmaf chain,
// j ascending, and the line's copies are those of csrc/elementwise.hip word for word, so the bits are equal --, a fresh
// one reads its state as zeros whatever the buffer holds, a paused one copies its state through (the history rule with
// n = 0), stores zeros and reads none of x.  A table value reaches addressing only through the clamped window [0, t_out]
// and the two flags.  Plain vector stores only.
#include "stream_common.h"

#include <stdint.h>

namespace pwg {

#define GRID_STRIDE(i, n) \
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// Output column t of an item's n * s reads X[floor((t + j - 2 s) / s)], j = 0 .. 2 s, of X = concat(hist (rows, 2), x
// (rows, n)); threads past the outputs write hist_out = the last 2 columns of X (paused: of the history alone).
__global__ __launch_bounds__(256) void stretch_conv_stream_slots_kernel(
    const float* __restrict__ x, const float* __restrict__ hist_in, float* __restrict__ hist_out, const float* __restrict__ w,
    float* __restrict__ y, int channels, int n, int s, int act, float slope, const int32_t* __restrict__ slots, int rate,
    int out_delay) {
  const int b = blockIdx.y;
  const int t_out = n * s;
  const StreamSlotItem item = stream_slot_item(slots, b, rate, out_delay, t_out);
  const long r0 = (long)b * channels;
  const float* __restrict__ hb = item.fresh ? nullptr : hist_in + 2 * r0;
  const long total = (long)channels * t_out;
  GRID_STRIDE(i, total + 2 * channels) {
    if (i < total) {
      const long r = i / t_out;
      const int t = (int)(i - r * t_out);
      if (item.paused || t < item.valid_lo || t >= item.valid_hi) {
        y[r0 * t_out + i] = 0.f;
        continue;
      }
      const float* xr = x + (r0 + r) * n;
      float acc = 0.f;
      for (int j = 0; j <= 2 * s; ++j) {
        const int q = (t + j) / s - 2;  // in [-2, n)
        const float v = q >= 0 ? xr[q] : (hb ? hb[2 * r + 2 + q] : 0.f);
        acc = __builtin_fmaf(w[j], v, acc);
      }
      y[r0 * t_out + i] = apply_act(acc, act, slope);
    } else {
      const long k = i - total;
      const long r = k >> 1;
      const int col = (item.paused ? 0 : n) + (int)(k & 1);  // column of X; the last two are n, n + 1 (paused: n = 0)
      hist_out[2 * r0 + k] = col >= 2 ? x[(r0 + r) * n + col - 2] : (hb ? hb[2 * r + col] : 0.f);
    }
  }
}

// X = concat(line_in (rows, L), x (rows, n)); line_out = the last L columns of X, delayed_out = the first n.  No window:
// the line's output is whatever went in, late; the launches behind it store the zeros.
__global__ __launch_bounds__(256) void delay_line_slots_kernel(const float* __restrict__ x, const float* __restrict__ line_in,
                                                               float* __restrict__ line_out, float* __restrict__ delayed_out,
                                                               int channels, int n, int L, const int32_t* __restrict__ slots) {
  const int b = blockIdx.y;
  const StreamSlotItem item = stream_slot_item(slots, b, 1, 0, n);
  const float* __restrict__ xb = x + (long)b * channels * n;
  const float* __restrict__ lb = item.fresh ? nullptr : line_in + (long)b * channels * L;
  stream_write_history<1>(xb, lb, line_out + (long)b * channels * L, channels, item.paused ? 0 : n, L, false, blockIdx.x,
                          gridDim.x);
  if (delayed_out) {
    float* __restrict__ ob = delayed_out + (long)b * channels * n;
    GRID_STRIDE(i, (long)channels * n) {
      const long r = i / n;
      const int j = (int)(i - r * n);
      ob[i] = item.paused ? 0.f : (j >= L ? xb[r * n + (j - L)] : (lb ? lb[r * L + j] : 0.f));
    }
  }
}

// Seeds the history of a layer that starts from its first column replicated (conv_in): every item whose row says fresh
// and not paused gets column 0 of its x in all `cols` columns of its history; every other item's is left untouched.
__global__ __launch_bounds__(256) void slot_seed_history_kernel(const float* __restrict__ x, float* __restrict__ hist,
                                                                int channels, int n, int cols,
                                                                const int32_t* __restrict__ slots) {
  const int b = blockIdx.y;
  const StreamSlotItem item = stream_slot_item(slots, b, 1, 0, n);
  if (!item.fresh || item.paused) return;
  GRID_STRIDE(i, (long)channels * cols) {
    const long r = i / cols;
    hist[(long)b * channels * cols + i] = x[((long)b * channels + r) * n];
  }
}

// ---- host side: items x rows-per-item instead of rows, the table instead of the window (or of nothing); every state
// input is required -- the start of a stream is an item's, in the table
static int slot_table_check(const char* name, const int32_t* slots, int64_t items, int32_t channels) {
  PWG_REQUIRE(slots != nullptr, PWG_ERR_NULL, "%s: slots is NULL", name);
  PWG_REQUIRE((reinterpret_cast<uintptr_t>(slots) & 3u) == 0, PWG_ERR_BAD_SHAPE, "%s: unaligned slot table", name);
  PWG_REQUIRE(items >= 1 && items <= 65535 && channels >= 1, PWG_ERR_BAD_SHAPE,
              "%s: bad geometry (%lld items of %d channels; 1 .. 65535 items)", name, (long long)items, channels);
  return PWG_OK;
}

// Workgroups per item: enough for `work` elements, all items together within the cap of the 1-D element-wise launches
static dim3 slot_grid(long work, int64_t items) {
  const long cap = 4096 / items > 0 ? 4096 / items : 1;
  long blocks = (work + 255) / 256;
  blocks = blocks > cap ? cap : (blocks < 1 ? 1 : blocks);
  return dim3((unsigned)blocks, (unsigned)items);
}

}  // namespace pwg

using namespace pwg;

extern "C" int pwg_stretch_conv_stream_slots(const float* x, const float* hist_in, float* hist_out, const float* w, float* y,
                                             int64_t items, int32_t channels, int32_t n, int32_t scale, int32_t freq_kernel,
                                             int32_t act, float slope, const int32_t* slots, int32_t rate, int32_t delay,
                                             void* stream) {
  const char* name = "stretch_conv_stream_slots";
  PWG_REQUIRE(x && hist_out && w && y, PWG_ERR_NULL, "%s: NULL pointer", name);
  PWG_REQUIRE(hist_in != nullptr, PWG_ERR_NULL, "%s: hist_in is NULL (the start of a stream is an item's, in the table)",
              name);
  PWG_REQUIRE(hist_in != hist_out, PWG_ERR_BAD_SHAPE,
              "%s: hist_in and hist_out must be distinct buffers (other threads read the history)", name);
  const int rc = slot_table_check(name, slots, items, channels);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(rate >= 1 && delay >= 0, PWG_ERR_BAD_SHAPE, "%s: rate = %d, delay = %d (needs rate >= 1, delay >= 0)", name,
              rate, delay);
  PWG_REQUIRE(freq_kernel == 1, PWG_ERR_UNSUPPORTED,
              "%s: freq_kernel = %d (only 1: taps along the channel axis are not built for streams)", name, freq_kernel);
  PWG_REQUIRE(act == PWG_ACT_NONE || act == PWG_ACT_LEAKY_RELU || act == PWG_ACT_RELU || act == PWG_ACT_TANH,
              PWG_ERR_UNSUPPORTED, "%s: activation %d", name, act);
  PWG_REQUIRE(n > 0 && scale > 0 && (long)n * scale < (1L << 31) && (long)channels * n * scale < (1L << 31),
              PWG_ERR_BAD_SHAPE, "%s: bad geometry (%d channels, n %d, scale %d)", name, channels, n, scale);
  const long per_item = (long)channels * n * scale, total = items * per_item;
  ProfScope prof((hipStream_t)stream, "stretch_conv_stream_slots_kernel", 2.0 * total * (2 * scale + 1),
                 4.0 * ((double)items * channels * (n + 4) + total));
  hipLaunchKernelGGL(stretch_conv_stream_slots_kernel, slot_grid(per_item + 2 * channels, items), dim3(256), 0,
                     (hipStream_t)stream, x, hist_in, hist_out, w, y, channels, n, scale, act, slope, slots, rate, delay);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

extern "C" int pwg_delay_line_slots_forward(const float* x, const float* line_in, float* line_out, float* delayed_out,
                                            int64_t items, int32_t channels, int32_t n, int32_t columns,
                                            const int32_t* slots, void* stream) {
  const char* name = "delay_line_slots_forward";
  PWG_REQUIRE(x && line_out, PWG_ERR_NULL, "%s: NULL pointer", name);
  PWG_REQUIRE(line_in != nullptr, PWG_ERR_NULL, "%s: line_in is NULL (the start of a stream is an item's, in the table)",
              name);
  PWG_REQUIRE(line_in != line_out, PWG_ERR_BAD_SHAPE,
              "%s: line_in and line_out must be distinct buffers (other threads read the line)", name);
  PWG_REQUIRE(delayed_out != x, PWG_ERR_BAD_SHAPE, "%s: delayed_out must not alias x", name);
  const int rc = slot_table_check(name, slots, items, channels);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(n > 0 && columns > 0 && (long)channels * columns < (1L << 31) && (long)channels * n < (1L << 31),
              PWG_ERR_BAD_SHAPE, "%s: bad geometry (%d channels, n %d, %d columns; int element indices per item)", name,
              channels, n, columns);
  const double rows = (double)items * channels;
  ProfScope prof((hipStream_t)stream, "delay_line_slots_kernel", 0.0,
                 4.0 * rows * (2.0 * columns + (delayed_out ? 2.0 * n : (double)n)));
  hipLaunchKernelGGL(delay_line_slots_kernel, slot_grid((long)channels * (columns > n ? columns : n), items), dim3(256), 0,
                     (hipStream_t)stream, x, line_in, line_out, delayed_out, channels, n, columns, slots);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

extern "C" int pwg_slot_seed_history(const float* x, float* hist, int64_t items, int32_t channels, int32_t n, int32_t columns,
                                     const int32_t* slots, void* stream) {
  const char* name = "slot_seed_history";
  PWG_REQUIRE(x != nullptr, PWG_ERR_NULL, "%s: x is NULL", name);
  PWG_REQUIRE(hist != nullptr, PWG_ERR_NULL, "%s: hist is NULL (the history the fresh items' first column goes to)", name);
  const int rc = slot_table_check(name, slots, items, channels);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(n > 0 && columns > 0 && (long)channels * columns < (1L << 31) && (long)channels * n < (1L << 31),
              PWG_ERR_BAD_SHAPE, "%s: bad geometry (%d channels, n %d, %d columns; int element indices per item)", name,
              channels, n, columns);
  ProfScope prof((hipStream_t)stream, "slot_seed_history_kernel", 0.0, 4.0 * (double)items * channels * (columns + 1.0));
  hipLaunchKernelGGL(slot_seed_history_kernel, slot_grid((long)channels * columns, items), dim3(256), 0, (hipStream_t)stream,
                     x, hist, channels, n, columns, slots);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}
