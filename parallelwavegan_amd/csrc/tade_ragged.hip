// tade_ragged.hip -- the ragged forms of StyleMelGAN's element-wise stages (layers/tade_res_block.py):
// instance norm, nearest upsampling (+ addend), the TADE modulation and the softmax / sigmoid x tanh gate over a batch
// whose items have their own lengths -- the batched form of the decode loop of bin/decode.py:214-243.  Forward only,
// fp32.
//
// Every kernel reads the device table `frames` (batch,): item b ends at e = min(frames[b] * rate, t), t stays the row
// stride.  Nothing at or past e is read, every column in [e, t) is stored as +0.0f, and the columns below e are the
// plain kernel of csrc/elementwise.hip on the item alone, a contiguous (1, C, e) tensor, bit for bit: the value
// expressions are that file's word for word (same compiler flags, so the same FMA contraction), and the one reduction,
// the instance norm's, adds in the same order -- thread-strided partial sums over [0, e), then block_sum_256.
// A table value reaches addressing only through the clamped e.  Plain vector stores only.
#include "common.h"

#include <stdint.h>

namespace pwg {

// (csrc/elementwise.hip's, word for word: the order of the additions is part of the contract above)
__device__ __forceinline__ float block_sum_256(float s, float* red) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const float t = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return t;
}

// Item b's end in columns of a row of t columns at `rate` columns per frame.
__device__ __forceinline__ long ragged_end(const int32_t* frames, int b, int rate, long t) {
  const long e = (long)frames[b] * rate;
  return e < 0 ? 0 : e < t ? e : t;
}

// InstanceNorm1d (affine = False, biased variance, eps) over [0, e): one workgroup per (b, c) row.  e == 0 stores a
// row of zeros and divides by nothing.
__global__ __launch_bounds__(256) void instance_norm_ragged_kernel(const float* x, float* y, const int32_t* frames,
                                                                   int channels, int t, int rate, float eps) {
  __shared__ float red[4];
  const int e = (int)ragged_end(frames, blockIdx.x / channels, rate, t);
  const float* xr = x + (long)blockIdx.x * t;
  float* yr = y + (long)blockIdx.x * t;
  if (e > 0) {  // (workgroup-uniform)
    float s = 0.f;
    for (int i = threadIdx.x; i < e; i += 256) s += xr[i];
    const float mu = block_sum_256(s, red) / e;
    __syncthreads();
    float v = 0.f;
    for (int i = threadIdx.x; i < e; i += 256) {
      const float d = xr[i] - mu;
      v += d * d;
    }
    const float rs = rsqrtf(block_sum_256(v, red) / e + eps);
    for (int i = threadIdx.x; i < e; i += 256) yr[i] = (xr[i] - mu) * rs;
  }
  for (int i = e + threadIdx.x; i < t; i += 256) yr[i] = 0.f;
}

// The two row-wise kernels: a workgroup owns kRaggedCols columns of one (b, c) row, blockIdx = (column tile, c, b);
// a thread's columns are 256 apart (coalesced).  A tile at or past e stores zeros and reads nothing.
constexpr int kRaggedCols = 1024;

// y[b][c][t] = x[b][c][t / s] (+ add[b][c][t]) below e
__global__ __launch_bounds__(256) void upsample_nearest_ragged_kernel(const float* x, const float* add, float* y,
                                                                      const int32_t* frames, int channels, int t_in, int s,
                                                                      int rate_out) {
  const int t_out = t_in * s;
  const int e = (int)ragged_end(frames, blockIdx.z, rate_out, t_out);
  const long r = (long)blockIdx.z * channels + blockIdx.y;
  const long i0 = r * t_out;
  for (int k = 0; k < kRaggedCols / 256; ++k) {
    const int t = blockIdx.x * kRaggedCols + k * 256 + threadIdx.x;
    if (t >= t_out) break;
    float v = 0.f;
    if (t < e) {
      v = x[r * t_in + t / s];
      if (add) v += add[i0 + t];
    }
    y[i0 + t] = v;
  }
}

// TADE modulation: y[b][c][t] = cg[b][c][t] * xn[b][c][t / s] + cg[b][C + c][t] below e
__global__ __launch_bounds__(256) void tade_modulate_ragged_kernel(const float* xn, const float* cg, float* y,
                                                                   const int32_t* frames, int channels, int t_in, int s,
                                                                   int rate_out) {
  const int t_out = t_in * s;
  const int e = (int)ragged_end(frames, blockIdx.z, rate_out, t_out);
  const long b = blockIdx.z;
  const int c = blockIdx.y;
  const long r = b * channels + c;
  for (int k = 0; k < kRaggedCols / 256; ++k) {
    const int t = blockIdx.x * kRaggedCols + k * 256 + threadIdx.x;
    if (t >= t_out) break;
    float v = 0.f;
    if (t < e) {
      const long g1 = ((b * 2 * channels + c) * (long)t_out) + t;
      v = cg[g1] * xn[r * t_in + t / s] + cg[g1 + (long)channels * t_out];
    }
    y[r * t_out + t] = v;
  }
}

// Gated activation z (B, 2C, T) -> y (B, C, T) below e; one thread per (b, t) column, coalesced along t, blockIdx =
// (column tile, b).  A column at or past e stores its C zeros and reads nothing.
__global__ __launch_bounds__(256) void softmax_gate_ragged_kernel(const float* z, float* y, const int32_t* frames,
                                                                  int channels, long t, int rate, int use_softmax) {
  const long b = blockIdx.y;
  const long e = ragged_end(frames, blockIdx.y, rate, t);
  const long tt = (long)blockIdx.x * 256 + threadIdx.x;
  if (tt >= t) return;
  const float* za = z + (b * 2 * channels) * t + tt;
  const float* zb = za + (long)channels * t;
  float* yo = y + (b * channels) * t + tt;
  if (tt >= e) {
    for (int c = 0; c < channels; ++c) yo[(long)c * t] = 0.f;
  } else if (use_softmax) {
    float mx = -INFINITY;
    for (int c = 0; c < channels; ++c) mx = fmaxf(mx, za[(long)c * t]);
    float den = 0.f;
    for (int c = 0; c < channels; ++c) den += expf(za[(long)c * t] - mx);
    for (int c = 0; c < channels; ++c) yo[(long)c * t] = expf(za[(long)c * t] - mx) / den * tanhf(zb[(long)c * t]);
  } else {
    for (int c = 0; c < channels; ++c)
      yo[(long)c * t] = 1.f / (1.f + expf(-za[(long)c * t])) * tanhf(zb[(long)c * t]);
  }
}

// ---- host side: pwg_zero_tail's refusals (a message, nothing launched)
static int ragged_check(const char* name, const void* a, const void* b, const void* opt, const void* y,
                        const int32_t* frames, int32_t batch, int32_t channels, int32_t rate) {
  PWG_REQUIRE(a && b && y && frames, PWG_ERR_NULL, "%s: NULL pointer", name);
  PWG_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(opt) |
                reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(frames)) & 3u) == 0,
              PWG_ERR_BAD_SHAPE, "%s: the tensors and the frames table must be 4-B aligned", name);
  PWG_REQUIRE(rate > 0, PWG_ERR_BAD_SHAPE, "%s: rate = %d (columns per frame, >= 1)", name, rate);
  PWG_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 1 && channels <= 65535, PWG_ERR_BAD_SHAPE,
              "%s: bad shape (batch %d, channels %d; 1 .. 65535 each)", name, batch, channels);
  return PWG_OK;
}

// the geometry of the two kernels that upsample: t_out = t_in * scale columns per row, int element indices within a row
static int ragged_upsample_check(const char* name, int32_t t_in, int32_t scale) {
  PWG_REQUIRE(t_in >= 1 && scale >= 1 && (int64_t)t_in * scale + kRaggedCols < (1LL << 31), PWG_ERR_BAD_SHAPE,
              "%s: bad shape (t_in %d, scale %d)", name, t_in, scale);
  return PWG_OK;
}

}  // namespace pwg

using namespace pwg;

extern "C" int pwg_instance_norm_ragged(const float* x, float* y, const int32_t* frames, int32_t batch, int32_t channels,
                                        int32_t t, int32_t rate, float eps, void* stream) {
  const char* name = "instance_norm_ragged";
  const int rc = ragged_check(name, x, x, nullptr, y, frames, batch, channels, rate);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(t >= 1 && t < 0x7fffffff - 256, PWG_ERR_BAD_SHAPE, "%s: bad shape (t %d)", name, t);
  const long rows = (long)batch * channels;
  ProfScope prof((hipStream_t)stream, "instance_norm_ragged_kernel", 0, 12.0 * rows * t);
  hipLaunchKernelGGL(instance_norm_ragged_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, y, frames,
                     channels, t, rate, eps);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

extern "C" int pwg_upsample_nearest_ragged(const float* x, const float* add, float* y, const int32_t* frames, int32_t batch,
                                           int32_t channels, int32_t t_in, int32_t scale, int32_t rate_out, void* stream) {
  const char* name = "upsample_nearest_ragged";
  int rc = ragged_check(name, x, x, add, y, frames, batch, channels, rate_out);
  if (rc == PWG_OK) rc = ragged_upsample_check(name, t_in, scale);
  if (rc != PWG_OK) return rc;
  const int t_out = t_in * scale;
  const double n = (double)batch * channels * t_out;
  ProfScope prof((hipStream_t)stream, "upsample_nearest_ragged_kernel", 0, 4.0 * n * (add ? 3 : 2));
  hipLaunchKernelGGL(upsample_nearest_ragged_kernel, dim3((t_out + kRaggedCols - 1) / kRaggedCols, channels, batch),
                     dim3(256), 0, (hipStream_t)stream, x, add, y, frames, channels, t_in, scale, rate_out);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

extern "C" int pwg_tade_modulate_ragged(const float* xn, const float* cg, float* y, const int32_t* frames, int32_t batch,
                                        int32_t channels, int32_t t_in, int32_t scale, int32_t rate_out, void* stream) {
  const char* name = "tade_modulate_ragged";
  int rc = ragged_check(name, xn, cg, nullptr, y, frames, batch, channels, rate_out);
  if (rc == PWG_OK) rc = ragged_upsample_check(name, t_in, scale);
  if (rc != PWG_OK) return rc;
  const int t_out = t_in * scale;
  const double n = (double)batch * channels * t_out;
  ProfScope prof((hipStream_t)stream, "tade_modulate_ragged_kernel", 2.0 * n, 16.0 * n);
  hipLaunchKernelGGL(tade_modulate_ragged_kernel, dim3((t_out + kRaggedCols - 1) / kRaggedCols, channels, batch),
                     dim3(256), 0, (hipStream_t)stream, xn, cg, y, frames, channels, t_in, scale, rate_out);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

extern "C" int pwg_softmax_gate_ragged(const float* z, float* y, const int32_t* frames, int32_t batch, int32_t channels,
                                       int64_t t, int32_t rate, int32_t use_softmax, void* stream) {
  const char* name = "softmax_gate_ragged";
  const int rc = ragged_check(name, z, z, nullptr, y, frames, batch, channels, rate);
  if (rc != PWG_OK) return rc;
  const int64_t col_tiles = t > 0 ? (t + 255) / 256 : 0;
  PWG_REQUIRE(t >= 1 && col_tiles <= 0x7fffffff, PWG_ERR_BAD_SHAPE, "%s: bad shape (t %lld)", name, (long long)t);
  ProfScope prof((hipStream_t)stream, "softmax_gate_ragged_kernel", 0, 12.0 * batch * channels * (double)t);
  hipLaunchKernelGGL(softmax_gate_ragged_kernel, dim3((unsigned)col_tiles, batch), dim3(256), 0, (hipStream_t)stream, z, y,
                     frames, channels, (long)t, rate, use_softmax);
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}
