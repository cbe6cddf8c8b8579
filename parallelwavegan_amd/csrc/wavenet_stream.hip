// wavenet_stream.hip -- stateful (streaming) form of the causal gated residual layer of the Parallel WaveGAN generator:
// ONE launch per layer and chunk, fp32 on the exact-fp32 MFMA.
//
// A causal layer (layers/residual_block.py:74-76,102-140 of the reference: the dilated convolution is padded (k-1)*d on
// both sides and the future part of its output dropped, i.e. left-only padding) reads x at n - 2d, n - d and n, so from
// the past it needs only the last H = (k-1)*d = 2d columns of its raw input.  One launch takes the chunk x (B, 64, n),
// the aux features c (B, 80, n), the running skip sum and the history hist_in (B, 64, H), computes
//
//     X      = concat(hist_in, x)                                   (hist_in == NULL: start of stream, zeros)
//     z      = sum_tap W_dil[tap] X[n + (tap - 2) d] + b_dil + W_aux c      (128 rows; K = 3 * 64 + 80 = 272)
//     g      = tanh(z[:64]) * sigmoid(z[64:])
//     skips' = (W_skip g + b_skip + skips) * skip_mul
//     x'     = (W_out g + b_out + x) * out_mul
//
// and writes hist_out = the last H columns of X (raw), also when n < H (part of hist_in carries over).  hist_in and
// hist_out are distinct buffers: other workgroups of the launch read hist_in while this one writes hist_out.
//
// The kernel is wavenet_layer_kernel<80> of csrc/wavenet.hip (a 4-wave workgroup per 64 columns of one item, a 272 x 64
// fp32 operand tile in LDS, v_mfma_f32_32x32x2_f32 with the A operands streamed from the SAME pre-swizzled image --
// its row order tap0, tap1, tap2, aux does not depend on causality -- gate_fast, two workgroups per CU) with three
// differences:
//   * two-source tap windows.  Window `tap` starts at chunk-relative column f0 = n0 + (tap - 2) d.  Columns < 0 come
//     from hist_in[H + f] (zeros at start of stream), columns >= 0 from x.  A window that lies wholly inside one
//     source keeps the 16-B LDS-DMA pass (16 B per lane at 4-B aligned addresses, all lanes in range: the form the
//     whole-utterance kernel uses); a window that straddles the boundary, leaves the data, or is all start-of-stream
//     zeros is staged per sample through registers with range checks (plain loads, plain LDS stores).
//   * the residual x is the LAST tap window (rows 128..191), so the epilogue's wave-private transposition scratch
//     cannot sit in rows 128.. as in the whole-utterance kernel.  It sits in the aux rows 192..271, which every wave
//     has finished reading when phase 1 ends (there is a workgroup barrier between phase 1 and the first scratch
//     write); the 80 rows hold one 32 x 36 tile per wave, so the skip tile and the out tile are transposed one after the
//     other through the same scratch.  Nobody writes rows 128..191.
//   * the history write: the item's 64 * H elements of hist_out are dealt over the item's column workgroups, at the end
//     of the same launch.
//
// Sum order.  An output element is sum over K in the fixed order of the image -- tap 0, tap 1, tap 2, aux; inside a tap
// channel ascending, two channels per MFMA step -- accumulated in one MFMA accumulator register, then the K = 64
// contraction over g in channel order, then + bias, + skips / + x, * scale.  One workgroup owns a column over the whole
// reduction: no split across workgroups or waves, no workspace, no atomics.  That order depends on the layer alone --
// not on n, the batch, the chunk's position in the stream, or the column's place in the tile (a column is one MFMA
// lane position; its accumulator sees the same operand sequence wherever it sits, a padded or history operand is the
// same value through either staging path) -- so any partition of a stream gives bit-identical results.  DESIGN.md s11.3.
//
// The delayed form (pwg_wavenet_stream_delayed_*) is the NON-causal layer of a stream with a fixed
// look-ahead: the same kernel body (wavenet_stream_kernel<WnDelayedArgs>) on a time axis shifted by d.  The taps
// x~[n - 2d], x~[n - d], x~[n] are the causal ones, the output is d columns later than the input, and
//   * the residual is the MIDDLE tap window (rows 64..127 = x~[n - d]), which nobody writes either;
//   * the aux window starts at n0 - c_delay and is staged from two sources by the rule of the tap windows: columns < 0
//     from the conditioning line c_line[c_cols + f] (zeros when NULL), columns >= 0 from the chunk c; the 16-B LDS-DMA
//     pass when the window lies in one source, per sample otherwise;
//   * the skip addend of output column j is concat(skip_line_in, skips)[j] (a delay of d columns, read in the epilogue
//     as the delayed conv kernel reads its addends), and skip_line_out = the last d columns of that concatenation,
//     dealt over the workgroups as the history is;
//   * outside [valid_lo, valid_hi) 0.0f is STORED to x_out and skips_out: the next layer's zero padding.
// Sum order of the delayed form: that of the causal form, word for word -- the image's K order in one accumulator, the
// K = 64 contraction, + bias, + the skip addend / + the residual, * scale.  It depends on the layer alone: not on n, the
// batch, the chunk's position, c_delay or its alignment, or which staging path a window took (an operand is the same
// fp32 value through the DMA pass and through registers; the addend is the same value from the line and from the chunk).
//
// The slotted form (pwg_wavenet_stream_slots_forward) is the delayed form with one position per item
// (wavenet_stream_kernel<WnSlotsArgs>): every workgroup reads its item's row of the device table of stream_common.h and
// derives the item's valid window itself.  A running item is from there on the delayed form, the same code and the same
// bits; a fresh item reads hist_in, c_line and skip_line_in as NULL; a paused item copies its state through, stores zeros
// and returns in front of every barrier.
#include "stream_common.h"
#include "wavenet_gate.h"
#include "wavenet_stream.h"

#include <stdint.h>

#include <type_traits>

namespace pwg {
namespace {

constexpr int WS_AUX = 80;
constexpr int WS_ROWS = WN_K * WN_R + WS_AUX;  // 272 operand rows

struct WnStreamArgs {
  const float* x;        // (B, 64, n)
  const float* c;        // (B, 80, n)
  const float* skips;    // (B, 64, n) or NULL
  const float* hist_in;  // (B, 64, H) or NULL (start of stream)
  float* hist_out;       // (B, 64, H)
  const float* w1;       // image [ROWS / 8][4 row tiles][64 lanes][4]
  const float* w2;       // image [8][4 row tiles][64 lanes][4]
  const float* b_dil;    // (128), may be NULL
  const float* b_skip;   // (64), may be NULL
  const float* b_out;    // (64), may be NULL
  float* x_out;          // (B, 64, n)
  float* skips_out;      // (B, 64, n) (may alias skips)
  int n, dil;
  float out_mul, skip_mul;
  int vec_ok;  // x_out / skips / skips_out are 16-B aligned
};

// What the delayed form adds (file header).  skips_out must not alias skips: tiles read their neighbours' skip columns.
struct WnDelayedArgs : WnStreamArgs {
  const float* c_line;        // (B, 80, c_cols) or NULL (zeros): the conditioning columns before this chunk
  const float* skip_line_in;  // (B, 64, d) or NULL (zeros)
  float* skip_line_out;       // (B, 64, d); unused without skips
  int c_cols, c_delay;        // 0 <= c_delay <= c_cols
  int valid_lo, valid_hi;     // output columns (chunk-relative)
};

// The slotted form (pwg_wavenet_stream_slots_forward): the delayed form with one position per item,
// read from the device table of stream_common.h.  A running item IS a delayed launch with its own window; a fresh one
// reads hist_in, c_line and skip_line_in as NULL; a paused one copies its state through (the history rule with n = 0),
// stores zeros and returns in front of every barrier, reading none of x, c, skips.
struct WnSlotsArgs : WnStreamArgs {
  const float* c_line;        // (B, 80, c_cols) or NULL (zeros)
  const float* skip_line_in;  // (B, 64, d); required with skips
  float* skip_line_out;       // (B, 64, d); unused without skips
  int c_cols, c_delay;        // 0 <= c_delay <= c_cols
  const int32_t* slots;       // (B, kStreamSlotInts)
  int rate, out_delay;        // output columns per frame, delay of the output
};

template <class ARGS>
__global__ __launch_bounds__(256, 2) void wavenet_stream_kernel(ARGS a) {
  constexpr bool SLOTTED = std::is_same<ARGS, WnSlotsArgs>::value;
  constexpr bool DELAYED = std::is_same<ARGS, WnDelayedArgs>::value || SLOTTED;
  constexpr int NQ1 = WS_ROWS / 8;  // 16-B weight records per lane and row tile in phase 1 (4 k-steps each)
  constexpr int NQ2 = WN_R / 8;     // phase 2: K = 64 rows of g
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [ROWS][64]; rows 0..63 are overwritten by g
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = wave >> 1, cn = wave & 1;
  const int l31 = lane & 31, lhi = lane >> 5;
  const int b = blockIdx.y;
  const int n0 = blockIdx.x * WN_COLS;
  const int n = a.n;
  const int H = 2 * a.dil;
  const float* __restrict__ xb = a.x + (long)b * WN_R * n;
  const float* __restrict__ cb = a.c + (long)b * WS_AUX * n;
  // SLOTTED: what this item's table row resolves to -- fresh, paused and its own window
  [[maybe_unused]] StreamSlotItem item{};
  bool fresh = false;
  if constexpr (SLOTTED) {
    item = stream_slot_item(a.slots, b, a.rate, a.out_delay, n);
    fresh = item.fresh;
  }
  const float* __restrict__ hb = a.hist_in && !fresh ? a.hist_in + (long)b * WN_R * H : nullptr;
  // the aux window's past (delayed form): the conditioning line, c_cols columns; the window starts c_delay columns early
  const float* __restrict__ lb = nullptr;
  // ... its skip line (all items'; NULL: zeros) and its valid window: the launch's, or the item's
  [[maybe_unused]] const float* __restrict__ sli = nullptr;
  [[maybe_unused]] int valid_lo = 0, valid_hi = 0;
  int L = 0, c_delay = 0;
  if constexpr (DELAYED) {
    L = a.c_cols;
    c_delay = a.c_delay;
    lb = a.c_line && !fresh ? a.c_line + (long)b * WS_AUX * L : nullptr;
    sli = fresh ? nullptr : a.skip_line_in;
    if constexpr (SLOTTED) {
      valid_lo = item.valid_lo;
      valid_hi = item.valid_hi;
    } else {
      valid_lo = a.valid_lo;
      valid_hi = a.valid_hi;
    }
  }
  if constexpr (SLOTTED) {
    if (item.paused) {  // (workgroup-uniform) state out = state in, zeros for both output tiles; in front of every barrier
      stream_write_history<4>(xb, hb, a.hist_out + (long)b * WN_R * H, WN_R, 0, H, false, blockIdx.x, gridDim.x);
      if (a.skips)
        stream_write_history<4>(a.skips + (long)b * WN_S * n, sli ? sli + (long)b * WN_S * a.dil : nullptr,
                                a.skip_line_out + (long)b * WN_S * a.dil, WN_S, 0, a.dil, false, blockIdx.x, gridDim.x);
      for (int e = tid; e < WN_R * WN_COLS; e += 256) {
        const int row = e / WN_COLS, j = n0 + (e - row * WN_COLS);
        if (j >= n) continue;
        const long o = ((long)b * WN_R + row) * n + j;
        a.x_out[o] = 0.f;
        a.skips_out[o] = 0.f;
      }
      return;
    }
  }

  // ---- stage the operand tile: window `tap` of X starts at chunk-relative column n0 + (tap - 2) d, the aux window at
  // n0 - c_delay
  {
    __amdgpu_buffer_rsrc_t x_rs = uniform_buffer_rsrc(xb, (unsigned)(WN_R * n) * 4u);
    __amdgpu_buffer_rsrc_t c_rs = uniform_buffer_rsrc(cb, (unsigned)(WS_AUX * n) * 4u);
    __amdgpu_buffer_rsrc_t h_rs = uniform_buffer_rsrc(hb ? hb : xb, hb ? (unsigned)(WN_R * H) * 4u : 0u);
    __amdgpu_buffer_rsrc_t l_rs = uniform_buffer_rsrc(lb ? lb : xb, lb ? (unsigned)(WS_AUX * L) * 4u : 0u);
    for (int q = wave; q < WS_ROWS / 4; q += 4) {  // 4 rows (1 KiB of LDS) per wave instruction
      const int r0 = 4 * q;
      const bool is_x = r0 < WN_K * WN_R;
      const int tap = r0 / WN_R;
      const int f0 = is_x ? n0 + (tap - 2) * a.dil : n0 - c_delay;  // first column of the window (< 0: the past)
      const int ch0 = is_x ? r0 - tap * WN_R : r0 - WN_K * WN_R;
      const float* __restrict__ pb = is_x ? hb : lb;  // the window's past source and its columns
      const int P = is_x ? H : L;
      const int in_chunk = __builtin_amdgcn_readfirstlane((f0 >= 0 && f0 + WN_COLS <= n) ? 1 : 0);
      const int in_past = __builtin_amdgcn_readfirstlane((pb != nullptr && f0 + WN_COLS <= 0) ? 1 : 0);
      if (in_chunk) {
        const unsigned off = (unsigned)((ch0 + (lane >> 4)) * n + f0 + 4 * (lane & 15)) * 4u;
        if (is_x) __builtin_amdgcn_raw_ptr_buffer_load_lds(x_rs, (lds_ptr_t)(tile + r0 * WN_COLS), 16, off, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(c_rs, (lds_ptr_t)(tile + r0 * WN_COLS), 16, off, 0, 0, 0);
      } else if (in_past) {
        // (f0 >= -P: P + f0 >= 0, and P + f0 + 64 <= P)
        const unsigned off = (unsigned)((ch0 + (lane >> 4)) * P + P + f0 + 4 * (lane & 15)) * 4u;
        if (is_x) __builtin_amdgcn_raw_ptr_buffer_load_lds(h_rs, (lds_ptr_t)(tile + r0 * WN_COLS), 16, off, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(l_rs, (lds_ptr_t)(tile + r0 * WN_COLS), 16, off, 0, 0, 0);
      } else {
        // the window straddles past and chunk, leaves the chunk on the right, or is start-of-stream padding:
        // per sample, range-checked, zeros outside
        const int f = f0 + lane;
        const float* __restrict__ sb = is_x ? xb : cb;
        float v[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          v[rr] = 0.f;
          if (f < 0) {
            if (pb) v[rr] = pb[(long)(ch0 + rr) * P + (P + f)];
          } else if (f < n) {
            v[rr] = sb[(long)(ch0 + rr) * n + f];
          }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) tile[(r0 + rr) * WN_COLS + lane] = v[rr];
      }
    }
  }

  // biases of this lane's accumulator rows: row = 8 * (r >> 2) + 4 * lhi + (r & 3) of the wave's 32-row block
  f32x16 bt, bs, bsk, bo;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = h * 32 + 8 * (r >> 2) + 4 * lhi + (r & 3);
    bt[r] = a.b_dil ? a.b_dil[row] : 0.f;
    bs[r] = a.b_dil ? a.b_dil[WN_R + row] : 0.f;
    bsk[r] = a.b_skip ? a.b_skip[row] : 0.f;
    bo[r] = a.b_out ? a.b_out[row] : 0.f;
  }

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // ---- phase 1: z rows [32 h, +32) (tanh half) and [64 + 32 h, +32) (sigmoid half) over K = ROWS
  {
    const float4* wa = reinterpret_cast<const float4*>(a.w1) + (h * 64 + lane);        // row tile h
    const float4* wb = reinterpret_cast<const float4*>(a.w1) + ((2 + h) * 64 + lane);  // row tile 2 + h
    float4 A[3][2];
    A[0][0] = wa[0];
    A[0][1] = wb[0];
    A[1][0] = wa[4 * 64];
    A[1][1] = wb[4 * 64];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the DMA pass (and its first weight records)
    __syncthreads();
    const float* bl = tile + lhi * WN_COLS + cn * 32 + l31;  // + (8 q + 2 j) * 64
    float B0[4], B1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) B0[j] = bl[(2 * j) * WN_COLS];
#pragma unroll
    for (int q = 0; q < NQ1; ++q) {
      const int qn = q + 2 < NQ1 ? q + 2 : NQ1 - 1;
      A[(q + 2) % 3][0] = wa[(long)qn * 4 * 64];
      A[(q + 2) % 3][1] = wb[(long)qn * 4 * 64];
      float(&Bc)[4] = (q & 1) ? B1 : B0;
      float(&Bn)[4] = (q & 1) ? B0 : B1;
      const int q1 = q + 1 < NQ1 ? q + 1 : q;
#pragma unroll
      for (int j = 0; j < 4; ++j) Bn[j] = bl[(8 * q1 + 2 * j) * WN_COLS];
      __builtin_amdgcn_sched_barrier(0);
      const float4 a0 = A[q % 3][0], a1 = A[q % 3][1];
      const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[j], Bc[j], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[j], Bc[j], acc[1], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- gate in registers; g to LDS rows 0..63 (every wave is done with the first window and with the aux rows)
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rl = 8 * (r >> 2) + 4 * lhi + (r & 3);
    tile[(h * 32 + rl) * WN_COLS + cn * 32 + l31] = gate_fast(acc[0][r] + bt[r], acc[1][r] + bs[r]);
    acc[0][r] = 0.f;
    acc[1][r] = 0.f;
  }
  __syncthreads();

  // ---- phase 2: skip rows [32 h, +32) and out rows [32 h, +32) over K = 64 rows of g
  {
    const float4* wa = reinterpret_cast<const float4*>(a.w2) + (h * 64 + lane);
    const float4* wb = reinterpret_cast<const float4*>(a.w2) + ((2 + h) * 64 + lane);
    const float* bl = tile + lhi * WN_COLS + cn * 32 + l31;
    float4 A0[NQ2], A1[NQ2];
#pragma unroll
    for (int q = 0; q < NQ2; ++q) {
      A0[q] = wa[q * 4 * 64];
      A1[q] = wb[q * 4 * 64];
    }
#pragma unroll
    for (int q = 0; q < NQ2; ++q) {
      float Bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) Bv[j] = bl[(8 * q + 2 * j) * WN_COLS];
      const float av0[4] = {A0[q].x, A0[q].y, A0[q].z, A0[q].w}, av1[4] = {A1[q].x, A1[q].y, A1[q].z, A1[q].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[j], Bv[j], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[j], Bv[j], acc[1], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: D layout col = lane & 31 (time), rows as above.  Each wave transposes its two 32 x 32 result tiles,
  // one after the other, through a private 32 x 36 scratch in the aux rows (dead since phase 1) so that a lane owns 4
  // consecutive samples of a row: 16-B loads of the skip sum, 16-B stores of both outputs.  The residual comes from the
  // last tap window (rows 128..191 = x[n]; the delayed form: from the middle one, rows 64..127 = x~[n - d]), which no
  // wave writes.  (Wave-private scratch: no workgroup barrier, the wave's own LDS accesses are ordered.)
  constexpr int RES_TAP = DELAYED ? 1 : 2;
  float* scr = tile + (WN_K * WN_R) * WN_COLS + wave * (32 * 36);
  const int trow = lane >> 3, tcol = (lane & 7) * 4;
  const int nq = n0 + cn * 32 + tcol;
  const bool vec = ((n & 3) == 0) && a.vec_ok;
  const long ob = (long)b * WN_R * n + nq;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = 8 * (r >> 2) + 4 * lhi + (r & 3);
      if (pass == 0) {
        scr[rl * 36 + l31] = acc[0][r] + bsk[r];
      } else {
        const float xc = tile[(RES_TAP * WN_R + h * 32 + rl) * WN_COLS + cn * 32 + l31];
        scr[rl * 36 + l31] = (acc[1][r] + bo[r] + xc) * a.out_mul;
      }
    }
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int rl = ps * 8 + trow;
      const long o = ob + (long)(h * 32 + rl) * n;
      float4 v = *reinterpret_cast<const float4*>(scr + rl * 36 + tcol);
      if constexpr (DELAYED) {
        // per element: the skip addend through its delay line, then zeros outside the valid window; the same values
        // whether the store below is a float4 or four floats
        float e4[4] = {v.x, v.y, v.z, v.w};
        float* __restrict__ out = pass == 0 ? a.skips_out : a.x_out;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = nq + e;
          if (j >= n) continue;
          if (pass == 0) {
            if (a.skips)
              e4[e] += stream_delayed_addend(a.skips, sli, a.dil, (size_t)b * WN_S + h * 32 + rl, n, j);
            if (a.skip_mul != 1.0f) e4[e] *= a.skip_mul;
          }
          if (j < valid_lo || j >= valid_hi) e4[e] = 0.f;
          if (!vec) out[o + e] = e4[e];
        }
        if (vec && nq < n) *reinterpret_cast<float4*>(out + o) = make_float4(e4[0], e4[1], e4[2], e4[3]);
      } else if (vec) {
        if (nq < n) {  // (n % 4 == 0: a float4 is inside the chunk or outside it)
          if (pass == 0) {
            if (a.skips) {
              const float4 k = *reinterpret_cast<const float4*>(a.skips + o);
              v.x += k.x; v.y += k.y; v.z += k.z; v.w += k.w;
            }
            if (a.skip_mul != 1.0f) { v.x *= a.skip_mul; v.y *= a.skip_mul; v.z *= a.skip_mul; v.w *= a.skip_mul; }
            *reinterpret_cast<float4*>(a.skips_out + o) = v;
          } else {
            *reinterpret_cast<float4*>(a.x_out + o) = v;
          }
        }
      } else {
        const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (nq + e < n) {
            if (pass == 0) {
              float s = e4[e] + (a.skips ? a.skips[o + e] : 0.f);
              if (a.skip_mul != 1.0f) s *= a.skip_mul;
              a.skips_out[o + e] = s;
            } else {
              a.x_out[o + e] = e4[e];
            }
          }
        }
      }
    }
  }

  // ---- hist_out = last H columns of concat(hist_in, x), raw (start of stream: zeros)
  stream_write_history<4>(xb, hb, a.hist_out + (long)b * WN_R * H, WN_R, n, H, false, blockIdx.x, gridDim.x);
  // ---- delayed form: skip_line_out = last d columns of concat(skip_line_in, skips), raw
  if constexpr (DELAYED) {
    if (a.skips)
      stream_write_history<4>(a.skips + (long)b * WN_S * n, sli ? sli + (long)b * WN_S * a.dil : nullptr,
                              a.skip_line_out + (long)b * WN_S * a.dil, WN_S, n, a.dil, false, blockIdx.x, gridDim.x);
  }
}

}  // namespace

static bool aligned(const void* p, unsigned m) { return (reinterpret_cast<uintptr_t>(p) & m) == 0; }

// ---- the host rules of both precisions (wavenet_stream.h)
int wavenet_stream_geometry(const pwg_wavenet_desc* d, bool delayed) {
  PWG_REQUIRE(d != nullptr, PWG_ERR_NULL, "wavenet_stream: NULL descriptor");
  if (delayed)
    PWG_REQUIRE(!d->causal, PWG_ERR_UNSUPPORTED,
                "wavenet_stream_delayed: a causal layer streams without look-ahead (pwg_wavenet_stream_forward)");
  else
    PWG_REQUIRE(d->causal, PWG_ERR_UNSUPPORTED,
                "wavenet_stream: not a causal layer (a stream keeps only past columns; non-causal layers look ahead)");
  PWG_REQUIRE(d->kernel == WN_K, PWG_ERR_UNSUPPORTED, "wavenet_stream: kernel = %d (only kernel 3)", d->kernel);
  PWG_REQUIRE(d->residual_channels == WN_R && d->gate_channels == WN_G && d->skip_channels == WN_S, PWG_ERR_UNSUPPORTED,
              "wavenet_stream: residual / gate / skip channels = %d / %d / %d (only 64 / 128 / 64)", d->residual_channels,
              d->gate_channels, d->skip_channels);
  PWG_REQUIRE(d->aux_channels == WS_AUX, PWG_ERR_UNSUPPORTED, "wavenet_stream: aux channels = %d (only 80)",
              d->aux_channels);
  PWG_REQUIRE(d->batch >= 1 && d->batch <= 65535, PWG_ERR_UNSUPPORTED, "wavenet_stream: batch = %d (1 .. 65535)", d->batch);
  PWG_REQUIRE(d->t >= 1, PWG_ERR_BAD_SHAPE, "wavenet_stream: t = %d columns per push (>= 1)", d->t);
  PWG_REQUIRE(d->dilation >= 1, PWG_ERR_BAD_SHAPE, "wavenet_stream: dilation = %d (>= 1)", d->dilation);
  // byte offsets inside one item of x / c / the history are 32-bit (buffer addressing), element indices int
  PWG_REQUIRE((long)WN_G * d->t * 4 < (1L << 31), PWG_ERR_UNSUPPORTED, "wavenet_stream: t = %d columns per push is too long",
              d->t);
  PWG_REQUIRE((long)WN_R * 2 * d->dilation * 4 < (1L << 31), PWG_ERR_UNSUPPORTED,
              "wavenet_stream: dilation = %d: the history of one item is too long", d->dilation);
  return PWG_OK;
}

int wavenet_delayed_geometry(const pwg_wavenet_desc* d, int32_t c_delay) {
  const int rc = wavenet_stream_geometry(d, true);
  if (rc != PWG_OK) return rc;
  PWG_REQUIRE(c_delay >= 0, PWG_ERR_BAD_SHAPE, "wavenet_stream_delayed: c_delay = %d is negative", c_delay);
  PWG_REQUIRE((long)WS_AUX * c_delay * 4 < (1L << 31), PWG_ERR_UNSUPPORTED,
              "wavenet_stream_delayed: c_delay = %d: the conditioning line of one item is too long", c_delay);
  return PWG_OK;
}

int wavenet_stream_pointers(const char* name, const float* x, const float* c, const float* hist_in, const float* hist_out,
                            const void* packed, const float* x_out, const float* skips_out) {
  PWG_REQUIRE(x && c && packed && x_out && skips_out && hist_out, PWG_ERR_NULL, "%s: NULL pointer", name);
  PWG_REQUIRE(hist_in != hist_out, PWG_ERR_BAD_SHAPE,
              "%s: hist_in and hist_out must be distinct buffers (other workgroups read the history)", name);
  PWG_REQUIRE(x != x_out, PWG_ERR_BAD_SHAPE, "%s: x_out must not alias x (tiles read their neighbours' samples)", name);
  PWG_REQUIRE(aligned(x, 3) && aligned(c, 3) && aligned(hist_in, 3) && aligned(hist_out, 3) && aligned(packed, 15),
              PWG_ERR_BAD_SHAPE, "%s: unaligned tensor (4 B; the weight image 16 B)", name);
  return PWG_OK;
}

int wavenet_delayed_pointers(const char* name, const pwg_wavenet_desc* d, const float* c_line, int32_t c_cols,
                             int32_t c_delay, const float* skips, const float* skip_line_in, const float* skip_line_out,
                             const float* skips_out) {
  PWG_REQUIRE(c_line == nullptr || (c_cols >= c_delay && (long)WS_AUX * c_cols * 4 < (1L << 31)), PWG_ERR_BAD_SHAPE,
              "%s: a conditioning line of %d columns cannot serve c_delay = %d (c_delay .. 2^31 bytes per item)", name,
              c_cols, c_delay);
  PWG_REQUIRE(skips == nullptr || skip_line_out != nullptr, PWG_ERR_NULL,
              "%s: skips needs skip_line_out (the layer keeps %d columns of the skip sum)", name, d->dilation);
  PWG_REQUIRE(skips == nullptr || skip_line_in != skip_line_out, PWG_ERR_BAD_SHAPE,
              "%s: skip_line_in and skip_line_out must be distinct buffers (other workgroups read the line)", name);
  PWG_REQUIRE(skips == nullptr || skips != skips_out, PWG_ERR_BAD_SHAPE,
              "%s: skips_out must not alias skips (tiles read their neighbours' skip columns)", name);
  PWG_REQUIRE(aligned(c_line, 3) && aligned(skips, 3) && aligned(skip_line_in, 3) && aligned(skip_line_out, 3),
              PWG_ERR_BAD_SHAPE, "%s: unaligned tensor (4 B)", name);
  return PWG_OK;
}

int wavenet_slots_pointers(const char* name, const pwg_wavenet_desc* d, int32_t c_delay, const float* c_line,
                           const float* skips, const float* skip_line_in, const float* hist_in, const int32_t* slots,
                           int32_t rate, int32_t delay) {
  PWG_REQUIRE(slots != nullptr, PWG_ERR_NULL, "%s: slots is NULL", name);
  PWG_REQUIRE(aligned(slots, 3), PWG_ERR_BAD_SHAPE, "%s: unaligned slot table", name);
  PWG_REQUIRE(rate >= 1 && delay >= 0, PWG_ERR_BAD_SHAPE, "%s: rate = %d, delay = %d (needs rate >= 1, delay >= 0)", name,
              rate, delay);
  PWG_REQUIRE(hist_in != nullptr, PWG_ERR_NULL,
              "%s: hist_in is NULL (the start of a stream is an item's, in the table)", name);
  PWG_REQUIRE(c_line != nullptr || c_delay == 0, PWG_ERR_NULL,
              "%s: c_line is NULL with c_delay = %d (a fresh item does not read it)", name, c_delay);
  PWG_REQUIRE(skips == nullptr || skip_line_in != nullptr, PWG_ERR_NULL,
              "%s: skips needs skip_line_in (%d columns; a fresh item does not read it)", name, d->dilation);
  return PWG_OK;
}

namespace {

// The argument fields the two forms share, behind the pointer rules
static int wavenet_stream_fill(const char* name, WnStreamArgs* a, const pwg_wavenet_desc* d, const float* x, const float* c,
                               const float* skips, const float* hist_in, float* hist_out, const float* packed,
                               const float* b_dil, const float* b_skip, const float* b_out, float* x_out, float* skips_out) {
  const int rc = wavenet_stream_pointers(name, x, c, hist_in, hist_out, packed, x_out, skips_out);
  if (rc != PWG_OK) return rc;
  a->x = x;
  a->c = c;
  a->skips = skips;
  a->hist_in = hist_in;
  a->hist_out = hist_out;
  a->w1 = packed;
  a->w2 = packed + (size_t)WS_ROWS * WN_G;
  a->b_dil = b_dil;
  a->b_skip = b_skip;
  a->b_out = b_out;
  a->x_out = x_out;
  a->skips_out = skips_out;
  a->n = d->t;
  a->dil = d->dilation;
  a->out_mul = d->out_mul;
  a->skip_mul = d->skip_mul;
  a->vec_ok = aligned(x_out, 15) && aligned(skips, 15) && aligned(skips_out, 15);
  return PWG_OK;
}

// state_floats: what the launch reads and writes besides the chunk (history; the delayed form's lines)
template <class ARGS>
static int wavenet_stream_launch(const char* name, const char* kernel_name, const pwg_wavenet_desc* d, const ARGS& a,
                                 double state_floats, hipStream_t stream) {
  const size_t lds = (size_t)WS_ROWS * WN_COLS * sizeof(float);
  void (*kern)(ARGS) = wavenet_stream_kernel<ARGS>;
  if (!lds_limit_is_set(reinterpret_cast<const void*>(kern), lds)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    PWG_REQUIRE(e == hipSuccess, PWG_ERR_LAUNCH, "%s: cannot raise the LDS limit to %zu: %s", name, lds,
                hipGetErrorString(e));
  }
  const double samples = (double)d->batch * d->t;
  const double flops = 2.0 * samples * (WN_G * (double)WS_ROWS + (double)(WN_S + WN_R) * WN_R);
  const double bytes = 4.0 * (samples * (WN_R * 4 + WS_AUX + (a.skips ? WN_S : 0)) + state_floats) +
                       4.0 * ((double)WS_ROWS * WN_G + (double)WN_R * (WN_S + WN_R));
  maybe_poison_lds(stream);
  {
    ProfScope prof(stream, kernel_name, flops, bytes);
    hipLaunchKernelGGL(kern, dim3(ceil_div(d->t, WN_COLS), d->batch), dim3(256), lds, stream, a);
  }
  PWG_CHECK_LAUNCH(name);
  return PWG_OK;
}

}  // namespace
}  // namespace pwg

using namespace pwg;

extern "C" int pwg_wavenet_stream_supported(const pwg_wavenet_desc* d) {
  return wavenet_stream_geometry(d) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_wavenet_stream_hist_floats(const pwg_wavenet_desc* d) {
  if (wavenet_stream_geometry(d) != PWG_OK) return 0;
  return (size_t)d->batch * WN_R * (size_t)(d->kernel - 1) * d->dilation;
}

extern "C" int pwg_wavenet_stream_forward(const pwg_wavenet_desc* d, const float* x, const float* c, const float* skips,
                                          const float* hist_in, float* hist_out, const float* packed, const float* b_dil,
                                          const float* b_skip, const float* b_out, float* x_out, float* skips_out,
                                          void* stream_) {
  int rc = wavenet_stream_geometry(d);
  if (rc != PWG_OK) return rc;
  WnStreamArgs a;
  rc = wavenet_stream_fill("wavenet_stream_forward", &a, d, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out,
                           x_out, skips_out);
  if (rc != PWG_OK) return rc;
  return wavenet_stream_launch("wavenet_stream_forward", "wavenet_stream_kernel", d, a,
                               2.0 * d->batch * WN_R * 2.0 * d->dilation, (hipStream_t)stream_);
}

extern "C" int pwg_wavenet_stream_delayed_supported(const pwg_wavenet_desc* d, int32_t c_delay) {
  return wavenet_delayed_geometry(d, c_delay) == PWG_OK ? 1 : 0;
}

extern "C" size_t pwg_wavenet_stream_delayed_hist_floats(const pwg_wavenet_desc* d) {
  if (wavenet_stream_geometry(d, true) != PWG_OK) return 0;
  return (size_t)d->batch * WN_R * (size_t)(d->kernel - 1) * d->dilation;
}

extern "C" int pwg_wavenet_stream_delayed_forward(const pwg_wavenet_desc* d, const float* x, const float* c,
                                                  const float* c_line, int32_t c_cols, int32_t c_delay, const float* skips,
                                                  const float* skip_line_in, float* skip_line_out, const float* hist_in,
                                                  float* hist_out, const float* packed, const float* b_dil,
                                                  const float* b_skip, const float* b_out, int32_t valid_lo,
                                                  int32_t valid_hi, float* x_out, float* skips_out, void* stream_) {
  const char* name = "wavenet_stream_delayed_forward";
  int rc = wavenet_delayed_geometry(d, c_delay);
  if (rc != PWG_OK) return rc;
  rc = wavenet_delayed_pointers(name, d, c_line, c_cols, c_delay, skips, skip_line_in, skip_line_out, skips_out);
  if (rc != PWG_OK) return rc;
  WnDelayedArgs a;
  rc = wavenet_stream_fill(name, &a, d, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, x_out, skips_out);
  if (rc != PWG_OK) return rc;
  a.c_line = c_line;
  a.c_cols = c_line ? c_cols : 0;
  a.c_delay = c_delay;
  a.skip_line_in = skips ? skip_line_in : nullptr;
  a.skip_line_out = skips ? skip_line_out : nullptr;
  a.valid_lo = valid_lo;
  a.valid_hi = valid_hi;
  return wavenet_stream_launch(name, "wavenet_stream_delayed_kernel", d, a,
                               (double)d->batch * (2.0 * WN_R * 2.0 * d->dilation + (skips ? 2.0 * WN_S * d->dilation : 0.0)),
                               (hipStream_t)stream_);
}

// The slotted form: pwg_wavenet_stream_delayed_forward with the window replaced by the table, its rate and delay
extern "C" int pwg_wavenet_stream_slots_forward(const pwg_wavenet_desc* d, const float* x, const float* c,
                                                const float* c_line, int32_t c_cols, int32_t c_delay, const float* skips,
                                                const float* skip_line_in, float* skip_line_out, const float* hist_in,
                                                float* hist_out, const float* packed, const float* b_dil,
                                                const float* b_skip, const float* b_out, const int32_t* slots,
                                                int32_t rate, int32_t delay, float* x_out, float* skips_out,
                                                void* stream_) {
  const char* name = "wavenet_stream_slots_forward";
  int rc = wavenet_delayed_geometry(d, c_delay);
  if (rc != PWG_OK) return rc;
  rc = wavenet_slots_pointers(name, d, c_delay, c_line, skips, skip_line_in, hist_in, slots, rate, delay);
  if (rc != PWG_OK) return rc;
  rc = wavenet_delayed_pointers(name, d, c_line, c_cols, c_delay, skips, skip_line_in, skip_line_out, skips_out);
  if (rc != PWG_OK) return rc;
  WnSlotsArgs a;
  rc = wavenet_stream_fill(name, &a, d, x, c, skips, hist_in, hist_out, packed, b_dil, b_skip, b_out, x_out, skips_out);
  if (rc != PWG_OK) return rc;
  a.c_line = c_line;
  a.c_cols = c_line ? c_cols : 0;
  a.c_delay = c_delay;
  a.skip_line_in = skips ? skip_line_in : nullptr;
  a.skip_line_out = skips ? skip_line_out : nullptr;
  a.slots = slots;
  a.rate = rate;
  a.out_delay = delay;
  return wavenet_stream_launch(name, "wavenet_stream_slots_kernel", d, a,
                               (double)d->batch * (2.0 * WN_R * 2.0 * d->dilation + (skips ? 2.0 * WN_S * d->dilation : 0.0)),
                               (hipStream_t)stream_);
}
