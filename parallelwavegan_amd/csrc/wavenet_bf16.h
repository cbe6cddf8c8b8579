// wavenet_bf16.h -- what the bf16-operand forms of the fused Parallel WaveGAN layer share (csrc/wavenet_bf16.hip: whole
// utterance; csrc/wavenet_stream_bf16.hip: one chunk of a stream): the PWG.v1 layer geometry, the layout of the operand
// tiles in LDS and of the packed weight image, and the fp32 gate.  Internal to csrc/.
//
// Operand tile: [column][channel] bf16, K1 = 288 channels per column (tap 0, tap 1, tap 2 of x, 64 channels each; the 80
// aux rows; 16 zeros), column stride RS = 37 x 16 B (odd).  Gate tile: [column][64 channels] bf16, stride RG = 9 x 16 B.
// Weight image (pwg_wavenet_bf16_pack_weights): 16-B fragments [K / 8][128 rows][8], phase 1 (K1) then phase 2 (K2).
#pragma once
#include "bf16_mfma.h"

#include <stddef.h>

namespace pwg {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // 16-B load at a 4-B aligned address

constexpr int BR = 64;                  // residual channels
constexpr int BG = 128;                 // gate channels
constexpr int BS = 64;                  // skip channels
constexpr int BA = 80;                  // aux channels
constexpr int BK = 3;                   // taps
constexpr int BCOLS = 64;               // columns per workgroup
constexpr int K1 = 288;                 // phase-1 reduction: 3 * 64 + 80 = 272, padded to 32-channel chunks
constexpr int OCT1 = K1 / 8;            // 36 channel octets per column
constexpr int K2 = BR;                  // phase-2 reduction: the 64 gate outputs
constexpr int RS = K1 + 8;              // bf16 per column of the operand tile (592 B = 37 x 16 B)
constexpr int RG = K2 + 8;              // bf16 per column of the gate tile (144 B = 9 x 16 B)
constexpr size_t kLds = (size_t)BCOLS * (RS + RG) * sizeof(__bf16) + (BG + BS + BR) * sizeof(float);
constexpr int RING = 4;                 // phase-1 weight fragments in flight (k-steps)

// tanh(t) * sigmoid(s) on the hardware exp2 / rcp: the form of wavenet.hip (gate_fast), so that the fp32 gate of the
// kernels is the same function
__device__ __forceinline__ float gate_fp32(float t, float s) {
  const float L2E = 1.4426950408889634f;
  const float sg = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-s * L2E));
  const float th = 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-2.f * L2E * t)) - 1.f;
  return th * sg;
}

}  // namespace pwg
