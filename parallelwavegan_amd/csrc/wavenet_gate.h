// wavenet_gate.h -- what the fused WaveNet layer kernels share: the PWG.v1 layer geometry, the MFMA accumulator type
// and the gate (csrc/wavenet.hip: whole utterance; csrc/wavenet_stream.hip: one chunk of a causal stream).
#pragma once

namespace pwg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int WN_R = 64;     // residual channels
constexpr int WN_G = 128;    // gate channels
constexpr int WN_S = 64;     // skip channels
constexpr int WN_K = 3;      // taps
constexpr int WN_COLS = 64;  // columns per workgroup

// tanh(t) * sigmoid(s) on the hardware exp2 / rcp (1 ulp each): sigmoid(v) = 1 / (1 + 2^(-v log2 e)),
// tanh(t) = 2 sigmoid(2 t) - 1; saturates correctly (2^inf = inf -> rcp = 0).  Absolute error ~1e-7, against
// 8 % of the kernel for libm's tanhf + expf (profiles/r03_wavenet_ablation.txt).
__device__ __forceinline__ float gate_fast(float t, float s) {
  const float L2E = 1.4426950408889634f;
  const float sg = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-s * L2E));
  const float th = 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-2.f * L2E * t)) - 1.f;
  return th * sg;
}

}  // namespace pwg
