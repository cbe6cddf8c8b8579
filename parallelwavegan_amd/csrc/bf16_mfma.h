// What the bf16-operand kernels (conv1d_bf16.hip, wavenet_bf16.hip) share: the operand / accumulator vector types, the
// two bf16 MFMA shapes of gfx950 behind one template, and the accumulator layout.  Internal to csrc/; the staging loops
// of the kernels differ on purpose and stay with them.
#pragma once

namespace pwg {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// TILE: MFMA shape (32: 32x32x16, 16: 16x16x32)
template <int TILE>
struct Mfma;
template <>
struct Mfma<32> {
  typedef f32x16 acc_t;
  static __device__ __forceinline__ acc_t run(bf16x8 a, bf16x8 b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma<16> {
  typedef f32x4 acc_t;
  static __device__ __forceinline__ acc_t run(bf16x8 a, bf16x8 b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

// Accumulator layout of both shapes: register i of a lane holds column lane % TILE and, in a tile whose first row is
// row0, this row (lane_group = lane / TILE)
template <int TILE>
__device__ __forceinline__ int mfma_acc_row(int row0, int i, int lane_group) {
  constexpr int HL = 64 / TILE;  // lane groups along the reduction (2 / 4)
  return row0 + (i & 3) + 4 * lane_group + 4 * HL * (i >> 2);
}

}  // namespace pwg
