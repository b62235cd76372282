// The register vector types of the MFMA kernels and the two matrix instructions the small-channel convolutions use
// (conv_t32*.hip, conv_h16*.hip, conv_h3.hip, conv_up.hip, conv_pair_strip*).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;

// v_mfma_f32_16x16x4_f32: D[16][16] += A[16][4] B[4][16], one float of A and of B per lane
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// v_mfma_f32_16x16x16_f16: D[16][16] += A[16][16] B[16][16], four binary16 values of A and of B per lane
__device__ __forceinline__ f32x4 mfma16(f16x4 a, f16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
