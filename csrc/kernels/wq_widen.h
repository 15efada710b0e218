// Weight-only quantization formats of the GEMMs that stream codes (gemm_w8.hip, gemm_mw8.hip)
// and the exact widening of one A fragment (8 consecutive k of one weight row) to bf16 in
// registers. The layouts are those of xgserve/ops/linear.py quantize_fp8 / _int8 / _int4.
#pragma once

#include "common.h"

namespace xgk {

enum : int { WQ_FP8 = 0, WQ_INT8 = 1, WQ_INT4 = 2 };

// 8 int8 codes (k order) -> bf16x8 A fragment (exact)
__device__ __forceinline__ bf16x8_t int8x8_to_bf16(uint2 v) {
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t wv = j ? v.y : v.x;
    const float a = static_cast<float>(static_cast<int8_t>(wv & 0xFF));
    const float b = static_cast<float>(static_cast<int8_t>((wv >> 8) & 0xFF));
    const float c = static_cast<float>(static_cast<int8_t>((wv >> 16) & 0xFF));
    const float d = static_cast<float>(static_cast<int8_t>(wv >> 24));
    // exact integers: the bf16 of each is its top 16 bits
    o[2 * j] = (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xFFFF0000u);
    o[2 * j + 1] = (__float_as_uint(c) >> 16) | (__float_as_uint(d) & 0xFFFF0000u);
  }
  return as_frag(make_uint4(o[0], o[1], o[2], o[3]));
}

// 8 offset-binary nibbles (pair-interleaved, see WQ_INT4) -> bf16x8 of 136 + q
__device__ __forceinline__ bf16x8_t u4x8_to_bf16(uint32_t v) {
  return as_frag(make_uint4((v & 0x000F000Fu) | 0x43004300u, ((v >> 4) & 0x000F000Fu) | 0x43004300u,
                            ((v >> 8) & 0x000F000Fu) | 0x43004300u, ((v >> 12) & 0x000F000Fu) | 0x43004300u));
}

// 8 E4M3 bytes (k order) -> bf16x8 A fragment
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16(uint2 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.x, 1.0f, false);
  const auto b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.x, 1.0f, true);
  const auto c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.y, 1.0f, false);
  const auto d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.y, 1.0f, true);
  return as_frag(make_uint4(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                            __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d)));
#else
  return bf16x8_t{};
#endif
}

}  // namespace xgk
