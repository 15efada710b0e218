// What the samplers (sampling.hip) and the speculative verify kernels (spec_sample.hip)
// share: the counter hash behind every draw and the per-element-type row readers. The
// written contract of the hash is tests/test_sampling_gpu.py.
#pragma once
#include "glds.h"

namespace xgk {

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

template <typename T> struct VecW { static constexpr int W = 8; };
template <> struct VecW<float> { static constexpr int W = 4; };

template <typename T>
__device__ __forceinline__ float scalar_at(const T* row, int i);
template <> __device__ __forceinline__ float scalar_at<uint16_t>(const uint16_t* r, int i) { return bf2f(r[i]); }
template <> __device__ __forceinline__ float scalar_at<float>(const float* r, int i) { return r[i]; }

}  // namespace xgk
