// The reader of split-K partial sums.
//
// A split-K GEMM never reduces its own output: it leaves S fp32 slabs
// part[S][rows][width] (PendingSum in xgserve/ops/linear.py) and the next kernel sums
// them in its prologue or tail. This header is the one definition of that sum:
//   * slab order s = 0, 1, ..., S - 1, in fp32, added to whatever the caller put in f
//     (zero, or the residual) -- so the only rounding is the caller's one at the end;
//   * every load is 16 B per lane; W = 4 or 8 columns per lane.
// add_partials<W, SP> reads every slab of one (row, col); SP picks static or serial.
// (The clamped, masked batches of decode_attention.hip and gemm_m64g.hip's tails, and the
// loops of comm/custom_allreduce.hip, add_partials_rmsnorm and reduce_partials, sum in the
// same order but keep their own form: profiles/partials_reader.md says why.)
//
// SP, a kernel's template argument, means the same in every consumer:
//   SP > 0   exactly SP slabs, all loads issued before the first add
//   SP == 0  runtime S, one dependent load per slab (S L2 round trips in a row)
//   SP == -1 not slabs at all: the kernel's bf16 row source (rope_cache, moe combine)
// (sp_dispatch in cfg_dispatch.h turns a runtime S into SP on the host.)
#pragma once

#include "common.h"

namespace xgk {

// f[0..W) += v[0..W/4)
template <int W>
__device__ __forceinline__ void add_quads(float* f, const float4* v) {
#pragma unroll
  for (int q = 0; q < W / 4; ++q) {
    f[4 * q + 0] += v[q].x; f[4 * q + 1] += v[q].y; f[4 * q + 2] += v[q].z; f[4 * q + 3] += v[q].w;
  }
}

// f[0..W) += sum_s part[(s * rows + row) * width + col + 0..W), s = 0 .. in order.
template <int W, int SP>
__device__ __forceinline__ void add_partials(const float* part, int S, int rows, int row, int width, int col,
                                             float* f) {
  static_assert((W == 4 || W == 8) && SP >= 0, "4 or 8 columns per lane; SP < 0 is not a slab source");
  constexpr int Q = W / 4;
  if constexpr (SP > 0) {
    float4 v[SP][Q];
#pragma unroll
    for (int s = 0; s < SP; ++s) {
      const float* p = part + (static_cast<int64_t>(s) * rows + row) * width + col;
#pragma unroll
      for (int q = 0; q < Q; ++q) v[s][q] = *reinterpret_cast<const float4*>(p + 4 * q);
    }
#pragma unroll
    for (int s = 0; s < SP; ++s) add_quads<W>(f, v[s]);
  } else {
    for (int s = 0; s < S; ++s) {
      const float* p = part + (static_cast<int64_t>(s) * rows + row) * width + col;
      float4 v[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) v[q] = *reinterpret_cast<const float4*>(p + 4 * q);
      add_quads<W>(f, v);
    }
  }
}

}  // namespace xgk
