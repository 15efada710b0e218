// Host entry points of gemm_m64g.hip and gemm_w8.hip: the one declaration shared by the
// kernels' translation units and the pybind11 layer (ops.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace xgk {

// GG_MOE_RESID (grouped w2 of the fused decode layer, TP = 1): the MoE combine inside
// the w2 launch. Every workgroup stores its fp32 partial rows write-through and takes a
// ticket on its column tile; the tile's last arriver (all real row tiles x S splits
// have stored) adds, per token t, sum_j w[t, j] * sum_s part[s, dest[t, j]] over the
// tile's columns into the bf16 residual stream and writes the new residual's sum of
// squares ss_out[tile * T + t] (the next RMSNorm reads N / cols partial sums per row).
// Replaces the separate combine_resid launch (6 us per layer at Mixtral batch 1).
struct MoeResidEpi {
  const int32_t* dest;   // [T * k] padded row of each (token, choice), -1 = not local
  const float* w;        // [T * k] routing weights
  uint16_t* resid;       // [T, N] bf16 residual stream, updated in place
  float* ss_out;         // [N / cols, T]
  int* counters;         // one ticket per column tile, zero between launches
  int T;
  int k;
};

int gemm_m64g(const uint16_t* x, int M, int K, const uint16_t* w, int N, float* part, uint16_t* out, int S, int mode,
              int nw, int cfg, hipStream_t st);
int gemm_m64g_ex(const uint16_t* x, int M, int K, const uint16_t* w, int N, float* part, uint16_t* out, int S,
                 int mode, int nw, int cfg, const float* ss_in, int ss_n, int ss_stride, float eps, uint16_t* resid,
                 float* ss_out, int* counters, hipStream_t st);
int gemm_m64g_ar(const uint16_t* x, int M, int K, const uint16_t* w, int N, float* part, int S, int nw, int cfg,
                 uint16_t* resid, float* ss_out, int* counters, const void* desc, hipStream_t st);
int m64g_ar_desc_bytes();
int moe_gemm_m64g(const uint16_t* x, const int32_t* rows, const int32_t* offs, int E, int K, const uint16_t* w, int N,
                  int P, float* part, uint16_t* out, int S, int mode, int nw, int cfg, int max_rows, hipStream_t st,
                  const int32_t* valid, const MoeResidEpi* mre = nullptr, int pairs = 0);
void set_k_rotation(int mode);
int gemm_w8(const uint16_t* x, int M, int K, const uint8_t* w, const float* scale, int N, float* part, uint16_t* out,
            int S, int mode, int cfg, hipStream_t st, int fmt);

}  // namespace xgk
