// Host side of the hand-written GEMM families (gemm_m64g.hip dense and grouped,
// gemm_w8.hip, gemm_mw.hip, gemm_pf.hip dense and grouped): the one declaration of their
// entry points, of the row type of each family's configuration table (the table itself
// sits next to its kernel) and of the no-launch shape predicates, shared by the kernels'
// translation units and the pybind11 layer (ops.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace xgk {

constexpr int LDS_BYTES = 160 * 1024;  // per workgroup (gfx950)

// A family's table is indexed by the `cfg` argument of its entry points; *_cfgs returns
// the table and its length.
struct M64Cfg {
  int wv, kc;    // waves per workgroup, k per chunk
  bool nt;       // non-temporal weight DMA
  int ns;        // ring slots: 3, or deeper (one x tile only)
  bool grouped;  // also a cfg of moe_gemm_m64g
  constexpr int cols(int nw) const { return 16 * nw * wv; }  // columns per workgroup
};
struct W8Cfg {
  int nw, wv, kc;  // 16-column tiles per wave, waves per workgroup, k per chunk
  constexpr int cols() const { return 16 * nw * wv; }
};
struct MwCfg {
  int wn, nwt, d;  // waves along N (8 / wn along M), 16-column tiles per wave, weight ring depth
  bool nt;
  constexpr int cols() const { return 16 * wn * nwt; }
};
struct PfCfg {
  int bm, mtp, lag;  // tile rows, 16-row m tiles per wave per phase, DMA lag (phases)
  bool grouped;      // also a cfg of gemm_pf_grouped
};
int m64g_cfgs(const M64Cfg** rows);
int w8_cfgs(const W8Cfg** rows);
int mw_cfgs(const MwCfg** rows);
int pf_cfgs(const PfCfg** rows);

constexpr int M64G_MAX_M = 64, W8_MAX_M = 64, MW_MAX_M = 320;
constexpr int WQ_GROUP = 128;       // k per int4 scale group
constexpr int WQ_SC_FLOATS = 4096;  // int4 scales staged per workgroup (groups x columns)

// What an entry point takes, pointers aside (the entry points check these first).
bool m64g_supports(int M, int K, int N, int S, int mode, int nw, int cfg);
bool moe_m64g_supports(int E, int K, int N, int P, int S, int mode, int nw, int cfg, int max_rows);
bool w8_supports(int M, int K, int N, int S, int mode, int cfg, int fmt);
bool mw_supports(int M, int K, int N, int S, int mode, int cfg);
bool pf_supports(int M, int K, int N, int S, int mode, int cfg);
bool pf_grouped_supports(int E, int P, int K, int N, int max_pairs, int S, int mode, int cfg);

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
int k_rotation(int S);  // gemm_m64g.hip; gemm_mw follows the same policy
int gemm_w8(const uint16_t* x, int M, int K, const uint8_t* w, const float* scale, int N, float* part, uint16_t* out,
            int S, int mode, int cfg, hipStream_t st, int fmt);
int gemm_mw(const uint16_t* x, int M, int K, const uint16_t* w, int N, float* part, uint16_t* out, int S, int mode,
            int cfg, hipStream_t st);
int gemm_pf(const uint16_t* x, int M, int K, const uint16_t* w, int N, float* part, uint16_t* out, int S, int mode,
            int cfg, hipStream_t st);
int gemm_pf_grouped(const uint16_t* x, const int32_t* rows, const int32_t* offs, int E, int P, int K,
                    const uint16_t* w, int N, int max_pairs, float* part, uint16_t* out, int S, int mode, int cfg,
                    hipStream_t st);
void set_pf_krot(int on);

}  // namespace xgk
