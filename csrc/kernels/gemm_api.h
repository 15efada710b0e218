// Host side of the hand-written GEMM families (gemm_m64g.hip dense and grouped,
// gemm_w8.hip, moe_gemm_w8.hip, gemm_mw.hip, gemm_mw8.hip, gemm_pf.hip dense and grouped, gemm_f8.hip, gemm_i4.hip): the one declaration of their
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
struct Mw8Cfg {
  int wn, nwt, dw;  // waves along N (8 / wn along M), 16-column tiles per wave, code ring slots
  constexpr int cols() const { return 16 * wn * nwt; }
};
struct PfCfg {
  int bm, mtp, lag;  // tile rows, 16-row m tiles per wave per phase, DMA lag (phases)
  bool grouped;      // also a cfg of gemm_pf_grouped
};
struct F8Cfg {
  int bm, ns;  // tile rows, LDS ring slots (one 128-deep K tile of codes each)
};
struct I4Cfg {
  int bm, ns;  // tile rows, LDS ring slots (one 128-deep K tile of A codes, packed W codes and group scales each)
};
int m64g_cfgs(const M64Cfg** rows);
int w8_cfgs(const W8Cfg** rows);
int moe_w8_cfgs(const W8Cfg** rows);
int mw_cfgs(const MwCfg** rows);
int mw8_cfgs(const Mw8Cfg** rows);
int pf_cfgs(const PfCfg** rows);
int f8_cfgs(const F8Cfg** rows);
int i4_cfgs(const I4Cfg** rows);

constexpr int M64G_MAX_M = 64, W8_MAX_M = 64, MW_MAX_M = 320;
constexpr int WQ_GROUP = 128;       // k per int4 scale group
constexpr int WQ_SC_FLOATS = 4096;  // int4 scales staged per workgroup (groups x columns)

// What an entry point takes, pointers aside (the entry points check these first).
bool m64g_supports(int M, int K, int N, int S, int mode, int nw, int cfg);
bool moe_m64g_supports(int E, int K, int N, int P, int S, int mode, int nw, int cfg, int max_rows);
bool w8_supports(int M, int K, int N, int S, int mode, int cfg, int fmt);
bool moe_w8_supports(int E, int K, int N, int P, int S, int mode, int cfg, int fmt, int max_rows);
bool mw_supports(int M, int K, int N, int S, int mode, int cfg);
bool mw8_supports(int M, int K, int N, int S, int mode, int cfg, int fmt);
bool pf_supports(int M, int K, int N, int S, int mode, int cfg);
bool pf_grouped_supports(int E, int P, int K, int N, int max_pairs, int S, int mode, int cfg);
bool f8_supports(int M, int K, int N, int S, int mode, int cfg);
bool moe_f8_supports(int E, int P, int K, int N, int max_pairs, int S, int mode, int cfg);
bool i8_supports(int M, int K, int N, int S, int mode, int cfg);  // f8_supports and K <= 131,072
bool i4_supports(int M, int K, int N, int S, int mode, int cfg);

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
// moe_gemm_w8.hip: moe_gemm_m64g's layout operands on expert codes (fmt WQ_*: fp8 / int8 codes
// [E, N, K] + scales [E, N]; int4 codes [E, N, K / 2] + group scales [E, K / 128, N])
int moe_gemm_w8(const uint16_t* x, const int32_t* rows, const int32_t* offs, int E, int K, const uint8_t* w,
                const float* scale, int N, int P, float* part, uint16_t* out, int S, int mode, int cfg, int fmt,
                int max_rows, hipStream_t st, const int32_t* valid, int pairs = 0);
int gemm_mw(const uint16_t* x, int M, int K, const uint16_t* w, int N, float* part, uint16_t* out, int S, int mode,
            int cfg, hipStream_t st);
// gemm_mw8.hip: gemm_mw's range, epilogues and split-K contract on fp8 / int8 / int4 codes
// (fmt WQ_*: the layouts gemm_w8 reads); bytes of LDS a (cfg, M, fmt) needs, 0 = does not fit
int gemm_mw8(const uint16_t* x, int M, int K, const uint8_t* w, const float* scale, int N, float* part, uint16_t* out,
             int S, int mode, int cfg, int fmt, hipStream_t st);
int mw8_lds_bytes(int M, int cfg, int fmt);
int gemm_pf(const uint16_t* x, int M, int K, const uint16_t* w, int N, float* part, uint16_t* out, int S, int mode,
            int cfg, hipStream_t st);
int gemm_pf_grouped(const uint16_t* x, const int32_t* rows, const int32_t* offs, int E, int P, int K,
                    const uint16_t* w, int N, int max_pairs, float* part, uint16_t* out, int S, int mode, int cfg,
                    hipStream_t st);
void set_pf_krot(int on);
// gemm_f8.hip: E4M3 codes on both sides (a [M, K] with row scales sx [M], w [N, K] with channel
// scales sw [N]) on the K = 128 FP8 matrix instruction; quant_rows_fp8 makes (a, sx) from bf16 rows
int gemm_f8(const uint8_t* a, const float* sx, int M, int K, const uint8_t* w, const float* sw, int N, float* part,
            uint16_t* out, int S, int mode, int cfg, hipStream_t st);
int quant_rows_fp8(const uint16_t* x, int M, int K, uint8_t* codes, float* sx, hipStream_t st);
// its grouped form over moe_align's expert-sorted rows (the prompt-sized expert GEMMs on fp8 expert
// codes): w [E, N, K], sw [E, N]; rows gathers a and sx (nullptr: both are in sorted order);
// F8_SILU -> out [P, N / 2], F8_PARTIAL -> part [S, P, N]
int moe_gemm_f8(const uint8_t* a, const float* sx, const int32_t* rows, const int32_t* offs, int E, int P, int K,
                const uint8_t* w, const float* sw, int N, int max_pairs, float* part, uint16_t* out, int S, int mode,
                int cfg, hipStream_t st);
// the same kernel on int8 codes (w as quantize_int8 stores it) and v_mfma_i32_16x16x64_i8: int32 sums,
// converted once per split; quant_rows_int8 makes (a, sx) with round-half-even codes in -127 .. 127
int gemm_i8(const uint8_t* a, const float* sx, int M, int K, const uint8_t* w, const float* sw, int N, float* part,
            uint16_t* out, int S, int mode, int cfg, hipStream_t st);
int quant_rows_int8(const uint16_t* x, int M, int K, uint8_t* codes, float* sx, hipStream_t st);
// gemm_i4.hip: int8 row codes against the packed int4 codes of quantize_int4 (w [N, K / 2], group scales
// gs [K / 128, N]) on v_mfma_i32_16x16x64_i8, one int32 sum per 128-k group folded into fp32 with the
// group's scale. a is in kernel order: within every 16 k the bytes are k (0, 4, 1, 5), (8, 12, 9, 13),
// (2, 6, 3, 7), (10, 14, 11, 15); quant_rows_int8_i4 is quant_rows_int8 storing that order
int gemm_i4(const uint8_t* a, const float* sx, int M, int K, const uint8_t* w, const float* gs, int N, float* part,
            uint16_t* out, int S, int mode, int cfg, hipStream_t st);
int quant_rows_int8_i4(const uint16_t* x, int M, int K, uint8_t* codes, float* sx, hipStream_t st);
// lm_head_score.hip: per row of h [M, K] (row stride ldh) against the LM head w [>= V, K] (row stride
// ldw), lp = z[t] - logsumexp(z), best_id = argmax z, best_lp = max z - logsumexp(z) over v < V, from
// one (max, sum, argmax) partial per BM x BN tile of z = h w^T: no logits are written. targets int32
// [M], a value outside [0, V) = no target (lp 0); ws holds lm_head_score_ws_floats(M, V) floats.
// One tile configuration, no plan table. K >= 64, K % 64 == 0, V >= 1, M >= 0 (0 launches nothing)
int lm_head_score(const uint16_t* h, int64_t ldh, int M, int K, const uint16_t* w, int64_t ldw, int V,
                  const int32_t* targets, float* ws, float* lp, int32_t* best_id, float* best_lp, hipStream_t st);
int64_t lm_head_score_ws_floats(int M, int V);
int lm_head_score_bm();
int lm_head_score_bn();

}  // namespace xgk
