// Speculative sampling: rejection-sampling verification of sampled verify blocks
// (Leviathan et al. / Chen et al., 2023). Block j holds k_j draft tokens d_0..d_{k-1},
// k_j + 1 target rows (distribution p) and k_j draft rows (distribution q), all scaled by
// the block's temperature: y = scaled_logit(x, 1 / T), lp = y_p - logZ_p, lq = y_q - logZ_q.
//
//   accept (i < k):    log(u_i) + lq_i(d_i) <= lp_i(d_i)
//   residual (i < k):  r_i = argmax_x [lp_i(x) + log(1 - exp(lq_i(x) - lp_i(x))) + g_i(x)]
//                      over lp_i(x) > lq_i(x), ties to the lowest index; no such token
//                      (p == q): the row's p-argmax
//   bonus (i = k):     r_k = argmax_x [y_p(x) + g_k(x)]  (sample_tokens of the row, step 2)
//   a_j = first i that does not accept, else k_j; out_tok = d_0..d_{a-1}, r_a; out_lp = lp
//   of each emitted token; rows after a_j are not written.
//
// The RNG is the samplers' counter hash of (seed, step, index); per position seed, stream
// (step) 0 belongs to the draft's own draw of d_i, stream 1 index 0 is u_i, stream 2 index
// x is the Gumbel noise g_i(x). Weights are unnormalised under Gumbel-max, so the residual
// needs no normalisation pass.
//
// Three launches, data handed between workgroups at kernel boundaries only (no tickets,
// no atomics, nothing that must be zero on entry):
//   K1 spec_stats:  per chunk of every target and draft row, (max y, sum exp(y - max)).
//   K2 spec_draw:   per chunk of every target row, the best (score, index, lp) of the
//                   residual or bonus draw (and the chunk's p-argmax on residual rows).
//   K3 spec_select: one wave per block: merges the chunk winners in chunk order, runs
//                   the k accept tests and writes tokens, logprobs and accepted[j].
// Rows are addressed by index (p_row0 / q_row0), so blocks may share rows; a position is
// a "logical row": lrow0[j] = sum over j' < j of (k_j' + 1).
//
// Truncated blocks (top_p < 1 or 0 < top_k < V). p' = norm(p restricted to K_p) and
// q' = norm(q restricted to K_q), K(row) the split-row sampler's kept set for the block's
// (T, top_p, top_k): the row maximum, and every token whose (bin, sub) = samp_bin(M - y)
// lies at or before the top-p boundary and before the top-k boundary (samp_kept). With
// lp'(x) = y_p(x) - logZ'_p on K_p (-inf off it), lq' likewise:
//   accept:   d not in K_p: reject; d in K_p but not in K_q: accept (the draft drew d with
//             this very sampler, so this arises only where the last ulp of logZ differs
//             between the draft sampler's chunking and this file's and moves a boundary by
//             one sub-bin: q'(d) is then as good as 0 < p'(d)); else log u + lq'(d) <= lp'(d)
//   residual: over K_p (tokens off it are skipped before any arithmetic), weight lp' off
//             K_q, else lp' + log(1 - exp(lq' - lp')) where lp' > lq'; none: the p-argmax
//   bonus:    argmax over K_p of y_p + g: sample_tokens(step 2) of the row with top_p / top_k
//   out_lp:   still y_p - logZ_p of the whole row (logprobs refer to the untruncated row)
// A launch with a truncated block runs six kernels: K1, which also zeroes the truncated
// rows' histograms and tickets; H1 and H2, the sampler's two histogram levels over u64
// fixed-point mass and counts (order-independent), per chunk in LDS, added to the row's
// global histogram with atomics, scanned by the row's last workgroup into (bp, bk) and
// (sp, sk) -- samp_hist_level of samp_common.h, the body of the sampler's own passes; KZ,
// the kept mass of every chunk; K2 and K3 as above with the kept sets applied. Untruncated
// blocks of such a launch run the same arithmetic as in a launch without one, and a launch
// without one runs K1, K2, K3 only.
// Workspace rule: each truncated logical row (target and draft) owns one spec::TRow
// (~24 KB) in the workspace, sized by spec_ws_bytes(Lp, Lq, V, truncated rows). Unlike the
// sampler's, it need not be zero on entry and nothing relies on what a launch leaves
// behind: K1 clears every TRow the launch uses, and the kernel boundary orders that before H1.
#include <algorithm>
#include <type_traits>

#include "samp_common.h"

namespace xgk {

namespace spec {
constexpr int NT = 256;   // threads per workgroup of K1 / K2
constexpr int PMAX = 64;  // chunks per row: one wave merges them
// -log(-log u) < 16.64 for u <= 1 - 2^-24 (sampling.hip samp_draw_kernel)
constexpr float GMAX = 17.5f;

struct Block {
  int p_row0, q_row0;  // first target / draft logits row
  int d_off;           // first draft token in the draft-token array
  int k;               // draft tokens (>= 1)
  int lrow0;           // first logical row: seeds, workspace
  int out_row0;        // first row of out_tok / out_lp
  float temp;          // > 0
  int top_k;           // >= 0; 0 or >= V: off
  float top_p;         // (0, 1]; 1: off
  int trow0;           // truncated block: its first TRow (k + 1 target rows, then k draft rows)
};

// scratch of one truncated logical row: the two histogram levels and what their scans found
// (the fields of the sampler's samp::Row, with the same meaning)
struct TRow {
  unsigned long long h1m[samp::NB];
  unsigned int h1c[samp::NB];
  unsigned long long h2m[samp::NB];
  unsigned int h2c[samp::NB];
  unsigned long long mass_before_p;  // H1 -> H2
  int bp, bk, cnt_before_k, sp, sk;  // bp / bk == NB: no boundary (keep u < RANGE)
  int tickets[2];
  int pad[3];
};
static_assert(NT == samp::NT, "samp_scan and samp_ticket run with the sampler's workgroup size");
static_assert(sizeof(TRow) % 16 == 0, "TRow rows stay 16-byte aligned");
}  // namespace spec

int spec_block_words() { return sizeof(spec::Block) / 4; }
size_t spec_trow_bytes() { return sizeof(spec::TRow); }

// chunks per row: ~2 workgroups per CU over all target rows, >= 2048 logits per chunk.
// spec_parts, spec_ws_bytes and sizeof(spec::TRow) have a Python copy (spec_ws_need and
// SPEC_TROW in xgserve/ops/sampling.py: the workspace cap also guards the CPU path and the
// engine's start-up check); tests/test_spec_trunc_cpu.py holds the two equal. Change both.
int spec_parts(int Lp, int V) {
  int P = std::max(1, std::min(spec::PMAX, (512 + Lp - 1) / std::max(1, Lp)));
  return std::max(1, std::min(P, (V + 2047) / 2048));
}

// workspace: draw [Lp][P][2] float4 | stats [Lp + Lq][P] float2 | rowz [Lp] float2, and with
// nT > 0 truncated logical rows: (16-B aligned) rowt [Lp] float4 | trow [nT] TRow | kept [nT][P] float
static size_t spec_ws_base(int Lp, int Lq, size_t P) {
  return static_cast<size_t>(Lp) * P * 32 + (static_cast<size_t>(Lp) + Lq) * P * 8 + static_cast<size_t>(Lp) * 8;
}
size_t spec_ws_bytes(int Lp, int Lq, int V, int nT) {
  const size_t P = spec_parts(Lp, V);
  const size_t base = spec_ws_base(Lp, Lq, P);
  if (nT <= 0) return base;
  return ((base + 15) & ~size_t(15)) + static_cast<size_t>(Lp) * 16 + static_cast<size_t>(nT) * sizeof(spec::TRow) +
         static_cast<size_t>(nT) * P * 4;
}

__device__ __forceinline__ uint32_t spec_stream_key(uint64_t seed, uint32_t step) {
  return hash32(static_cast<uint32_t>(seed) ^ hash32(static_cast<uint32_t>(seed >> 32) + 0x85ebca6bU) ^
                hash32(step * 0x27d4eb2fU + 0x165667b1U));
}

// 23 bits: n + 0.5 is exact in fp32, so u stays inside [2^-24, 1 - 2^-24]
__device__ __forceinline__ float spec_uniform(uint32_t key, int i) {
  const uint32_t hsh = hash32(key ^ hash32(static_cast<uint32_t>(i) * 0x9E3779B9U));
  return (static_cast<float>(hsh >> 9) + 0.5f) * (1.f / 8388608.f);
}

__device__ __forceinline__ void spec_chunk(int V, int P, int p, int& lo, int& hi) {
  const int per = ((V + P - 1) / P + 7) & ~7;
  lo = min(V, p * per);
  hi = min(V, lo + per);
}

// f(i, x0, x1) over [lo, hi) of one (NR = 1: x1 = 0) or two rows, each thread in
// increasing i. 16-B vectors when every row's chunk start is 16-B aligned, else scalar
// loads; all loads of a batch are issued before any is used.
template <typename T, int NR, class F>
__device__ __forceinline__ void spec_visit(const T* r0, const T* r1, int lo, int hi, F f) {
  constexpr int W = VecW<T>::W, U = NR == 1 ? 8 : 4;
  const T* b0 = r0 + lo;
  const T* b1 = r1 + lo;
  const bool vec = ((reinterpret_cast<uintptr_t>(b0) | (NR == 2 ? reinterpret_cast<uintptr_t>(b1) : 0)) & 15) == 0;
  int done = lo;
  if (vec) {
    const int nvec = (hi - lo) / W;
    for (int v0 = static_cast<int>(threadIdx.x); v0 < nvec; v0 += U * spec::NT) {
      uint4 ra[U], rb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t o = static_cast<int64_t>(min(v0 + u * spec::NT, nvec - 1)) * W;
        ra[u] = ld16(b0 + o);
        if constexpr (NR == 2) rb[u] = ld16(b1 + o);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int vi = v0 + u * spec::NT;
        if (vi >= nvec) break;
        float fa[8], fb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (W == 8) {
          unpack8(ra[u], fa);
          if constexpr (NR == 2) unpack8(rb[u], fb);
        } else {
          fa[0] = __uint_as_float(ra[u].x); fa[1] = __uint_as_float(ra[u].y);
          fa[2] = __uint_as_float(ra[u].z); fa[3] = __uint_as_float(ra[u].w);
          if constexpr (NR == 2) {
            fb[0] = __uint_as_float(rb[u].x); fb[1] = __uint_as_float(rb[u].y);
            fb[2] = __uint_as_float(rb[u].z); fb[3] = __uint_as_float(rb[u].w);
          }
        }
#pragma unroll
        for (int k = 0; k < W; ++k) f(lo + vi * W + k, fa[k], fb[k]);
      }
    }
    done = lo + nvec * W;
  }
  for (int i0 = done + static_cast<int>(threadIdx.x); i0 < hi; i0 += U * spec::NT) {
    float va[U], vb[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int i = min(i0 + j * spec::NT, hi - 1);
      va[j] = scalar_at<T>(r0, i);
      vb[j] = NR == 2 ? scalar_at<T>(r1, i) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (i0 + j * spec::NT < hi) f(i0 + j * spec::NT, va[j], vb[j]);
  }
}

__device__ __forceinline__ void spec_lse_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mn));
  m = mn;
}

struct SpecArgs {
  const void* p_logits;
  const void* q_logits;
  int64_t ps, qs;
  int V, P, Lp, Lq, nb;
  const spec::Block* blk;
  const int32_t* rmap;  // logical target rows [0, Lp), then logical draft rows: the block
  const uint64_t* seeds;
  const int32_t* draft;
  float4* draw;
  float2* stats;
  float2* rowz;
  int32_t* out_tok;
  float* out_lp;
  int32_t* accepted;
};
// what the kernels of a launch with truncated blocks get on top (the three kernels of a
// launch without one keep the arguments they had)
struct SpecTArgs : SpecArgs {
  int nT;               // truncated logical rows
  float4* rowt;         // [Lp] (logZ'_p, logZ'_q, M_p, M_q) of a truncated block's positions
  spec::TRow* trow;     // [nT]
  float* kept;          // [nT][P] sum over the chunk's kept tokens of exp(y - M)
};
template <bool TR> using SpecArgsOf = std::conditional_t<TR, SpecTArgs, SpecArgs>;

__device__ __forceinline__ bool spec_truncated(const spec::Block& b, int V) {
  return b.top_p < 1.f || (b.top_k > 0 && b.top_k < V);
}

// the TRow of a truncated block's target row i (target) or draft row i; nullptr: outside
// the workspace (the binding has checked trow0 on the host)
__device__ __forceinline__ spec::TRow* spec_trow(const SpecTArgs& a, const spec::Block& b, bool target, int i) {
  const int t = b.trow0 + (target ? i : b.k + 1 + i);
  return t >= 0 && t < a.nT ? a.trow + t : nullptr;
}

// K1: grid (Lp + Lq) * P, row-major. TR: a launch with truncated blocks -- the row's
// workgroups also clear its TRow (histograms, scan results, tickets).
template <typename T, bool TR>
__global__ void __launch_bounds__(spec::NT) spec_stats_kernel(const SpecArgsOf<TR> a) {
  const int R = blockIdx.x / a.P, c = blockIdx.x % a.P;
  const int j = min(max(a.rmap[R], 0), a.nb - 1);
  const spec::Block b = a.blk[j];
  const bool target = R < a.Lp;
  const int i = target ? R - b.lrow0 : R - a.Lp - (b.lrow0 - j);
  if (i < 0 || i > b.k - (target ? 0 : 1)) return;  // a row map that disagrees with the blocks
  const T* row = target ? static_cast<const T*>(a.p_logits) + static_cast<int64_t>(b.p_row0 + i) * a.ps
                        : static_cast<const T*>(a.q_logits) + static_cast<int64_t>(b.q_row0 + i) * a.qs;
  const float it = 1.f / b.temp;
  int lo, hi;
  spec_chunk(a.V, a.P, c, lo, hi);
  if constexpr (TR) {
    spec::TRow* tr = spec_truncated(b, a.V) ? spec_trow(a, b, target, i) : nullptr;
    if (tr != nullptr) {
      uint32_t* w = reinterpret_cast<uint32_t*>(tr);
      for (int x = c * spec::NT + static_cast<int>(threadIdx.x); x < static_cast<int>(sizeof(spec::TRow) / 4);
           x += a.P * spec::NT)
        w[x] = 0u;
    }
  }
  float m = -INFINITY, sv = 0.f;
  spec_visit<T, 1>(row, row, lo, hi, [&](int, float x, float) {
    const float y = scaled_logit(x, it);
    if (y > m) { sv = (m == -INFINITY ? 0.f : sv * __expf(m - y)) + 1.f; m = y; } else { sv += __expf(y - m); }
  });
  __shared__ float rm[spec::NT / 64], rs[spec::NT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) spec_lse_merge(m, sv, __shfl_xor(m, o, 64), __shfl_xor(sv, o, 64));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { rm[wid] = m; rs[wid] = sv; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = -INFINITY, S = 0.f;
    for (int w = 0; w < spec::NT / 64; ++w) spec_lse_merge(M, S, rm[w], rs[w]);
    a.stats[static_cast<int64_t>(R) * a.P + c] = make_float2(M, S);
  }
}

// log Z of a row from its K1 partials, one wave, a fixed butterfly over the chunks
__device__ __forceinline__ float spec_row_mz(const float2* s, int P, int lane, float& M) {
  float m = -INFINITY, sv = 0.f;
  if (lane < P) { const float2 v = s[lane]; m = v.x; sv = v.y; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) spec_lse_merge(m, sv, __shfl_xor(m, o, 64), __shfl_xor(sv, o, 64));
  M = m;
  return m + __logf(sv);
}
__device__ __forceinline__ float spec_row_logz(const float2* s, int P, int lane) {
  float m;
  return spec_row_mz(s, P, lane, m);
}

// ---------------------------------------------------------------- truncated rows
// The kept set of a truncated row once H1 / H2 have run: samp_draw_kernel's rule.
struct SpecKeep {
  bool use_p, use_k;
  int bp, sp, bk, sk;
  float M;
  __device__ __forceinline__ bool has(float y) const {
    return !(y < M) || samp_kept(M - y, use_p, bp, sp, use_k, bk, sk);
  }
};
__device__ __forceinline__ SpecKeep spec_keep(const spec::Block& b, int V, const spec::TRow& r, float M) {
  SpecKeep k;
  k.use_p = b.top_p < 1.f;
  k.use_k = b.top_k > 0 && b.top_k < V;
  k.bp = k.use_p ? r.bp : samp::NB;
  k.bk = k.use_k ? r.bk : samp::NB;
  k.sp = k.bp < samp::NB ? r.sp : 0;
  k.sk = k.bk < samp::NB ? r.sk : 0;
  k.M = M;
  return k;
}

// block, kind and position of logical row R (K1's addressing); false: a row map that
// disagrees with the blocks, or an untruncated block
__device__ __forceinline__ bool spec_trunc_row(const SpecArgs& a, int R, spec::Block& b, bool& target, int& i) {
  const int j = min(max(a.rmap[R], 0), a.nb - 1);
  b = a.blk[j];
  target = R < a.Lp;
  i = target ? R - b.lrow0 : R - a.Lp - (b.lrow0 - j);
  if (i < 0 || i > b.k - (target ? 0 : 1)) return false;
  return spec_truncated(b, a.V);
}

template <typename T>
__device__ __forceinline__ const T* spec_row_ptr(const SpecArgs& a, const spec::Block& b, bool target, int i) {
  return target ? static_cast<const T*>(a.p_logits) + static_cast<int64_t>(b.p_row0 + i) * a.ps
                : static_cast<const T*>(a.q_logits) + static_cast<int64_t>(b.q_row0 + i) * a.qs;
}

// H1 / H2: grid (Lp + Lq) * P as K1; the sampler's histogram level (samp_hist_level) on the
// truncated rows.
template <typename T, int LEVEL>
__global__ void __launch_bounds__(spec::NT) spec_hist_kernel(const SpecTArgs a) {
  const int R = blockIdx.x / a.P, c = blockIdx.x % a.P, P = a.P;
  spec::Block b;
  bool target;
  int i;
  if (!spec_trunc_row(a, R, b, target, i)) return;
  spec::TRow* rp = spec_trow(a, b, target, i);
  if (rp == nullptr) return;
  spec::TRow& r = *rp;
  const float it = 1.f / b.temp;
  const T* row = spec_row_ptr<T>(a, b, target, i);
  int lo, hi;
  spec_chunk(a.V, P, c, lo, hi);
  __shared__ float shz[2];
  samp_hist_level<LEVEL>(
      r, &r.tickets[LEVEL - 1], P, b.top_p < 1.f, b.top_k > 0 && b.top_k < a.V, b.top_p, b.top_k,
      [&](float& M, float& logZ) {  // from the K1 partials, by wave 0
        if (threadIdx.x < 64) {
          float m;
          const float z = spec_row_mz(a.stats + static_cast<int64_t>(R) * P, P, threadIdx.x, m);
          if (threadIdx.x == 0) { shz[0] = m; shz[1] = z; }
        }
        __syncthreads();
        M = shz[0];
        logZ = shz[1];
      },
      [&](auto f) { spec_visit<T, 1>(row, row, lo, hi, [&](int, float x, float) { f(scaled_logit(x, it)); }); });
}

// KZ: grid (Lp + Lq) * P; the chunk's share of a truncated row's kept mass, in units of
// exp(M). Chunks are summed in a fixed order by their readers (spec_row_kept).
template <typename T>
__global__ void __launch_bounds__(spec::NT) spec_kept_kernel(const SpecTArgs a) {
  const int R = blockIdx.x / a.P, c = blockIdx.x % a.P, P = a.P;
  spec::Block b;
  bool target;
  int i;
  if (!spec_trunc_row(a, R, b, target, i)) return;
  const spec::TRow* rp = spec_trow(a, b, target, i);
  if (rp == nullptr) return;
  __shared__ float shm;
  __shared__ float rs[spec::NT / 64];
  if (threadIdx.x < 64) {
    float m;
    spec_row_mz(a.stats + static_cast<int64_t>(R) * P, P, threadIdx.x, m);
    if (threadIdx.x == 0) shm = m;
  }
  __syncthreads();
  const SpecKeep keep = spec_keep(b, a.V, *rp, shm);
  const float it = 1.f / b.temp;
  const T* row = spec_row_ptr<T>(a, b, target, i);
  int lo, hi;
  spec_chunk(a.V, P, c, lo, hi);
  float sv = 0.f;
  spec_visit<T, 1>(row, row, lo, hi, [&](int, float x, float) {
    const float y = scaled_logit(x, it);
    if (keep.has(y)) sv += __expf(y - keep.M);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sv += __shfl_xor(sv, o, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) rs[wid] = sv;
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = 0.f;
    for (int w = 0; w < spec::NT / 64; ++w) S += rs[w];
    a.kept[static_cast<int64_t>(rp - a.trow) * P + c] = S;
  }
}

// log Z' of a truncated row: M + log of its chunks' kept mass, one wave, a fixed butterfly
__device__ __forceinline__ float spec_row_kept(const float* kp, int P, int lane, float M) {
  float sv = lane < P ? kp[lane] : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sv += __shfl_xor(sv, o, 64);
  return M + __logf(sv);
}

// K2: grid (P, Lp). TR: a launch with truncated blocks.
template <typename T, bool TR>
__global__ void __launch_bounds__(spec::NT) spec_draw_kernel(const SpecArgsOf<TR> a) {
  const int r = blockIdx.y, c = blockIdx.x, P = a.P;
  const int j = min(max(a.rmap[r], 0), a.nb - 1);
  const spec::Block b = a.blk[j];
  const int i = r - b.lrow0;
  if (i < 0 || i > b.k) return;
  const bool resid = i < b.k;
  const float it = 1.f / b.temp;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __shared__ float shz[2];
  __shared__ float sht[4];  // truncated block: logZ'_p, logZ'_q, M_p, M_q
  bool trunc = false;
  const spec::TRow* tp = nullptr;
  const spec::TRow* tq = nullptr;
  if constexpr (TR) {
    if (spec_truncated(b, a.V)) {
      tp = spec_trow(a, b, true, i);
      tq = resid ? spec_trow(a, b, false, i) : tp;
      trunc = tp != nullptr && tq != nullptr;
    }
  }
  if (wid == 0) {
    float m;
    const float z = spec_row_mz(a.stats + static_cast<int64_t>(r) * P, P, lane, m);
    if (lane == 0) shz[0] = z;
    if constexpr (TR) {
      if (trunc) {
        const float zt = spec_row_kept(a.kept + static_cast<int64_t>(tp - a.trow) * P, P, lane, m);
        if (lane == 0) { sht[0] = zt; sht[2] = m; }
      }
    }
  } else if (wid == 1 && resid) {
    float m;
    const float z = spec_row_mz(a.stats + static_cast<int64_t>(a.Lp + b.lrow0 - j + i) * P, P, lane, m);
    if (lane == 0) shz[1] = z;
    if constexpr (TR) {
      if (trunc) {
        const float zt = spec_row_kept(a.kept + static_cast<int64_t>(tq - a.trow) * P, P, lane, m);
        if (lane == 0) { sht[1] = zt; sht[3] = m; }
      }
    }
  }
  __syncthreads();
  const float zp = shz[0], zq = resid ? shz[1] : 0.f;
  const uint32_t key = spec_stream_key(a.seeds[r], 2u);
  float bv = -INFINITY, bl = -INFINITY, av = -INFINITY;
  int bi = 0x7fffffff, ai = 0x7fffffff;
  int lo, hi;
  spec_chunk(a.V, P, c, lo, hi);
  const T* pr = static_cast<const T*>(a.p_logits) + static_cast<int64_t>(b.p_row0 + i) * a.ps;
  if (trunc) {
    const float ztp = sht[0], ztq = resid ? sht[1] : 0.f;
    const SpecKeep kp = spec_keep(b, a.V, *tp, sht[2]);
    if (resid) {
      const SpecKeep kq = spec_keep(b, a.V, *tq, sht[3]);
      const T* qr = static_cast<const T*>(a.q_logits) + static_cast<int64_t>(b.q_row0 + i) * a.qs;
      spec_visit<T, 2>(pr, qr, lo, hi, [&](int x, float xp, float xq) {
        const float yp = scaled_logit(xp, it);
        if (yp > av) { av = yp; ai = x; }
        if (!kp.has(yp)) return;  // p'(x) = 0, before any arithmetic on lp'
        const float lp = yp - ztp;
        if (lp + spec::GMAX < bv) return;  // as below: exact
        float wl = lp;  // off K_q: q'(x) = 0, the weight is p'(x)
        const float yq = scaled_logit(xq, it);
        if (kq.has(yq)) {
          const float lq = yq - ztq;
          if (!(lp > lq)) return;  // weight 0
          wl = lp + __logf(-expm1f(lq - lp));
        }
        const float score = wl - __logf(-__logf(spec_uniform(key, x)));
        if (score > bv) { bv = score; bi = x; bl = yp - zp; }
      });
    } else {
      spec_visit<T, 1>(pr, pr, lo, hi, [&](int x, float xp, float) {
        const float yp = scaled_logit(xp, it);
        if (yp + spec::GMAX < bv) return;
        if (!kp.has(yp)) return;
        const float score = yp - __logf(-__logf(spec_uniform(key, x)));
        if (score > bv) { bv = score; bi = x; bl = yp - zp; }
      });
    }
  } else if (resid) {
    const T* qr = static_cast<const T*>(a.q_logits) + static_cast<int64_t>(b.q_row0 + i) * a.qs;
    spec_visit<T, 2>(pr, qr, lo, hi, [&](int x, float xp, float xq) {
      const float yp = scaled_logit(xp, it);
      if (yp > av) { av = yp; ai = x; }
      const float lp = yp - zp;
      // the weight's log is <= lp and the noise < GMAX: the token cannot win (exact)
      if (lp + spec::GMAX < bv) return;
      const float lq = scaled_logit(xq, it) - zq;
      if (!(lp > lq)) return;  // weight 0
      const float wl = lp + __logf(-expm1f(lq - lp));
      const float score = wl - __logf(-__logf(spec_uniform(key, x)));
      if (score > bv) { bv = score; bi = x; bl = lp; }
    });
  } else {
    spec_visit<T, 1>(pr, pr, lo, hi, [&](int x, float xp, float) {
      const float yp = scaled_logit(xp, it);
      if (yp + spec::GMAX < bv) return;
      const float score = yp - __logf(-__logf(spec_uniform(key, x)));
      if (score > bv) { bv = score; bi = x; bl = yp - zp; }
    });
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, 64), l2 = __shfl_xor(bl, o, 64), a2 = __shfl_xor(av, o, 64);
    const int i2 = __shfl_xor(bi, o, 64), j2 = __shfl_xor(ai, o, 64);
    if (v2 > bv || (v2 == bv && i2 < bi)) { bv = v2; bi = i2; bl = l2; }
    if (a2 > av || (a2 == av && j2 < ai)) { av = a2; ai = j2; }
  }
  __shared__ float rv[spec::NT / 64], rl[spec::NT / 64], ra[spec::NT / 64];
  __shared__ int ri[spec::NT / 64], rj[spec::NT / 64];
  if (lane == 0) { rv[wid] = bv; ri[wid] = bi; rl[wid] = bl; ra[wid] = av; rj[wid] = ai; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < spec::NT / 64; ++w) {
      if (rv[w] > rv[0] || (rv[w] == rv[0] && ri[w] < ri[0])) { rv[0] = rv[w]; ri[0] = ri[w]; rl[0] = rl[w]; }
      if (ra[w] > ra[0] || (ra[w] == ra[0] && rj[w] < rj[0])) { ra[0] = ra[w]; rj[0] = rj[w]; }
    }
    float4* d = a.draw + (static_cast<int64_t>(r) * P + c) * 2;
    d[0] = make_float4(rv[0], __int_as_float(ri[0]), rl[0], 0.f);
    d[1] = make_float4(ra[0], __int_as_float(rj[0]), 0.f, 0.f);
    if (c == 0) {
      a.rowz[r] = make_float2(zp, zq);
      if constexpr (TR) {
        if (trunc) a.rowt[r] = make_float4(sht[0], resid ? sht[1] : 0.f, sht[2], resid ? sht[3] : 0.f);
      }
    }
  }
}

// K3: one wave per block. TR: a launch with truncated blocks.
template <typename T, bool TR>
__global__ void __launch_bounds__(64) spec_select_kernel(const SpecArgsOf<TR> a) {
  const int j = blockIdx.x, lane = threadIdx.x, P = a.P;
  const spec::Block b = a.blk[j];
  const float it = 1.f / b.temp;
  bool trunc = false;
  if constexpr (TR) trunc = spec_truncated(b, a.V) && b.trow0 >= 0 && b.trow0 + 2 * b.k + 1 <= a.nT;
  int acc = b.k;
  for (int i = 0; i <= b.k; ++i) {
    const int r = b.lrow0 + i, orow = b.out_row0 + i;
    const float2 z = a.rowz[r];
    if (i < b.k) {
      const int d = a.draft[b.d_off + i];
      bool ok = false;
      float lpd = -INFINITY;
      if (d >= 0 && d < a.V) {  // a token outside the vocabulary is rejected, never read
        const T* pr = static_cast<const T*>(a.p_logits) + static_cast<int64_t>(b.p_row0 + i) * a.ps;
        const T* qr = static_cast<const T*>(a.q_logits) + static_cast<int64_t>(b.q_row0 + i) * a.qs;
        if constexpr (TR) {
          if (trunc) {
            const float4 zt = a.rowt[r];
            const float yp = scaled_logit(scalar_at<T>(pr, d), it), yq = scaled_logit(scalar_at<T>(qr, d), it);
            lpd = yp - z.x;  // the logprob stays that of the whole row
            if (!spec_keep(b, a.V, a.trow[b.trow0 + i], zt.z).has(yp)) {
              ok = false;  // p'(d) = 0
            } else if (!spec_keep(b, a.V, a.trow[b.trow0 + b.k + 1 + i], zt.w).has(yq)) {
              ok = true;   // q'(d) = 0 < p'(d): see the head of the file
            } else {
              ok = __logf(spec_uniform(spec_stream_key(a.seeds[r], 1u), 0)) + (yq - zt.y) <= yp - zt.x;
            }
          }
        }
        if (!trunc) {
          lpd = scaled_logit(scalar_at<T>(pr, d), it) - z.x;
          const float lqd = scaled_logit(scalar_at<T>(qr, d), it) - z.y;
          ok = __logf(spec_uniform(spec_stream_key(a.seeds[r], 1u), 0)) + lqd <= lpd;
        }
      }
      if (ok) {
        if (lane == 0) { a.out_tok[orow] = d; a.out_lp[orow] = lpd; }
        continue;
      }
      acc = i;
    }
    // the chunk winners of position i: max score, lowest index
    const float4* dr = a.draw + static_cast<int64_t>(r) * P * 2;
    float v = -INFINITY, l = -INFINITY;
    int idx = 0x7fffffff;
    if (lane < P) { const float4 w = dr[lane * 2]; v = w.x; idx = __float_as_int(w.y); l = w.z; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(v, o, 64), l2 = __shfl_xor(l, o, 64);
      const int i2 = __shfl_xor(idx, o, 64);
      if (v2 > v || (v2 == v && i2 < idx)) { v = v2; idx = i2; l = l2; }
    }
    if (i < b.k && v == -INFINITY) {  // no token with p > q: the row's p-argmax
      float y = -INFINITY;
      idx = 0x7fffffff;
      if (lane < P) { const float4 w = dr[lane * 2 + 1]; y = w.x; idx = __float_as_int(w.y); }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float y2 = __shfl_xor(y, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        if (y2 > y || (y2 == y && i2 < idx)) { y = y2; idx = i2; }
      }
      l = y - z.x;
    }
    if (static_cast<unsigned>(idx) >= static_cast<unsigned>(a.V)) idx = 0;  // a row without one finite logit
    if (lane == 0) { a.out_tok[orow] = idx; a.out_lp[orow] = l; }
    break;
  }
  if (lane == 0) a.accepted[j] = acc;
}

template <typename T>
static void launch_spec(const SpecTArgs& a, hipStream_t st) {
  const dim3 rows((a.Lp + a.Lq) * a.P), nt(spec::NT);
  if (a.nT > 0) {
    hipLaunchKernelGGL((spec_stats_kernel<T, true>), rows, nt, 0, st, a);
    hipLaunchKernelGGL((spec_hist_kernel<T, 1>), rows, nt, 0, st, a);
    hipLaunchKernelGGL((spec_hist_kernel<T, 2>), rows, nt, 0, st, a);
    hipLaunchKernelGGL(spec_kept_kernel<T>, rows, nt, 0, st, a);
    hipLaunchKernelGGL((spec_draw_kernel<T, true>), dim3(a.P, a.Lp), nt, 0, st, a);
    hipLaunchKernelGGL((spec_select_kernel<T, true>), dim3(a.nb), dim3(64), 0, st, a);
    return;
  }
  const SpecArgs& u = a;
  hipLaunchKernelGGL((spec_stats_kernel<T, false>), rows, nt, 0, st, u);
  hipLaunchKernelGGL((spec_draw_kernel<T, false>), dim3(a.P, a.Lp), nt, 0, st, u);
  hipLaunchKernelGGL((spec_select_kernel<T, false>), dim3(a.nb), dim3(64), 0, st, u);
}

// blk: nb descriptors (spec::Block); rmap: int32 [Lp + Lq], the block of every logical
// target row, then of every logical draft row; seeds: [Lp]; nT: the TRows of the truncated
// blocks (sum of 2 k + 1 over them, 0: no block is truncated); ws: spec_ws_bytes(Lp, Lq, V,
// nT), 16-B aligned, any content. The caller has checked every index on the host (ops.cpp).
void spec_verify_sample(const void* p_logits, int64_t ps, const void* q_logits, int64_t qs, int is_f32, int V, int nb,
                        int Lp, int Lq, int nT, const void* blk, const int32_t* rmap, const uint64_t* seeds,
                        const int32_t* draft, int32_t* out_tok, float* out_lp, int32_t* accepted, void* ws,
                        hipStream_t st) {
  if (nb <= 0) return;
  SpecTArgs a;
  a.p_logits = p_logits; a.q_logits = q_logits; a.ps = ps; a.qs = qs;
  a.V = V; a.P = spec_parts(Lp, V); a.Lp = Lp; a.Lq = Lq; a.nb = nb;
  a.blk = static_cast<const spec::Block*>(blk); a.rmap = rmap; a.seeds = seeds; a.draft = draft;
  char* w = static_cast<char*>(ws);
  a.draw = reinterpret_cast<float4*>(w);
  w += static_cast<size_t>(Lp) * a.P * 32;
  a.stats = reinterpret_cast<float2*>(w);
  w += (static_cast<size_t>(Lp) + Lq) * a.P * 8;
  a.rowz = reinterpret_cast<float2*>(w);
  a.nT = std::max(nT, 0); a.rowt = nullptr; a.trow = nullptr; a.kept = nullptr;
  if (a.nT > 0) {
    w = static_cast<char*>(ws) + ((spec_ws_base(Lp, Lq, a.P) + 15) & ~size_t(15));
    a.rowt = reinterpret_cast<float4*>(w);
    w += static_cast<size_t>(Lp) * 16;
    a.trow = reinterpret_cast<spec::TRow*>(w);
    w += static_cast<size_t>(a.nT) * sizeof(spec::TRow);
    a.kept = reinterpret_cast<float*>(w);
  }
  a.out_tok = out_tok; a.out_lp = out_lp; a.accepted = accepted;
  if (is_f32) launch_spec<float>(a, st); else launch_spec<uint16_t>(a, st);
}

}  // namespace xgk
