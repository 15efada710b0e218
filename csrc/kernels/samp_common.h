// What the samplers (sampling.hip) and the speculative verify kernels (spec_sample.hip)
// share: the counter hash behind every draw, the per-element-type row readers, and the
// split-row sampler's top-p / top-k machinery (bin arithmetic, kept-set rule, histogram
// level, scan, row ticket) -- one copy, so a token the draft sampler kept is a token the verify
// kernels keep. The written contract of the hash is tests/test_sampling_gpu.py.
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

// The split-row sampler's geometry (sampling.hip "sample v2"), shared with the truncated
// verify kernels of spec_sample.hip: both must put a token into the same (bin, sub-bin).
namespace samp {
constexpr int NT = 256;       // threads per workgroup
constexpr int NB = 1024;      // bins per histogram level
constexpr int PMAX = 64;      // workgroups per row
constexpr float RANGE = 40.f; // u beyond this is never kept by top-p / top-k
constexpr float FIX = 1099511627776.f;  // 2^40: fixed-point probability mass

}  // namespace samp

// Row ticket (see gemm_m64g.hip agent_ticket): drain, one relaxed agent-scope add;
// the winner acquires before reading what the other workgroups published.
__device__ __forceinline__ bool samp_ticket(int* cnt, int last_value) {
  __shared__ int flag;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int prev = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == last_value;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    flag = last;
  }
  __syncthreads();
  return flag != 0;
}

// First bin (in order) where base + cumulative mass reaches `target` (or NB) and first
// bin where base + cumulative count exceeds `kmax` (or NB), with the exclusive prefix
// at those bins. Run by a whole workgroup over global histograms h_m / h_c, which it
// re-zeroes.
__device__ inline void samp_scan(unsigned long long* h_m, unsigned int* h_c, bool do_p, unsigned long long target,
                          bool do_k, long long kmax, int& bin_p, unsigned long long& before_p, int& bin_k,
                          long long& before_k) {
  constexpr int PER = samp::NB / samp::NT;
  __shared__ unsigned long long sm[samp::NT];
  __shared__ long long sc[samp::NT];
  __shared__ int best_p, best_k;
  const int t = threadIdx.x;
  unsigned long long lm[PER];
  unsigned int lc[PER];
  unsigned long long tm = 0;
  long long tc = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    lm[j] = do_p ? __hip_atomic_load(h_m + t * PER + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    lc[j] = do_k ? __hip_atomic_load(h_c + t * PER + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    tm += lm[j];
    tc += lc[j];
  }
  if (t == 0) { best_p = samp::NB; best_k = samp::NB; }
  sm[t] = tm;
  sc[t] = tc;
  __syncthreads();
  for (int o = 1; o < samp::NT; o <<= 1) {  // inclusive Hillis-Steele scan
    const unsigned long long am = t >= o ? sm[t - o] : 0ull;
    const long long ac = t >= o ? sc[t - o] : 0ll;
    __syncthreads();
    sm[t] += am;
    sc[t] += ac;
    __syncthreads();
  }
  unsigned long long cm = sm[t] - tm;  // exclusive
  long long cc = sc[t] - tc;
  int fp = samp::NB, fk = samp::NB;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (fp == samp::NB && cm + lm[j] >= target) fp = t * PER + j;
    if (fk == samp::NB && cc + lc[j] > kmax) fk = t * PER + j;
    if (fp == samp::NB) cm += lm[j];
    if (fk == samp::NB) cc += lc[j];
  }
  if (do_p && fp < samp::NB) atomicMin(&best_p, fp);
  if (do_k && fk < samp::NB) atomicMin(&best_k, fk);
  __syncthreads();
  bin_p = best_p;
  bin_k = best_k;
  // the owners of the boundary bins publish the exclusive prefixes
  __shared__ unsigned long long bp_before;
  __shared__ long long bk_before;
  if (do_p && fp == best_p && fp < samp::NB) bp_before = cm;
  if (do_k && fk == best_k && fk < samp::NB) bk_before = cc;
  __syncthreads();
  before_p = bin_p < samp::NB ? bp_before : 0ull;
  before_k = bin_k < samp::NB ? bk_before : 0ll;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (do_p) h_m[t * PER + j] = 0ull;
    if (do_k) h_c[t * PER + j] = 0u;
  }
}

// level-1 bin of u = M - y (>= NB: outside the range) and the sub-bin within it
__device__ __forceinline__ int samp_bin(float u, int& sub) {
  const float tt = u * (samp::NB / samp::RANGE);
  const int b = tt < static_cast<float>(samp::NB) ? static_cast<int>(tt) : samp::NB;
  sub = min(samp::NB - 1, max(0, static_cast<int>((tt - static_cast<float>(b)) * samp::NB)));
  return b;
}

// The kept-set rule for a token below the row maximum, u = M - y > 0 (the maximum itself
// is always kept): inside the range, at or before the top-p boundary (bp, sp) and before
// the top-k boundary (bk, sk); bp / bk == NB: that boundary does not exist.
__device__ __forceinline__ bool samp_kept(float u, bool use_p, int bp, int sp, bool use_k, int bk, int sk) {
  int sub;
  const int bin = samp_bin(u, sub);
  if (bin >= samp::NB) return false;
  if (use_p && bp < samp::NB && (bin > bp || (bin == bp && sub > sp))) return false;
  if (use_k && bk < samp::NB && (bin > bk || (bin == bk && sub >= sk))) return false;
  return true;
}

// One histogram level of one row, run by every workgroup of the row (samp_hist_kernel of
// sampling.hip and spec_hist_kernel of spec_sample.hip are this function with their own row
// addressing): LEVEL 1 bins u = M - y over [0, RANGE), LEVEL 2 the sub-bins of the two
// boundary bins; fixed-point mass exp(y - logZ) * FIX and counts, per chunk in LDS, added to
// the row's global histogram with atomics; the row's last workgroup (ticket) scans it,
// stores the boundaries into the row and re-zeroes the histogram. Row: h1m / h1c / h2m /
// h2c [NB], mass_before_p, bp, bk, cnt_before_k, sp, sk. stats(M, logZ): the row's maximum
// and log Z, in every thread; visit(f): f(y) for every y of this workgroup's chunk.
template <int LEVEL, class Row, class Stats, class Visit>
__device__ __forceinline__ void samp_hist_level(Row& r, int* ticket, int P, bool use_p, bool use_k, float top_p,
                                                int top_k, Stats stats, Visit visit) {
  const bool do_p = use_p && (LEVEL == 1 || r.bp < samp::NB);
  const bool do_k = use_k && (LEVEL == 1 || r.bk < samp::NB);
  if (!do_p && !do_k) return;  // uniform per row: no workgroup of it takes a ticket
  const int bp = LEVEL == 2 ? r.bp : 0, bk = LEVEL == 2 ? r.bk : 0;
  float M, logZ;
  stats(M, logZ);
  __shared__ unsigned long long hm[samp::NB];
  __shared__ unsigned int hc[samp::NB];
  for (int i = threadIdx.x; i < samp::NB; i += samp::NT) { hm[i] = 0ull; hc[i] = 0u; }
  __syncthreads();
  visit([&](float y) {
    int sub;
    const int bin = samp_bin(M - y, sub);
    if (bin >= samp::NB) return;
    if (LEVEL == 1) {
      if (do_p) atomicAdd(&hm[bin], static_cast<unsigned long long>(__expf(y - logZ) * samp::FIX));
      if (do_k) atomicAdd(&hc[bin], 1u);
    } else {
      if (do_p && bin == bp) atomicAdd(&hm[sub], static_cast<unsigned long long>(__expf(y - logZ) * samp::FIX));
      if (do_k && bin == bk) atomicAdd(&hc[sub], 1u);
    }
  });
  __syncthreads();
  unsigned long long* gm = LEVEL == 1 ? r.h1m : r.h2m;
  unsigned int* gc = LEVEL == 1 ? r.h1c : r.h2c;
  for (int i = threadIdx.x; i < samp::NB; i += samp::NT) {
    if (do_p && hm[i]) atomicAdd(gm + i, hm[i]);
    if (do_k && hc[i]) atomicAdd(gc + i, hc[i]);
  }
  if (!samp_ticket(ticket, P - 1)) return;
  const unsigned long long target = static_cast<unsigned long long>(static_cast<double>(top_p) * samp::FIX);
  const unsigned long long base_p = LEVEL == 1 ? 0ull : r.mass_before_p;
  const long long base_k = LEVEL == 1 ? 0ll : r.cnt_before_k;
  int fp, fk;
  unsigned long long bef_p;
  long long bef_k;
  samp_scan(gm, gc, do_p, target > base_p ? target - base_p : 0ull, do_k, top_k - base_k, fp, bef_p, fk, bef_k);
  if (threadIdx.x == 0) {
    if (LEVEL == 1) {
      r.bp = use_p ? fp : samp::NB;
      r.bk = use_k ? fk : samp::NB;
      r.mass_before_p = bef_p;
      r.cnt_before_k = static_cast<int>(bef_k);
    } else {
      r.sp = do_p ? (fp < samp::NB ? fp : samp::NB - 1) : 0;  // sub-bins <= sp kept
      r.sk = do_k ? fk : 0;                                   // sub-bins < sk kept
    }
  }
}

}  // namespace xgk
