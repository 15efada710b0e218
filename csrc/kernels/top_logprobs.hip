// K9c: the top-K tokens of a logits row and their log-probabilities.
//
// For each asked row: y = scaled_logit(x, 1 / T) (y = x on a greedy row), lp = y - logZ with
// logZ over the whole row -- the distribution the samplers' per-token logprob refers to.
// Order: y descending, equal y to the lower token id (ArgLse::merge's rule, so entry 0 of a
// greedy row is argmax_logprob's token). -inf logits are never listed; slots past the last
// finite entry hold id -1 and lp -inf.
//
// One pass over the row. An element is a 64-bit key (order-preserving bits of y << 32 |
// ~id): keys are unique, a larger key is a better entry, and ties need no special case.
// A workgroup of 256 threads walks its slice one 16-B vector per thread at a time (8 loads
// in flight); a thread appends a key to the LDS candidate buffer only if it beats the
// running bound, the K-th best key seen so far. When the buffer passes TL_TRIG entries it is
// compacted to its best K and the bound raised (tl_compact: a threshold from the per-thread
// maxima cuts the buffer to a short list, whose keys find their places by counting -- no
// sort, no per-thread K-entry array, cost independent of K). The first step therefore
// costs one compaction; after it random data passes a few keys per step. An ascending row
// passes everything and compacts every step.
// Alongside, every thread keeps an online (max, sum exp) of its elements.
//
// V >= ARGMAX_SPLIT_MIN_V (the caller's choice, by passing a workspace): TL_PARTS
// workgroups per row, as argmax_split_kernel -- a slice's K winners and its (max, sum) go to
// the workspace write-through, a per-row ticket elects the last arriver, which merges the
// slices in slice order, writes the row's lists and re-arms the ticket.
#include "glds.h"

namespace xgk {

constexpr int TOPLP_MAX = 20;
constexpr int TL_NT = 256;
constexpr int TL_PARTS = 8;
constexpr int TL_U = 8;                          // 16-B loads in flight per thread
constexpr int TL_STEP = TL_NT * 8;               // most keys one step can append (bf16: 8 per thread)
constexpr int TL_TRIG = 1024;                    // compact once the buffer holds more
constexpr int TL_CAP = TL_TRIG + TL_STEP;        // 3072 keys = 24 KB of LDS
constexpr int TL_E = TL_CAP / TL_NT;             // keys per thread in a compaction
constexpr int TL_SLOT = TOPLP_MAX + 2;           // workspace u64 per (row, slice): K keys | (m, s) | pad

typedef unsigned long long tl_key;

__device__ __forceinline__ tl_key tl_make_key(float y, int id) {
  y += 0.f;  // -0 -> +0: equal values, equal bits
  uint32_t u = __float_as_uint(y);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return (static_cast<tl_key>(u) << 32) | (0xffffffffu - static_cast<uint32_t>(id));
}
__device__ __forceinline__ float tl_key_y(tl_key k) {
  uint32_t u = static_cast<uint32_t>(k >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
  return __uint_as_float(u);
}
__device__ __forceinline__ int tl_key_id(tl_key k) { return static_cast<int>(0xffffffffu - static_cast<uint32_t>(k)); }

struct TlShared {
  tl_key buf[TL_CAP];
  tl_key tmax[TL_NT];    // a compaction's per-thread maxima
  tl_key small[TL_NT];   // its short list: the keys that may be among the best K
  tl_key thr;
  tl_key bound;   // a key must beat this to be appended (0: fewer than K so far)
  int cnt;        // keys in buf
  int nsmall;
  float red_m[TL_NT / 64], red_s[TL_NT / 64];
  float logz;
  int flag;
};

// number of keys in a[0, n) above `my`. Every lane reads the same address (an LDS
// broadcast) and the reads do not depend on each other, so the loop runs at issue rate.
__device__ __forceinline__ int tl_rank(const tl_key* a, int n, tl_key my) {
  int r = 0;
#pragma unroll 8
  for (int j = 0; j < n; ++j) r += a[j] > my;
  return r;
}

// sh.small[0, n) (n <= TL_NT, zero keys are "none") -> its best K keys, descending, in
// sh.buf[0, ..); sets sh.cnt and sh.bound. Keys are unique, so a key's rank is its place.
// Whole workgroup, n uniform.
__device__ __forceinline__ void tl_rank_select(TlShared& sh, int n, int K) {
  const int tid = threadIdx.x;
  const tl_key my = tid < n ? sh.small[tid] : 0ull;
  if (tid == 0) sh.bound = 0ull;
  const int nnz = __syncthreads_count(my != 0ull);  // also: buf is no longer read by anyone
  if (my != 0ull) {
    const int r = tl_rank(sh.small, n, my);
    if (r < K) sh.buf[r] = my;
    // the K-th best itself stays in the buffer, so only a better key is appended
    if (r == K - 1) sh.bound = my;
  }
  if (tid == 0) sh.cnt = min(nnz, K);
  __syncthreads();
}

// buf[0, cnt) -> its best min(cnt, K) keys, descending, in buf[0, ..); sets sh.cnt and
// sh.bound. Whole workgroup, cnt uniform and <= TL_CAP; zero keys are "none".
// No sort and no K-entry list per thread: the K-th largest of the 256 per-thread maxima is
// a lower bound of the K-th largest key, and only the K threads whose maximum reaches it
// hold keys above it -- at most K * TL_E = 240 <= TL_NT keys, one per thread of the short
// list, each of which then finds its place by counting the keys above it.
__device__ __forceinline__ void tl_compact(TlShared& sh, int cnt, int K) {
  static_assert(TOPLP_MAX * TL_E <= TL_NT && TL_PARTS * TOPLP_MAX <= TL_NT, "the short list is one key per thread");
  const int tid = threadIdx.x;
  if (cnt <= TL_NT) {  // already a short list (a slice's last compaction, as a rule)
    sh.small[tid] = tid < cnt ? sh.buf[tid] : 0ull;
    __syncthreads();
    tl_rank_select(sh, cnt, K);
    return;
  }
  tl_key r[TL_E];
  tl_key tm = 0ull;
#pragma unroll
  for (int e = 0; e < TL_E; ++e) {
    r[e] = (e * TL_NT + tid < cnt) ? sh.buf[e * TL_NT + tid] : 0ull;
    tm = r[e] > tm ? r[e] : tm;
  }
  sh.tmax[tid] = tm;
  if (tid == 0) { sh.thr = 0ull; sh.nsmall = 0; }
  __syncthreads();
  // thr: the K-th largest maximum (0 if fewer than K threads hold a key)
  if (tm != 0ull && tl_rank(sh.tmax, TL_NT, tm) == K - 1) sh.thr = tm;
  __syncthreads();
  const tl_key thr = sh.thr;
  if (tm >= thr && tm != 0ull) {
#pragma unroll
    for (int e = 0; e < TL_E; ++e)
      if (r[e] >= thr && r[e] != 0ull) sh.small[atomicAdd(&sh.nsmall, 1)] = r[e];
  }
  __syncthreads();
  tl_rank_select(sh, sh.nsmall, K);
}

template <typename T> struct TlVec { static constexpr int W = 8; };
template <> struct TlVec<float> { static constexpr int W = 4; };
template <typename T> __device__ __forceinline__ float tl_scalar(const T* p);
template <> __device__ __forceinline__ float tl_scalar<uint16_t>(const uint16_t* p) { return bf2f(*p); }
template <> __device__ __forceinline__ float tl_scalar<float>(const float* p) { return *p; }

// One step: this thread's NW values f[0, nw) (ids id0 ..), `ok` false for a thread past the
// slice's end. Appends, updates (m, s), compacts when the buffer is past TL_TRIG. Whole
// workgroup, called the same number of times by every thread.
template <int NW>
__device__ __forceinline__ void tl_step(TlShared& sh, const float* f, int id0, bool ok, float it, int K, float& m,
                                        float& s) {
  const tl_key bound = sh.bound;
  float y[NW];
  float bm = -INFINITY;
  bool over = false;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    y[k] = ok ? scaled_logit(f[k], it) : -INFINITY;
    bm = fmaxf(bm, y[k]);
    if (y[k] != -INFINITY) {
      const tl_key key = tl_make_key(y[k], id0 + k);
      if (key > bound) {
        const int pos = atomicAdd(&sh.cnt, 1);  // < TL_CAP: at most TL_TRIG before a step, TL_STEP appended by it
        sh.buf[pos] = key;
        over |= pos >= TL_TRIG;
      }
    }
  }
  if (bm != -INFINITY) {
    const float mn = fmaxf(m, bm);
    float bs = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) bs += __expf(y[k] - mn);  // exp(-inf) = 0
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + bs;
    m = mn;
  }
  // one barrier per step: it orders this step's appends before the next step's read of the
  // bound, and carries the (uniform) decision to compact
  if (__syncthreads_or(over)) tl_compact(sh, sh.cnt, K);
}

template <typename T>
__global__ void __launch_bounds__(TL_NT) top_logprobs_kernel(const T* __restrict__ logits, int64_t stride,
                                                             int num_rows, int V, const int32_t* __restrict__ rows,
                                                             const float* __restrict__ temps, int K,
                                                             int32_t* __restrict__ out_ids,
                                                             float* __restrict__ out_lps, tl_key* ws, int* tickets) {
  constexpr int W = TlVec<T>::W;
  __shared__ TlShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int P = gridDim.x, part = blockIdx.x, o = blockIdx.y;
  const int r = rows ? rows[o] : o;
  if (r < 0 || r >= num_rows) {  // uniform over the row's workgroups: nobody takes a ticket
    if (part == 0 && tid < K) { out_ids[o * K + tid] = -1; out_lps[o * K + tid] = -INFINITY; }
    return;
  }
  const float temp = temps[r];
  const float it = temp > 0.f ? 1.f / temp : 1.f;
  const T* row = logits + r * stride;
  const int per = ((V + P - 1) / P + 7) & ~7;
  const int lo = min(V, part * per), hi = min(V, lo + per);
  if (tid == 0) { sh.cnt = 0; sh.bound = 0ull; }
  __syncthreads();

  float m = -INFINITY, s = 0.f;
  const T* base = row + lo;
  int done = lo;
  if ((reinterpret_cast<uintptr_t>(base) & 15) == 0) {
    const int nvec = (hi - lo) / W;
    for (int v0 = 0; v0 < nvec; v0 += TL_U * TL_NT) {
      uint4 raw[TL_U];
#pragma unroll
      for (int u = 0; u < TL_U; ++u)
        raw[u] = ld16(base + static_cast<int64_t>(min(v0 + u * TL_NT + tid, nvec - 1)) * W);
#pragma unroll
      for (int u = 0; u < TL_U; ++u) {
        if (v0 + u * TL_NT >= nvec) break;  // uniform
        const int vi = v0 + u * TL_NT + tid;
        float f[8];
        if constexpr (W == 8) {
          unpack8(raw[u], f);
        } else {
          f[0] = __uint_as_float(raw[u].x); f[1] = __uint_as_float(raw[u].y);
          f[2] = __uint_as_float(raw[u].z); f[3] = __uint_as_float(raw[u].w);
        }
        tl_step<W>(sh, f, lo + vi * W, vi < nvec, it, K, m, s);
      }
    }
    done = lo + nvec * W;
  }
  // a slice that does not start 16-B aligned, and the elements past the last full vector
  for (int i0 = done; i0 < hi; i0 += TL_U * TL_NT) {
    float v[TL_U];
#pragma unroll
    for (int u = 0; u < TL_U; ++u) v[u] = tl_scalar<T>(row + min(i0 + u * TL_NT + tid, hi - 1));
#pragma unroll
    for (int u = 0; u < TL_U; ++u) {
      if (i0 + u * TL_NT >= hi) break;  // uniform
      const int i = i0 + u * TL_NT + tid;
      tl_step<1>(sh, &v[u], i, i < hi, it, K, m, s);
    }
  }
  tl_compact(sh, sh.cnt, K);  // buf[0, K): the slice's winners, descending, 0 = none

  // the slice's (max, sum exp)
#pragma unroll
  for (int of = 32; of > 0; of >>= 1) {
    const float m2 = __shfl_xor(m, of, 64), s2 = __shfl_xor(s, of, 64);
    const float mn = fmaxf(m, m2);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mn));
    m = mn;
  }
  if (lane == 0) { sh.red_m[wid] = m; sh.red_s[wid] = s; }
  __syncthreads();
  float M = -INFINITY, S = 0.f;
  for (int w = 0; w < TL_NT / 64; ++w) {
    const float mn = fmaxf(M, sh.red_m[w]);
    S = (M == -INFINITY ? 0.f : S * __expf(M - mn)) + (sh.red_m[w] == -INFINITY ? 0.f : sh.red_s[w] * __expf(sh.red_m[w] - mn));
    M = mn;
  }

  if (P > 1) {
    tl_key* slot = ws + (static_cast<int64_t>(o) * P + part) * TL_SLOT;
    if (tid < TOPLP_MAX) {
      const tl_key k = tid < sh.cnt ? sh.buf[tid] : 0ull;
      st8_sc1(slot + tid, make_uint2(static_cast<uint32_t>(k), static_cast<uint32_t>(k >> 32)));
    } else if (tid == TOPLP_MAX) {
      st8_sc1(slot + TOPLP_MAX, make_uint2(__float_as_uint(M), __float_as_uint(S)));
    }
    // row ticket (sampling.hip samp_ticket): every storing wave drains, one relaxed
    // agent-scope add; the winner acquires before anyone reads the other slices
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const int prev = __hip_atomic_fetch_add(tickets + o, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = prev == P - 1;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(tickets + o, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
      }
      sh.flag = last;
    }
    __syncthreads();
    if (!sh.flag) return;
    tl_key* rs = ws + static_cast<int64_t>(o) * P * TL_SLOT;
    if (tid < P * TOPLP_MAX) {
      const int q = tid / TOPLP_MAX, k = tid % TOPLP_MAX;
      sh.small[tid] = __hip_atomic_load(rs + q * TL_SLOT + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (wid == 1) {  // (max, sum) of the slices, combined in slice order
      const tl_key ms = lane < P ? __hip_atomic_load(rs + lane * TL_SLOT + TOPLP_MAX, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)
                                 : 0ull;
      const float pm = __uint_as_float(static_cast<uint32_t>(ms)), ps = __uint_as_float(static_cast<uint32_t>(ms >> 32));
      M = -INFINITY;
      S = 0.f;
      for (int q = 0; q < P; ++q) {
        const float qm = __shfl(pm, q, 64), qs = __shfl(ps, q, 64);
        const float mn = fmaxf(M, qm);
        S = (M == -INFINITY ? 0.f : S * __expf(M - mn)) + (qm == -INFINITY ? 0.f : qs * __expf(qm - mn));
        M = mn;
      }
      if (lane == 0) sh.logz = M + __logf(S);
    }
    __syncthreads();
    tl_rank_select(sh, P * TOPLP_MAX, K);
  } else {
    if (tid == 0) sh.logz = M + __logf(S);
    __syncthreads();
  }
  if (tid < K) {
    const bool has = tid < sh.cnt;
    const tl_key k = sh.buf[tid];
    out_ids[o * K + tid] = has ? tl_key_id(k) : -1;
    out_lps[o * K + tid] = has ? tl_key_y(k) - sh.logz : -INFINITY;
  }
}

int top_logprobs_max() { return TOPLP_MAX; }
int top_logprobs_parts() { return TL_PARTS; }
// u64 words of workspace per asked row of a split launch
int top_logprobs_ws_words() { return TL_PARTS * TL_SLOT; }

// ws / tickets (both or neither): n x top_logprobs_ws_words() u64 and n zeroed ints -> the
// split form (TL_PARTS workgroups per row); tickets are re-armed by every launch.
int top_logprobs(const void* logits, int is_f32, int64_t stride, int num_rows, int V, const int32_t* rows, int n,
                 const float* temps, int K, int32_t* out_ids, float* out_lps, void* ws, int* tickets,
                 hipStream_t st) {
  if (K < 1 || K > TOPLP_MAX || V < 1 || n < 0 || num_rows < 1) return 1;
  if (n == 0) return 0;
  const int P = (ws != nullptr && tickets != nullptr) ? TL_PARTS : 1;
  const dim3 grid(P, n);
  if (is_f32)
    hipLaunchKernelGGL(top_logprobs_kernel<float>, grid, dim3(TL_NT), 0, st, static_cast<const float*>(logits),
                       stride, num_rows, V, rows, temps, K, out_ids, out_lps, static_cast<tl_key*>(ws), tickets);
  else
    hipLaunchKernelGGL(top_logprobs_kernel<uint16_t>, grid, dim3(TL_NT), 0, st,
                       static_cast<const uint16_t*>(logits), stride, num_rows, V, rows, temps, K, out_ids, out_lps,
                       static_cast<tl_key*>(ws), tickets);
  return 0;
}

}  // namespace xgk
