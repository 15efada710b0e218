// K9b: logit processors in front of the samplers -- repetition / frequency / presence
// penalties, logit_bias and min_p -- and the per-slot token statistics they read.
//
// State table: one row of V uint16 cells per engine slot; bit 15 = the token occurs in
// the owner's prompt, low 15 bits = how often the owner generated it (saturating).
//   logit_state_reset : zero the rows of newly bound slots, scatter prompt flags and the
//                       counts of tokens generated before the bind (host-deduplicated).
//   logit_state_update: after sampling, count[slot][token] += 1 per tracked row.
//   process_logits    : per row, on x = fp32(logit), each step rounded on its own:
//                         seen:  x = x > 0 ? x / r : x * r
//                         x = x - (f * float(c));  c > 0: x = x - p
//                         listed tokens: x = x + b
//                         T > 0: y = x * (1 / T); y < max(y) + ln(min_p): x = -inf
//                       into an fp32 [rows, V] scratch the samplers then read. -inf is
//                       "masked" for both samplers, so they need nothing else.
// process_logits with per-row extra history (speculative verification: k + 1 rows of one
// slot in one step, row i as if the block's first i draft tokens had been emitted): a row
// gets (offset, length <= LP_HIST_MAX) into an int32 token list; the effective cell of a
// token is its table cell with the count raised by the token's multiplicity in the row's
// list (saturating, flag kept; ids outside [0, V) ignored; slot -1: zero cells). The list
// is handled as logit_bias is: staged in LDS, the chunk's listed tokens marked in an LDS
// bitmap, and only marked tokens walk the list. An 8-wide vector of unmarked tokens costs
// one LDS byte of the bitmap on top of the plain kernel's load of logits, load of cells
// and two stores. Measured at 256 rows x 128256 it takes 5 % longer than the plain kernel
// (53.6 us against 51.0 us, profiles/r7_spec_processors.md): the unrolled body carries the
// marked-token path eight times (42-44 VGPRs against 22-25, twice the instructions).
//   logit_state_add   : count[slot][token] += 1 for every entry of a list in which slots
//                       and (slot, token) pairs may repeat (a verify block's emitted tokens).
//                       Shape chosen: one thread per entry, a compare-and-swap loop on the
//                       aligned 32-bit word that holds the 16-bit cell -- entries need no
//                       order or grouping, and a lost race only repeats the loop.
// A row is split into chunks of LP_CHUNK tokens, one workgroup each. min_p needs the
// row maximum, so it is a second launch: pass 1 leaves each chunk's max(y) in `ws`,
// pass 2 combines them (max is exact in any order) and masks its chunk.
#include "common.h"

namespace xgk {

constexpr int LP_NT = 256;
constexpr int LP_CHUNK = 4096;     // tokens per workgroup: 2 vectors of 8 per thread
constexpr int LP_BIAS_MAX = 128;   // logit_bias entries per row
constexpr int LP_COUNT_MAX = 0x7fff;
constexpr int LP_HIST_MAX = 16;    // extra-history tokens per row

struct LpRow {
  int slot, boff, blen;
  float rep, freq, pres;
};

__device__ __forceinline__ float lp_penalise(float x, uint32_t cell, const LpRow& q) {
#pragma clang fp contract(off)
  const int c = cell & LP_COUNT_MAX;
  if (cell != 0) x = x > 0.f ? x / q.rep : x * q.rep;
  const float fc = q.freq * static_cast<float>(c);
  x = x - fc;
  if (c > 0) x = x - q.pres;
  return x;
}

// y = x * (1 / T): the samplers' scaled_logit (sampling.hip), rounded on its own
__device__ __forceinline__ float lp_scaled(float x, float it) {
#pragma clang fp contract(off)
  return x * it;
}

__device__ __forceinline__ float lp_add(float x, float b) {
#pragma clang fp contract(off)
  return x + b;
}

template <typename T>
__device__ __forceinline__ float lp_load(const T* p);
template <> __device__ __forceinline__ float lp_load<uint16_t>(const uint16_t* p) { return bf2f(*p); }
template <> __device__ __forceinline__ float lp_load<float>(const float* p) { return *p; }

template <typename T>
__device__ __forceinline__ void lp_load8(const T* p, float* f);
template <> __device__ __forceinline__ void lp_load8<uint16_t>(const uint16_t* p, float* f) { unpack8(ld16(p), f); }
template <> __device__ __forceinline__ void lp_load8<float>(const float* p, float* f) {
  const uint4 a = ld16(p), b = ld16(p + 4);
  f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y); f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
  f[4] = __uint_as_float(b.x); f[5] = __uint_as_float(b.y); f[6] = __uint_as_float(b.z); f[7] = __uint_as_float(b.w);
}

__device__ __forceinline__ bool lp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the cell a token has after m more generated occurrences: count saturating, flag kept
__device__ __forceinline__ uint32_t lp_cell_plus(uint32_t cell, int m) {
  return (cell & 0x8000u) | static_cast<uint32_t>(min(static_cast<int>(cell & LP_COUNT_MAX) + m, LP_COUNT_MAX));
}

// One chunk of one row; the body of both kernels below. HIST: the row's extra history
// ph = [offset | length] x pstride into hist_ids (hist_cap entries).
template <typename T, bool HIST>
__device__ __forceinline__ void lp_process_chunk(
    const T* __restrict__ in, int64_t in_stride, float* __restrict__ out, int64_t out_stride, int V,
    const uint16_t* __restrict__ state, int num_slots, const int32_t* __restrict__ pi,
    const float* __restrict__ pf, int pstride, const float* __restrict__ temps,
    const int32_t* __restrict__ bias_ids, const float* __restrict__ bias_vals, int bias_cap,
    float* __restrict__ ws, const int32_t* __restrict__ hist_ids, int hist_cap, const int32_t* __restrict__ ph) {
  const int row = blockIdx.y, part = blockIdx.x, P = gridDim.x;
  const int lo = part * LP_CHUNK, hi = min(V, lo + LP_CHUNK);
  LpRow q;
  q.slot = pi[row];
  q.boff = pi[pstride + row];
  q.blen = min(pi[2 * pstride + row], LP_BIAS_MAX);
  q.rep = pf[row];
  q.freq = pf[pstride + row];
  q.pres = pf[2 * pstride + row];
  const float lm = pf[3 * pstride + row];
  const float temp = temps[row];
  const bool minp = temp > 0.f && lm > -INFINITY;
  const float it = temp > 0.f ? 1.f / temp : 1.f;
  if (q.slot >= num_slots) q.slot = -1;
  if (q.boff < 0 || q.boff + q.blen > bias_cap) q.blen = 0;

  // this chunk's biased tokens: a bitmap over the chunk + the row's list in LDS
  __shared__ uint32_t bmap[LP_CHUNK / 32];
  __shared__ int32_t b_id[LP_BIAS_MAX];
  __shared__ float b_val[LP_BIAS_MAX];
  __shared__ float red[LP_NT / 64];
  if (q.blen > 0) {  // uniform per row
    if (threadIdx.x < LP_CHUNK / 32) bmap[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x < q.blen) {
      const int id = bias_ids[q.boff + threadIdx.x];
      b_id[threadIdx.x] = id;
      b_val[threadIdx.x] = bias_vals[q.boff + threadIdx.x];
      if (id >= lo && id < hi) atomicOr(&bmap[(id - lo) >> 5], 1u << ((id - lo) & 31));
    }
    __syncthreads();
  }
  // this chunk's extra-history tokens, the same way
  __shared__ uint32_t hmap[HIST ? LP_CHUNK / 32 : 1];
  __shared__ int32_t h_id[HIST ? LP_HIST_MAX : 1];
  int hlen = 0;
  if constexpr (HIST) {
    const int hoff = ph[row];
    hlen = min(ph[pstride + row], LP_HIST_MAX);
    if (hoff < 0 || hlen < 0 || hoff + hlen > hist_cap) hlen = 0;
    if (hlen > 0) {  // uniform per row
      if (threadIdx.x < LP_CHUNK / 32) hmap[threadIdx.x] = 0;
      __syncthreads();
      if (threadIdx.x < hlen) {
        const int id = hist_ids[hoff + threadIdx.x];
        h_id[threadIdx.x] = id;
        if (id >= lo && id < hi) atomicOr(&hmap[(id - lo) >> 5], 1u << ((id - lo) & 31));
      }
      __syncthreads();
    }
  }
  auto hist_cell = [&](int i, uint32_t cell) -> uint32_t {  // i: a marked token of this chunk
    int m = 0;
    for (int k = 0; k < hlen; ++k) m += h_id[k] == i;
    return lp_cell_plus(cell, m);
  };
  auto biased = [&](int i, float x) -> float {  // i: token id inside this chunk
    if (q.blen > 0 && ((bmap[(i - lo) >> 5] >> ((i - lo) & 31)) & 1u)) {
      for (int k = 0; k < q.blen; ++k)
        if (b_id[k] == i) return lp_add(x, b_val[k]);
    }
    return x;
  };

  const T* ip = in + row * in_stride;
  float* op = out + row * out_stride;
  const uint16_t* sp = q.slot >= 0 ? state + static_cast<int64_t>(q.slot) * V : nullptr;
  float m = -INFINITY;
  const bool vec = lp_aligned16(ip) && lp_aligned16(op) && (sp == nullptr || lp_aligned16(sp));
  int done = lo;
  if (vec) {
    const int nvec = (hi - lo) / 8;
    for (int v = threadIdx.x; v < nvec; v += LP_NT) {
      const int i0 = lo + v * 8;
      float f[8];
      lp_load8<T>(ip + i0, f);
      uint32_t cells[4] = {0u, 0u, 0u, 0u};
      if (sp != nullptr) {
        const uint4 c = ld16(sp + i0);
        cells[0] = c.x; cells[1] = c.y; cells[2] = c.z; cells[3] = c.w;
      }
      uint32_t hbits = 0;  // the vector's 8 bits of the history bitmap (i0 - lo is a multiple of 8)
      if constexpr (HIST)
        if (hlen > 0) hbits = (hmap[(i0 - lo) >> 5] >> ((i0 - lo) & 31)) & 0xffu;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        uint32_t cell = (cells[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
        if constexpr (HIST)
          if ((hbits >> k) & 1u) cell = hist_cell(i0 + k, cell);
        f[k] = biased(i0 + k, lp_penalise(f[k], cell, q));
        m = fmaxf(m, lp_scaled(f[k], it));
      }
      *reinterpret_cast<float4*>(op + i0) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<float4*>(op + i0 + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
    done = lo + nvec * 8;
  }
  for (int i = done + threadIdx.x; i < hi; i += LP_NT) {
    uint32_t cell = sp != nullptr ? sp[i] : 0u;
    if constexpr (HIST)
      if (hlen > 0 && ((hmap[(i - lo) >> 5] >> ((i - lo) & 31)) & 1u)) cell = hist_cell(i, cell);
    const float x = biased(i, lp_penalise(lp_load<T>(ip + i), cell, q));
    m = fmaxf(m, lp_scaled(x, it));
    op[i] = x;
  }
  if (!minp) return;  // uniform per row
  m = wave_max(m);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = red[0];
    for (int w = 1; w < LP_NT / 64; ++w) r = fmaxf(r, red[w]);
    ws[row * P + part] = r;
  }
}

// pi: [slot | bias offset | bias length] x pstride (int32); pf: [rep | freq | pres | lm] x pstride
template <typename T>
__global__ void __launch_bounds__(LP_NT) process_logits_kernel(
    const T* __restrict__ in, int64_t in_stride, float* __restrict__ out, int64_t out_stride, int V,
    const uint16_t* __restrict__ state, int num_slots, const int32_t* __restrict__ pi,
    const float* __restrict__ pf, int pstride, const float* __restrict__ temps,
    const int32_t* __restrict__ bias_ids, const float* __restrict__ bias_vals, int bias_cap,
    float* __restrict__ ws) {
  lp_process_chunk<T, false>(in, in_stride, out, out_stride, V, state, num_slots, pi, pf, pstride, temps, bias_ids,
                             bias_vals, bias_cap, ws, nullptr, 0, nullptr);
}

// the same with per-row extra history; ph: [offset | length] x pstride into hist_ids
template <typename T>
__global__ void __launch_bounds__(LP_NT) process_logits_hist_kernel(
    const T* __restrict__ in, int64_t in_stride, float* __restrict__ out, int64_t out_stride, int V,
    const uint16_t* __restrict__ state, int num_slots, const int32_t* __restrict__ pi,
    const float* __restrict__ pf, int pstride, const float* __restrict__ temps,
    const int32_t* __restrict__ bias_ids, const float* __restrict__ bias_vals, int bias_cap,
    float* __restrict__ ws, const int32_t* __restrict__ hist_ids, int hist_cap, const int32_t* __restrict__ ph) {
  lp_process_chunk<T, true>(in, in_stride, out, out_stride, V, state, num_slots, pi, pf, pstride, temps, bias_ids,
                            bias_vals, bias_cap, ws, hist_ids, hist_cap, ph);
}

// min_p: mask the tokens of this chunk whose y lies below max(y) + ln(min_p)
__global__ void __launch_bounds__(LP_NT) min_p_mask_kernel(float* __restrict__ out, int64_t out_stride, int V,
                                                           const float* __restrict__ pf, int pstride,
                                                           const float* __restrict__ temps,
                                                           const float* __restrict__ ws) {
  const int row = blockIdx.y, part = blockIdx.x, P = gridDim.x;
  const float lm = pf[3 * pstride + row];
  const float temp = temps[row];
  if (!(temp > 0.f && lm > -INFINITY)) return;
  const float it = 1.f / temp;
  float M = -INFINITY;
  for (int p = 0; p < P; ++p) M = fmaxf(M, ws[row * P + p]);
  const float thr = lp_add(M, lm);
  const int lo = part * LP_CHUNK, hi = min(V, lo + LP_CHUNK);
  float* op = out + row * out_stride;
  int done = lo;
  if (lp_aligned16(op)) {
    const int nvec = (hi - lo) / 4;
    for (int v = threadIdx.x; v < nvec; v += LP_NT) {
      float4 x = *reinterpret_cast<const float4*>(op + lo + v * 4);
      const bool k0 = lp_scaled(x.x, it) < thr, k1 = lp_scaled(x.y, it) < thr, k2 = lp_scaled(x.z, it) < thr,
                 k3 = lp_scaled(x.w, it) < thr;
      if (k0 | k1 | k2 | k3) {
        if (k0) x.x = -INFINITY;
        if (k1) x.y = -INFINITY;
        if (k2) x.z = -INFINITY;
        if (k3) x.w = -INFINITY;
        *reinterpret_cast<float4*>(op + lo + v * 4) = x;
      }
    }
    done = lo + nvec * 4;
  }
  for (int i = done + threadIdx.x; i < hi; i += LP_NT)
    if (lp_scaled(op[i], it) < thr) op[i] = -INFINITY;
}

int logit_proc_parts(int V) { return (V + LP_CHUNK - 1) / LP_CHUNK; }
int logit_bias_max() { return LP_BIAS_MAX; }
int logit_count_max() { return LP_COUNT_MAX; }
int logit_hist_max() { return LP_HIST_MAX; }

// ws: rows x logit_proc_parts(V) floats. Two launches; the second only masks (min_p).
int process_logits(const void* in, int is_f32, int64_t in_stride, float* out, int64_t out_stride, int rows, int V,
                   const uint16_t* state, int num_slots, const int32_t* pi, const float* pf, int pstride,
                   const float* temps, const int32_t* bias_ids, const float* bias_vals, int bias_cap, float* ws,
                   hipStream_t st) {
  if (rows <= 0) return 0;
  if (V <= 0 || rows > pstride || rows > 65535 || out_stride < V || in_stride < V || ws == nullptr) return 1;
  if (state == nullptr) num_slots = 0;
  if (bias_ids == nullptr || bias_vals == nullptr) bias_cap = 0;
  const dim3 grid(logit_proc_parts(V), rows);
  if (is_f32)
    hipLaunchKernelGGL(process_logits_kernel<float>, grid, dim3(LP_NT), 0, st, static_cast<const float*>(in),
                       in_stride, out, out_stride, V, state, num_slots, pi, pf, pstride, temps, bias_ids, bias_vals,
                       bias_cap, ws);
  else
    hipLaunchKernelGGL(process_logits_kernel<uint16_t>, grid, dim3(LP_NT), 0, st, static_cast<const uint16_t*>(in),
                       in_stride, out, out_stride, V, state, num_slots, pi, pf, pstride, temps, bias_ids, bias_vals,
                       bias_cap, ws);
  hipLaunchKernelGGL(min_p_mask_kernel, grid, dim3(LP_NT), 0, st, out, out_stride, V, pf, pstride, temps, ws);
  return 0;
}

// process_logits with per-row extra history: ph = [offset | length] x pstride into the
// hist_cap int32 ids of hist_ids. The min_p pass is the plain one.
int process_logits_hist(const void* in, int is_f32, int64_t in_stride, float* out, int64_t out_stride, int rows, int V,
                        const uint16_t* state, int num_slots, const int32_t* pi, const float* pf, int pstride,
                        const float* temps, const int32_t* bias_ids, const float* bias_vals, int bias_cap, float* ws,
                        const int32_t* hist_ids, int hist_cap, const int32_t* ph, hipStream_t st) {
  if (rows <= 0) return 0;
  if (V <= 0 || rows > pstride || rows > 65535 || out_stride < V || in_stride < V || ws == nullptr) return 1;
  if (ph == nullptr || hist_cap < 0) return 1;
  if (state == nullptr) num_slots = 0;
  if (bias_ids == nullptr || bias_vals == nullptr) bias_cap = 0;
  if (hist_ids == nullptr) hist_cap = 0;
  const dim3 grid(logit_proc_parts(V), rows);
  if (is_f32)
    hipLaunchKernelGGL(process_logits_hist_kernel<float>, grid, dim3(LP_NT), 0, st, static_cast<const float*>(in),
                       in_stride, out, out_stride, V, state, num_slots, pi, pf, pstride, temps, bias_ids, bias_vals,
                       bias_cap, ws, hist_ids, hist_cap, ph);
  else
    hipLaunchKernelGGL(process_logits_hist_kernel<uint16_t>, grid, dim3(LP_NT), 0, st,
                       static_cast<const uint16_t*>(in), in_stride, out, out_stride, V, state, num_slots, pi, pf,
                       pstride, temps, bias_ids, bias_vals, bias_cap, ws, hist_ids, hist_cap, ph);
  hipLaunchKernelGGL(min_p_mask_kernel, grid, dim3(LP_NT), 0, st, out, out_stride, V, pf, pstride, temps, ws);
  return 0;
}

// desc: nres x (slot, offset, n); ids / cells: the entries of reset j at [offset, offset + n).
// grid (chunks of the row, nres): a workgroup zeroes its chunk, then stores the entries
// that fall into it (ids are unique per reset, and two resets never share a slot).
__global__ void __launch_bounds__(LP_NT) logit_state_reset_kernel(uint16_t* __restrict__ state, int num_slots, int V,
                                                                  const int32_t* __restrict__ desc,
                                                                  const int32_t* __restrict__ ids,
                                                                  const int32_t* __restrict__ cells, int total) {
  const int j = blockIdx.y;
  const int slot = desc[3 * j], off = desc[3 * j + 1], n = desc[3 * j + 2];
  if (slot < 0 || slot >= num_slots) return;
  const int lo = blockIdx.x * LP_CHUNK, hi = min(V, lo + LP_CHUNK);
  uint16_t* sp = state + static_cast<int64_t>(slot) * V;
  for (int i = lo + threadIdx.x; i < hi; i += LP_NT) sp[i] = 0;
  if (off < 0 || n < 0 || off + n > total) return;
  __syncthreads();  // this workgroup's zeroes are ordered before its own scatter
  for (int e = threadIdx.x; e < n; e += LP_NT) {
    const int id = ids[off + e];
    if (id >= lo && id < hi) sp[id] = static_cast<uint16_t>(cells[off + e]);
  }
}

int logit_state_reset(uint16_t* state, int num_slots, int V, const int32_t* desc, int nres, const int32_t* ids,
                      const int32_t* cells, int total, hipStream_t st) {
  if (nres <= 0) return 0;
  if (state == nullptr || V <= 0 || nres > 65535 || total < 0) return 1;
  hipLaunchKernelGGL(logit_state_reset_kernel, dim3(logit_proc_parts(V), nres), dim3(LP_NT), 0, st, state, num_slots,
                     V, desc, ids, cells, total);
  return 0;
}

// One thread per sampled row; two rows of a step never share a slot, so a plain
// read-modify-write is enough. The prompt flag (bit 15) is kept.
__global__ void __launch_bounds__(LP_NT) logit_state_update_kernel(uint16_t* __restrict__ state, int num_slots, int V,
                                                                   const int32_t* __restrict__ slots,
                                                                   const int32_t* __restrict__ toks, int n) {
  const int i = blockIdx.x * LP_NT + threadIdx.x;
  if (i >= n) return;
  const int slot = slots[i], tok = toks[i];
  if (slot < 0 || slot >= num_slots || tok < 0 || tok >= V) return;
  uint16_t* cell = state + static_cast<int64_t>(slot) * V + tok;
  const uint16_t c = *cell;
  if ((c & LP_COUNT_MAX) < LP_COUNT_MAX) *cell = c + 1;
}

int logit_state_update(uint16_t* state, int num_slots, int V, const int32_t* slots, const int32_t* toks, int n,
                       hipStream_t st) {
  if (n <= 0) return 0;
  if (state == nullptr || V <= 0) return 1;
  hipLaunchKernelGGL(logit_state_update_kernel, dim3((n + LP_NT - 1) / LP_NT), dim3(LP_NT), 0, st, state, num_slots,
                     V, slots, toks, n);
  return 0;
}

// One thread per entry; entries may repeat a slot and a (slot, token) pair, so the cell
// is raised by a compare-and-swap loop on the aligned 32-bit word that holds it (the
// table's base is 4-byte aligned and it has an even number of cells, checked at launch,
// so the word lies inside the table). Saturates at LP_COUNT_MAX; the prompt flag is kept.
__global__ void __launch_bounds__(LP_NT) logit_state_add_kernel(uint16_t* __restrict__ state, int num_slots, int V,
                                                                const int32_t* __restrict__ slots,
                                                                const int32_t* __restrict__ toks, int n) {
  const int i = blockIdx.x * LP_NT + threadIdx.x;
  if (i >= n) return;
  const int slot = slots[i], tok = toks[i];
  if (slot < 0 || slot >= num_slots || tok < 0 || tok >= V) return;
  const int64_t idx = static_cast<int64_t>(slot) * V + tok;
  uint32_t* word = reinterpret_cast<uint32_t*>(state) + (idx >> 1);
  const int sh = static_cast<int>(idx & 1) * 16;
  uint32_t old = *word;
  for (;;) {
    const uint32_t cell = (old >> sh) & 0xffffu;
    if ((cell & LP_COUNT_MAX) >= LP_COUNT_MAX) return;
    const uint32_t want = (old & ~(0xffffu << sh)) | ((cell + 1u) << sh);
    const uint32_t seen = atomicCAS(word, old, want);
    if (seen == old) return;
    old = seen;
  }
}

int logit_state_add(uint16_t* state, int num_slots, int V, const int32_t* slots, const int32_t* toks, int n,
                    hipStream_t st) {
  if (n <= 0) return 0;
  if (state == nullptr || V <= 0 || num_slots < 0) return 1;
  if ((reinterpret_cast<uintptr_t>(state) & 3) != 0 || ((static_cast<int64_t>(num_slots) * V) & 1) != 0) return 1;
  hipLaunchKernelGGL(logit_state_add_kernel, dim3((n + LP_NT - 1) / LP_NT), dim3(LP_NT), 0, st, state, num_slots, V,
                     slots, toks, n);
  return 0;
}

}  // namespace xgk
