// lm_head_score: prompt scoring without a logits buffer.
//
//   z[m, v]   = sum_k h[m, k] w[v, k]                (bf16 operands, fp32 accumulation, never rounded)
//   lp[m]     = z[m, t_m] - logsumexp_{v < V} z[m, v]       (0 where t_m is no token of the vocabulary)
//   best_id   = argmax_{v < V} z[m, v] (lowest index of a tie),  best_lp = max_v z - logsumexp
//
// Two launches, no tickets, nothing [M, V] in memory:
//
// lm_head_score_kernel -- one 512-thread workgroup owns a BM x BN = 128 x 256 tile of z over
// 64-deep K tiles (a row of a K tile is 128 B of bf16), multiplies it on v_mfma_f32_16x16x32_bf16
// and reduces it, in registers and LDS, to one (max, sum exp(z - max), argmax) per row, written to
// a workspace slot per (row, column tile). The tile that holds a row's target column also writes
// that one logit. 8 waves as 2 (M) x 4 (N): wave (wr, wc) owns 64 rows x 64 columns = 4 x 4
// accumulator tiles of 16 x 16. The W fragment is the instruction's first operand, so a lane ends
// with 4 consecutive columns of one row and a row's 256 columns of the tile sit in 4 lanes
// (g = 0 .. 3) of 4 waves (wc): 16 values in the lane, two shuffles, one LDS exchange.
//   * Fragments. Lane (g = lane / 16, li = lane % 16) takes row li and k 8 g .. 8 g + 7 of a
//     32-deep step: 16 B. A K tile is two steps: granule g, then granule g + 4 of the 128-B row.
//   * Staging, ring and waits are those of gemm_f8's BM 128 form (the images have the same byte
//     geometry): LDS-DMA of 8 rows x 128 B per wave instruction into lane-linear images with the
//     16-B granule XOR swizzle (granule ^ row & 7) on the global source address and on the
//     ds_read_b128; 3 slots of 48 KB; ONE s_barrier per K tile; fragments of tile t + 1 are read
//     into the other register set while tile t is multiplied, so the slot of tile t is refilled at
//     the start of iteration t with tile t + 3:
//         s_waitcnt vmcnt((NS - 2) ND); s_waitcnt lgkmcnt(0); s_barrier
//         DMA tile t + NS -> slot t % NS      (ND = 2 + 4 instructions per wave: A, then W)
//         ds_read tile t + 1 -> register set (t + 1) & 1
//         4 x 4 x 2 MFMAs on register set t & 1
//     The DMA is inline asm hipcc's waitcnt pass does not see (glds.h); the counts come from the
//     issue order (lms::wait_count) and are asserted below. Near the end of K: vmcnt(0).
//   * W (the whole LM head, 1.05 GB at the 8B shape) is read once per row tile: XCD-bijective
//     tile order, GROUP_M row tiles of one column tile adjacent, so one L2 reads a W tile once.
//   * Tails. h rows past M - 1 re-read row M - 1 and are not written. W rows past V - 1 re-read
//     row V - 1 (padding rows of w are never touched) and their columns are masked to -inf.
//
// lm_head_score_merge_kernel -- one wave per row folds the row's ceil(V / BN) partials in a fixed
// order (lane-strided, then a butterfly), so the result does not depend on which tile ran when.
#include <climits>
#include <type_traits>

#include "gemm_api.h"
#include "glds.h"

namespace xgk {

namespace lms {
constexpr int BM = 128;      // rows per workgroup
constexpr int BN = 256;      // vocabulary columns per workgroup (4 waves x 64)
constexpr int KT = 64;       // k per K tile (one 128-B row of bf16)
constexpr int NS = 3;        // LDS ring slots
constexpr int GROUP_M = 8;   // row tiles per group of the tile order
constexpr int MT = BM / 32;  // 16-row m tiles per wave
constexpr int NA = BM / 64;  // A DMA instructions per wave per K tile
constexpr int NW = 4;        // W DMA instructions per wave per K tile
constexpr int ASZ = BM * 128;
constexpr int SLOT = ASZ + BN * 128;
constexpr int MERGE_ROWS = 4;  // rows (waves) per merge workgroup
constexpr int n_dma() { return NA + NW; }
// vmcnt at the wait of iteration t: tile t + 1 has landed, tiles t + 2 .. t + NS - 1 may be in flight
constexpr int wait_count() { return (NS - 2) * n_dma(); }
static_assert(wait_count() == 6, "lm_head_score wait count");
static_assert(NS * SLOT <= LDS_BYTES && 4 * BM * 3 * 4 <= SLOT, "lm_head_score LDS");
}  // namespace lms

// (max, sum exp(z - max), argmax) of two column sets -> of their union; the lower index wins a tie.
// A set with no column is (-inf, 0, INT_MAX): exp(-inf - finite) = 0, and two empty sets stay empty.
// FAST: the hardware exponential (the tile kernel), else expf (the merge).
template <bool FAST>
__device__ __forceinline__ void lms_fold(float& m, float& s, int& i, float om, float os, int oi) {
  const float mx = fmaxf(m, om);
  const float a = m == mx ? 1.f : (FAST ? __expf(m - mx) : expf(m - mx));
  const float b = om == mx ? 1.f : (FAST ? __expf(om - mx) : expf(om - mx));
  i = (om > m || (om == m && oi < i)) ? oi : i;
  s = s * a + os * b;
  m = mx;
}

typedef __attribute__((ext_vector_type(4))) int lms_i32x4_t;

__global__ void __launch_bounds__(512, 1)
    lm_head_score_kernel(const uint16_t* __restrict__ h, int64_t ldh, int M, int K, const uint16_t* __restrict__ w,
                         int64_t ldw, int V, const int32_t* __restrict__ targets, float* __restrict__ pmax,
                         float* __restrict__ psum, int32_t* __restrict__ pidx, float* __restrict__ zt) {
  using namespace lms;
  __shared__ __attribute__((aligned(1024))) uint8_t smem[NS * SLOT];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const int g = lane >> 4, li = lane & 15;

  // XCD-bijective virtual block id, then GROUP_M row tiles x every column tile per group, rows fastest
  const int TM = (M + BM - 1) / BM, TN = (V + BN - 1) / BN;
  const int nb = gridDim.x, bid = blockIdx.x;
  const int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7;
  const int u = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int GM = TM < GROUP_M ? TM : GROUP_M;
  const int gsz = GM * TN, gid = u / gsz, first_m = gid * GM;
  const int gm = TM - first_m < GM ? TM - first_m : GM;
  const int ug = u - gid * gsz;
  const int tn = ug / gm;
  const int m0 = (first_m + ug % gm) * BM, n0 = tn * BN;
  const int nk = K / KT;

  // DMA lanes: row dr of an 8-row piece, physical granule dj holding logical dj ^ dr
  const int dr = lane >> 3, dj = lane & 7;
  const int swz = 8 * (dj ^ dr);      // in elements
  const int wrow = wc * 64;           // W rows of this wave within the W image
  const int arow = wr * (BM / 2);     // h rows of this wave within the A image
  const int sl = li & 7;              // swizzle key of every fragment row this lane reads

  // wave wid stages A pieces wid + 8 i (rows 8 piece ..) and W pieces 4 wid + i
  const uint16_t* asrc[NA];
  const uint16_t* wsrc[NW];
#pragma unroll
  for (int i = 0; i < NA; ++i) asrc[i] = h + static_cast<int64_t>(min(m0 + 8 * (wid + 8 * i) + dr, M - 1)) * ldh + swz;
#pragma unroll
  for (int i = 0; i < NW; ++i) wsrc[i] = w + static_cast<int64_t>(min(n0 + 8 * (4 * wid + i) + dr, V - 1)) * ldw + swz;
  auto issue = [&](int t) {
    uint8_t* slot = smem + (t % NS) * SLOT;
#pragma unroll
    for (int i = 0; i < NA; ++i) glds16(asrc[i] + t * KT, slot + (wid + 8 * i) * 1024);
#pragma unroll
    for (int i = 0; i < NW; ++i) glds16(wsrc[i] + t * KT, slot + ASZ + (4 * wid + i) * 1024);
  };

  f32x4_t acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // register double buffer: both 32-k steps of a tile's fragments, [step][tile]
  lms_i32x4_t fa[2][2][MT], fw[2][2][4];
  auto read_frags = [&](int t, auto b_c) {
    constexpr int B = decltype(b_c)::value;
    const uint8_t* slot = smem + (t % NS) * SLOT;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const uint8_t* row = slot + ASZ + (wrow + 16 * nt + li) * 128;
      fw[B][0][nt] = *reinterpret_cast<const lms_i32x4_t*>(row + ((g ^ sl) << 4));
      fw[B][1][nt] = *reinterpret_cast<const lms_i32x4_t*>(row + (((4 + g) ^ sl) << 4));
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const uint8_t* row = slot + (arow + 16 * mt + li) * 128;
      fa[B][0][mt] = *reinterpret_cast<const lms_i32x4_t*>(row + ((g ^ sl) << 4));
      fa[B][1][mt] = *reinterpret_cast<const lms_i32x4_t*>(row + (((4 + g) ^ sl) << 4));
    }
  };
  // prologue: tiles 0 .. NS - 1 in flight, tile 0 into register set 0
#pragma unroll
  for (int t = 0; t < NS; ++t)
    if (t < nk) issue(t);
  if (nk >= NS) wait_vmcnt<(NS - 1) * n_dma()>();
  else wait_vmcnt<0>();
  raw_barrier();
  read_frags(0, std::integral_constant<int, 0>{});

  auto step = [&](int t, auto b_c) {
    constexpr int B = decltype(b_c)::value;
    if (t + 1 < nk) {
      // steady iff every tile the count assumes was issued (tiles .. t + NS - 1)
      if (t + NS - 1 < nk) wait_vmcnt<wait_count()>();
      else wait_vmcnt<0>();
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();
    if (t + NS < nk) issue(t + NS);
    if (t + 1 < nk) read_frags(t + 1, std::integral_constant<int, 1 - B>{});
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[mt][nt] = mfma16x16x32(__builtin_bit_cast(bf16x8_t, fw[B][ks][nt]),
                                     __builtin_bit_cast(bf16x8_t, fa[B][ks][mt]), acc[mt][nt]);
  };
  for (int t = 0; t < nk; t += 2) {
    step(t, std::integral_constant<int, 0>{});
    if (t + 1 < nk) step(t + 1, std::integral_constant<int, 1>{});
  }

  // ---- epilogue: acc[mt][nt][r] = z[m0 + arow + 16 mt + li][n0 + wrow + 16 nt + 4 g + r]
  __syncthreads();  // every wave is past its last fragment read: the ring becomes the exchange
  float* red_m = reinterpret_cast<float*>(smem);  // [4 wc][BM]
  float* red_s = red_m + 4 * BM;
  int* red_i = reinterpret_cast<int*>(red_s + 4 * BM);
  const int cb = n0 + wrow + 4 * g;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int rl = arow + 16 * mt + li, m = m0 + rl;
    const int t = m < M ? targets[m] : -1;
    float mx = -INFINITY;
    int ix = INT_MAX;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = cb + 16 * nt + r;  // ascending: the first maximum is the lowest index
        const float z = acc[mt][nt][r];
        if (col < V && z > mx) {
          mx = z;
          ix = col;
        }
        if (col == t && col < V) zt[m] = z;  // one lane of one tile per row
      }
    float sm = 0.f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (cb + 16 * nt + r < V) sm += __expf(acc[mt][nt][r] - mx);
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sm, o, 64);
      const int oi = __shfl_xor(ix, o, 64);
      lms_fold<true>(mx, sm, ix, om, os, oi);
    }
    if (g == 0) {
      red_m[wc * BM + rl] = mx;
      red_s[wc * BM + rl] = sm;
      red_i[wc * BM + rl] = ix;
    }
  }
  __syncthreads();
  if (tid < BM && m0 + tid < M) {
    float mx = red_m[tid], sm = red_s[tid];
    int ix = red_i[tid];
#pragma unroll
    for (int c = 1; c < 4; ++c) lms_fold<true>(mx, sm, ix, red_m[c * BM + tid], red_s[c * BM + tid], red_i[c * BM + tid]);
    const int64_t slot = static_cast<int64_t>(m0 + tid) * TN + tn;
    pmax[slot] = mx;
    psum[slot] = sm;
    pidx[slot] = ix;
  }
}

__global__ void __launch_bounds__(64 * lms::MERGE_ROWS)
    lm_head_score_merge_kernel(int M, int V, int TN, const int32_t* __restrict__ targets, const float* __restrict__ pmax,
                               const float* __restrict__ psum, const int32_t* __restrict__ pidx,
                               const float* __restrict__ zt, float* __restrict__ lp, int32_t* __restrict__ best_id,
                               float* __restrict__ best_lp) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * lms::MERGE_ROWS + (threadIdx.x >> 6);
  if (m >= M) return;
  float mx = -INFINITY, sm = 0.f;
  int ix = INT_MAX;
  const int64_t base = static_cast<int64_t>(m) * TN;
  for (int j = lane; j < TN; j += 64) lms_fold<false>(mx, sm, ix, pmax[base + j], psum[base + j], pidx[base + j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sm, o, 64);
    const int oi = __shfl_xor(ix, o, 64);
    lms_fold<false>(mx, sm, ix, om, os, oi);
  }
  if (lane == 0) {
    const float ls = logf(sm);
    const int t = targets[m];
    lp[m] = (t >= 0 && t < V) ? (zt[m] - mx) - ls : 0.f;
    best_id[m] = ix;
    best_lp[m] = -ls;
  }
}

// floats of workspace for M rows of a V-token vocabulary: three partials per (row, column tile)
// and one target logit per row
int64_t lm_head_score_ws_floats(int M, int V) {
  if (M < 0 || V < 1) return -1;
  return static_cast<int64_t>(M) * (3 * ((V + lms::BN - 1) / lms::BN) + 1);
}
int lm_head_score_bm() { return lms::BM; }
int lm_head_score_bn() { return lms::BN; }

// h bf16 [M, K] (row stride ldh elements), w bf16 [>= V, K] (row stride ldw), targets int32 [M];
// ws: lm_head_score_ws_floats(M, V) floats; lp, best_id, best_lp [M]. Pointers 16-B aligned, strides
// % 8 == 0. Returns 0, or 1 for what it cannot take; M == 0 launches nothing.
int lm_head_score(const uint16_t* h, int64_t ldh, int M, int K, const uint16_t* w, int64_t ldw, int V,
                  const int32_t* targets, float* ws, float* lp, int32_t* best_id, float* best_lp, hipStream_t st) {
  if (K < lms::KT || K % lms::KT || V < 1 || M < 0) return 1;
  if (M == 0) return 0;
  if (h == nullptr || w == nullptr || targets == nullptr || ws == nullptr || lp == nullptr || best_id == nullptr ||
      best_lp == nullptr)
    return 1;
  if (ldh < K || ldw < K || ldh % 8 || ldw % 8) return 1;
  if ((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(w)) & 15) return 1;
  const int64_t TM = (M + lms::BM - 1) / lms::BM, TN = (V + lms::BN - 1) / lms::BN;
  if (TM * TN >= (int64_t{1} << 31)) return 1;
  const int64_t n = static_cast<int64_t>(M) * TN;
  float* pmax = ws;
  float* psum = ws + n;
  int32_t* pidx = reinterpret_cast<int32_t*>(ws + 2 * n);
  float* zt = ws + 3 * n;
  hipLaunchKernelGGL(lm_head_score_kernel, dim3(static_cast<unsigned>(TM * TN)), dim3(512), 0, st, h, ldh, M, K, w, ldw,
                     V, targets, pmax, psum, pidx, zt);
  hipLaunchKernelGGL(lm_head_score_merge_kernel, dim3((M + lms::MERGE_ROWS - 1) / lms::MERGE_ROWS),
                     dim3(64 * lms::MERGE_ROWS), 0, st, M, V, static_cast<int>(TN), targets, pmax, psum, pidx, zt, lp,
                     best_id, best_lp);
  return static_cast<int>(hipGetLastError());
}

}  // namespace xgk
