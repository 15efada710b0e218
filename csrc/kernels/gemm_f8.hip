// gemm_f8 / gemm_i8: prompt-sized GEMM (M > 320) of fp8 and int8 models on the 8-bit matrix
// instructions, and the row quantizers that make their other operand:
//
//   quant_rows_fp8:  x bf16 [M, K]  ->  codes E4M3 [M, K],  sx fp32 [M]
//   quant_rows_int8: x bf16 [M, K]  ->  codes int8 [M, K],  sx fp32 [M]
//   gemm_f8, gemm_i8: out[M, N] = diag(sx) (A[M, K] . W[N, K]^T) diag(sw)
//   moe_gemm_f8:      gemm_f8 per expert over moe_align's sorted rows (F8Grp below):
//                     out[p, :] = sx[r(p)] (A[r(p), :] . W[e]^T) sw[e, :],  p in [offs[e], offs[e + 1])
//
// One kernel, two operand policies (F8Ops, I8Ops below): the byte images, the staging, the ring
// and the epilogues do not depend on what a byte means. gemm_i8 reads int8 codes (W as
// quantize_int8 stores it), accumulates in int32 on v_mfma_i32_16x16x64_i8 -- two instructions
// per 32-B fragment, granule g (k 16g .. 16g + 15 of the low 64-k half) then granule g + 4 (the
// same of the high half) -- and converts the integer sum once (v_cvt_f32_i32) before the scales.
// |a w| <= 2^14 and the launcher refuses K > 131,072 = 2^17, so a whole-K sum stays inside int32;
// a split converts its own sum, so a slab is float(sum_s) * sx * sw. quant_rows_int8 is
// quant_rows_fp8 with sx = max(amax / 127, 1e-12) and code = clamp(rint(x / sx), -127, 127)
// (v_rndne_f32: round half to even), bit-identical to quantize_rows_int8 of xgserve/ops/linear.py.
// quant_rows_int8_i4 is quant_rows_int8 storing every 16 consecutive k in the byte order that
// gemm_i4.hip multiplies without a shuffle (I8CodesI4::K_OF, i4_order of xgserve/ops/linear.py).
// What follows describes gemm_f8; read "K = 128 instruction" as the instruction pair for int8.
//
// A and W are OCP E4M3 codes (W as quantize_fp8 stores it: [N, K] row-major, one fp32 scale per
// output channel); the products are accumulated in fp32 by v_mfma_f32_16x16x128_f8f6f4 (the
// K = 128 form of gfx950, specified at twice the bf16 rate; the older K = 32 *_fp8_fp8 forms run
// at the bf16 rate) and both scales are applied in the epilogue, the row scale first.
//
// quant_rows_fp8 -- one 256-thread workgroup per row. A lane holds its share of the row in
// registers (16 bf16 = two 16-B loads per step, at most 7 steps: K <= 28,672), so x is read from
// HBM once; the row maximum is a wave reduction plus one LDS exchange; then
//   sx = max(amax / 448, 1e-12),  code = e4m3(clamp(x / sx, -448, 448))
// with a true fp32 division (hipcc divides correctly rounded unless told otherwise, and the build
// passes no fast-math flag), the clamp ahead of the conversion (no dependence on its overflow
// mode), v_cvt_pk_fp8_f32 (round to nearest even, subnormals kept) and one 16-B store of 16
// codes per step: bit-identical to quantize_rows_fp8 of xgserve/ops/linear.py.
//
// gemm_f8 -- one 512-thread workgroup per CU owns a BM x 256 output tile (BM = 256 or 128) over
// 128-deep K tiles: a row of a K tile is 128 B of codes. 8 waves as 2 (M) x 4 (N): wave (wr, wc)
// owns BM / 2 rows x 64 columns = MT x 4 accumulator tiles of 16 x 16 (BM 256: 128 accumulator
// registers per lane). The W fragment is the instruction's first operand, so a lane ends with
// 4 consecutive columns of one output row.
//   * Fragments. An operand of the K = 128 instruction is 32 B per lane: lane (g = lane / 16,
//     li = lane % 16) takes row li and the two 16-B granules g and g + 4 of the row's 128 B.
//     Both operands use the same k order, so which k a byte stands for cancels in the sum.
//   * Staging. Both operands by LDS-DMA (global_load_lds_dwordx4, 8 rows x 128 B per wave
//     instruction) into lane-linear images, 16-B granule XOR swizzle (granule ^ row & 7) on the
//     global source address and on the ds_read_b128 fragment reads, as gemm_pf: conflict-free.
//   * The loop is a ring of NS LDS slots (one K tile of A and W each), ONE s_barrier per K tile,
//     in two forms chosen by the registers a tile leaves (512 threads = 2 waves per SIMD = 256
//     registers per lane):
//     BM 128, 3 slots of 48 KB, register double buffer (64 accumulator + 2 x 64 fragment
//     registers). While the matrix unit works on K tile t out of one register set (MT + 4
//     fragments of 8 registers), the wave reads tile t + 1 from its slot into the other set and
//     the DMA of tiles t + 2 .. t + NS is in flight. The fragments of a tile are all in registers
//     one iteration before they are used, so the slot of tile t is free when iteration t begins
//     and is refilled at once, with tile t + NS: the ring is one tile deeper than its slots.
//         s_waitcnt vmcnt((NS - 2) ND)    this wave's pieces of tile t + 1 have landed
//         s_waitcnt lgkmcnt(0)            its reads of tile t's slot have retired
//         s_barrier                       ... and everyone else's
//         DMA tile t + NS -> slot t % NS  (ND = BM / 64 + 4 instructions per wave)
//         ds_read tile t + 1 -> register set (t + 1) & 1
//         MT x 4 MFMAs on register set t & 1   (the compiler interleaves them with the reads)
//     BM 256, 2 slots of 64 KB, streamed A fragments (128 accumulator registers leave no room
//     for a second fragment set). Tile t is read and multiplied in iteration t: the four W
//     fragments once, the A fragments two at a time, the next one read under the four MFMAs of
//     the current one. Its slot is refilled when iteration t + 1 begins, so iteration t issues
//     tile t + NS - 1 and one tile of DMA is in flight under each tile's 32 MFMAs:
//         s_waitcnt vmcnt((NS - 2) ND); s_waitcnt lgkmcnt(0); s_barrier
//         DMA tile t + NS - 1 -> slot (t + NS - 1) % NS
//         W fragments; A fragment mt + 1 | 4 MFMAs on A fragment mt   (mt = 0 .. MT - 1)
//     The DMA is inline asm that hipcc's waitcnt pass does not see (glds.h), so completion is
//     tracked by the counted waits alone; the counts are derived from the issue order
//     (f8::wait_count) and asserted below. Near the end of a K range, where fewer tiles were
//     issued than the count assumes, the wait is vmcnt(0).
//     Twice the k per byte at twice the matrix rate makes the loop twice as sensitive to LDS
//     traffic as gemm_pf: per K tile a wave reads (MT + 4) x 32 B x 64 lanes for MT x 4
//     instructions; BM 256 moves 0.375 fragments per MFMA, BM 128 one half.
//   * XCD-bijective tile order with the M tiles of one W tile adjacent (one L2 reads it once);
//     split-K over uneven K-tile ranges, fp32 slabs [S, M, N] already scaled (partials.h and
//     every consumer as they are).
//   * Tail rows: A rows past M - 1 re-read row M - 1 and are not stored.
// Epilogues: bf16, fp32 partials, or silu(gate) * up of a block-16 interleaved gate|up weight
// (scaled before the gate).
#include <type_traits>

#include "cfg_dispatch.h"
#include "gemm_api.h"
#include "glds.h"

namespace xgk {

enum : int { F8_BF16 = 0, F8_PARTIAL = 1, F8_SILU = 2 };

namespace f8 {
constexpr int BN = 256;         // output columns per workgroup (4 waves x 64)
constexpr int KT = 128;         // k per K tile (one 128-B row of codes)
constexpr int GROUP_M = 8;      // M tiles per group of the tile order
constexpr int QT = 256;         // quantizer threads
constexpr int Q_STEPS = 7;      // quantizer steps of 16 elements per lane
constexpr int Q_MAX_K = QT * 16 * Q_STEPS;
static_assert(Q_MAX_K == 28672, "the quantizer holds a row of the 70B down projection");

constexpr int n_dma(int bm) { return bm / 64 + 4; }  // DMA instructions per wave per K tile (A, then W)
// vmcnt at the wait of an iteration: the tile about to be read has landed and the NS - 2 tiles issued
// after it may still be in flight (double-buffered form: tile t + 1 of tiles .. t + NS - 1; streamed
// form: tile t of tiles .. t + NS - 2)
constexpr int wait_count(int ns, int bm) { return (ns - 2) * n_dma(bm); }
static_assert(wait_count(2, 256) == 0 && wait_count(3, 128) == 6, "f8 wait counts");
}  // namespace f8

typedef __attribute__((ext_vector_type(8))) int i32x8_t;   // operand of the K = 128 instruction
typedef __attribute__((ext_vector_type(4))) int i32x4_t;

// Operand policies: the accumulator of one 16 x 16 tile, the product of one 32-B fragment pair
// added to it, and the accumulator as a float.
struct F8Ops {
  using acc_t = f32x4_t;
  static __device__ __forceinline__ acc_t mma(i32x8_t w, i32x8_t a, acc_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    // formats 0 = E4M3 for both operands; scale arguments 0: the plain (unscaled) instruction
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, a, c, 0, 0, 0, 0, 0, 0);
#else
    return c;
#endif
  }
  static __device__ __forceinline__ float to_float(float v) { return v; }
};
struct I8Ops {
  using acc_t = i32x4_t;
  static __device__ __forceinline__ acc_t mma(i32x8_t w, i32x8_t a, acc_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    // the low 64 k (granule g) and the high 64 k (granule g + 4) of the fragment
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_shufflevector(w, w, 0, 1, 2, 3),
                                              __builtin_shufflevector(a, a, 0, 1, 2, 3), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_shufflevector(w, w, 4, 5, 6, 7),
                                              __builtin_shufflevector(a, a, 4, 5, 6, 7), c, 0, 0, 0);
#endif
    return c;
  }
  static __device__ __forceinline__ float to_float(int v) { return static_cast<float>(v); }  // v_cvt_f32_i32
};

// 32 B of a fragment: granules c0 and c0 + 4 of an image row (already swizzled by the caller)
__device__ __forceinline__ i32x8_t f8_frag(const uint8_t* row, int g, int sl) {
  const i32x4_t lo = *reinterpret_cast<const i32x4_t*>(row + ((g ^ sl) << 4));
  const i32x4_t hi = *reinterpret_cast<const i32x4_t*>(row + (((4 + g) ^ sl) << 4));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Grouped (MoE expert) form, GRP -- moe_gemm_f8: the M dimension is moe_align's expert-sorted,
// 64-padded row space [P]; expert e owns rows [offs[e], offs[e + 1]), its own codes w + e N K and
// its own channel scales sw + e N. Tile slot mi of a column tile is the mi-th (expert, row tile) in
// expert order, found by walking offs; the slots past the last tile leave as a whole workgroup.
// They sit at the end of the order, so the tiles go out in plain dispatch order (block b on XCD
// b % 8 spreads the real tiles over every XCD; the XCD-contiguous order would leave XCDs idle).
// The A gather moves only source addresses: DMA lane (piece, dr) reads code row rows[p] of its
// sorted row p (rows == nullptr: row p; -1 = a pad: row 0, finite data never combined), rows at or
// past the segment end re-read the segment's last row and are not stored, and the epilogue takes
// the row scale from the same place, sx[rows[p]]. The issue order, and so every wait count, is the
// dense kernel's.
struct F8Grp {
  const int32_t* rows;
  const int32_t* offs;
  int E;
  int mt;  // tile slots per column tile (host bound on the experts' tiles)
};

template <class Ops, int BM, int NS, bool DB, bool GRP = false>
__global__ void __launch_bounds__(512, 1) gemm_f8_kernel(const uint8_t* __restrict__ a, const float* __restrict__ sx,
                                                          int M, int K, const uint8_t* __restrict__ w,
                                                          const float* __restrict__ sw, int N, int S,
                                                          float* __restrict__ part, uint16_t* __restrict__ out,
                                                          int mode, F8Grp grp) {
  constexpr int BN = f8::BN;
  constexpr int MT = BM / 32;            // 16-row m tiles per wave
  constexpr int NA = BM / 64;            // A DMA instructions per wave per K tile
  constexpr int NW = 4;                  // W DMA instructions per wave per K tile
  constexpr int ASZ = BM * 128;          // A image
  constexpr int SLOT = ASZ + BN * 128;   // + the W image
  static_assert(BM % 64 == 0 && NS >= 2 && NS * SLOT <= LDS_BYTES, "gemm_f8 geometry");
  static_assert(NA + NW == f8::n_dma(BM), "gemm_f8 DMA count");
  __shared__ __attribute__((aligned(1024))) uint8_t smem[NS * SLOT];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 2, wc = wid & 3;
  const int g = lane >> 4, li = lane & 15;

  // XCD-bijective virtual block id, then GROUP_M M tiles x every N tile per group, M fastest
  const int TM = (M + BM - 1) / BM, TN = N / BN;
  const int nb = gridDim.x, bid = blockIdx.x;
  const int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7;
  const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  int s, m0, n0, m_hi = M;   // m_hi: one past the last row this tile loads and stores
  if constexpr (GRP) {
    const int per_split = grp.mt * TN;
    s = bid / per_split;
    const int u = bid - s * per_split, mi = u / TN;
    n0 = (u - mi * TN) * BN;
    int e = 0, base = 0, lo = 0, hi = 0;
    for (; e < grp.E; ++e) {
      lo = grp.offs[e];
      hi = grp.offs[e + 1];
      const int nt = (hi - lo + BM - 1) / BM;
      if (mi < base + nt) break;
      base += nt;
    }
    if (e == grp.E) return;  // past the last tile: the whole workgroup leaves (uniform)
    m0 = lo + (mi - base) * BM;   // < hi: the expert has more than mi - base tiles
    m_hi = hi;
    w += static_cast<int64_t>(e) * N * K;
    sw += static_cast<int64_t>(e) * N;
  } else {
    const int per_split = TM * TN;
    s = v / per_split;
    const int u = v - s * per_split;
    const int GM = TM < f8::GROUP_M ? TM : f8::GROUP_M;
    const int gsz = GM * TN, gid = u / gsz, first_m = gid * GM;
    const int gm = TM - first_m < GM ? TM - first_m : GM;
    const int ug = u - gid * gsz;
    m0 = (first_m + ug % gm) * BM;
    n0 = (ug / gm) * BN;
  }
  const int nk_all = K / f8::KT;
  const int kt_lo = static_cast<int>(static_cast<int64_t>(s) * nk_all / S);
  const int nk = static_cast<int>(static_cast<int64_t>(s + 1) * nk_all / S) - kt_lo;

  // DMA lanes: row dr of an 8-row piece, physical granule dj holding logical dj ^ dr
  const int dr = lane >> 3, dj = lane & 7;
  const int swz = 16 * (dj ^ dr);
  const int wrow = wc * 64;           // W rows of this wave within the W image
  const int arow = wr * (BM / 2);     // A rows of this wave within the A image
  const int sl = li & 7;              // swizzle key of every fragment row this lane reads

  // wave wid stages A pieces wid + 8 i (rows 8 piece ..) and W pieces 4 wid + i
  const uint8_t* asrc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    int row = min(m0 + 8 * (wid + 8 * i) + dr, m_hi - 1);
    if constexpr (GRP) row = grp.rows != nullptr ? max(grp.rows[row], 0) : row;
    asrc[i] = a + static_cast<int64_t>(row) * K + static_cast<int64_t>(kt_lo) * f8::KT + swz;
  }
  const uint8_t* wsrc = w + static_cast<int64_t>(n0 + 32 * wid + dr) * K + static_cast<int64_t>(kt_lo) * f8::KT + swz;
  auto issue = [&](int t) {
    uint8_t* slot = smem + (t % NS) * SLOT;
#pragma unroll
    for (int i = 0; i < NA; ++i) glds16(asrc[i] + static_cast<int64_t>(t) * f8::KT, slot + (wid + 8 * i) * 1024);
#pragma unroll
    for (int i = 0; i < NW; ++i)
      glds16(wsrc + static_cast<int64_t>(8 * i) * K + static_cast<int64_t>(t) * f8::KT,
             slot + ASZ + (4 * wid + i) * 1024);
  };

  typename Ops::acc_t acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = typename Ops::acc_t{0, 0, 0, 0};
  auto w_frag = [&](int t, int nt) { return f8_frag(smem + (t % NS) * SLOT + ASZ + (wrow + 16 * nt + li) * 128, g, sl); };
  auto a_frag = [&](int t, int mt) { return f8_frag(smem + (t % NS) * SLOT + (arow + 16 * mt + li) * 128, g, sl); };

  if constexpr (DB) {
    // ---- register double buffer: tile t + 1 is read while tile t is multiplied
    i32x8_t fa[2][MT], fw[2][4];
    auto read_frags = [&](int t, auto b_c) {
      constexpr int B = decltype(b_c)::value;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) fw[B][nt] = w_frag(t, nt);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) fa[B][mt] = a_frag(t, mt);
    };
    // prologue: tiles 0 .. NS - 1 in flight, tile 0 into register set 0
#pragma unroll
    for (int t = 0; t < NS; ++t)
      if (t < nk) issue(t);
    if (nk >= NS) wait_vmcnt<(NS - 1) * f8::n_dma(BM)>();
    else wait_vmcnt<0>();
    raw_barrier();
    read_frags(0, std::integral_constant<int, 0>{});

    auto step = [&](int t, auto b_c) {
      constexpr int B = decltype(b_c)::value;
      if (t + 1 < nk) {
        // steady iff every tile the count assumes was issued (tiles .. t + NS - 1)
        if (t + NS - 1 < nk) wait_vmcnt<f8::wait_count(NS, BM)>();
        else wait_vmcnt<0>();
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      raw_barrier();
      if (t + NS < nk) issue(t + NS);
      if (t + 1 < nk) read_frags(t + 1, std::integral_constant<int, 1 - B>{});
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = Ops::mma(fw[B][nt], fa[B][mt], acc[mt][nt]);
    };
    for (int t = 0; t < nk; t += 2) {
      step(t, std::integral_constant<int, 0>{});
      if (t + 1 < nk) step(t + 1, std::integral_constant<int, 1>{});
    }
  } else {
    // ---- streamed A fragments: tile t is read and multiplied in iteration t; its slot is
    // refilled (tile t + NS) when iteration t + 1 begins, i.e. iteration t issues tile t + NS - 1
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
      if (t < nk) issue(t);
    for (int t = 0; t < nk; ++t) {
      // tile t has landed; in flight stay the NS - 2 tiles after it, where all were issued
      if (t + NS - 2 < nk) wait_vmcnt<f8::wait_count(NS, BM)>();
      else wait_vmcnt<0>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      raw_barrier();
      if (t + NS - 1 < nk) issue(t + NS - 1);
      i32x8_t fw[4], fa[2];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) fw[nt] = w_frag(t, nt);
      fa[0] = a_frag(t, 0);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (mt + 1 < MT) fa[(mt + 1) & 1] = a_frag(t, mt + 1);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = Ops::mma(fw[nt], fa[mt & 1], acc[mt][nt]);
      }
    }
  }

  // ---- epilogue: acc[mt][nt][r] = out[m0 + arow + 16 mt + li][n0 + wrow + 16 nt + 4 g + r]
  const int mb = m0 + arow + li;
  const int nb0 = n0 + wrow + 4 * g;
  float4 cs[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) cs[nt] = *reinterpret_cast<const float4*>(sw + nb0 + 16 * nt);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = mb + 16 * mt;
    if (m >= m_hi) continue;
    const float rs = sx[GRP && grp.rows != nullptr ? max(grp.rows[m], 0) : m];
    float o[4][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      o[nt][0] = Ops::to_float(acc[mt][nt][0]) * rs * cs[nt].x;
      o[nt][1] = Ops::to_float(acc[mt][nt][1]) * rs * cs[nt].y;
      o[nt][2] = Ops::to_float(acc[mt][nt][2]) * rs * cs[nt].z;
      o[nt][3] = Ops::to_float(acc[mt][nt][3]) * rs * cs[nt].w;
    }
    if (mode == F8_PARTIAL) {
      float* pp = part + (static_cast<int64_t>(s) * M + m) * N + nb0;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        *reinterpret_cast<float4*>(pp + 16 * nt) = make_float4(o[nt][0], o[nt][1], o[nt][2], o[nt][3]);
    } else if (mode == F8_BF16) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        *reinterpret_cast<uint2*>(out + static_cast<int64_t>(m) * N + nb0 + 16 * nt) =
            make_uint2(pack2(o[nt][0], o[nt][1]), pack2(o[nt][2], o[nt][3]));
    } else {
      // SiLU gate: n tiles 2j (gate) / 2j + 1 (up) are one interleaved 16-row block pair
      const int F = N / 2, f0 = (n0 + wrow) / 2 + 4 * g;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gt = o[2 * j][r];
          y[r] = gt / (1.f + __expf(-gt)) * o[2 * j + 1][r];
        }
        *reinterpret_cast<uint2*>(out + static_cast<int64_t>(m) * F + f0 + 16 * j) =
            make_uint2(pack2(y[0], y[1]), pack2(y[2], y[3]));
      }
    }
  }
}

// ---------------------------------------------------------------- row quantizers
// Code policies: the largest code magnitude, four scaled, clamped values as one dword of codes, and
// K_OF[b]: which of 16 consecutive k is stored as byte b of their 16 B.
struct NaturalOrder {
  static constexpr int K_OF[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
};
struct F8Codes : NaturalOrder {
  static constexpr float QMAX = 448.f;
  static __device__ __forceinline__ uint32_t pack4(float a, float b, float c, float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return static_cast<uint32_t>(v);
#else
    return 0;
#endif
  }
};
struct I8Arith {
  static constexpr float QMAX = 127.f;
  // the clamp commutes with the rounding (its ends are integers), so it may come first
  static __device__ __forceinline__ uint32_t byte(float v) { return static_cast<uint32_t>(static_cast<int>(rintf(v))) & 255u; }
  static __device__ __forceinline__ uint32_t pack4(float a, float b, float c, float d) {
    return byte(a) | byte(b) << 8 | byte(c) << 16 | byte(d) << 24;
  }
};
struct I8Codes : I8Arith, NaturalOrder {};
// the kernel order of gemm_i4.hip (i4_order of xgserve/ops/linear.py): the k that the "even" and the
// "odd" widened words of a packed int4 weight hold, so that gemm_i4 selects registers, not bytes
struct I8CodesI4 : I8Arith {
  static constexpr int K_OF[16] = {0, 4, 1, 5, 8, 12, 9, 13, 2, 6, 3, 7, 10, 14, 11, 15};
};

template <class Codes>
__global__ void __launch_bounds__(f8::QT) quant_rows_kernel(const uint16_t* __restrict__ x, int K,
                                                                uint8_t* __restrict__ codes, float* __restrict__ sx) {
  __shared__ float red[f8::QT / 64];
  const int m = blockIdx.x, tid = threadIdx.x;
  const uint16_t* xr = x + static_cast<int64_t>(m) * K;
  uint8_t* cr = codes + static_cast<int64_t>(m) * K;
  const int units = K / 16;   // 16 elements: 32 B in, 16 B out
  uint4 v[f8::Q_STEPS][2];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < f8::Q_STEPS; ++i) {
    const int un = tid + i * f8::QT;
    if (un < units) {
      v[i][0] = ld16(xr + 16 * un);
      v[i][1] = ld16(xr + 16 * un + 8);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float f[8];
        unpack8(v[i][h], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
      }
    }
  }
  amax = wave_max(amax);
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < f8::QT / 64; ++i) amax = fmaxf(amax, red[i]);
  const float sc = fmaxf(amax / Codes::QMAX, 1e-12f);
  if (tid == 0) sx[m] = sc;
#pragma unroll
  for (int i = 0; i < f8::Q_STEPS; ++i) {
    const int un = tid + i * f8::QT;
    if (un < units) {
      uint32_t o[4];
      float f[16];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        unpack8(v[i][h], f + 8 * h);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[8 * h + j] = fminf(fmaxf(f[8 * h + j] / sc, -Codes::QMAX), Codes::QMAX);
      }
#pragma unroll
      for (int d = 0; d < 4; ++d)
        o[d] = Codes::pack4(f[Codes::K_OF[4 * d]], f[Codes::K_OF[4 * d + 1]], f[Codes::K_OF[4 * d + 2]], f[Codes::K_OF[4 * d + 3]]);
      st16(cr + 16 * un, make_uint4(o[0], o[1], o[2], o[3]));
    }
  }
}

// x bf16 [M, K] -> codes [M, K], sx [M]. K % 16 == 0, K <= 28,672; 16-B aligned pointers.
template <class Codes>
static int quant_rows(const uint16_t* x, int M, int K, uint8_t* codes, float* sx, hipStream_t st) {
  if (x == nullptr || codes == nullptr || sx == nullptr || M < 1 || K < 16 || K % 16 || K > f8::Q_MAX_K) return 1;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(codes)) & 15) return 1;
  hipLaunchKernelGGL(quant_rows_kernel<Codes>, dim3(M), dim3(f8::QT), 0, st, x, K, codes, sx);
  return static_cast<int>(hipGetLastError());
}
int quant_rows_fp8(const uint16_t* x, int M, int K, uint8_t* codes, float* sx, hipStream_t st) {
  return quant_rows<F8Codes>(x, M, K, codes, sx, st);
}
int quant_rows_int8(const uint16_t* x, int M, int K, uint8_t* codes, float* sx, hipStream_t st) {
  return quant_rows<I8Codes>(x, M, K, codes, sx, st);
}
int quant_rows_int8_i4(const uint16_t* x, int M, int K, uint8_t* codes, float* sx, hipStream_t st) {
  return quant_rows<I8CodesI4>(x, M, K, codes, sx, st);
}

// ---------------------------------------------------------------- host side of gemm_f8 / gemm_i8
// The launch configurations of both formats: (tile rows, LDS ring slots).
constexpr F8Cfg F8_CFGS[] = {{256, 2}, {128, 3}};
constexpr int F8_NCFG = table_size(F8_CFGS);
int f8_cfgs(const F8Cfg** rows) {
  *rows = F8_CFGS;
  return F8_NCFG;
}

bool f8_supports(int M, int K, int N, int S, int mode, int cfg) {
  if (M < 1 || cfg < 0 || cfg >= F8_NCFG) return false;
  if (K < f8::KT || K % f8::KT || N < f8::BN || N % f8::BN || S < 1 || S > K / f8::KT) return false;
  const int64_t wgs = static_cast<int64_t>((M + F8_CFGS[cfg].bm - 1) / F8_CFGS[cfg].bm) * (N / f8::BN) * S;
  if (wgs >= (int64_t{1} << 31)) return false;
  return mode == F8_PARTIAL || ((mode == F8_BF16 || mode == F8_SILU) && S == 1);
}

// f8_supports, and a whole-K sum of |a w| <= 2^14 that stays inside int32
constexpr int I8_MAX_K = 131072;
bool i8_supports(int M, int K, int N, int S, int mode, int cfg) {
  return K <= I8_MAX_K && f8_supports(M, K, N, S, mode, cfg);
}

// a codes [M, K], sx [M]; w codes [N, K], sw [N] (16-B aligned); mode F8_PARTIAL: part [S, M, N]
// fp32; F8_BF16: out [M, N]; F8_SILU: out [M, N / 2]. Returns 0, or 1 for what it cannot take.
template <class Ops>
static int gemm_8bit(const uint8_t* a, const float* sx, int M, int K, const uint8_t* w, const float* sw, int N,
                     float* part, uint16_t* out, int S, int mode, int cfg, hipStream_t st) {
  if (a == nullptr || sx == nullptr || w == nullptr || sw == nullptr) return 1;
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(sw)) & 15) return 1;
  if (mode == F8_PARTIAL ? part == nullptr : out == nullptr) return 1;
  int rc = 1;
  cfg_dispatch<F8_NCFG>(cfg, [&](auto c) {
    static constexpr F8Cfg f = F8_CFGS[decltype(c)::value];
    const int tiles = ((M + f.bm - 1) / f.bm) * (N / f8::BN);
    hipLaunchKernelGGL((gemm_f8_kernel<Ops, f.bm, f.ns, f.bm <= 128>), dim3(tiles * S), dim3(512), 0, st, a, sx, M, K, w, sw, N, S,
                       part, out, mode, F8Grp{});
    rc = static_cast<int>(hipGetLastError());
  });
  return rc;
}
int gemm_f8(const uint8_t* a, const float* sx, int M, int K, const uint8_t* w, const float* sw, int N, float* part,
            uint16_t* out, int S, int mode, int cfg, hipStream_t st) {
  if (!f8_supports(M, K, N, S, mode, cfg)) return 1;
  return gemm_8bit<F8Ops>(a, sx, M, K, w, sw, N, part, out, S, mode, cfg, st);
}
int gemm_i8(const uint8_t* a, const float* sx, int M, int K, const uint8_t* w, const float* sw, int N, float* part,
            uint16_t* out, int S, int mode, int cfg, hipStream_t st) {
  if (!i8_supports(M, K, N, S, mode, cfg)) return 1;
  return gemm_8bit<I8Ops>(a, sx, M, K, w, sw, N, part, out, S, mode, cfg, st);
}

// ---------------------------------------------------------------- moe_gemm_f8 (the grouped form)
// Tile slots per column tile: the sum over experts of ceil(segment / bm), segments 64-padded, is
// at most (max_pairs + 63 E) / bm + E.
static int64_t moe_f8_slots(int E, int max_pairs, int bm) { return (max_pairs + int64_t{63} * E) / bm + E; }

bool moe_f8_supports(int E, int P, int K, int N, int max_pairs, int S, int mode, int cfg) {
  if (E < 1 || P < 64 || P % 64 || max_pairs < 1 || cfg < 0 || cfg >= F8_NCFG) return false;
  if (K < f8::KT || K % f8::KT || N < f8::BN || N % f8::BN || S < 1 || S > K / f8::KT) return false;
  if (moe_f8_slots(E, max_pairs, F8_CFGS[cfg].bm) * (N / f8::BN) * S >= (int64_t{1} << 31)) return false;
  return mode == F8_PARTIAL || (mode == F8_SILU && S == 1);
}

// a: E4M3 codes [., K] with one scale per row in sx; rows [P] gathers both (nullptr: they are in
// sorted order, [P, K] and [P]); offs [E + 1]; w codes [E, N, K], sw [E, N]; max_pairs bounds the
// real rows over all experts (it sizes the grid). F8_SILU: out bf16 [P, N / 2]; F8_PARTIAL: part
// fp32 [S, P, N]. Returns 0, or 1 for what it cannot take.
int moe_gemm_f8(const uint8_t* a, const float* sx, const int32_t* rows, const int32_t* offs, int E, int P, int K,
                const uint8_t* w, const float* sw, int N, int max_pairs, float* part, uint16_t* out, int S, int mode,
                int cfg, hipStream_t st) {
  if (!moe_f8_supports(E, P, K, N, max_pairs, S, mode, cfg)) return 1;
  if (a == nullptr || sx == nullptr || offs == nullptr || w == nullptr || sw == nullptr) return 1;
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(sw)) & 15) return 1;
  if (mode == F8_PARTIAL ? part == nullptr : out == nullptr) return 1;
  int rc = 1;
  cfg_dispatch<F8_NCFG>(cfg, [&](auto c) {
    static constexpr F8Cfg f = F8_CFGS[decltype(c)::value];
    const int mt = static_cast<int>(moe_f8_slots(E, max_pairs, f.bm));
    hipLaunchKernelGGL((gemm_f8_kernel<F8Ops, f.bm, f.ns, f.bm <= 128, true>), dim3(mt * (N / f8::BN) * S), dim3(512), 0,
                       st, a, sx, P, K, w, sw, N, S, part, out, mode, F8Grp{rows, offs, E, mt});
    rc = static_cast<int>(hipGetLastError());
  });
  return rc;
}

}  // namespace xgk
