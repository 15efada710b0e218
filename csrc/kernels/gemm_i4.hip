// gemm_i4: prompt-sized GEMM (M > 320) of int4 models on the INT8 matrix instruction, reading the
// int4 codes as quantize_int4 stores them (half a byte per weight):
//
//   out[m, n] = sx[m] sum_g gs[g, n] ( sum_{k in group g} a[m, k] q[n, k] )
//
// a: int8 activation codes [M, K] in KERNEL ORDER (quant_rows_int8_i4 of gemm_f8.hip, i4_order of
// xgserve/ops/linear.py), sx fp32 [M]; w: packed codes [N, K / 2], offset-binary u = q + 8, eight k
// per 32-bit word, element 2 j at bits 4 j and element 2 j + 1 at bits 16 + 4 j; gs fp32 [K / 128, N].
// A sibling of gemm_f8_kernel (same BM x 256 tiles over 128-deep K tiles, same DMA, tile order and
// epilogue forms), not a policy of it: the W image, the fragment path, the accumulators and what
// travels through the ring differ.
//
// One K tile is one scale group (f8::KT == WQ_GROUP == 128). Per K tile the kernel sums each
// 16 x 16 output tile in int32 on two v_mfma_i32_16x16x64_i8 and folds that sum into the fp32
// accumulator with the tile's group scale: acc = fmaf(float(sum), gs, acc), in group order. A sum
// spans 128 products of |16 q a| <= 16,256, far inside int32, so K has no bound of gemm_i8's kind.
//
//   * Free k order. The instruction multiplies slot (lane group g, byte b) of one operand with
//     the same slot of the other, so any k order serves as long as both operands use it. Lane
//     group g takes W granule g of the row's 64 B -- four packed words, k 32 g .. 32 g + 31 --
//     in ONE ds_read_b128, and A granules 2 g and 2 g + 1 of the row's 128 B.
//   * Widening, with the sign for free. For a packed word x, (x << 4) & 0xF0F0F0F0 holds
//     elements (0, 4, 1, 5) in the high nibbles of its bytes and x & 0xF0F0F0F0 holds (2, 6, 3, 7);
//     XOR 0x80808080 turns each byte into the signed int8 16 q. The four "even" words of a
//     granule are the W operand of the tile's first instruction, the four "odd" words that of
//     the second. The factor 16 is exact and leaves with sx in the epilogue (sx / 16).
//   * A in kernel order: within every 16 consecutive k the bytes are k (0, 4, 1, 5), (8, 12, 9, 13),
//     (2, 6, 3, 7), (10, 14, 11, 15), so the first instruction takes dwords (0, 1) of granule 2 g
//     and (0, 1) of granule 2 g + 1 and the second dwords (2, 3) of each: register selection.
//   * LDS slot of one K tile: A image BM x 128 B (gemm_f8's, granule ^ row & 7), W image
//     256 rows x 64 B (16 KB; a DMA instruction moves 16 rows, physical granule = granule ^
//     (row >> 2 & 3): the 16 lanes of a lane group cover all 64 banks once) and the tile's 256
//     group scales (1 KB, one contiguous row piece of gs, one more DMA instruction of wave 0).
//   * Ring of NS slots (BM 128: 4 x 33 KB; BM 256: 3 x 49 KB), streamed form: tile t is read and
//     multiplied in iteration t, iteration t issues tile t + NS - 1 into the slot that iteration
//     t - 1 left, ONE s_barrier per K tile:
//         s_waitcnt vmcnt((NS - 2) ND); s_waitcnt lgkmcnt(0); s_barrier
//         DMA tile t + NS - 1          (ND = BM / 64 + 2 instructions, wave 0 one more)
//         W fragments + scales, widen; per m tile: 4 + 4 MFMAs (dependent pairs four apart),
//         convert and fold under the MFMAs of the next m tile (the compiler's schedule)
//     The counts come from the issue order (i4::wait_count); vmcnt(0) where fewer tiles were
//     issued than the count assumes.
//   * 8 waves as 2 (M) x 4 (N); a lane ends with 4 consecutive columns of one output row.
//     Measured against it and dropped (profiles/i4.md): 1 x 8 waves, which widen each W fragment
//     once per workgroup but read twice the A fragments (up to 9 % slower), and a hand-packed
//     v_pk_fma_f32 fold (0-2 % faster, inside the spread; the compiler packs part of it anyway).
//   * Split-K over whole K tiles (a split never cuts a group), fp32 slabs [S, M, N]; tail rows
//     re-read row M - 1 and are not stored. Epilogues: bf16, partials, SiLU gate (gemm_f8's forms).
#include <type_traits>

#include "cfg_dispatch.h"
#include "gemm_api.h"
#include "glds.h"

namespace xgk {

enum : int { I4_BF16 = 0, I4_PARTIAL = 1, I4_SILU = 2 };

namespace i4 {
constexpr int BN = 256;       // output columns per workgroup (4 waves x 64)
constexpr int KT = 128;       // k per K tile: one scale group, 64 B of packed codes, 128 B of A
constexpr int GROUP_M = 8;    // M tiles per group of the tile order
static_assert(KT == WQ_GROUP, "one K tile is one scale group");

// DMA instructions per wave per K tile: A, W, and wave 0's scale piece
constexpr int n_dma(int bm, bool scales) { return bm / 64 + 2 + (scales ? 1 : 0); }
// vmcnt at the wait of iteration t: tile t has landed, the NS - 2 tiles issued after it may fly
constexpr int wait_count(int ns, int bm, bool scales) { return (ns - 2) * n_dma(bm, scales); }
static_assert(wait_count(4, 128, false) == 8 && wait_count(4, 128, true) == 10 && wait_count(3, 256, true) == 7,
              "i4 wait counts");
}  // namespace i4

typedef __attribute__((ext_vector_type(4))) int i4x4_t;   // operand / accumulator of the int8 instruction

__device__ __forceinline__ i4x4_t i4_mma(i4x4_t w, i4x4_t a, i4x4_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(w, a, c, 0, 0, 0);
#else
  return c;
#endif
}

template <int BM, int NS>
__global__ void __launch_bounds__(512, 1) gemm_i4_kernel(const uint8_t* __restrict__ a, const float* __restrict__ sx,
                                                          int M, int K, const uint8_t* __restrict__ w,
                                                          const float* __restrict__ gs, int N, int S,
                                                          float* __restrict__ part, uint16_t* __restrict__ out,
                                                          int mode) {
  constexpr int BN = i4::BN;
  constexpr int MT = BM / 32;            // 16-row m tiles per wave
  constexpr int NA = BM / 64;            // A DMA instructions per wave per K tile
  constexpr int NW = 2;                  // W DMA instructions per wave per K tile (16 rows x 64 B each)
  constexpr int ASZ = BM * 128;          // A image
  constexpr int WSZ = BN * 64;           // W image
  constexpr int SLOT = ASZ + WSZ + BN * 4;   // + the group scales
  static_assert(BM % 64 == 0 && NS >= 2 && NS * SLOT <= LDS_BYTES, "gemm_i4 geometry");
  static_assert(NA + NW == i4::n_dma(BM, false), "gemm_i4 DMA count");
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
  const int per_split = TM * TN;
  const int s = v / per_split, u = v - s * per_split;
  const int GM = TM < i4::GROUP_M ? TM : i4::GROUP_M;
  const int gsz = GM * TN, gid = u / gsz, first_m = gid * GM;
  const int gm = TM - first_m < GM ? TM - first_m : GM;
  const int ug = u - gid * gsz;
  const int m0 = (first_m + ug % gm) * BM, n0 = (ug / gm) * BN;
  const int nk_all = K / i4::KT;
  const int kt_lo = static_cast<int>(static_cast<int64_t>(s) * nk_all / S);
  const int nk = static_cast<int>(static_cast<int64_t>(s + 1) * nk_all / S) - kt_lo;

  const int wrow = wc * 64;           // W rows (output columns) of this wave within the tile
  const int arow = wr * (BM / 2);     // A rows of this wave within the A image
  const int64_t KB = K / 2;           // bytes of a W row

  // A DMA lanes: row dr of an 8-row piece, physical granule dj holding logical dj ^ dr.
  // wave wid stages A pieces wid + 8 i (rows 8 piece ..)
  const int dr = lane >> 3, dj = lane & 7;
  const uint8_t* asrc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int row = min(m0 + 8 * (wid + 8 * i) + dr, M - 1);
    asrc[i] = a + static_cast<int64_t>(row) * K + static_cast<int64_t>(kt_lo) * i4::KT + 16 * (dj ^ dr);
  }
  // W DMA lanes: row lane / 4 of a 16-row piece, physical granule lane % 4 holding logical
  // (lane % 4) ^ (row >> 2 & 3). wave wid stages W pieces 2 wid, 2 wid + 1 (rows 32 wid ..)
  const uint8_t* wsrc = w + static_cast<int64_t>(n0 + 32 * wid + (lane >> 2)) * KB + static_cast<int64_t>(kt_lo) * 64 +
                        16 * ((lane & 3) ^ ((lane >> 4) & 3));
  // scale piece of a K tile: gs[kt][n0 .. n0 + 255], 16 B per lane (wave 0)
  const float* ssrc = gs + static_cast<int64_t>(kt_lo) * N + n0 + 4 * lane;
  auto issue = [&](int t) {
    uint8_t* slot = smem + (t % NS) * SLOT;
#pragma unroll
    for (int i = 0; i < NA; ++i) glds16(asrc[i] + static_cast<int64_t>(t) * i4::KT, slot + (wid + 8 * i) * 1024);
#pragma unroll
    for (int i = 0; i < NW; ++i) glds16(wsrc + 16 * i * KB + static_cast<int64_t>(t) * 64, slot + ASZ + (2 * wid + i) * 1024);
    if (wid == 0) glds16(ssrc + static_cast<int64_t>(t) * N, slot + ASZ + WSZ);
  };
  // wave 0 has one more instruction per tile in flight than the others (wid comes out of
  // readfirstlane above, so this is a scalar branch: a wave takes one side whole)
  auto wait_steady = [&]() {
    if (wid == 0) wait_vmcnt<i4::wait_count(NS, BM, true)>();
    else wait_vmcnt<i4::wait_count(NS, BM, false)>();
  };

  f32x4_t acc[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int a_off = (arow + li) * 128, a_sl = li & 7;                         // A fragment rows: 16 mt further each
  const int w_off = ASZ + (wrow + li) * 64 + ((g ^ ((li >> 2) & 3)) << 4);    // W fragment granule: 16 nt rows further each
  const int s_off = ASZ + WSZ + (wrow + 4 * g) * 4;                           // this lane's 4 scales of n tile 0

#pragma unroll
  for (int t = 0; t < NS - 1; ++t)
    if (t < nk) issue(t);
  for (int t = 0; t < nk; ++t) {
    // tile t has landed; in flight stay the NS - 2 tiles after it, where all were issued
    if (t + NS - 2 < nk) wait_steady();
    else wait_vmcnt<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();
    if (t + NS - 1 < nk) issue(t + NS - 1);
    const uint8_t* slot = smem + (t % NS) * SLOT;
    i4x4_t we[4], wo[4];
    f32x4_t sc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const u32x4_t x = *reinterpret_cast<const u32x4_t*>(slot + w_off + nt * 16 * 64);
      we[nt] = __builtin_bit_cast(i4x4_t, ((x << 4) & 0xF0F0F0F0u) ^ 0x80808080u);
      wo[nt] = __builtin_bit_cast(i4x4_t, (x & 0xF0F0F0F0u) ^ 0x80808080u);
      sc[nt] = *reinterpret_cast<const f32x4_t*>(slot + s_off + nt * 64);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const uint8_t* ar = slot + a_off + mt * 16 * 128;
      const i4x4_t lo = *reinterpret_cast<const i4x4_t*>(ar + (((2 * g) ^ a_sl) << 4));
      const i4x4_t hi = *reinterpret_cast<const i4x4_t*>(ar + (((2 * g + 1) ^ a_sl) << 4));
      const i4x4_t a1 = __builtin_shufflevector(lo, hi, 0, 1, 4, 5);
      const i4x4_t a2 = __builtin_shufflevector(lo, hi, 2, 3, 6, 7);
      i4x4_t sum[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) sum[nt] = i4_mma(we[nt], a1, i4x4_t{0, 0, 0, 0});
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) sum[nt] = i4_mma(wo[nt], a2, sum[nt]);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[mt][nt][r] = fmaf(static_cast<float>(sum[nt][r]), sc[nt][r], acc[mt][nt][r]);   // v_cvt_f32_i32, one fma
    }
  }

  // ---- epilogue: acc[mt][nt][r] = 16 out[m0 + arow + 16 mt + li][n0 + wrow + 16 nt + 4 g + r] / sx
  const int mb = m0 + arow + li;
  const int nb0 = n0 + wrow + 4 * g;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = mb + 16 * mt;
    if (m >= M) continue;
    const float rs = sx[m] * 0.0625f;   // the widened codes are 16 q
    float o[4][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[nt][r] = acc[mt][nt][r] * rs;
    if (mode == I4_PARTIAL) {
      float* pp = part + (static_cast<int64_t>(s) * M + m) * N + nb0;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        *reinterpret_cast<float4*>(pp + 16 * nt) = make_float4(o[nt][0], o[nt][1], o[nt][2], o[nt][3]);
    } else if (mode == I4_BF16) {
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

// ---------------------------------------------------------------- host side
// The launch configurations: (tile rows, LDS ring slots).
constexpr I4Cfg I4_CFGS[] = {{256, 3}, {128, 4}};
constexpr int I4_NCFG = table_size(I4_CFGS);
int i4_cfgs(const I4Cfg** rows) {
  *rows = I4_CFGS;
  return I4_NCFG;
}

bool i4_supports(int M, int K, int N, int S, int mode, int cfg) {
  if (M < 1 || cfg < 0 || cfg >= I4_NCFG) return false;
  if (K < i4::KT || K % i4::KT || N < i4::BN || N % i4::BN || S < 1 || S > K / i4::KT) return false;
  const int64_t wgs = static_cast<int64_t>((M + I4_CFGS[cfg].bm - 1) / I4_CFGS[cfg].bm) * (N / i4::BN) * S;
  if (wgs >= (int64_t{1} << 31)) return false;
  return mode == I4_PARTIAL || ((mode == I4_BF16 || mode == I4_SILU) && S == 1);
}

// a codes [M, K] in kernel order, sx [M]; w packed codes [N, K / 2], gs [K / 128, N] (16-B aligned);
// mode I4_PARTIAL: part [S, M, N] fp32; I4_BF16: out [M, N]; I4_SILU: out [M, N / 2]. Returns 0, or 1
// for what it cannot take.
int gemm_i4(const uint8_t* a, const float* sx, int M, int K, const uint8_t* w, const float* gs, int N, float* part,
            uint16_t* out, int S, int mode, int cfg, hipStream_t st) {
  if (!i4_supports(M, K, N, S, mode, cfg)) return 1;
  if (a == nullptr || sx == nullptr || w == nullptr || gs == nullptr) return 1;
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(gs)) & 15) return 1;
  if (mode == I4_PARTIAL ? part == nullptr : out == nullptr) return 1;
  if ((reinterpret_cast<uintptr_t>(part) & 15) || (reinterpret_cast<uintptr_t>(out) & 7)) return 1;
  int rc = 1;
  cfg_dispatch<I4_NCFG>(cfg, [&](auto c) {
    static constexpr I4Cfg f = I4_CFGS[decltype(c)::value];
    const int tiles = ((M + f.bm - 1) / f.bm) * (N / i4::BN);
    hipLaunchKernelGGL((gemm_i4_kernel<f.bm, f.ns>), dim3(tiles * S), dim3(512), 0, st, a, sx, M, K, w, gs, N, S, part,
                       out, mode);
    rc = static_cast<int>(hipGetLastError());
  });
  return rc;
}

}  // namespace xgk
