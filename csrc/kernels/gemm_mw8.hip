// gemm_mw8: gemm_mw's step range (1 <= M <= 320, dispatched at 65..320), epilogues and split-K
// contract on weight-only quantized weights, streamed as CODES:
//
//   out[M, N] = x[M, K] . dequant(W)[N, K]^T      (x bf16, fp32 accumulate)
//   WQ_FP8 / WQ_INT8: codes [N, K], fp32 scale [N];  WQ_INT4: packed [N, K / 2] offset-binary
//   pair-interleaved nibbles, fp32 group scales [K / 128, N] -- quantize_weight's output as it is.
//
// Geometry. One 512-thread workgroup per CU owns WCOLS = 16 WN NWT columns and all XROWS = 64 XT
// rows of x (XT = ceil(M / 64)); x bytes per weight ELEMENT stay M / WCOLS as in gemm_mw, but per
// weight BYTE they are 2x (8-bit) / 4x (int4) the bf16 kernel's, so the x ring is the large one:
//   * a code chunk is one 128-B LDS row per column: KC = 128 k (8-bit) or 256 k (int4). It keeps
//     gemm_mw's DMA image (8 rows x 128 B per wave instruction, 16-B granule ^ (row & 7) applied
//     on the global source address and undone on the fragment read);
//   * x moves in gemm_mw's own unit, a "sub-chunk" of 64 k = one 128-B row per x row, R = KC / 64
//     = 2 / 4 sub-chunks per code chunk. Ring slots: code 128 WCOLS B (+ int4: the chunk's two
//     scale rows, 8 WCOLS B), x sub-chunk 128 XROWS B. A whole-chunk x slot would be 80 / 160 KB at
//     M = 320; in sub-chunks the x ring takes whatever the code ring leaves of the 160 KB:
//         DX = min(5, (160 KB - DW * code slot) / (128 XROWS))   and the cfg needs DX >= 2
//                           x slots DX at XROWS =  64 128 192 256 320   (8-bit | int4)
//       cfg 0  128 cols DW 3 (48 | 51 KB of codes)  5   5   4   3   2  |  5   5   4   3   -
//       cfg 1  128 cols DW 2 (32 | 34 KB)           5   5   5   4   3  |  5   5   5   3   -
//       cfg 2  256 cols DW 2 (64 | 68 KB)           5   5   4   3   2  |  5   5   -   -   -
//       cfg 3  128 cols DW 2, 2 x 4 waves           5   5   5   4   3  |  5   5   5   3   3
//     ("-": the LDS would hold it, the registers do not -- mw8_regs below.) 8-bit: every cfg takes
//     M = 320, cfg 1 / 3 with 3 x sub-chunks (120 KB) in the ring; int4 takes M > 256 on cfg 3 only.
//
// Widening in registers, after the fragment read (wq_widen.h, the forms gemm_w8 proves exact).
// An A fragment of v_mfma_f32_16x16x32_bf16 is 8 consecutive k of one column: 8 B of 8-bit codes
// (one ds_read_b64) or 4 B of nibbles (ds_read_b32). VALU per fragment: fp8 4 (v_cvt_scalef32_pk),
// int4 7 (3 shifts + 4 and_or), int8 about 20 (8 sign-extends, 8 converts, 4 packs). A fragment
// feeds MTW MFMAs of 16 cycles each; the WM waves of one column range repeat its conversion, so
//     VALU per MFMA = v / MTW = v * 16 WM / XROWS:
//                      XROWS = 128        192         320
//       4 x 2 (WM 2)   fp8 0.5  i4 0.9  i8 5.0 | 0.3 0.6 3.3 | 0.2 0.4 2.0
//       2 x 4 (WM 4)       1.0     1.8    10.0 | 0.7 1.2 6.7 | 0.4 0.7 4.0
// 4 VALU (4 cycles each on a wave64) fill one MFMA's 16 cycles, and the SIMD's other wave issues
// under them. 4 x 2 waves as N x M (WM = 2) halves the repeated conversion against 2 x 4 and is the
// only layout that hides int8's at 192 rows, so cfg 0 - 2 are WN = 4, WM = 2: NWT = WCOLS / 64
// column tiles, MTW = XROWS / 32 row tiles per wave, NWT ds_read_b64 / b32 + MTW ds_read_b128 per
// NWT MTW MFMAs. cfg 3 is the 2 x 4 layout, for int4 (whose widening is cheap) above 256 rows.
//
// Scales. fp8 / int8: one multiply per accumulator column in the epilogue. int4: the MFMAs
// accumulate sum x (136 + q) per 128-k group in a group accumulator; an all-ones A fragment gives
// sum x of the wave's own rows (MTW extra MFMAs per k step, 1 / NWT of the work -- chosen over a
// workgroup-wide sum in LDS, which would need a second barrier per group), and at each group end
// acc += s_g (acc_g - 136 sum x). The two scale rows of a code chunk travel through the code ring:
// 8 WCOLS B behind the chunk's codes, one more DMA instruction for the first WCOLS / 128 waves.
// Nothing is staged for the whole K range, so no K / S bound beyond the ring's LDS (mw8_lds_bytes),
// and a split owns whole chunks = whole groups (K % 256 == 0).
//
// vmcnt discipline. Two rings, in-order retirement, raw barrier per x sub-chunk j (code chunk
// c = j / R). After the barrier of step j every wave is past sub-chunk j - 1, so step j issues
// x(j + DX - 1) and, when j % R == 0, W(c + DW - 1) into the slots just freed; the prologue runs
// the same schedule for the virtual steps j < 0. Before step j, x(j) and W(c) must have landed;
// what may stay in flight is everything issued after BOTH. x(i) is issued at step i - DX + 1 and
// W(c') at step (c' - DW + 1) R (behind that step's x), so with sx = j - DX + 1, sw = (c - DW + 1) R:
//     nX = #{ j < i <= min(j + DX - 2, nsub - 1) : i - DX + 1 > sw }
//     nW = #{ c < c' <= min(floor((j - 1) / R) + DW - 1, nch - 1) : (c' - DW + 1) R >= sx }
//     s_waitcnt vmcnt(nX XI + nW WI')       XI = XROWS / 64, WI' = WCOLS / 64 (+ 1: scale DMA)
// The counts differ per format through R and WI' and are evaluated per step (scalar arithmetic).
//
// Weight (code) loads are non-temporal, x and scale loads are not; XCD-grouped block order, K-chunk
// rotation (in code chunks) and the three epilogues are gemm_mw's.
#include "cfg_dispatch.h"
#include "gemm_api.h"
#include "glds.h"
#include "wq_widen.h"

namespace xgk {

enum : int { MW_BF16 = 0, MW_PARTIAL = 1, MW_SILU = 2 };

constexpr int MW8_DX_MAX = 5;
constexpr int mw8_wslot(int cols, int fmt) { return cols * 128 + (fmt == WQ_INT4 ? 8 * cols : 0); }
constexpr int mw8_dx(const Mw8Cfg& c, int xt, int fmt) {
  const int d = (LDS_BYTES - c.dw * mw8_wslot(c.cols(), fmt)) / (64 * xt * 128);
  return d > MW8_DX_MAX ? MW8_DX_MAX : d;
}
// Accumulator and x-fragment registers of a wave (int4: + the group accumulators and sum x).
// Two waves per SIMD have 256 registers each; above 200 of these hipcc spills to scratch (the
// resource report of every instantiation: profiles/mw8.md), so such a (cfg, M, fmt) does not exist.
// The rule is fitted to the compiler, so the build does not rely on it: xgserve/_build.py reads
// the resource report of this file and fails if any instantiation uses scratch.
constexpr int MW8_MAX_REGS = 200;
constexpr int mw8_regs(const Mw8Cfg& c, int xt, int fmt) {
  const int mtw = 4 * xt / (8 / c.wn), k = fmt == WQ_INT4 ? 2 : 1;
  return 4 * (c.nwt * mtw * k + mtw * k);
}
constexpr bool mw8_fits(const Mw8Cfg& c, int xt, int fmt) {
  return mw8_dx(c, xt, fmt) >= 2 && mw8_regs(c, xt, fmt) <= MW8_MAX_REGS;
}
constexpr int mw8_lds(const Mw8Cfg& c, int xt, int fmt) {
  return c.dw * mw8_wslot(c.cols(), fmt) + mw8_dx(c, xt, fmt) * 64 * xt * 128;
}

// s_waitcnt vmcnt(nx XI + nw WI) for 0 <= nx <= A, 0 <= nw <= B (anything else: vmcnt(0))
template <int A, int B, int BMAX, int XI, int WI>
__device__ __forceinline__ void wait_rings(int nx, int nw) {
  if constexpr (A == 0 && B == 0) {
    wait_vmcnt<0>();
  } else {
    if (nx == A && nw == B) {
      wait_vmcnt<A * XI + B * WI>();
      return;
    }
    if constexpr (B > 0) wait_rings<A, B - 1, BMAX, XI, WI>(nx, nw);
    else wait_rings<A - 1, BMAX, BMAX, XI, WI>(nx, nw);
  }
}

template <int WN, int NWT, int MTW, int DW, int DX, int FMT>
__global__ void __launch_bounds__(512, 1) gemm_mw8_kernel(const uint16_t* __restrict__ x, int M, int K,
                                                           const uint8_t* __restrict__ w,
                                                           const float* __restrict__ wscale, int N, int S,
                                                           float* __restrict__ part, uint16_t* __restrict__ out,
                                                           int mode, int krot) {
  constexpr bool I4 = FMT == WQ_INT4;
  constexpr int WM = 8 / WN;
  constexpr int R = I4 ? 4 : 2, LR = I4 ? 2 : 1;  // x sub-chunks per code chunk (and its log2)
  constexpr int KC = 64 * R, RB = 128, RPI = 8;   // k per code chunk, bytes per LDS row, rows per DMA instruction
  constexpr int WCOLS = WN * 16 * NWT;
  constexpr int XROWS = WM * 16 * MTW;
  constexpr int WSLOT = mw8_wslot(WCOLS, FMT);
  constexpr int XSLOT = XROWS * RB;
  constexpr int WI = WCOLS / RPI / 8;             // code DMA instructions per wave per chunk
  constexpr int XI = XROWS / RPI / 8;             // x DMA instructions per wave per sub-chunk
  constexpr int SCI = I4 ? WCOLS / 128 : 0;       // waves that also fetch 1 KB of the chunk's scales
  static_assert(WN * WM == 8 && WI >= 1 && XI >= 1 && WCOLS % 128 == 0 && XROWS % 64 == 0, "bad gemm_mw8 geometry");
  static_assert(DW >= 2 && DW <= 3 && DX >= 2 && DX <= MW8_DX_MAX, "ring depths");
  static_assert(DW * WSLOT + DX * XSLOT <= LDS_BYTES, "LDS");
  static_assert((DX - 2) * XI + (DW - 1) * (WI + 1) < 64, "vmcnt range");
  __shared__ __attribute__((aligned(1024))) uint8_t smem[DW * WSLOT + DX * XSLOT];
  uint8_t* const wring = smem;
  uint8_t* const xring = smem + DW * WSLOT;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int wn = wid % WN, wm = wid / WN;

  // XCD-grouped virtual block id, as gemm_mw
  const int nb = gridDim.x, bid = blockIdx.x;
  const int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7;
  const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int ntiles = N / WCOLS;
  const int s = v / ntiles, tile = v - s * ntiles;
  const int nch_all = K / KC;
  const int c_lo = s * nch_all / S, c_hi = (s + 1) * nch_all / S;
  const int nch = c_hi - c_lo, nsub = nch * R;
  const int n0 = tile * WCOLS;
  const int64_t wrow_bytes = I4 ? K / 2 : K;

  // DMA sources: lane -> (row dr = lane / 8, physical granule dj = lane % 8) holding logical
  // granule dj ^ dr; a code chunk is 128 B of its row whatever the format
  const int dr = lane >> 3, dj = lane & 7;
  const uint8_t* wsrc[WI];
#pragma unroll
  for (int i = 0; i < WI; ++i)
    wsrc[i] = w + static_cast<int64_t>(n0 + 8 * (wid * WI + i) + dr) * wrow_bytes + static_cast<int64_t>(c_lo) * RB +
              16 * (dj ^ dr);
  const uint16_t* xsrc[XI];
#pragma unroll
  for (int i = 0; i < XI; ++i)
    xsrc[i] = x + static_cast<int64_t>(min(8 * (wid * XI + i) + dr, M - 1)) * K + c_lo * KC + 8 * (dj ^ dr);
  // int4 scales of a chunk: rows 2 c, 2 c + 1 of [K / 128, N] as a [2][WCOLS] fp32 image, 16 B per lane
  const int sf = (wid * 64 + lane) * 4;
  const float* ssrc = I4 ? wscale + static_cast<int64_t>(2 * c_lo + sf / WCOLS) * N + n0 + sf % WCOLS : nullptr;

  const int rot = krot ? (tile * 37) % nch : 0;  // K-chunk rotation (gemm_m64g.hip k_rotation)
  auto chunk_of = [&](int c) {
    const int cc = c + rot;
    return cc >= nch ? cc - nch : cc;
  };
  auto issue_w = [&](int c) {
    uint8_t* slot = wring + (c % DW) * WSLOT;
    const int cc = chunk_of(c);
#pragma unroll
    for (int i = 0; i < WI; ++i) glds16_nt(wsrc[i] + cc * RB, slot + (wid * WI + i) * 1024);
    if constexpr (I4) {
      if (wid < SCI) glds16(ssrc + static_cast<int64_t>(2 * cc) * N, slot + WCOLS * RB + wid * 1024);
    }
  };
  auto issue_x = [&](int j) {
    uint8_t* slot = xring + (j % DX) * XSLOT;
    const int kk = chunk_of(j >> LR) * KC + (j & (R - 1)) * 64;
#pragma unroll
    for (int i = 0; i < XI; ++i) glds16(xsrc[i] + kk, slot + (wid * XI + i) * 1024);
  };

  f32x4_t acc[NWT][MTW];
  // int4: the open group's sum x (136 + q) and sum x (every row of an all-ones MFMA)
  f32x4_t accg[I4 ? NWT : 1][I4 ? MTW : 1];
  f32x4_t xs[I4 ? MTW : 1];
#pragma unroll
  for (int nt = 0; nt < NWT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if constexpr (I4) accg[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
  if constexpr (I4) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) xs[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const bf16x8_t ones = as_frag(make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));

  const int wrow0 = wn * 16 * NWT, xrow0 = wm * 16 * MTW;
  // close group gi (0 / 1) of the code chunk in slot ws
  auto fold = [&](const uint8_t* ws, int gi) {
    const float* scl = reinterpret_cast<const float*>(ws + WCOLS * RB) + gi * WCOLS + wrow0 + 4 * g;
#pragma unroll
    for (int nt = 0; nt < NWT; ++nt) {
      const float4 sc = *reinterpret_cast<const float4*>(scl + 16 * nt);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        acc[nt][mt][0] += sc.x * (accg[nt][mt][0] - 136.f * xs[mt][0]);
        acc[nt][mt][1] += sc.y * (accg[nt][mt][1] - 136.f * xs[mt][1]);
        acc[nt][mt][2] += sc.z * (accg[nt][mt][2] - 136.f * xs[mt][2]);
        acc[nt][mt][3] += sc.w * (accg[nt][mt][3] - 136.f * xs[mt][3]);
        accg[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) xs[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  };

  // sub-chunk j: k = 64 r .. 64 r + 63 of code chunk c (r = j % R)
  auto compute = [&](int j) {
    const int c = j >> LR, r = j & (R - 1);
    const uint8_t* ws = wring + (c % DW) * WSLOT;
    const uint8_t* xsl = xring + (j % DX) * XSLOT;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint4 b[MTW];
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt)
        b[mt] = *reinterpret_cast<const uint4*>(xsl + (xrow0 + 16 * mt + li) * RB + (((4 * t + g) ^ (li & 7)) * 16));
#pragma unroll
      for (int nt = 0; nt < NWT; ++nt) {
        const uint8_t* wr = ws + (wrow0 + 16 * nt + li) * RB;
        bf16x8_t a;
        if constexpr (I4) {
          // k = 64 r + 32 t + 8 g ..: nibble granule 2 r + t (32 k each), bytes 4 g .. 4 g + 3
          a = u4x8_to_bf16(*reinterpret_cast<const uint32_t*>(wr + (((2 * r + t) ^ (li & 7)) * 16) + 4 * g));
        } else {
          // k = 64 r + 32 t + 8 g ..: byte granule 4 r + 2 t + g / 2 (16 k each), half g & 1
          const uint2 a8 =
              *reinterpret_cast<const uint2*>(wr + (((4 * r + 2 * t + (g >> 1)) ^ (li & 7)) * 16) + (g & 1) * 8);
          a = FMT == WQ_INT8 ? int8x8_to_bf16(a8) : fp8x8_to_bf16(a8);
        }
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
          if constexpr (I4) accg[nt][mt] = mfma16x16x32(a, as_frag(b[mt]), accg[nt][mt]);
          else acc[nt][mt] = mfma16x16x32(a, as_frag(b[mt]), acc[nt][mt]);
        }
      }
      if constexpr (I4) {
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) xs[mt] = mfma16x16x32(ones, as_frag(b[mt]), xs[mt]);
      }
    }
    if constexpr (I4) {
      if (r & 1) fold(ws, r >> 1);
    }
  };

  // the counted wait before sub-chunk j (header: vmcnt discipline)
  auto wait_for = [&](int j) {
    const int c = j >> LR;
    const int sx = j - DX + 1, sw = (c - DW + 1) * R;
    const int nx = max(0, min(j + DX - 2, nsub - 1) - max(j, sw + DX - 1));
    const int hiw = min(((j - 1 + R) >> LR) - 1 + DW - 1, nch - 1);
    const int cw = ((sx + R - 1) >> LR) + DW - 1;  // first c' issued at or after step sx (arithmetic shift: floor)
    const int nw = max(0, hiw - max(c, cw - 1));
    if (I4 && wid < SCI) wait_rings<DX - 2, DW - 1, DW - 1, XI, WI + 1>(nx, nw);
    else wait_rings<DX - 2, DW - 1, DW - 1, XI, WI>(nx, nw);
  };

  // prologue: the virtual steps j < 0 of the schedule
  constexpr int JMIN = -(DX - 1) < -(DW - 1) * R ? -(DX - 1) : -(DW - 1) * R;
#pragma unroll
  for (int j = JMIN; j < 0; ++j) {
    if (j + DX - 1 >= 0 && j + DX - 1 < nsub) issue_x(j + DX - 1);
    if (j % R == 0 && j / R + DW - 1 >= 0 && j / R + DW - 1 < nch) issue_w(j / R + DW - 1);
  }
  for (int j = 0; j < nsub; ++j) {
    wait_for(j);
    raw_barrier();
    // refills the slots read by sub-chunk j - 1 (every wave is past the barrier)
    if (j + DX - 1 < nsub) issue_x(j + DX - 1);
    if ((j & (R - 1)) == 0 && (j >> LR) + DW - 1 < nch) issue_w((j >> LR) + DW - 1);
    compute(j);
  }

  // acc[nt][mt][r] = out[m = xrow0 + 16 mt + li][n = n0 + wrow0 + 16 nt + 4 g + r]
  // (fp8 / int8: before the column scale; int4: the group scales are folded in)
  if constexpr (!I4) {
#pragma unroll
    for (int nt = 0; nt < NWT; ++nt) {
      const float4 sc = *reinterpret_cast<const float4*>(wscale + n0 + wrow0 + 16 * nt + 4 * g);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        acc[nt][mt][0] *= sc.x;
        acc[nt][mt][1] *= sc.y;
        acc[nt][mt][2] *= sc.z;
        acc[nt][mt][3] *= sc.w;
      }
    }
  }
  if (mode == MW_PARTIAL) {
    float* pp = part + static_cast<int64_t>(s) * M * N;
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      const int m = xrow0 + 16 * mt + li;
      if (m >= M) continue;
#pragma unroll
      for (int nt = 0; nt < NWT; ++nt)
        *reinterpret_cast<float4*>(pp + static_cast<int64_t>(m) * N + n0 + wrow0 + 16 * nt + 4 * g) =
            make_float4(acc[nt][mt][0], acc[nt][mt][1], acc[nt][mt][2], acc[nt][mt][3]);
    }
  } else if (mode == MW_BF16) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      const int m = xrow0 + 16 * mt + li;
      if (m >= M) continue;
#pragma unroll
      for (int nt = 0; nt < NWT; ++nt) {
        uint2 o;
        o.x = pack2(acc[nt][mt][0], acc[nt][mt][1]);
        o.y = pack2(acc[nt][mt][2], acc[nt][mt][3]);
        *reinterpret_cast<uint2*>(out + static_cast<int64_t>(m) * N + n0 + wrow0 + 16 * nt + 4 * g) = o;
      }
    }
  } else if constexpr (NWT % 2 == 0) {
    // SiLU gate: n-tiles 2j (gate) / 2j + 1 (up) are one interleaved 16-row block pair
    const int F = N / 2, f0 = (n0 + wrow0) / 2 + 4 * g;
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
      const int m = xrow0 + 16 * mt + li;
      if (m >= M) continue;
#pragma unroll
      for (int j = 0; j < NWT / 2; ++j) {
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gt = acc[2 * j][mt][r];
          o[r] = gt / (1.f + __expf(-gt)) * acc[2 * j + 1][mt][r];
        }
        uint2 v2;
        v2.x = pack2(o[0], o[1]);
        v2.y = pack2(o[2], o[3]);
        *reinterpret_cast<uint2*>(out + static_cast<int64_t>(m) * F + f0 + 16 * j) = v2;
      }
    }
  }
}

// The launch configurations, indexed by cfg: (WN, NWT, code ring slots). 0 - 2: 4 x 2 waves as
// N x M (header: widening), 0 / 1: 128 columns, 2: 256; 3: 128 columns on 2 x 4 waves, the layout
// whose int4 accumulators still fit the registers at M > 256. The x ring depth follows (cfg, M, fmt).
constexpr Mw8Cfg MW8_CFGS[] = {{4, 2, 3}, {4, 2, 2}, {4, 4, 2}, {2, 4, 2}};
constexpr int MW8_NCFG = table_size(MW8_CFGS);
constexpr int MW8_MAX_XT = MW_MAX_M / 64;
constexpr int mw8_mtw(const Mw8Cfg& c, int xt) { return 4 * xt / (8 / c.wn); }
int mw8_cfgs(const Mw8Cfg** rows) {
  *rows = MW8_CFGS;
  return MW8_NCFG;
}

template <int C, int XT, int FMT>
static void launch_mw8(dim3 grid, hipStream_t st, const uint16_t* x, int M, int K, const uint8_t* w, const float* scale,
                       int N, int S, float* part, uint16_t* out, int mode) {
  static constexpr Mw8Cfg c = MW8_CFGS[C];
  if constexpr (mw8_fits(c, XT, FMT))
    hipLaunchKernelGGL((gemm_mw8_kernel<c.wn, c.nwt, mw8_mtw(c, XT), c.dw, mw8_dx(c, XT, FMT), FMT>), grid, dim3(512), 0,
                       st, x, M, K, w, scale, N, S, part, out, mode, k_rotation(S));
}

static bool mw8_args_ok(int M, int cfg, int fmt) {
  return M >= 1 && M <= MW_MAX_M && cfg >= 0 && cfg < MW8_NCFG && fmt >= WQ_FP8 && fmt <= WQ_INT4;
}

int mw8_lds_bytes(int M, int cfg, int fmt) {
  if (!mw8_args_ok(M, cfg, fmt) || !mw8_fits(MW8_CFGS[cfg], (M + 63) / 64, fmt)) return 0;
  return mw8_lds(MW8_CFGS[cfg], (M + 63) / 64, fmt);
}

bool mw8_supports(int M, int K, int N, int S, int mode, int cfg, int fmt) {
  if (!mw8_args_ok(M, cfg, fmt) || S < 1 || K < 1 || N < 1) return false;
  const int kc = fmt == WQ_INT4 ? 256 : 128;  // int4: a chunk is two whole groups, so no split cuts one
  if (K % kc || S > K / kc || N % MW8_CFGS[cfg].cols() || mw8_lds_bytes(M, cfg, fmt) == 0) return false;
  return mode == MW_PARTIAL || ((mode == MW_BF16 || mode == MW_SILU) && S == 1);
}

// x [M, K] bf16; w codes [N, K] (int4: [N, K / 2]), scale [N] (int4: [K / 128, N]) fp32, 16-B
// aligned. mode MW_PARTIAL: part [S, M, N] fp32; MW_BF16: out [M, N]; MW_SILU: out [M, N / 2]
// (S = 1). 0 = launched, 1 = a shape / configuration this kernel does not take (nothing launched).
int gemm_mw8(const uint16_t* x, int M, int K, const uint8_t* w, const float* scale, int N, float* part, uint16_t* out,
             int S, int mode, int cfg, int fmt, hipStream_t st) {
  if (!mw8_supports(M, K, N, S, mode, cfg, fmt)) return 1;
  if (x == nullptr || w == nullptr || scale == nullptr || (reinterpret_cast<uintptr_t>(scale) & 15)) return 1;
  if (mode == MW_PARTIAL ? part == nullptr : out == nullptr) return 1;
  const dim3 grid((N / MW8_CFGS[cfg].cols()) * S);
  cfg_dispatch<MW8_NCFG>(cfg, [&](auto c) {
    cfg_dispatch<MW8_MAX_XT>((M - 1) / 64, [&](auto xt) {
      constexpr int C = decltype(c)::value, XT = decltype(xt)::value + 1;
      if (fmt == WQ_FP8) launch_mw8<C, XT, WQ_FP8>(grid, st, x, M, K, w, scale, N, S, part, out, mode);
      else if (fmt == WQ_INT8) launch_mw8<C, XT, WQ_INT8>(grid, st, x, M, K, w, scale, N, S, part, out, mode);
      else launch_mw8<C, XT, WQ_INT4>(grid, st, x, M, K, w, scale, N, S, part, out, mode);
    });
  });
  return 0;
}

}  // namespace xgk
