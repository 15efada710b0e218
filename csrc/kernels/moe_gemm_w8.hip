// moe_gemm_w8: the grouped (MoE) form of gemm_w8 -- out[p] = x[rows[p]] . dequant(W[e(p)])^T
// over the block-64 padded expert-sorted layout of moe_align, with the expert weights as
// fp8 / int8 / int4 codes (the layouts of gemm_w8.hip, one matrix per expert):
//   fp8 / int8: codes uint8 [E, N, K], fp32 scale per output channel [E, N];
//   int4:       codes [E, N, K / 2] (pair-packed offset-binary), fp32 group scales
//               [E, K / 128, N].
// A batch-1 Mixtral step streams its two active experts' weights and nothing else: on codes
// that is half (a quarter) of the bf16 bytes.
//
// Work split: grid (column tiles, K splits, 64-row tiles of the padded layout), column
// tile fastest so consecutive workgroups spread over the XCDs. A workgroup finds its expert
// from offs[] and leaves on capacity padding; the z extent stops at the row tiles that can
// hold real rows (ceil(pairs / 64) + min(E, pairs)).
// Data movement: the LDS-DMA ring of m64_pipe.h (three slots, two chunks in flight, counted
// vmcnt + one raw barrier per chunk, swizzle on the global source address) with code rows
// of KC bytes (KC / 2 for int4) beside bf16 x rows of 2 KC bytes. x rows are gathered
// through rows[]; a pad row reads its tile's first row, so no address leaves x. Weight DMA
// is non-temporal only when the expert's segment is one 64-row tile: further row tiles
// re-read the column tile from L2 / MALL.
// Row bodies: with 1-byte or half-byte weights the x tile, re-read by every column tile of
// an expert, is the larger share of a workgroup's traffic (KC 128, 128 columns, 64 rows:
// 16 KB of x beside 16 / 8 KB of codes per chunk). Each workgroup counts the real rows of
// its tile in `valid` and runs the 16-, 32- or 64-row body; KC 256 configurations have the
// 16-row body only (max_rows <= 16), as in the dense kernel. Rows past the body's 16 * MT
// are not written (pads only: w2 runs the same body on the same rows).
// Arithmetic: codes widened in registers (wq_widen.h) into the bf16 MFMA. fp8 / int8 take
// expert e's channel scale in the epilogue. int4 stages expert e's group scales for the
// workgroup's columns and K split in LDS before the first DMA is in flight, accumulates
// sum x (136 + q) per group with sum x from an all-ones MFMA, and at every group end folds
// acc = fma(s, fma(-136, sum x, acc_g), acc): explicit fmaf, so the fold is the same two
// roundings however the compiler would contract it.
// Epilogues: fp32 split-K partials [S, P, N] (reduced by moe_combine) or bf16
// silu(gate) * up [P, N / 2] from block-16 interleaved gate|up rows (NW = 2, split 1).
#include <algorithm>

#include "m64_pipe.h"
#include "cfg_dispatch.h"
#include "gemm_api.h"
#include "wq_widen.h"

namespace xgk {

enum : int { W8G_PARTIAL = 1, W8G_SILU = 2 };

// One row tile on the MT-row-sub-tile geometry inside the kernel's ring buffers.
template <int NW, int WV, int KC, int MT, int FMT>
__device__ __forceinline__ void moe_w8_body(const uint16_t* __restrict__ x, const int32_t* __restrict__ rows, int e,
                                            bool nt, int rt, int K, const uint8_t* __restrict__ w,
                                            const float* __restrict__ wscale, int N, int P,
                                            float* __restrict__ part, uint16_t* __restrict__ out, int mode,
                                            uint8_t* lds0, uint8_t* lds1, uint8_t* lds2, const float* sc_lds,
                                            int krot) {
  constexpr bool I4 = FMT == WQ_INT4;
  using GM = M64Geom<NW, WV, KC, MT, I4 ? KC / 2 : KC>;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int S = gridDim.y, s = blockIdx.y;
  const int kws = K / S;
  const int k0 = s * kws;
  const int nchunks = kws / KC;
  const int nbase = blockIdx.x * GM::COLS + wid * GM::WROWS;
  const int64_t wrow = I4 ? K / 2 : K;  // bytes per code row
  const uint8_t* we = w + static_cast<int64_t>(e) * N * wrow + (I4 ? k0 / 2 : k0);
  const uint8_t* wsrc[GM::WI];
#pragma unroll
  for (int i = 0; i < GM::WI; ++i) {
    const int r = GM::w_row(i, lane);
    wsrc[i] = we + static_cast<int64_t>(nbase + r) * wrow + 16 * GM::w_gran(r, lane);
  }
  // x rows gathered through the layout; a pad row reads the tile's first row
  const int first = rows ? max(rows[rt], 0) : rt;
  const uint16_t* xsrc[GM::XI];
#pragma unroll
  for (int i = 0; i < GM::XI; ++i) {
    const int r = GM::x_row(wid, i, lane);
    int src = rows ? rows[rt + r] : rt + r;
    if (src < 0) src = first;
    xsrc[i] = x + static_cast<int64_t>(src) * K + k0 + 8 * GM::x_gran(r, lane);
  }
  // K-chunk rotation (k_rotation): expert e's column tiles spread over K
  const int rot = krot ? static_cast<int>((blockIdx.x * 37u + e * 11u) % static_cast<unsigned>(nchunks)) : 0;
  auto chunk_of = [&](int c) {
    const int cr = c + rot;
    return cr >= nchunks ? cr - nchunks : cr;
  };
  auto issue = [&](uint8_t* slot, int c) {
    const int kk = chunk_of(c) * KC;
    m64_issue<GM, true>(slot, wid, xsrc, kk, wsrc, I4 ? kk / 2 : kk, nt);
  };

  f32x4_t acc[NW][MT];
  m64_zero(acc);
  // int4: the open group's sum x (136 + q) and sum x (every row of an all-ones MFMA)
  f32x4_t accg[I4 ? NW : 1][I4 ? MT : 1];
  f32x4_t xs[I4 ? MT : 1];
  if constexpr (I4) {
    m64_zero(accg);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xs[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const bf16x8_t ones = as_frag(make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));
  // fold group gi of this split (int4): acc += s (acc_g - 136 sum x), then reopen
  auto fold = [&](int gi) {
#pragma unroll
    for (int nt2 = 0; nt2 < NW; ++nt2) {
      const float4 sc = *reinterpret_cast<const float4*>(sc_lds + gi * GM::COLS + wid * GM::WROWS + 16 * nt2 + 4 * g);
      const float scr[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[nt2][mt][r] = fmaf(scr[r], fmaf(-136.f, xs[mt][r], accg[nt2][mt][r]), acc[nt2][mt][r]);
        accg[nt2][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xs[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  };

  auto compute = [&](const uint8_t* slot, int c) {
    const uint8_t* xsl = slot;
    const uint8_t* ws = slot + GM::XBYTES + wid * GM::WBYTES;
    const int kc0 = chunk_of(c) * KC;  // this chunk's k within the split (int4: its groups)
#pragma unroll
    for (int t = 0; t < KC / 32; ++t) {
      // x (B operand): row 16 mt + li, k = 32 t + 8 g .. -> bf16 granule 4 t + g
      uint4 b[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int xr = 16 * mt + li;
        b[mt] = *reinterpret_cast<const uint4*>(xsl + xr * GM::XRB + (((4 * t + g) ^ (xr & (GM::XG - 1))) * 16));
      }
#pragma unroll
      for (int nt2 = 0; nt2 < NW; ++nt2) {
        const int row = 16 * nt2 + li;
        bf16x8_t a;
        if constexpr (I4) {
          // code row 16 nt + li, k = 32 t + 8 g .. -> 4-bit granule t, bytes 4 g .. 4 g + 3
          a = u4x8_to_bf16(*reinterpret_cast<const uint32_t*>(ws + row * GM::WRB +
                                                              ((t ^ (row & (GM::WG - 1))) * 16) + 4 * g));
        } else {
          // code row 16 nt + li, k = 32 t + 8 g .. -> byte granule 2 t + g / 2, byte (g & 1) * 8
          const uint2 a8 = *reinterpret_cast<const uint2*>(ws + row * GM::WRB +
                                                           (((2 * t + (g >> 1)) ^ (row & (GM::WG - 1))) * 16) +
                                                           (g & 1) * 8);
          a = FMT == WQ_INT8 ? int8x8_to_bf16(a8) : fp8x8_to_bf16(a8);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if constexpr (I4) accg[nt2][mt] = mfma16x16x32(a, as_frag(b[mt]), accg[nt2][mt]);
          else acc[nt2][mt] = mfma16x16x32(a, as_frag(b[mt]), acc[nt2][mt]);
        }
      }
      if constexpr (I4) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xs[mt] = mfma16x16x32(ones, as_frag(b[mt]), xs[mt]);
        if ((t + 1) % (WQ_GROUP / 32) == 0) fold((kc0 + 32 * t) / WQ_GROUP);
      }
    }
  };

  m64_ring_prologue(lds0, lds1, nchunks, issue);
  m64_ring<GM::G>(lds0, lds1, lds2, nchunks, issue, compute);

  // acc[nt][mt][r] = out[row rt + 16 mt + li][n = nbase + 16 nt + 4 g + r] / scale[e][n]
  // (int4: the group scales are already folded in)
  if constexpr (!I4) {
    const float* se = wscale + static_cast<int64_t>(e) * N + nbase;
#pragma unroll
    for (int nt2 = 0; nt2 < NW; ++nt2) {
      const float4 sc = *reinterpret_cast<const float4*>(se + 16 * nt2 + 4 * g);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[nt2][mt][0] *= sc.x;
        acc[nt2][mt][1] *= sc.y;
        acc[nt2][mt][2] *= sc.z;
        acc[nt2][mt][3] *= sc.w;
      }
    }
  }
  // rows are not guarded: a body writes all of its 16 * MT rows (pads past the real ones)
  if (mode == W8G_PARTIAL) {
    m64_store_f32<false>(acc, part + static_cast<int64_t>(s) * P * N, rt, 0, N, nbase, g, li, false);
  } else if constexpr (NW == 2) {
    m64_store_silu<false>(acc, out, rt, 0, N / 2, nbase, g, li);
  }
}

//   NW  16-column MFMA tiles per wave (SiLU needs 2: one gate + one up tile)
//   WV  waves per workgroup
//   KC  k per chunk
//   MT_MAX  the largest row body of this launch (4: 64 rows; 1: every expert holds <= 16 rows)
template <int NW, int WV, int KC, int MT_MAX, int FMT>
__global__ void __launch_bounds__(64 * WV, 1) moe_gemm_w8_kernel(const uint16_t* __restrict__ x,
                                                                 const int32_t* __restrict__ rows,
                                                                 const int32_t* __restrict__ offs,
                                                                 const int32_t* __restrict__ valid, int E, int K,
                                                                 const uint8_t* __restrict__ w,
                                                                 const float* __restrict__ wscale, int N, int P,
                                                                 float* __restrict__ part, uint16_t* __restrict__ out,
                                                                 int mode, int krot) {
  constexpr bool I4 = FMT == WQ_INT4;
  using GMX = M64Geom<NW, WV, KC, MT_MAX, I4 ? KC / 2 : KC>;
  static_assert(3 * GMX::SLOT + (I4 ? WQ_SC_FLOATS * 4 : 16) <= LDS_BYTES, "ring");
  __shared__ __attribute__((aligned(1024))) uint8_t lds0[GMX::SLOT];
  __shared__ __attribute__((aligned(1024))) uint8_t lds1[GMX::SLOT];
  __shared__ __attribute__((aligned(1024))) uint8_t lds2[GMX::SLOT];
  // int4: expert e's group scales of this workgroup [group of the split][column] (unused otherwise)
  __shared__ __attribute__((aligned(16))) float sc_lds[I4 ? WQ_SC_FLOATS : 4];
  const int rt0 = blockIdx.z * 64;
  int e = -1;
  for (int i = 0; i < E; ++i)
    if (rt0 >= offs[i] && rt0 < offs[i + 1]) e = i;
  if (e < 0) return;  // capacity padding past the last segment
  const int p0 = offs[e], p1 = offs[e + 1];
  if constexpr (I4) {
    // staged before any LDS-DMA is in flight (host: groups x COLS <= WQ_SC_FLOATS)
    const int kws = K / static_cast<int>(gridDim.y);
    const int ng = kws / WQ_GROUP, g0 = static_cast<int>(blockIdx.y) * ng, col0 = blockIdx.x * GMX::COLS;
    const float* se = wscale + static_cast<int64_t>(e) * (K / WQ_GROUP) * N;
    for (int i = threadIdx.x; i < ng * GMX::COLS; i += 64 * WV)
      sc_lds[i] = se[static_cast<int64_t>(g0 + i / GMX::COLS) * N + col0 + i % GMX::COLS];
    __syncthreads();
  }
  // the real rows of this tile (they lead it) -> the 16-, 32- or 64-row body
  int amt = MT_MAX;
  if (valid != nullptr && MT_MAX > 1) {
    const int t = threadIdx.x;
    const int real = __syncthreads_count(t < 64 && rt0 + t < p1 && valid[rt0 + t] >= 0);
    amt = (real + 15) / 16;
  }
  // non-temporal weight loads only when the expert's column tile is read once
  const bool nt = (p1 - p0) <= 64;
  if constexpr (MT_MAX >= 4) {
    if (amt > 2) {
      moe_w8_body<NW, WV, KC, 4, FMT>(x, rows, e, nt, rt0, K, w, wscale, N, P, part, out, mode, lds0, lds1, lds2,
                                      sc_lds, krot);
      return;
    }
    if (amt == 2) {
      moe_w8_body<NW, WV, KC, 2, FMT>(x, rows, e, nt, rt0, K, w, wscale, N, P, part, out, mode, lds0, lds1, lds2,
                                      sc_lds, krot);
      return;
    }
  }
  moe_w8_body<NW, WV, KC, 1, FMT>(x, rows, e, nt, rt0, K, w, wscale, N, P, part, out, mode, lds0, lds1, lds2, sc_lds,
                                  krot);
}

// The launch configurations, indexed by cfg: (NW, waves, KC), gemm_w8's rows. Every row has
// the 16-row kernel (max_rows <= 16); the KC 128 rows also the 16 / 32 / 64-row kernel (at
// KC 256 four x tiles are a 32 KB x slot, past the LDS on the 4-wave row).
constexpr W8Cfg MOE_W8_CFGS[] = {{2, 4, 128}, {2, 2, 128}, {1, 4, 128}, {2, 2, 256}, {2, 4, 256}};
constexpr int MOE_W8_NCFG = table_size(MOE_W8_CFGS);
constexpr bool moe_w8_has_mt4(const W8Cfg& c) { return c.kc == 128; }
int moe_w8_cfgs(const W8Cfg** rows) {
  *rows = MOE_W8_CFGS;
  return MOE_W8_NCFG;
}

template <int FMT, int C>
static void launch_moe_w8(dim3 grid, hipStream_t st, const uint16_t* x, const int32_t* rows, const int32_t* offs,
                          const int32_t* valid, int E, int K, const uint8_t* w, const float* scale, int N, int P,
                          float* part, uint16_t* out, int mode, int max_rows) {
  static constexpr W8Cfg c = MOE_W8_CFGS[C];
  auto go = [&](auto mt) {
    hipLaunchKernelGGL((moe_gemm_w8_kernel<c.nw, c.wv, c.kc, decltype(mt)::value, FMT>), grid, dim3(64 * c.wv), 0, st,
                       x, rows, offs, valid, E, K, w, scale, N, P, part, out, mode,
                       k_rotation(static_cast<int>(grid.y)));
  };
  if constexpr (moe_w8_has_mt4(c)) {
    if (max_rows > 16) return go(Int<4>{});
  }
  go(Int<1>{});
}

bool moe_w8_supports(int E, int K, int N, int P, int S, int mode, int cfg, int fmt, int max_rows) {
  if (E < 1 || P < 0 || P % 64 || S < 1 || max_rows < 1 || cfg < 0 || cfg >= MOE_W8_NCFG || fmt < WQ_FP8 ||
      fmt > WQ_INT4)
    return false;
  const W8Cfg& c = MOE_W8_CFGS[cfg];
  if (max_rows > 16 && !moe_w8_has_mt4(c)) return false;
  if (mode != W8G_PARTIAL && mode != W8G_SILU) return false;
  if (K < 1 || N < 1 || N % c.cols() || K % (S * c.kc)) return false;
  if (mode == W8G_SILU && (c.nw != 2 || S != 1)) return false;
  // int4: whole groups per split, and the workgroup's scales of one expert fit its LDS stage
  return fmt != WQ_INT4 || ((K / S) % WQ_GROUP == 0 && (K / S / WQ_GROUP) * c.cols() <= WQ_SC_FLOATS);
}

// The operand contract of moe_gemm_m64g (rows or nullptr, offs[E + 1], valid or nullptr,
// max_rows, pairs) on codes: w / scale in the layouts at the top of this file.
int moe_gemm_w8(const uint16_t* x, const int32_t* rows, const int32_t* offs, int E, int K, const uint8_t* w,
                const float* scale, int N, int P, float* part, uint16_t* out, int S, int mode, int cfg, int fmt,
                int max_rows, hipStream_t st, const int32_t* valid, int pairs) {
  if (!moe_w8_supports(E, K, N, P, S, mode, cfg, fmt, max_rows)) return 1;
  if (x == nullptr || offs == nullptr || w == nullptr || scale == nullptr) return 1;
  if (mode == W8G_SILU ? out == nullptr : part == nullptr) return 1;
  if (P == 0) return 0;
  const int ztiles = pairs > 0 ? std::min(P / 64, (pairs + 63) / 64 + std::min(E, pairs)) : P / 64;
  const dim3 grid(N / MOE_W8_CFGS[cfg].cols(), S, ztiles);
  cfg_dispatch<MOE_W8_NCFG>(cfg, [&](auto c) {
    constexpr int C = decltype(c)::value;
    if (fmt == WQ_FP8)
      launch_moe_w8<WQ_FP8, C>(grid, st, x, rows, offs, valid, E, K, w, scale, N, P, part, out, mode, max_rows);
    else if (fmt == WQ_INT8)
      launch_moe_w8<WQ_INT8, C>(grid, st, x, rows, offs, valid, E, K, w, scale, N, P, part, out, mode, max_rows);
    else
      launch_moe_w8<WQ_INT4, C>(grid, st, x, rows, offs, valid, E, K, w, scale, N, P, part, out, mode, max_rows);
  });
  return 0;
}

}  // namespace xgk
