// The LDS-DMA decode pipeline of gemm_m64g (dense and grouped; gemm_w8 runs the same
// pipeline from its own copy, see the note above its kernel):
// out = x . W^T for up to 16 * MT rows of bf16 x, every operand staged by
// global_load_lds_dwordx4 (glds.h) -- each wave instruction moves 1024 B of full rows
// straight into LDS:
//   * a K chunk is KC wide; 3 LDS slots, 2 chunks in flight;
//   * W: each wave DMAs its own 16 * NW rows into a wave-private region of the slot;
//     x: the WV waves share the 16 * MT rows (XI instructions each);
//   * LDS images are lane-linear (DMA writes base + lane * 16) with the 16-B granule
//     XOR-swizzle (granule ^ (row & 15)) applied on the GLOBAL source address and undone
//     on the ds_read_b128 fragment reads (conflict-free);
//   * one raw s_barrier per chunk after a COUNTED vmcnt (the next chunk stays in flight
//     across it), never __syncthreads (its fence would drain the DMA queue); WAR: a slot
//     is re-filled only after the barrier that follows its last reads
//     (cdna_hip_programming.md §5 "Pipelining across barriers");
//   * acc[nt][mt][r] = out[row 16 mt + li][column 16 nt + 4 g + r of the wave's 16 * NW],
//     lane = 16 g + li.
#pragma once

#include "glds.h"

namespace xgk {

// x DMA instructions per wave per chunk of a 16 * mt-row x tile (a wave instruction moves
// 1024 B = 512 / kc bf16 rows). 0: the tile is less than one instruction per wave, and no
// kernel of that shape exists (the launchers ask this; M64Geom asserts it).
constexpr int m64_x_dmas(int wv, int kc, int mt) { return 16 * mt / (512 / kc) / wv; }

// Slot geometry. x rows are bf16 (2 KC bytes); weight rows are WRB bytes (2 KC for bf16,
// KC for 8-bit codes, KC / 2 for 4-bit codes).
template <int NW, int WV, int KC, int MT, int WRB_ = 2 * KC>
struct M64Geom {
  static constexpr int XRB = 2 * KC, WRB = WRB_;                // bytes per LDS row
  static constexpr int XG = XRB / 16, WG = WRB / 16;            // 16-B granules per row
  static constexpr int XRPI = 1024 / XRB, WRPI = 1024 / WRB;    // rows per DMA instruction (64 lanes x 16 B)
  static constexpr int XROWS = 16 * MT, XBYTES = XROWS * XRB;
  static constexpr int XI = m64_x_dmas(WV, KC, MT);             // x DMA instructions per wave per chunk
  static constexpr int WROWS = 16 * NW, WBYTES = WROWS * WRB;   // weight rows / bytes per wave per slot
  static constexpr int WI = WROWS / WRPI;                       // weight DMA instructions per wave per chunk
  static constexpr int SLOT = XBYTES + WV * WBYTES;
  static constexpr int G = XI + WI;                             // DMAs per wave per chunk: the counted wait
  static constexpr int COLS = 16 * NW * WV;                     // columns per workgroup
  static_assert(XI >= 1 && WI >= 1 && XROWS % (XRPI * WV) == 0 && WROWS % WRPI == 0, "bad m64 geometry");
  // the row a lane fetches in its wave's i-th x / W instruction (x: of the tile, W: of
  // the wave's rows) and the swizzled 16-B source granule of that row
  static __device__ __forceinline__ int x_row(int wid, int i, int lane) { return XRPI * (wid * XI + i) + lane / XG; }
  static __device__ __forceinline__ int w_row(int i, int lane) { return WRPI * i + lane / WG; }
  static __device__ __forceinline__ int x_gran(int r, int lane) { return (lane % XG) ^ (r & (XG - 1)); }
  static __device__ __forceinline__ int w_gran(int r, int lane) { return (lane % WG) ^ (r & (WG - 1)); }
};

// One chunk's DMAs of a wave: x from xsrc[i] + kx, W from wsrc[i] + kw (non-temporal when
// NT and nt: a weight stream read once keeps the activations in L2).
template <class GM, bool NT, class TX, class TW>
__device__ __forceinline__ void m64_issue(uint8_t* slot, int wid, const TX* const (&xsrc)[GM::XI], int kx,
                                          const TW* const (&wsrc)[GM::WI], int kw, bool nt = true) {
#pragma unroll
  for (int i = 0; i < GM::XI; ++i) glds16(xsrc[i] + kx, slot + GM::XRPI * (wid * GM::XI + i) * GM::XRB);
  if (NT && nt) {
#pragma unroll
    for (int i = 0; i < GM::WI; ++i) glds16_nt(wsrc[i] + kw, slot + GM::XBYTES + wid * GM::WBYTES + i * 1024);
  } else {
#pragma unroll
    for (int i = 0; i < GM::WI; ++i) glds16(wsrc[i] + kw, slot + GM::XBYTES + wid * GM::WBYTES + i * 1024);
  }
}

// Three-slot ring over chunks 0 .. nchunks - 1: chunk c lives in slot c % 3. Prologue:
// chunks 0 and 1 into their slots (a kernel with loads of its own to place ahead of the
// first DMA issues them itself). Per chunk: counted wait (chunk c + 1 stays in flight; 0
// on the last), barrier, DMA chunk c + 2 into the slot that barrier freed, compute c.
// issue(slot, c), compute(slot, c).
template <class Issue>
__device__ __forceinline__ void m64_ring_prologue(uint8_t* s0, uint8_t* s1, int nchunks, Issue&& issue) {
  issue(s0, 0);
  if (nchunks > 1) issue(s1, 1);
}
template <int G, class Issue, class Compute>
__device__ __forceinline__ void m64_ring(uint8_t* s0, uint8_t* s1, uint8_t* s2, int nchunks, Issue&& issue,
                                         Compute&& compute) {
  auto step = [&](uint8_t* cur, uint8_t* nxt2, int c) {
    if (c + 1 < nchunks) wait_vmcnt<G>();
    else wait_vmcnt<0>();
    raw_barrier();
    if (c + 2 < nchunks) issue(nxt2, c + 2);
    compute(cur, c);
  };
  int c = 0;
  for (; c + 3 <= nchunks; c += 3) {
    step(s0, s2, c);
    step(s1, s0, c + 1);
    step(s2, s1, c + 2);
  }
  if (c < nchunks) step(s0, s2, c);
  if (c + 1 < nchunks) step(s1, s0, c + 1);
}

template <int NW, int MT>
__device__ __forceinline__ void m64_zero(f32x4_t (&acc)[NW][MT]) {
#pragma unroll
  for (int nt = 0; nt < NW; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}

// One chunk of bf16 x bf16 MFMAs from the swizzled LDS image of a slot.
template <class GM, int NW, int MT>
__device__ __forceinline__ void m64_compute_bf16(const uint8_t* slot, int wid, int g, int li, f32x4_t (&acc)[NW][MT]) {
  const uint8_t* xs = slot;
  const uint8_t* ws = slot + GM::XBYTES + wid * GM::WBYTES;
#pragma unroll
  for (int t = 0; t < GM::XRB / 64; ++t) {
    const int phys = (4 * t + g) ^ (li & (GM::XG - 1));
    uint4 b[MT], a[NW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) b[mt] = *reinterpret_cast<const uint4*>(xs + (16 * mt + li) * GM::XRB + phys * 16);
#pragma unroll
    for (int nt = 0; nt < NW; ++nt) a[nt] = *reinterpret_cast<const uint4*>(ws + (16 * nt + li) * GM::WRB + phys * 16);
#pragma unroll
    for (int nt = 0; nt < NW; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = mfma16x16x32(as_frag(a[nt]), as_frag(b[mt]), acc[nt][mt]);
  }
}

// Stores of an acc[NW][MT] tile: lane row = row0 + 16 mt + li (GUARD: rows >= M are
// skipped), lane columns col0 + 16 nt + 4 g .. + 3 (col0 = the wave's first), `ld` = row stride.
// fp32 partials: plain, or write-through (st16_sc1) for an in-launch hand-off.
template <bool GUARD, int NW, int MT>
__device__ __forceinline__ void m64_store_f32(const f32x4_t (&acc)[NW][MT], float* p, int row0, int M, int ld,
                                              int col0, int g, int li, bool write_through) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = row0 + 16 * mt + li;
    if (GUARD && m >= M) continue;
#pragma unroll
    for (int nt = 0; nt < NW; ++nt) {
      float* dst = p + static_cast<int64_t>(m) * ld + col0 + 16 * nt + 4 * g;
      if (write_through) st16_sc1(dst, acc[nt][mt]);
      else
        *reinterpret_cast<float4*>(dst) = make_float4(acc[nt][mt][0], acc[nt][mt][1], acc[nt][mt][2], acc[nt][mt][3]);
    }
  }
}

template <bool GUARD, int NW, int MT>
__device__ __forceinline__ void m64_store_bf16(const f32x4_t (&acc)[NW][MT], uint16_t* out, int row0, int M, int ld,
                                               int col0, int g, int li) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = row0 + 16 * mt + li;
    if (GUARD && m >= M) continue;
#pragma unroll
    for (int nt = 0; nt < NW; ++nt) {
      uint2 v;
      v.x = pack2(acc[nt][mt][0], acc[nt][mt][1]);
      v.y = pack2(acc[nt][mt][2], acc[nt][mt][3]);
      *reinterpret_cast<uint2*>(out + static_cast<int64_t>(m) * ld + col0 + 16 * nt + 4 * g) = v;
    }
  }
}

// SiLU gate (NW == 2: tile 0 = gate, tile 1 = up of the block-16 interleaved weight rows):
// out[m][col0 / 2 + 4 g .. + 3] = silu(gate) * up, `ld` = the output's row stride (N / 2).
template <bool GUARD, int NW, int MT>
__device__ __forceinline__ void m64_store_silu(const f32x4_t (&acc)[NW][MT], uint16_t* out, int row0, int M, int ld,
                                               int col0, int g, int li) {
  static_assert(NW == 2, "the SiLU gate needs a gate and an up tile");
  const int f0 = col0 / 2 + 4 * g;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = row0 + 16 * mt + li;
    if (GUARD && m >= M) continue;
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gt = acc[0][mt][r];
      o[r] = gt / (1.f + __expf(-gt)) * acc[1][mt][r];
    }
    uint2 v;
    v.x = pack2(o[0], o[1]);
    v.y = pack2(o[2], o[3]);
    *reinterpret_cast<uint2*>(out + static_cast<int64_t>(m) * ld + f0) = v;
  }
}

}  // namespace xgk
