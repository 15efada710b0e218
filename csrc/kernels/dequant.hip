// Quantized weight -> bf16 [N, K] (row-major, contiguous): the prompt-sized steps of a
// model that keeps ONLY its fp8 / int8 / int4 weights dequantize one projection at a
// time into a shared scratch that the library GEMM then reads.
//
// Reads the three layouts of gemm_w8.hip (WQ_FP8 / WQ_INT8: codes [N, K], fp32 scale
// [N]; WQ_INT4: packed [N, K / 2] offset-binary nibbles, pair-interleaved words, fp32
// group scales [K / 128, N]). Per element: the code widened to fp32 (exact), ONE fp32
// multiply by its scale, ONE round-to-nearest-even conversion to bf16 -- bit-identical
// to dequantize_weight(q, s, fmt).to(bfloat16) of xgserve/ops/linear.py. (The true
// value q is needed here, so neither the GEMM's epilogue scaling nor its 136 + q
// form applies.)
//
// Pure streaming, no LDS: a lane loads one 16-B unit of codes non-temporally (read
// once); the unit holds 16 (8-bit) or 32 (int4) values, i.e. 32 or 64 B of output.
// Stored by the lane that loaded them, each 16-B store instruction would touch 64
// different 64-B segments a quarter or half full (int4 ran at 3.1 TB/s, fp8 / int8 at
// 4.0-5.4 that way), so the four lanes of a quad first exchange their code words and
// scales with quad_perm DPP moves: every store instruction then writes whole 64-B
// segments, one per quad (plain stores: the GEMM reads them next). Rows are whole
// numbers of units, so the flat unit index u addresses codes at 16 u and output
// elements at 16 u / 32 u; only the scale needs the row (u / units-per-row). Any N;
// K a multiple of 16 (int4: 32).
#include "common.h"

namespace xgk {

namespace {

enum : int { DQ_FP8 = 0, DQ_INT8 = 1, DQ_INT4 = 2 };  // = WQ_* of gemm_w8.hip
constexpr int DQ_GROUP = 128;    // int4 scale group (k)
constexpr int DQ_THREADS = 256;
constexpr int DQ_MAX_BLOCKS = 256 * 8;  // 8 workgroups (32 waves) per CU

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// quad_perm DPP move: lane 4m + r reads v of lane 4m + ((CTRL >> 2r) & 3). Executed by
// whole waves only (the unit loop is wave-uniform), so every source lane is live.
template <int CTRL>
__device__ __forceinline__ uint32_t quad_mov(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, false));
#else
  return v;
#endif
}

struct Unit {   // one lane's 16 B of codes and the scale of their (row, group)
  uint4 c;
  float s;
};

template <int CTRL>
__device__ __forceinline__ Unit quad_mov(Unit a) {
  Unit b;
  b.c = make_uint4(quad_mov<CTRL>(a.c.x), quad_mov<CTRL>(a.c.y), quad_mov<CTRL>(a.c.z), quad_mov<CTRL>(a.c.w));
  b.s = __uint_as_float(quad_mov<CTRL>(__float_as_uint(a.s)));
  return b;
}

// 4 E4M3 bytes * s -> two packed bf16 pairs
__device__ __forceinline__ uint2 fp8x4_scaled(uint32_t v, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(v, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(v, true);
  return make_uint2(pack2(lo[0] * s, lo[1] * s), pack2(hi[0] * s, hi[1] * s));
#else
  return make_uint2(0, 0);
#endif
}

// 4 int8 bytes * s -> two packed bf16 pairs
__device__ __forceinline__ uint2 i8x4_scaled(uint32_t v, float s) {
  const float a = static_cast<float>(static_cast<int8_t>(v & 0xFF));
  const float b = static_cast<float>(static_cast<int8_t>((v >> 8) & 0xFF));
  const float c = static_cast<float>(static_cast<int8_t>((v >> 16) & 0xFF));
  const float d = static_cast<float>(static_cast<int8_t>(v >> 24));
  return make_uint2(pack2(a * s, b * s), pack2(c * s, d * s));
}

// one int4 word (8 consecutive k: element 2j at bits 4j, element 2j + 1 at bits 16 + 4j) * s
__device__ __forceinline__ uint4 u4x8_scaled(uint32_t v, float s) {
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = static_cast<float>(static_cast<int>((v >> (4 * j)) & 15u) - 8);
    const float b = static_cast<float>(static_cast<int>((v >> (16 + 4 * j)) & 15u) - 8);
    o[j] = pack2(a * s, b * s);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// two 8-bit code words (8 consecutive k) * s -> 8 bf16
template <int FMT>
__device__ __forceinline__ uint4 b8x8_scaled(uint32_t w0, uint32_t w1, float s) {
  const uint2 p0 = FMT == DQ_FP8 ? fp8x4_scaled(w0, s) : i8x4_scaled(w0, s);
  const uint2 p1 = FMT == DQ_FP8 ? fp8x4_scaled(w1, s) : i8x4_scaled(w1, s);
  return make_uint4(p0.x, p0.y, p1.x, p1.y);
}

// The units qu .. qu + 3 of one quad (a = this lane's own unit, lane r of the quad) ->
// their bf16 values. Each store instruction covers one 64-B segment per quad:
//   int4 : store i = unit qu + i, lane r writes its word r (8 values);
//   8-bit: store h = units qu + 2h and qu + 2h + 1, lane r writes words 2 (r & 1) and
//          2 (r & 1) + 1 of unit qu + 2h + r / 2 (8 values).
// Units at or past `total` are not written.
template <int FMT>
__device__ __forceinline__ void store_quad(Unit a, uint32_t qu, int r, uint32_t total, uint16_t* __restrict__ out) {
  if constexpr (FMT == DQ_INT4) {
    uint16_t* o = out + static_cast<int64_t>(qu) * 32 + 8 * r;
#define XGK_DQ_STORE(I)                                                                        \
    {                                                                                          \
      const Unit b = quad_mov<0x55 * I>(a); /* unit qu + I in every lane of the quad */        \
      const uint32_t w = r == 0 ? b.c.x : r == 1 ? b.c.y : r == 2 ? b.c.z : b.c.w;             \
      if (qu + I < total) st16(o + 32 * I, u4x8_scaled(w, b.s));                               \
    }
    XGK_DQ_STORE(0) XGK_DQ_STORE(1) XGK_DQ_STORE(2) XGK_DQ_STORE(3)
#undef XGK_DQ_STORE
  } else {
    uint16_t* o = out + static_cast<int64_t>(qu) * 16 + 8 * r;
    const bool hi = r & 1;
    const Unit b0 = quad_mov<0x50>(a);  // lanes 0 0 1 1 of the quad
    if (qu + (r >> 1) < total) st16(o, b8x8_scaled<FMT>(hi ? b0.c.z : b0.c.x, hi ? b0.c.w : b0.c.y, b0.s));
    const Unit b1 = quad_mov<0xFA>(a);  // lanes 2 2 3 3
    if (qu + 2 + (r >> 1) < total) st16(o + 32, b8x8_scaled<FMT>(hi ? b1.c.z : b1.c.x, hi ? b1.c.w : b1.c.y, b1.s));
  }
}

//   total  16-B code units in the matrix (N * upr), upr = units per row
template <int FMT>
__global__ void __launch_bounds__(DQ_THREADS) dequant_w8_kernel(const uint8_t* __restrict__ q,
                                                                const float* __restrict__ scale, int N,
                                                                uint32_t upr, uint32_t total,
                                                                uint16_t* __restrict__ out) {
  constexpr int EPU = FMT == DQ_INT4 ? 32 : 16;   // elements per unit
  const uint32_t stride = gridDim.x * DQ_THREADS;
  const int lane = threadIdx.x & 63, r = lane & 3;
  auto load = [&](uint32_t u) {
    Unit a;
    a.c = make_uint4(0, 0, 0, 0);
    a.s = 0.f;
    if (u < total) {
      a.c = ld16_nt(q + static_cast<int64_t>(u) * 16);
      const uint32_t row = u / upr;
      if constexpr (FMT == DQ_INT4) {
        const uint32_t g = (u - row * upr) / (DQ_GROUP / EPU);  // a unit lies inside one group
        a.s = scale[static_cast<int64_t>(g) * N + row];
      } else {
        a.s = scale[row];
      }
    }
    return a;
  };
  // wb: the wave's first unit -- the loop is wave-uniform (whole waves reach the quad
  // exchange). Two units per lane and pass: both code loads are in flight before the
  // first conversion.
  for (uint32_t wb = blockIdx.x * DQ_THREADS + (threadIdx.x - lane); wb < total; wb += 2 * stride) {
    const Unit a0 = load(wb + lane);
    const Unit a1 = load(wb + stride + lane);
    store_quad<FMT>(a0, wb + (lane - r), r, total, out);
    if (wb + stride < total) store_quad<FMT>(a1, wb + stride + (lane - r), r, total, out);
  }
}

}  // namespace

// q: WQ_FP8 / WQ_INT8 codes [N, K] (scale [N]) or WQ_INT4 packed [N, K / 2] (scale
// [ceil(K / 128), N]) -> out bf16 [N, K]. Returns 0, or 1 for a shape it cannot take.
int dequant_w8(const uint8_t* q, const float* scale, int N, int K, uint16_t* out, int fmt, hipStream_t st) {
  if (q == nullptr || scale == nullptr || out == nullptr || N < 1 || K < 1) return 1;
  if (fmt != DQ_FP8 && fmt != DQ_INT8 && fmt != DQ_INT4) return 1;
  const int epu = fmt == DQ_INT4 ? 32 : 16;
  if (K % epu) return 1;  // rows of whole 16-B units
  const int64_t upr = K / epu, total = upr * N;
  if (total >= (int64_t{1} << 31)) return 1;
  const int64_t want = (total + 2 * DQ_THREADS - 1) / (2 * DQ_THREADS);
  const dim3 grid(static_cast<unsigned>(want < DQ_MAX_BLOCKS ? want : DQ_MAX_BLOCKS));
#define XGK_DQ(FMT)                                                                                   \
  hipLaunchKernelGGL((dequant_w8_kernel<FMT>), grid, dim3(DQ_THREADS), 0, st, q, scale, N,            \
                     static_cast<uint32_t>(upr), static_cast<uint32_t>(total), out)
  if (fmt == DQ_FP8) XGK_DQ(DQ_FP8);
  else if (fmt == DQ_INT8) XGK_DQ(DQ_INT8);
  else XGK_DQ(DQ_INT4);
#undef XGK_DQ
  return 0;
}

}  // namespace xgk
