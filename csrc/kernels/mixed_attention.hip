// Attention of a mixed step -- decode rows (one query token per running sequence) and
// prompt rows (prefill chunks) packed into one batch -- in ONE launch after rope_cache.
//
// The two halves are independent (different rows of QKV in, different rows out) and
// limited by different things: the prompt rows' prefill_attn2 workgroups run a serial
// key-tile chain on a fraction of the CUs with their K/V in L2, the decode rows'
// workgroups stream the paged cache from HBM with the MFMA pipe idle. Launched back to
// back each leaves the other's resource unused. Here they share a grid:
//   blocks [0, n_prefill)             prefill_attn2_body in the 8-wave configuration
//                                     prefill_attention picks for these prompt rows on
//                                     its own (pf2_default), heavy row tiles first as
//                                     in its own launch;
//   blocks [n_prefill, + n_decode)    decode_attn_body, the unfused no-split-K form
//                                     (KL for G <= 4, NB = 2) that decode_attention
//                                     launches for such a step.
// The branch is on blockIdx.x (block-uniform), the LDS is one buffer sized to the
// larger user, and no block waits for another: no tickets, no spins, no atomics. Both
// bodies are the code of their own kernels (included from their files) in the
// configurations of the separate launches, so every output row is computed by the
// same arithmetic in the same order: the results are bit-identical.
//
// A decode block holds TWO (sequence, kv head) items, waves 0-3 and waves 4-7 with an
// LDS region each: the prefill ring (96 or 128 KiB) allows one 8-wave block per CU, and
// the pair keeps the decode rows at the 8 waves per CU (two 4-wave workgroups) of their
// own launch. The one __syncthreads of the decode body then joins both items' waves;
// each item executes it exactly once, and an odd last item's partner waves have exited,
// which the barrier does not count. (Measurements, and the block shapes that lost:
// profiles/mixed_attn.md.)
#include <hip/hip_runtime.h>

#define XGK_ATTN_DEVICE_ONLY 1
#include "decode_attention.hip"
#include "prefill_attention.hip"

namespace xgk {

int rope_cache(uint16_t* qkv, int64_t row_stride, const int32_t* positions, const float* cos_sin, uint16_t* k_cache,
               uint16_t* v_cache, const int32_t* slot_mapping, int T, int Hq, int Hkv, int D, int block_size,
               int apply_rope, hipStream_t st);

struct MixedPrefillArgs {
  const uint16_t* q;
  const int32_t* block_tables;
  const int32_t* qsl;
  const int32_t* seq_lens;
  uint16_t* out;
  int bt_stride, num_seqs, tiles_per_seq, n_hg, n_blocks;
  float scale_log2;
};
struct MixedDecodeArgs {
  const uint16_t* q;
  const int32_t* block_tables;
  const int32_t* seq_lens;
  uint16_t* out;
  int bt_stride, n_items;
  float scale;
};

template <int GH, int KS, int NSLOT, int G>
struct MixedCfg {
  static constexpr int D = 128, NW = 8;
  static constexpr bool KL = G <= 4;  // as launch_decode
  static constexpr int PF_LDS = NSLOT * Pf2Cfg<NW, GH, KS, NSLOT>::SLOT;
  static constexpr int DEC_LDS = (DecodeSmem<D, G, false, KL>::BYTES + 15) / 16 * 16;
  static constexpr int LDS = PF_LDS > 2 * DEC_LDS ? PF_LDS : 2 * DEC_LDS;
  static_assert(LDS <= 160 * 1024, "LDS");
};

template <int GH, int KS, int NSLOT, int G>
__global__ void __launch_bounds__(512, 1) mixed_attn_kernel(MixedPrefillArgs p, MixedDecodeArgs d, int64_t q_stride,
                                                            const uint16_t* kc, const uint16_t* vc,
                                                            int64_t out_stride, int Hq, int Hkv, int bs) {
  using C = MixedCfg<GH, KS, NSLOT, G>;
  __shared__ __attribute__((aligned(16))) char lds[C::LDS];
  const int bid = blockIdx.x;
  if (bid < p.n_blocks) {
    prefill_attn2_body<C::NW, GH, KS, NSLOT>(bid, lds, p.q, q_stride, kc, vc, p.block_tables, p.bt_stride, p.qsl,
                                             p.seq_lens, p.out, out_stride, p.num_seqs, Hq, Hkv, bs, p.scale_log2,
                                             p.tiles_per_seq, p.n_hg);
    return;
  }
  // decode item = (sequence, kv head), the kv head fastest as in decode_attention's grid
  const int half = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
  const int item = (bid - p.n_blocks) * 2 + half;
  if (item >= d.n_items) return;
  const QkvFuse nofuse{nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  decode_attn_body<C::D, G, false, C::KL, 2, 0, true>(item % Hkv, item / Hkv, 0, threadIdx.x & 255, 256,
                                                      lds + half * C::DEC_LDS, d.q, q_stride, kc, vc, d.block_tables,
                                                      d.bt_stride, d.seq_lens, nullptr, nullptr, d.out, out_stride,
                                                      Hq, Hkv, bs, d.scale, 1, nofuse);
}

// the launch; p holds the grid split (tiles_per_seq, n_hg, n_blocks) and `blocks` the whole grid
template <int GH, int KS, int NSLOT, int G>
static void launch_mixed(const MixedPrefillArgs& p, const MixedDecodeArgs& d, unsigned blocks, int64_t q_stride,
                         const uint16_t* kc, const uint16_t* vc, int64_t out_stride, int Hq, int Hkv, int bs,
                         hipStream_t st) {
  hipLaunchKernelGGL((mixed_attn_kernel<GH, KS, NSLOT, G>), dim3(blocks), dim3(512), 0, st, p, d, q_stride, kc, vc,
                     out_stride, Hq, Hkv, bs);
}
using MixedLaunch = void (*)(const MixedPrefillArgs&, const MixedDecodeArgs&, unsigned, int64_t, const uint16_t*,
                             const uint16_t*, int64_t, int, int, int, hipStream_t);

// the instantiation for a GQA group and a prefill configuration of pf2_default, or nullptr
static MixedLaunch mixed_launcher(int G, const Pf2Choice& c) {
  if (c.nw != 8 || !((c.ks == 1 && c.ns == 3) || (c.ks == 2 && c.ns == 2))) return nullptr;
#define XGK_MIX(GH, GG) \
  if (G == GG && c.gh == GH) return c.ks == 1 ? &launch_mixed<GH, 1, 3, GG> : &launch_mixed<GH, 2, 2, GG>;
  XGK_MIX(1, 1) XGK_MIX(2, 2) XGK_MIX(2, 4) XGK_MIX(2, 8)
#undef XGK_MIX
  return nullptr;
}

// rope_cache over all T rows of qkv [T, (Hq + 2 Hkv) D], then the attention of rows
// [0, nd) (decode: one token per sequence) and [nd, T) (num_pre prompt chunks) in one
// launch. Returns -1 for what the fused form does not cover -- D != 128, a GQA group
// outside {1, 2, 4, 8}, no decode row or no prompt row, a grid past 2^31 - 1 blocks --,
// and every such exit lies before the first launch: a refusal has enqueued nothing.
int mixed_attention(uint16_t* qkv, int64_t row_stride, const int32_t* positions, const float* cos_sin,
                    uint16_t* kc, uint16_t* vc, const int32_t* slot_mapping, int T, int nd, const int32_t* dec_bt,
                    int dec_bt_stride, const int32_t* dec_seq_lens, const int32_t* pre_bt, int pre_bt_stride,
                    const int32_t* pre_qsl, const int32_t* pre_seq_lens, int num_pre, int max_q_len, uint16_t* out,
                    int64_t out_stride, int Hq, int Hkv, int D, int bs, float scale, int apply_rope,
                    hipStream_t st) {
  if (D != 128 || nd <= 0 || T <= nd || num_pre <= 0 || max_q_len <= 0) return -1;
  if (Hkv <= 0 || Hq % Hkv != 0 || bs <= 0 || bs % 16 != 0) return -1;
  const int G = Hq / Hkv;
  const Pf2Choice c = pf2_default(num_pre, max_q_len, Hq, G);  // {8, G even ? 2 : 1, KS, NSLOT}: (1, 3) or (2, 2)
  const MixedLaunch launch = mixed_launcher(G, c);
  if (launch == nullptr) return -1;
  const int bm = 32 * (c.nw / c.gh / c.ks);
  const int tiles_per_seq = (max_q_len + bm - 1) / bm, n_hg = Hq / c.gh;
  const int64_t n_items = static_cast<int64_t>(nd) * Hkv;
  const int64_t n_prefill = static_cast<int64_t>(num_pre) * tiles_per_seq * n_hg;
  const int64_t n_decode = (n_items + 1) / 2;
  if (n_items > 0x7fffffff || n_prefill + n_decode > 0x7fffffff) return -1;
  // (rope_cache refuses only T <= 0 and D outside {64, 128}, both excluded above)
  if (rope_cache(qkv, row_stride, positions, cos_sin, kc, vc, slot_mapping, T, Hq, Hkv, D, bs, apply_rope, st) != 0)
    return -1;
  const MixedPrefillArgs p{qkv + static_cast<int64_t>(nd) * row_stride, pre_bt, pre_qsl, pre_seq_lens,
                           out + static_cast<int64_t>(nd) * out_stride, pre_bt_stride, num_pre, tiles_per_seq, n_hg,
                           static_cast<int>(n_prefill), scale * 1.4426950408889634f};
  const MixedDecodeArgs d{qkv, dec_bt, dec_seq_lens, out, dec_bt_stride, static_cast<int>(n_items), scale};
  launch(p, d, static_cast<unsigned>(n_prefill + n_decode), row_stride, kc, vc, out_stride, Hq, Hkv, bs, st);
  return 0;
}

}  // namespace xgk
