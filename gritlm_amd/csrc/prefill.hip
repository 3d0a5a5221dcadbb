// Prompt prefill on top of a K/V cache for gfx950: a chunk of P prompt tokens per sequence, behind a cached prefix of lens[b] tokens.
//
// Replaces, for the native decoder's "gemm" prefill (gritlm_amd/decoder.py), the reference's sdpa attention with a cache
// (scripts/modeling_mistral_gritlm.py:619-705, the causal mask offset by the past length :1005-1036): query i of sequence b attends to
// keys 0 .. lens[b] + i of that sequence (GQA by index).  The q|k|v projections, RoPE at positions lens[b] + i, o_proj and the MLP are the
// encoder's MFMA GEMMs; this file holds the two launches that sit between them:
//
//   grit_kv_append_chunk         the chunk's post-RoPE k / v heads -> cache rows lens[b] + i (a copy: the GEMM epilogue rotated them)
//   grit_attn_prefill_cached_*   flash attention of the chunk's queries over cache rows 0 .. lens[b] + i
//
// The attention runs the tile loop and epilogue of attn_bidir_fwd_k (attn_tile.h) with one query block per workgroup and the same XCD
// grouping of the workgroups that read one (sequence, kv head)'s K / V.  What differs from the forward kernel (attention.hip):
//   * K and V are two allocations [B, nkv, Lmax, 128] with a 256-byte row: every piece carries its own per-lane address (key clamped to
//     the block's last visible key -- rows past it are finite copies, masked, so nothing outside the written cache is ever read);
//   * tiles that lie wholly at or before lens[b] + (the wave's first query) take the unmasked path; only the last tiles of a block carry
//     the causal mask; tiles past the block's last visible key are never loaded;
//   * Q rows come straight from global memory (one block per workgroup: no seam to hide them under);
//   * rows i >= plen[b] (right padding of the chunk) are written as zeros; no LSE.
#include "attn_tile.h"

namespace grit {

template <bool F16>
__global__ void __launch_bounds__(256, 2)
attn_prefill_cached_k(const uint16_t* __restrict__ q, const uint16_t* __restrict__ cache_k, const uint16_t* __restrict__ cache_v,
                      const int32_t* __restrict__ lens, const int32_t* __restrict__ plen, uint16_t* __restrict__ out, int P, int nq, int nkv,
                      int Lmax, int64_t q_stride, int64_t out_stride, float scale_log2, int nqb, int n_sets) {
  extern __shared__ __attribute__((aligned(256))) char smem[];
  typedef typename att_frag<F16>::type frag_t;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int gqa = nq / nkv;
  ATT_WG_DECODE(gqa * nqb, member)                // U = (heads per kv head) x (query blocks)
  const int h = hk * gqa + member % gqa;
  const int qb = member / gqa;
  int pl = plen[b], L0 = lens[b];
  pl = pl < 0 ? 0 : (pl > P ? P : pl);
  L0 = L0 < 0 ? 0 : (L0 > Lmax - 1 ? Lmax - 1 : L0);
  char* o_base = reinterpret_cast<char*>(out + (int64_t)b * P * out_stride + (int64_t)h * ATT_D);
  const uint32_t q_stride_b = (uint32_t)q_stride * 2u, out_stride_b = (uint32_t)out_stride * 2u;

  if (qb * ATT_QB >= pl) {
    // a block of padding rows only: zeros, 16 B per thread and pass (uniform per workgroup)
    const u32x4_t z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int pass = 0; pass < ATT_QB / 16; ++pass) {
      const int r = qb * ATT_QB + pass * 16 + (tid >> 4);
      if (r < P) *reinterpret_cast<u32x4_t*>(o_base + ((uint32_t)r * out_stride_b + (uint32_t)((tid & 15) << 4))) = z;
    }
    return;
  }
  const int qlast = (qb * ATT_QB + ATT_QB - 1) < (pl - 1) ? (qb * ATT_QB + ATT_QB - 1) : (pl - 1);
  const int kend = (L0 + qlast + 1) < Lmax ? (L0 + qlast + 1) : Lmax;          // keys 0 .. kend-1: what some row of the block sees
  const int ntiles = (kend + ATT_KB - 1) / ATT_KB;

  const char* q_base = reinterpret_cast<const char*>(q + (int64_t)b * P * q_stride + (int64_t)h * ATT_D);
  const char* k_base = reinterpret_cast<const char*>(cache_k + ((int64_t)b * nkv + hk) * Lmax * ATT_D);
  const char* v_base = reinterpret_cast<const char*>(cache_v + ((int64_t)b * nkv + hk) * Lmax * ATT_D);
  const int ql = lane & 31, hi = lane >> 5;

  // ---- LDS-DMA roles (as in attention.hip): wave w stages keys 16w .. 16w+15 of a tile, four 1-KiB pieces for K and four for V (4 keys each);
  //      lane -> LDS key row 16w + 4i + (lane>>4), physical 16-byte unit lane&15, which holds the LOGICAL unit (lane&15) ^ swizzle(row):
  //      K unit ^= row & 15, V unit ^= 4 (row & 3).  The swizzle follows the LDS row; the SOURCE row is clamped to kend - 1.
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int st_key = 16 * wv + (lane >> 4);
  const uint32_t v_unit_b = (uint32_t)(((lane & 15) ^ (4 * ((lane >> 4) & 3))) << 4);
  auto stage_piece = [&](int t, int buf, int i, int is_v) {
    char* dst = smem + buf * ATT_STAGE_BYTES + wv * 4096 + (is_v ? K_LDS_BYTES : 0) + i * 1024;
    int key = t * ATT_KB + st_key + 4 * i;
    key = key < kend ? key : kend - 1;
    const uint32_t unit_b = is_v ? v_unit_b : (uint32_t)(((lane & 15) ^ ((4 * i + (lane >> 4)) & 15)) << 4);
    const char* src = (is_v ? v_base : k_base) + ((uint32_t)key * (uint32_t)V_PITCH + unit_b);
    __builtin_amdgcn_global_load_lds((att_gptr_t)src, (att_lptr_t)dst, 16, 0, 0);
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) { stage_piece(0, 0, i, 0); stage_piece(0, 0, i, 1); }

  // ---- Q fragments (B operand), row per lane: Q[q][16ks + 8hi .. +8]; rows past plen read the last valid row (finite; stored as zeros)
  const int q_row = qb * ATT_QB + wave * 32 + ql;
  const int q_eff = q_row < pl ? q_row : pl - 1;
  frag_t qf[8];
  {
    const char* qp = q_base + ((uint32_t)q_eff * q_stride_b + (uint32_t)hi * 16u);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const frag_t*>(qp + ks * 32);
  }
  char* xs = smem + 2 * ATT_STAGE_BYTES + wv * ATT_XPOSE_BYTES;
  const int q_swz = (ql >> 1) & 7;

  const int kf_row = ql * 256, kf_x = lane & 15;   // K / V fragment addresses (attn_tile.h)
  const int vt_lane = ATT_VT_LANE(lane, hi);
  // the wave's first query sees keys 0 .. L0 + qw0: tiles wholly inside that range need no mask
  const int qw0 = qb * ATT_QB + wave * 32;
  const int n_row = L0 + q_eff + 1;                                   // keys the lane's query sees

  f32x16_t oacc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  ATT_WAIT_VM0();                                                      // first tile + Q rows
  for (int t = 0; t < ntiles; ++t) {
    if (t > 0) ATT_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // behind the last tile the pieces re-stage it into the idle stage (nobody reads it; waited for before the stores)
    const int st_t = (t + 1 < ntiles) ? t + 1 : t, st_buf = (t + 1) & 1;
    const char* k_lds = smem + (t & 1) * ATT_STAGE_BYTES;
    const char* v_lds = k_lds + K_LDS_BYTES;
    uint64_t word = ~0ull;
    bool fast = true;
    if (t * ATT_KB + ATT_KB - 1 > L0 + qw0) {                           // the tile reaches past what the wave's first query sees
      const int n = n_row - t * ATT_KB;
      word = n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull));
      fast = false;
    }

    f32x16_t sacc[2];
    ATT_TILE_QK(k_lds)
    ATT_TILE_PV(v_lds)
  }
  ATT_WAIT_VM0();                                                      // the re-staged last tile has landed before the workgroup leaves

  ATT_STORE_OUT(qw0, qr < P, qr < pl)
}

// The chunk's k / v heads (columns nq .. nq + 2 nkv of the fused q|k|v rows, already rotated) -> cache rows lens[b] + i, i < plen[b].
// One workgroup per chunk row, 16 bytes per thread: a 16-bit copy, the same for bf16 and fp16 caches.
__global__ void __launch_bounds__(256)
kv_append_chunk_k(const uint16_t* __restrict__ qkv, uint16_t* __restrict__ cache_k, uint16_t* __restrict__ cache_v, const int32_t* __restrict__ lens,
                  const int32_t* __restrict__ plen, int P, int nq, int nkv, int Lmax, int64_t qkv_stride) {
  const int row = blockIdx.x;
  const int b = row / P, i = row - b * P;
  if (i >= plen[b]) return;
  const int pos = lens[b] + i;
  if (pos < 0 || pos >= Lmax) return;                                 // (a chunk that does not fit the cache is not written past it)
  const uint16_t* src = qkv + (int64_t)row * qkv_stride + (int64_t)nq * ATT_D;
  for (int j = threadIdx.x; j < 2 * nkv * 16; j += blockDim.x) {
    const int head = j >> 4, unit = j & 15;                           // head < nkv: k head; else v head head - nkv
    const bool is_v = head >= nkv;
    const int hk = is_v ? head - nkv : head;
    uint16_t* dst = (is_v ? cache_v : cache_k) + (((int64_t)b * nkv + hk) * Lmax + pos) * ATT_D + unit * 8;
    *reinterpret_cast<u32x4_t*>(dst) = *reinterpret_cast<const u32x4_t*>(src + (int64_t)head * ATT_D + unit * 8);
  }
}

}  // namespace grit

using namespace grit;

template <bool F16>
static void prefill_launch(dim3 grid, hipStream_t st, const uint16_t* q, const uint16_t* cache_k, const uint16_t* cache_v, const int32_t* lens,
                           const int32_t* plen, uint16_t* out, int P, int nq, int nkv, int Lmax, int64_t q_stride, int64_t out_stride,
                           float scale_log2, int nqb, int n_sets) {
  static std::atomic<uint64_t> optin{0};
  attn_lds_optin(attn_prefill_cached_k<F16>, optin);
  hipLaunchKernelGGL(attn_prefill_cached_k<F16>, grid, dim3(256), ATT_LDS_BYTES, st, q, cache_k, cache_v, lens, plen, out, P, nq, nkv, Lmax,
                     q_stride, out_stride, scale_log2, nqb, n_sets);
}

static int prefill_attn(const char* name, bool f16, const void* q, const void* cache_k, const void* cache_v, const int32_t* lens,
                        const int32_t* plen, void* out, int B, int P, int nq, int nkv, int d, int Lmax, int64_t q_stride, int64_t out_stride,
                        float scale, void* stream) {
  GRIT_REQUIRE(q && cache_k && cache_v && lens && plen && out, GRIT_E_BADARG, "%s: null pointer", name);
  GRIT_REQUIRE(d == ATT_D, GRIT_E_UNSUPPORTED, "%s: head_dim=%d (only 128 is built)", name, d);
  GRIT_REQUIRE(B > 0 && P >= 1 && Lmax > 0 && nq > 0 && nkv > 0 && nq <= 65535 && nkv <= 65535, GRIT_E_BADARG,
               "%s: bad sizes (B=%d, P=%d, Lmax=%d, nq=%d, nkv=%d)", name, B, P, Lmax, nq, nkv);
  GRIT_REQUIRE(nq % nkv == 0, GRIT_E_BADARG, "%s: nq=%d not a multiple of nkv=%d", name, nq, nkv);
  GRIT_REQUIRE(q_stride % 8 == 0 && q_stride >= (int64_t)nq * d && out_stride % 8 == 0 && out_stride >= (int64_t)nq * d, GRIT_E_BADARG,
               "%s: bad strides", name);
  GRIT_REQUIRE(aligned16(q) && aligned16(cache_k) && aligned16(cache_v) && aligned16(out), GRIT_E_BADARG, "%s: pointers must be 16-byte aligned",
               name);
  GRIT_REQUIRE((int64_t)P * q_stride * 2 < (1ll << 31) && (int64_t)P * out_stride * 2 < (1ll << 31) && (int64_t)Lmax * V_PITCH < (1ll << 31),
               GRIT_E_UNSUPPORTED, "%s: one sequence spans more than 2 GiB (32-bit row offsets)", name);
  const int nqb = (P + ATT_QB - 1) / ATT_QB, n_sets = B * nkv;
  const int64_t grid = 8ll * ((n_sets + 7) / 8) * (nq / nkv) * nqb;
  GRIT_REQUIRE(grid < (1ll << 30), GRIT_E_UNSUPPORTED, "%s: grid too large", name);
  (f16 ? prefill_launch<true> : prefill_launch<false>)(dim3((unsigned)grid), (hipStream_t)stream, (const uint16_t*)q, (const uint16_t*)cache_k,
                                                       (const uint16_t*)cache_v, lens, plen, (uint16_t*)out, P, nq, nkv, Lmax, q_stride,
                                                       out_stride, scale * 1.4426950408889634f, nqb, n_sets);
  GRIT_CHECK_LAUNCH(name);
  return GRIT_OK;
}

extern "C" int grit_attn_prefill_cached_fwd(const void* q, const void* cache_k, const void* cache_v, const int32_t* lens, const int32_t* plen,
                                            void* out, int B, int P, int nq, int nkv, int d, int Lmax, int64_t q_stride, int64_t out_stride,
                                            float scale, void* stream) {
  return prefill_attn("grit_attn_prefill_cached_fwd", false, q, cache_k, cache_v, lens, plen, out, B, P, nq, nkv, d, Lmax, q_stride, out_stride,
                      scale, stream);
}
extern "C" int grit_attn_prefill_cached_f16_fwd(const void* q, const void* cache_k, const void* cache_v, const int32_t* lens, const int32_t* plen,
                                                void* out, int B, int P, int nq, int nkv, int d, int Lmax, int64_t q_stride, int64_t out_stride,
                                                float scale, void* stream) {
  return prefill_attn("grit_attn_prefill_cached_f16_fwd", true, q, cache_k, cache_v, lens, plen, out, B, P, nq, nkv, d, Lmax, q_stride, out_stride,
                      scale, stream);
}

extern "C" int grit_kv_append_chunk(const void* qkv, void* cache_k, void* cache_v, const int32_t* lens, const int32_t* plen, int B, int P, int nq,
                                    int nkv, int d, int Lmax, int64_t qkv_stride, void* stream) {
  const char* name = "grit_kv_append_chunk";
  GRIT_REQUIRE(qkv && cache_k && cache_v && lens && plen, GRIT_E_BADARG, "%s: null pointer", name);
  GRIT_REQUIRE(d == ATT_D, GRIT_E_UNSUPPORTED, "%s: head_dim=%d (only 128 is built)", name, d);
  GRIT_REQUIRE(B > 0 && P >= 1 && Lmax > 0 && nq > 0 && nkv > 0 && nkv <= 65535 && (int64_t)B * P < (1ll << 31), GRIT_E_BADARG,
               "%s: bad sizes (B=%d, P=%d, Lmax=%d, nq=%d, nkv=%d)", name, B, P, Lmax, nq, nkv);
  GRIT_REQUIRE(nq % nkv == 0, GRIT_E_BADARG, "%s: nq=%d not a multiple of nkv=%d", name, nq, nkv);
  GRIT_REQUIRE(qkv_stride % 8 == 0 && qkv_stride >= (int64_t)(nq + 2 * nkv) * d, GRIT_E_BADARG, "%s: bad stride", name);
  GRIT_REQUIRE(aligned16(qkv) && aligned16(cache_k) && aligned16(cache_v), GRIT_E_BADARG, "%s: pointers must be 16-byte aligned", name);
  hipLaunchKernelGGL(kv_append_chunk_k, dim3((unsigned)(B * P)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)qkv, (uint16_t*)cache_k,
                     (uint16_t*)cache_v, lens, plen, P, nq, nkv, Lmax, qkv_stride);
  GRIT_CHECK_LAUNCH(name);
  return GRIT_OK;
}
