// Bidirectional (non-causal) flash attention forward for gfx950, GQA, head_dim 128, key-padding bitmask.
//
// Replaces repeat_kv + the additive [B,1,S,S] mask + F.scaled_dot_product_attention of
// scripts/modeling_mistral_gritlm.py (:182-191, :1017-1036, :690-698).  No repeat_kv copy (the kv head is
// index arithmetic), no mask tensor (one uint64 per 64 keys), no S x S score matrix.
//
// Structure: one 256-thread workgroup walks up to `qpw` consecutive 128-row query blocks of one (batch, head); each wave owns 32 rows of
// a block; two workgroups per CU.  The K/V tile stream runs THROUGH the block seams (the first tile of the next block is staged, and
// its Q rows are fetched into the same registers, under the last tile of the current one), so the per-block prologue (Q + first-tile latency) is paid once
// per workgroup and the output stores of a block drain under the next block's first tile.  Workgroups that share K/V (the GQA
// group's heads x query-block groups of one (batch, kv head)) are dealt to the SAME XCD back to back (block v runs on XCD v % 8).
// The tile loop itself -- LDS-DMA ring, swizzled K / V images, counted inline-asm LDS reads, the swapped products and the online
// softmax -- and the output epilogue are attn_tile.h, shared with the cached-K/V prefill (prefill.hip); this file holds the tile
// ranges, the key masks, the buffer-addressed K/V staging, the Q staging and the block seam.
#include <stdlib.h>

#include "attn_tile.h"

// ATT_TIMING (diagnostic build, tools/attn_phase_probe.sh): thread 0 of every workgroup writes s_memtime stamps (cycles since kernel entry) as
// raw u32 into the workgroup's LSE rows instead of the LSE -- where a workgroup's time goes between prologue, tiles, seams and stores
// (profiles/r05_attn_phase_probe.json).  Three scheduling experiments built on that picture were measured and did NOT ship
// (profiles/r05_attn_{prio,hpw}_ab.log; the priority variants are in git history, commit "ATT_PRIO_MODE"): a static
// s_setprio asymmetry between the two co-resident workgroups (+-1 %), 2 / 4 heads of a kv group per workgroup (-2 % / -12 %), and
// dropping the two lgkmcnt(0) of the output transposition (0 %).
#ifdef ATT_TIMING
#define ATT_STAMP() do { if (tid == 0 && att_ns < att_cap) { att_st[att_ns] = (uint32_t)(__builtin_readcyclecounter() - att_t0); ++att_ns; } } while (0)
#else
#define ATT_STAMP() do { } while (0)
#endif
// (ATT_DEFER_MAX (attn_tile.h) and ATT_ABLATE_STORES are the A/B knobs of tools/ubench/attn_ab.cpp.  The levers of round 3 -- asm reads, spread /
//  buffer-addressed / unconditional DMA pieces, early V reads, s_setprio over QK, xor K addresses, hoisted mask word, permlane row
//  maximum -- were each A/B'd as a compile-time variant against the kernel of the previous commit, bit-identical every time
//  (profiles/r03_attn_fwd_ab_asm_reads.log, 773 -> 870 TF at B 256 x S 512); the variants are resolved in this file, the round-2
//  kernel is rebuilt from git history by tools/ubench/build_attn_ab.sh.)

namespace grit {

// VARLEN: sequences are packed back to back (no padding rows at all); cu_seqlens[b] is the first row of sequence b and
// every key of a sequence is valid, so the key bitmask is synthesised from the length.
// CAUSAL: additionally key <= query (the generative branch of unified training, MistralSdpaAttention with is_causal=True,
// modeling_mistral_gritlm.py:690-698 / :1017-1036); tiles past the workgroup's last query are skipped.
// CAUSAL with window > 0 (Mistral's sliding window, modeling_mistral_gritlm.py:381-385 / the sliding-window causal mask of
// _prepare_4d_causal_attention_mask, :1005-1036): a query sees the `window` keys q - window + 1 .. q; tiles that lie wholly in front
// of a query block's first visible key are skipped as well.
// F16 (round 5, the encoder's "f16_operands" precision policy): q | k | v and the output hold IEEE fp16 (attn_tile.h).
template <bool VARLEN, bool CAUSAL, bool F16 = false>
__global__ void __launch_bounds__(256, 2)
attn_bidir_fwd_k(const uint16_t* __restrict__ qkv, const uint64_t* __restrict__ key_bits, const int32_t* __restrict__ cu_seqlens,
                 uint16_t* __restrict__ out, float* __restrict__ lse, int S_arg, int nq, int nkv, int64_t qkv_stride,
                 int64_t out_stride, float scale_log2, int qpw, int ngx, int n_sets, int window) {
  extern __shared__ __attribute__((aligned(256))) char smem[];          // 256: the asm read addresses OR / XOR lane constants into bits 7:4
  typedef typename att_frag<F16>::type frag_t;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int gqa = nq / nkv;
  ATT_WG_DECODE(gqa * ngx, member)                // U = (heads per kv head) x (query-block groups)
  const int h = hk * gqa + member % gqa;
  const int qb_first = (member / gqa) * qpw;
  ATT_SEQ_BOUNDS()
  if (qb_first * ATT_QB >= S) return;            // uniform per workgroup
#ifdef ATT_TIMING
  const uint64_t att_t0 = __builtin_readcyclecounter();
  uint32_t* att_st = reinterpret_cast<uint32_t*>(lse + ((int64_t)b * nq + h) * S_arg + (int64_t)qb_first * ATT_QB);
  int att_ns = 0;
  const int att_cap = qpw * ATT_QB;
  ATT_STAMP();                                                                      // [0] = 0
  if (tid == 0) {
    att_st[att_ns++] = (uint32_t)__builtin_amdgcn_s_memrealtime();                   // [1] = 100 MHz wall clock at entry
    att_st[att_ns++] = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);          // [2] = HW_REG_HW_ID
    att_st[att_ns++] = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20);         // [3] = HW_REG_XCC_ID
  }
#endif
  const int nqb = (S + ATT_QB - 1) / ATT_QB;
  const int nblk = (nqb - qb_first) < qpw ? (nqb - qb_first) : qpw;

  // Global addressing = workgroup-uniform 64-bit base (SGPR pair) + 32-bit per-lane byte offset: no 64-bit per-lane pointers to keep
  // alive (or spill) around the tile loop.  The launcher guarantees rows * stride * 2 < 2^31.
  const char* q_base = reinterpret_cast<const char*>(qkv + row0 * qkv_stride + (int64_t)h * ATT_D);
  const char* k_base = reinterpret_cast<const char*>(qkv + row0 * qkv_stride + (int64_t)(nq + hk) * ATT_D);
  const char* v_base = reinterpret_cast<const char*>(qkv + row0 * qkv_stride + (int64_t)(nq + nkv + hk) * ATT_D);
  char* o_base = reinterpret_cast<char*>(out + row0 * out_stride + (int64_t)h * ATT_D);
  const uint32_t qkv_stride_b = (uint32_t)qkv_stride * 2u, out_stride_b = (uint32_t)out_stride * 2u;

  const int ql = lane & 31, hi = lane >> 5;

  // ---- LDS-DMA roles: wave w stages keys 16w .. 16w+15 of a tile, four 1-KiB instructions for K and four for V (4 keys each);
  //      lane -> key 16w + 4i + (lane>>4), physical 16-byte unit lane&15, which holds the LOGICAL unit (lane&15) ^ swizzle(key)
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int st_key = 16 * wv + (lane >> 4);                                     // + 4i
  const uint32_t v_unit_b = (uint32_t)(((lane & 15) ^ (4 * ((lane >> 4) & 3))) << 4);   // V: unit ^= 4 (key & 3); key & 3 == (lane>>4) & 3
  auto stage_tile = [&](int t, int buf) {
    char* kdst = smem + buf * ATT_STAGE_BYTES + wv * 4096;
    char* vdst = kdst + K_LDS_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int key = t * ATT_KB + st_key + 4 * i;
      key = key < S ? key : S - 1;
      const uint32_t k_unit_b = (uint32_t)(((lane & 15) ^ ((4 * i + (lane >> 4)) & 15)) << 4);   // K: unit ^= key & 15
      const uint32_t row_b = (uint32_t)key * qkv_stride_b;
      __builtin_amdgcn_global_load_lds((att_gptr_t)(k_base + (row_b + k_unit_b)), (att_lptr_t)(kdst + i * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((att_gptr_t)(v_base + (row_b + v_unit_b)), (att_lptr_t)(vdst + i * 1024), 16, 0, 0);
    }
  };
  // one 1-KiB piece of a tile (the eight pieces of the next tile are issued BETWEEN the QK products of the current one --
  // an LDS-DMA instruction costs 60-185 issue cycles (guide, 'LDS-DMA piece issue cost'), eight of them in front of the first K read
  // held the whole tile back; between MFMAs the cost sits under the matrix pipe)
  // Buffer-addressed LDS-DMA (buffer_load_dwordx4 ... offen lds): the descriptor's range check zero-fills rows past the sequence (their
  // keys are masked anyway: finite K -> score -> -inf, P = 0 x finite V), so a piece needs no per-lane clamp / 32-bit multiply: the
  // lane's offset inside a tile (row + swizzled unit; V: + the distance of the V heads from the K heads) is a constant VGPR per piece,
  // the tile's row offset ONE scalar operand for all eight pieces, and ONE descriptor serves K and V (a V row of the last valid key
  // ends exactly at num_records; the next row of either operand starts (nq + nkv) x 256 - 256 >= 0 bytes behind it).
  const uint32_t v_delta_b = (uint32_t)nkv * ATT_D * 2u;
  const auto kv_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(k_base), (short)0, (int)((uint32_t)(S - 1) * qkv_stride_b + 256u + v_delta_b), 0x00020000);
  uint32_t pc_k[4], pc_v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pc_k[i] = (uint32_t)(st_key + 4 * i) * qkv_stride_b + (uint32_t)(((lane & 15) ^ ((4 * i + (lane >> 4)) & 15)) << 4);
    pc_v[i] = (uint32_t)(st_key + 4 * i) * qkv_stride_b + v_unit_b + v_delta_b;
  }
  auto stage_piece = [&](int t, int buf, int i, int is_v) {
    char* dst = smem + buf * ATT_STAGE_BYTES + wv * 4096 + (is_v ? K_LDS_BYTES : 0) + i * 1024;
    const uint32_t tile_b = (uint32_t)__builtin_amdgcn_readfirstlane(t * ATT_KB) * qkv_stride_b;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(kv_rsrc, (att_lptr_t)dst, 16, (int)(is_v ? pc_v[i] : pc_k[i]), (int)tile_b, 0, 0);
  };
  // the first tile's DMA goes out before anything else (tile 0 always exists: S > 0); with a window the first tile of the first block
  // is known only after the key bitmask has been scanned (below)
  if (!(CAUSAL && window > 0)) stage_tile(0, 0);

  // ---- Q fragments (B operand): lane holds Q[q][16ks + 8hi .. +8] of query block qb.  A row-per-lane global load touches 32 rows x 32 B
  //      per instruction (measured: the per-block Q fetch + O store in that shape cost 18 % of the kernel at S = 512), so Q comes
  //      in through the wave's private 4 KiB transposition buffer instead, one 64-column half (32 rows x 128 B) at a time: LDS-DMA of
  //      whole 128-byte row segments (4 instructions x 8 rows, 16-byte units swizzled by (row>>1)&7), then ds_read_b128 of the half's
  //      four k-slices.
  frag_t qf[8];
  char* xs = smem + 2 * ATT_STAGE_BYTES + wv * ATT_XPOSE_BYTES;
  const int q_swz = (ql >> 1) & 7;                                               // swizzle of the lane's own row
  // (per-block address arithmetic is recomputed from a laundered lane id where it is used: hoisted to kernel entry it would be spilled
  //  around the tile loop, and a scratch reload's vmcnt wait would sit in front of the hand-placed DMA)
  auto q_stage_half = [&](int qb, int half) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int x_row = ln >> 3, x_unit = ln & 7;                                  // row (+ 8j) and physical unit of a DMA piece
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 8 * j + x_row;
      int qr = qb * ATT_QB + wave * 32 + r;
      qr = qr < S ? qr : S - 1;
      const uint32_t unit_b = (uint32_t)((half * 8 + (x_unit ^ ((r >> 1) & 7))) << 4);   // logical unit held by physical unit x_unit of row r
      __builtin_amdgcn_global_load_lds((att_gptr_t)(q_base + ((uint32_t)qr * qkv_stride_b + unit_b)), (att_lptr_t)(xs + j * 1024), 16, 0, 0);
    }
  };
  auto q_read_half = [&](int half) {
    const char* rp = xs + ql * 128;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[half * 4 + ks] = *reinterpret_cast<const frag_t*>(rp + (((2 * ks + hi) ^ q_swz) << 4));
    ATT_WAIT_LGKM0();                           // the reads must have left the buffer before it is refilled (DMA) or rewritten (O staging)
  };
  // the workgroup's FIRST block takes its Q rows straight from global memory (row-per-lane loads, one round trip that overlaps the
  // first tile's DMA; two dependent passes through the 4 KiB buffer would put two memory latencies in front of the first product)
  {
    const int qr0 = qb_first * ATT_QB + wave * 32 + ql;
    const char* qp = q_base + ((uint32_t)(qr0 < S ? qr0 : S - 1) * qkv_stride_b + (uint32_t)hi * 16u);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      qf[ks] = *reinterpret_cast<const frag_t*>(qp + ks * 32);
    }
  }

  // number of KV tiles that contain at least one valid key (trailing padding is never loaded)
  int ntiles_all = 0;
  const uint64_t* bits = nullptr;
  if constexpr (VARLEN) {
    ntiles_all = (S + 63) >> 6;
  } else {
    const int W = (S + 63) >> 6;
    bits = key_bits + (int64_t)b * W;
    for (int w = W - 1; w >= 0; --w)
      if (bits[w] != 0) { ntiles_all = w + 1; break; }
  }

  const int kf_row = ql * 256, kf_x = lane & 15;   // K / V fragment addresses (attn_tile.h)
  const int vt_lane = ATT_VT_LANE(lane, hi);

  // KV tiles [t0, t1) of query block qb
  auto tile_range = [&](int qb, int& t0, int& t1) {
    t0 = 0;
    t1 = ntiles_all;
    if constexpr (CAUSAL) {
      const int lim = 2 * qb + 2;               // tiles holding keys <= the last query of this block
      t1 = t1 < lim ? t1 : lim;
      if (window > 0) {
        const int lo = qb * ATT_QB - window + 1;                // first key the block's FIRST query sees
        t0 = lo > 0 ? lo >> 6 : 0;
        t0 = t0 < t1 ? t0 : (t1 > 0 ? t1 - 1 : 0);             // never an empty range while the sequence has keys (the K/V stream
      }                                                        // through the block seams counts on one tile per block); its keys are
    }                                                          // then masked for every row
  };
  if (CAUSAL && window > 0) {
    int f0, f1;
    tile_range(qb_first, f0, f1);
    stage_tile(f0, 0);
  }

  int gt = 0;                                   // tiles consumed so far by this workgroup: tile g lives in stage g & 1
  ATT_WAIT_VM0();                               // first tile + first Q rows
  ATT_STAMP();                                  // [4] prologue done
  for (int qi = 0; qi < nblk; ++qi) {
    const int qb = qb_first + qi;
    const int q_row = qb * ATT_QB + wave * 32 + ql;
    int t_first, ntiles, next_first = 0, next_end;
    tile_range(qb, t_first, ntiles);
    const bool more = qi + 1 < nblk;
    if (more) tile_range(qb + 1, next_first, next_end);

    f32x16_t oacc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int t = t_first; t < ntiles; ++t, ++gt) {
      // tile t has landed (this wave's share: vmcnt; everybody's: the barrier) and every wave is done reading the other stage.  The
      // first tile of a block was waited for before the block loop / at the seam (before the previous block stored its output:
      // vmcnt counts stores, and the stores should drain under this tile, not in front of it).
      if (t > t_first) ATT_WAIT_VM0();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      ATT_STAMP();                              // per tile: past the barrier
      // the eight pieces are issued unconditionally: behind the workgroup's very last tile they re-stage that tile into the idle stage
      // (nobody reads it; the wait in front of the block's output stores covers it) instead of costing a uniform branch per piece
      const int st_t = (t + 1 < ntiles) ? t + 1 : (more ? next_first : t), st_buf = (gt + 1) & 1;
      // next block's Q, first 64 columns: fetched a whole tile ahead (the buffer is idle), so the wait at the top of the last tile
      // already covers it
      if (more && t + 2 == ntiles) q_stage_half(qb + 1, 0);
      const char* k_lds = smem + (gt & 1) * ATT_STAGE_BYTES;
      const char* v_lds = k_lds + K_LDS_BYTES;
      // the tile's key-mask word is fetched HERE (a scalar load; its latency sits under the QK products) and turned into `fast` before
      // the asm LDS reads of the PV products are requested: fetched where it is used, hipcc's lgkmcnt(0) for the scalar load waited for
      // the load's own round trip AND for the sixteen V reads just issued -- once per tile
      uint64_t word;
      if constexpr (VARLEN) {
        const int rem = S - t * ATT_KB;
        word = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull);
      } else {
        word = bits[t];
      }
      bool fast = (word == ~0ull);
      if constexpr (CAUSAL) {
        const int qw0 = qb * ATT_QB + wave * 32;                   // this wave's first query
        // tile reaches past the wave's first query, or starts in front of the first key the wave's LAST query sees: per-lane bounds
        if (t * ATT_KB + ATT_KB - 1 > qw0 || (window > 0 && t * ATT_KB < qw0 + 32 - window)) {
          const int n = q_row - t * ATT_KB + 1;                    // keys of this tile the lane's query may see
          word &= n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull));
          if (window > 0) {
            const int lo = n - window;                             // keys of this tile in front of the lane's window
            word &= lo <= 0 ? ~0ull : (lo >= 64 ? 0ull : (~0ull << lo));
          }
          fast = false;
        }
      }

      f32x16_t sacc[2];
      ATT_TILE_QK(k_lds)
      // the next block's Q rows replace this block's as soon as its last QK product has read them: the fetch lands under the
      // softmax and PV of the last tile, no second register set
      const bool q_next = more && t + 1 == ntiles;
      if (q_next) {
        if (ntiles - t_first == 1) { q_stage_half(qb + 1, 0); ATT_WAIT_VM0(); }
        q_read_half(0);
        q_stage_half(qb + 1, 1);    // the other 64 columns land under the softmax and the PV products
      }
      ATT_TILE_PV(v_lds)
    }

    // ---- block seam: the next block's first tile and Q rows (issued one tile ago) are waited for BEFORE this block's stores go out
    ATT_STAMP();                                // block: tile loop done
    ATT_WAIT_VM0();
    if (more) q_read_half(1);
    ATT_STAMP();                                // block: seam wait done

    // ---- epilogue (ATT_ABLATE_STORES: the stores are compiled but never executed)
#ifdef ATT_ABLATE_STORES
    ATT_STORE_OUT(qb * ATT_QB + wave * 32, qr < S && scale_log2 < -1e30f, true)
#else
    ATT_STORE_OUT(qb * ATT_QB + wave * 32, qr < S, true)
#endif
    ATT_STAMP();                                // block: output stores issued
#ifdef ATT_TIMING
    if (qi + 1 == nblk && tid == 0 && att_ns + 1 < att_cap) { att_st[att_ns++] = (uint32_t)__builtin_amdgcn_s_memrealtime(); att_st[att_ns++] = 0xffffffffu; }
#else
    if (q_row < S && lse != nullptr && hi == 0) {
      if constexpr (VARLEN) lse[(row0 + q_row) * nq + h] = (m_run + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f;  // [T, nq]
      else lse[((int64_t)b * nq + h) * S + q_row] = (m_run + __builtin_amdgcn_logf(l_tot)) * 0.6931471805599453f;
    }
#endif
  }
}


}  // namespace grit

using namespace grit;

template <bool VARLEN, bool CAUSAL, bool F16>
static void attn_launch(dim3 grid, hipStream_t st, const uint16_t* qkv, const uint64_t* key_bits, const int32_t* cu, uint16_t* out, float* lse,
                        int S, int nq, int nkv, int64_t qkv_stride, int64_t out_stride, float scale_log2, int qpw, int ngx, int n_sets,
                        int window) {
  static std::atomic<uint64_t> optin{0};
  attn_lds_optin(attn_bidir_fwd_k<VARLEN, CAUSAL, F16>, optin);
  hipLaunchKernelGGL((attn_bidir_fwd_k<VARLEN, CAUSAL, F16>), grid, dim3(256), ATT_LDS_BYTES, st, qkv, key_bits, cu, out, lse, S, nq, nkv, qkv_stride,
                     out_stride, scale_log2, qpw, ngx, n_sets, window);
}

// Launch geometry: query blocks per workgroup (the K/V stream runs through the block seams, so more blocks per workgroup amortise the
// prologue) -- as many as 4 while the launch still has >= 4 workgroups per CU-slot pair -- and the XCD-aware 1-D grid.
struct AttnGeom {
  int qpw, ngx, n_sets;
  unsigned grid;
};
static AttnGeom attn_geom(int B, int max_len, int nq, int nkv, bool causal) {
  const int nqb = (max_len + ATT_QB - 1) / ATT_QB;
  static const int forced = getenv("GRIT_ATTN_QPW") ? atoi(getenv("GRIT_ATTN_QPW")) : 0;      // A/B knob
  int qpw = 1;
  // causal: consecutive query blocks see 2, 4, 6, ... KV tiles, so a workgroup walking 4 of them is up to 4x longer than its neighbour;
  // 2 blocks per workgroup balance better (B 64 x S 2048: 869 -> 893 TF, profiles/r03_attn_fwd_ab_asm_reads.log)
  for (int c = causal ? 2 : 4; c >= 1; c >>= 1)
    if ((int64_t)B * nq * ((nqb + c - 1) / c) >= 2048 || c == 1) { qpw = c; break; }
  if (forced > 0) qpw = forced;
  if (qpw > nqb) qpw = nqb;
  AttnGeom g;
  g.qpw = qpw;
  g.ngx = (nqb + qpw - 1) / qpw;
  g.n_sets = B * nkv;
  g.grid = (unsigned)(8 * ((g.n_sets + 7) / 8) * (nq / nkv) * g.ngx);
  return g;
}

// Padded batches (varlen = false: S rows per sequence, key_bits) and packed ones (varlen = true: cu_seqlens, S = the longest sequence).
static int attn_fwd(const char* name, bool varlen, bool causal, bool f16, int window, const void* qkv, const uint64_t* key_bits,
                    const int32_t* cu_seqlens, void* out, float* lse, int B, int S, int nq, int nkv, int d, int64_t qkv_stride, int64_t out_stride,
                    float scale, void* stream) {
  GRIT_REQUIRE(qkv && (varlen ? (const void*)cu_seqlens : key_bits) && out, GRIT_E_BADARG, "%s: null pointer", name);
  GRIT_REQUIRE(B > 0 && S > 0 && nq > 0 && nkv > 0 && S <= (1 << 30) && nq <= 65535 && nkv <= 65535, GRIT_E_BADARG, "%s: bad sizes", name);
  GRIT_REQUIRE(d == ATT_D, GRIT_E_UNSUPPORTED, "%s: head_dim=%d (only 128 is built)", name, d);
  GRIT_REQUIRE(nq % nkv == 0, GRIT_E_BADARG, "%s: nq=%d not a multiple of nkv=%d", name, nq, nkv);
  GRIT_REQUIRE(window >= 0 && (causal || window == 0), GRIT_E_BADARG, "%s: window=%d (>= 1 keys per query, causal attention only)", name, window);
  GRIT_REQUIRE(qkv_stride % 8 == 0 && qkv_stride >= (int64_t)(nq + 2 * nkv) * d && out_stride % 8 == 0 && out_stride >= (int64_t)nq * d,
               GRIT_E_BADARG, "%s: bad strides", name);
  GRIT_REQUIRE(aligned16(qkv) && aligned16(out), GRIT_E_BADARG, "%s: pointers must be 16-byte aligned", name);
  GRIT_REQUIRE((int64_t)B * nq * ((S + ATT_QB - 1) / ATT_QB) < (1ll << 30), GRIT_E_UNSUPPORTED, "%s: grid too large", name);
  GRIT_REQUIRE((int64_t)S * qkv_stride * 2 < (1ll << 31) && (int64_t)S * out_stride * 2 < (1ll << 31), GRIT_E_UNSUPPORTED,
               "%s: one sequence spans more than 2 GiB (32-bit row offsets)", name);
  typedef void (*launch_t)(dim3, hipStream_t, const uint16_t*, const uint64_t*, const int32_t*, uint16_t*, float*, int, int, int, int64_t,
                           int64_t, float, int, int, int, int);
  static const launch_t launch[2][2][2] = {      // [varlen][!causal][!f16]
      {{attn_launch<false, true, true>, attn_launch<false, true, false>}, {attn_launch<false, false, true>, attn_launch<false, false, false>}},
      {{attn_launch<true, true, true>, attn_launch<true, true, false>}, {attn_launch<true, false, true>, attn_launch<true, false, false>}}};
  const AttnGeom g = attn_geom(B, S, nq, nkv, causal);
  launch[varlen][!causal][!f16](dim3(g.grid), (hipStream_t)stream, (const uint16_t*)qkv, key_bits, cu_seqlens, (uint16_t*)out, lse, S, nq, nkv,
                              qkv_stride, out_stride, scale * 1.4426950408889634f, g.qpw, g.ngx, g.n_sets, window);
  GRIT_CHECK_LAUNCH(name);
  return GRIT_OK;
}

extern "C" int grit_attn_bidir_fwd(const void* qkv, const uint64_t* key_bits, void* out, float* lse, int B, int S, int nq, int nkv,
                                   int d, int64_t qkv_stride, int64_t out_stride, float scale, void* stream) {
  return attn_fwd("grit_attn_bidir_fwd", false, false, false, 0, qkv, key_bits, nullptr, out, lse, 
                  B, S, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
// fp16-operand policy: qkv and out hold IEEE fp16.  Bidirectional (the embedding path) and -- ABI 5 -- causal, optionally with a sliding
// window of `window` keys (0: none): the causal prompt pass of a unified / generative model and the 'cc' embedding attention
extern "C" int grit_attn_causal_f16_fwd(const void* qkv, const uint64_t* key_bits, void* out, float* lse, int B, int S, int nq, int nkv,
                                        int d, int64_t qkv_stride, int64_t out_stride, float scale, int window, void* stream) {
  return attn_fwd("grit_attn_causal_f16_fwd", false, true, true, window, qkv, key_bits, nullptr, out, lse, 
                  B, S, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
extern "C" int grit_attn_causal_varlen_f16_fwd(const void* qkv, const int32_t* cu_seqlens, void* out, float* lse, int B, int max_len, int nq,
                                               int nkv, int d, int64_t qkv_stride, int64_t out_stride, float scale, int window, void* stream) {
  return attn_fwd("grit_attn_causal_varlen_f16_fwd", true, true, true, window, qkv, nullptr, cu_seqlens, out, lse, 
                  B, max_len, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
extern "C" int grit_attn_bidir_f16_fwd(const void* qkv, const uint64_t* key_bits, void* out, float* lse, int B, int S, int nq, int nkv,
                                       int d, int64_t qkv_stride, int64_t out_stride, float scale, void* stream) {
  return attn_fwd("grit_attn_bidir_f16_fwd", false, false, true, 0, qkv, key_bits, nullptr, out, lse, 
                  B, S, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
extern "C" int grit_attn_bidir_varlen_f16_fwd(const void* qkv, const int32_t* cu_seqlens, void* out, float* lse, int B, int max_len, int nq,
                                              int nkv, int d, int64_t qkv_stride, int64_t out_stride, float scale, void* stream) {
  return attn_fwd("grit_attn_bidir_varlen_f16_fwd", true, false, true, 0, qkv, nullptr, cu_seqlens, out, lse, 
                  B, max_len, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
extern "C" int grit_attn_causal_fwd(const void* qkv, const uint64_t* key_bits, void* out, float* lse, int B, int S, int nq, int nkv,
                                    int d, int64_t qkv_stride, int64_t out_stride, float scale, void* stream) {
  return attn_fwd("grit_attn_causal_fwd", false, true, false, 0, qkv, key_bits, nullptr, out, lse, 
                  B, S, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
extern "C" int grit_attn_bidir_varlen_fwd(const void* qkv, const int32_t* cu_seqlens, void* out, float* lse, int B, int max_len, int nq,
                                          int nkv, int d, int64_t qkv_stride, int64_t out_stride, float scale, void* stream) {
  return attn_fwd("grit_attn_bidir_varlen_fwd", true, false, false, 0, qkv, nullptr, cu_seqlens, out, lse, 
                  B, max_len, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
extern "C" int grit_attn_causal_varlen_fwd(const void* qkv, const int32_t* cu_seqlens, void* out, float* lse, int B, int max_len, int nq,
                                           int nkv, int d, int64_t qkv_stride, int64_t out_stride, float scale, void* stream) {
  return attn_fwd("grit_attn_causal_varlen_fwd", true, true, false, 0, qkv, nullptr, cu_seqlens, out, lse, 
                  B, max_len, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}

// Sliding-window causal attention: query q sees keys q - window + 1 .. q (window >= 1; window >= S is plain causal attention).
extern "C" int grit_attn_causal_window_fwd(const void* qkv, const uint64_t* key_bits, void* out, float* lse, int B, int S, int nq, int nkv,
                                           int d, int64_t qkv_stride, int64_t out_stride, float scale, int window, void* stream) {
  GRIT_REQUIRE(window >= 1, GRIT_E_BADARG, "grit_attn_causal_window_fwd: window=%d must be >= 1", window);
  return attn_fwd("grit_attn_causal_window_fwd", false, true, false, window, qkv, key_bits, nullptr, out, lse, 
                  B, S, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
extern "C" int grit_attn_causal_window_varlen_fwd(const void* qkv, const int32_t* cu_seqlens, void* out, float* lse, int B, int max_len, int nq,
                                                  int nkv, int d, int64_t qkv_stride, int64_t out_stride, float scale, int window,
                                                  void* stream) {
  GRIT_REQUIRE(window >= 1, GRIT_E_BADARG, "grit_attn_causal_window_varlen_fwd: window=%d must be >= 1", window);
  return attn_fwd("grit_attn_causal_window_varlen_fwd", true, true, false, window, qkv, nullptr, cu_seqlens, out, lse, 
                  B, max_len, nq, nkv, d, qkv_stride, out_stride, scale, stream);
}
