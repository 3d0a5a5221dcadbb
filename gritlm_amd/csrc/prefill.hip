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
// The attention is the MFMA structure of attn_bidir_fwd_k (attention.hip) with one query block per workgroup: 128 queries per 256-thread
// workgroup (32 per wave), 64-key tiles staged HBM -> LDS by LDS-DMA into a two-stage ring (the eight 1-KiB pieces of tile t+1 issued
// between the QK products of tile t), the same XOR-swizzled K / V images and counted inline-asm LDS reads, the swapped products
//   S^T = K Q^T  and  O^T = V^T P^T   (v_mfma_f32_32x32x16_{bf16,f16})
// that keep every softmax statistic lane-local, the deferred rescale (a row keeps its reference maximum while it grows by < 2^8), and the
// XCD grouping of the workgroups that read one (sequence, kv head)'s K / V.  What differs:
//   * K and V are two allocations [B, nkv, Lmax, 128] with a 256-byte row: every piece carries its own per-lane address (key clamped to
//     the block's last visible key -- rows past it are finite copies, masked, so nothing outside the written cache is ever read);
//   * tiles that lie wholly at or before lens[b] + (the wave's first query) take the unmasked path; only the last tiles of a block carry
//     the causal mask; tiles past the block's last visible key are never loaded;
//   * rows i >= plen[b] (right padding of the chunk) are written as zeros; no LSE.
#include <atomic>

#include "common.h"

namespace grit {

constexpr int PF_D = 128;
constexpr int PF_QB = 128;                       // query rows per workgroup
constexpr int PF_KB = 64;                        // keys per tile
constexpr int PF_PITCH = 256;                    // bytes per cache row / per LDS key row
constexpr int PF_K_LDS = PF_KB * PF_PITCH;       // 16384
constexpr int PF_STAGE = 2 * PF_K_LDS;           // K + V of one tile: 32 KiB, two stages
constexpr int PF_XPOSE = 4096;                   // per wave: the O-out transposition buffer (32 rows x 128 B)
constexpr int PF_LDS_BYTES = 2 * PF_STAGE + 4 * PF_XPOSE;   // 80 KiB: two workgroups per CU
typedef const __attribute__((address_space(1))) void* pf_gptr_t;
typedef __attribute__((address_space(3))) void* pf_lptr_t;
typedef __attribute__((ext_vector_type(4))) short pf_s16x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int pf_u32x4_t;

__device__ __forceinline__ f32x16_t pf_mma(bf16x8_t a, bf16x8_t b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16_t pf_mma(f16x8_t a, f16x8_t b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
template <bool F16> struct pf_frag { typedef bf16x8_t type; };
template <> struct pf_frag<true> { typedef f16x8_t type; };

// s_waitcnt vmcnt(0) through the builtin, so that the waitcnt pass sees it (attention.hip, ATT_WAIT_VM0)
#define PF_WAIT_VM0()                       \
  do {                                      \
    asm volatile("" ::: "memory");          \
    __builtin_amdgcn_s_waitcnt(0x0F70);     \
    asm volatile("" ::: "memory");          \
  } while (0)

template <bool F16>
__global__ void __launch_bounds__(256, 2)
attn_prefill_cached_k(const uint16_t* __restrict__ q, const uint16_t* __restrict__ cache_k, const uint16_t* __restrict__ cache_v,
                      const int32_t* __restrict__ lens, const int32_t* __restrict__ plen, uint16_t* __restrict__ out, int P, int nq, int nkv,
                      int Lmax, int64_t q_stride, int64_t out_stride, float scale_log2, int nqb, int n_sets) {
  extern __shared__ __attribute__((aligned(256))) char smem[];
  typedef typename pf_frag<F16>::type frag_t;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // XCD-aware decode: the k-th workgroup of XCD x belongs to K/V set (k / U) * 8 + x, U = (heads per kv head) x (query blocks)
  const int gqa = nq / nkv, U = gqa * nqb;
  const int kx = (int)blockIdx.x >> 3;
  const int set = (kx / U) * 8 + ((int)blockIdx.x & 7), member = kx % U;
  if (set >= n_sets) return;
  const int b = set / nkv, hk = set - b * nkv;
  const int h = hk * gqa + member % gqa;
  const int qb = member / gqa;
  int pl = plen[b], L0 = lens[b];
  pl = pl < 0 ? 0 : (pl > P ? P : pl);
  L0 = L0 < 0 ? 0 : (L0 > Lmax - 1 ? Lmax - 1 : L0);
  char* o_base = reinterpret_cast<char*>(out + (int64_t)b * P * out_stride + (int64_t)h * PF_D);
  const uint32_t q_stride_b = (uint32_t)q_stride * 2u, out_stride_b = (uint32_t)out_stride * 2u;

  if (qb * PF_QB >= pl) {
    // a block of padding rows only: zeros, 16 B per thread and pass (uniform per workgroup)
    const pf_u32x4_t z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int pass = 0; pass < PF_QB / 16; ++pass) {
      const int r = qb * PF_QB + pass * 16 + (tid >> 4);
      if (r < P) *reinterpret_cast<pf_u32x4_t*>(o_base + ((uint32_t)r * out_stride_b + (uint32_t)((tid & 15) << 4))) = z;
    }
    return;
  }
  const int qlast = (qb * PF_QB + PF_QB - 1) < (pl - 1) ? (qb * PF_QB + PF_QB - 1) : (pl - 1);
  const int kend = (L0 + qlast + 1) < Lmax ? (L0 + qlast + 1) : Lmax;          // keys 0 .. kend-1: what some row of the block sees
  const int ntiles = (kend + PF_KB - 1) / PF_KB;

  const char* q_base = reinterpret_cast<const char*>(q + (int64_t)b * P * q_stride + (int64_t)h * PF_D);
  const char* k_base = reinterpret_cast<const char*>(cache_k + ((int64_t)b * nkv + hk) * Lmax * PF_D);
  const char* v_base = reinterpret_cast<const char*>(cache_v + ((int64_t)b * nkv + hk) * Lmax * PF_D);
  const int ql = lane & 31, hi = lane >> 5;

  // ---- LDS-DMA roles (attention.hip): wave w stages keys 16w .. 16w+15 of a tile, four 1-KiB pieces for K and four for V (4 keys each);
  //      lane -> LDS key row 16w + 4i + (lane>>4), physical 16-byte unit lane&15, which holds the LOGICAL unit (lane&15) ^ swizzle(row):
  //      K unit ^= row & 15, V unit ^= 4 (row & 3).  The swizzle follows the LDS row; the SOURCE row is clamped to kend - 1.
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int st_key = 16 * wv + (lane >> 4);
  const uint32_t v_unit_b = (uint32_t)(((lane & 15) ^ (4 * ((lane >> 4) & 3))) << 4);
  auto stage_piece = [&](int t, int buf, int i, int is_v) {
    char* dst = smem + buf * PF_STAGE + wv * 4096 + (is_v ? PF_K_LDS : 0) + i * 1024;
    int key = t * PF_KB + st_key + 4 * i;
    key = key < kend ? key : kend - 1;
    const uint32_t unit_b = is_v ? v_unit_b : (uint32_t)(((lane & 15) ^ ((4 * i + (lane >> 4)) & 15)) << 4);
    const char* src = (is_v ? v_base : k_base) + ((uint32_t)key * (uint32_t)PF_PITCH + unit_b);
    __builtin_amdgcn_global_load_lds((pf_gptr_t)src, (pf_lptr_t)dst, 16, 0, 0);
  };
#pragma unroll
  for (int i = 0; i < 4; ++i) { stage_piece(0, 0, i, 0); stage_piece(0, 0, i, 1); }

  // ---- Q fragments (B operand), row per lane: Q[q][16ks + 8hi .. +8]; rows past plen read the last valid row (finite; stored as zeros)
  const int q_row = qb * PF_QB + wave * 32 + ql;
  const int q_eff = q_row < pl ? q_row : pl - 1;
  frag_t qf[8];
  {
    const char* qp = q_base + ((uint32_t)q_eff * q_stride_b + (uint32_t)hi * 16u);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const frag_t*>(qp + ks * 32);
  }
  char* xs = smem + 2 * PF_STAGE + wv * PF_XPOSE;
  const int q_swz = (ql >> 1) & 7;

  // K fragment address: row = 32kb + (lane&31), d-slot = 2ks + hi, swizzle by row&15 == lane&15; V fragments through the transposing
  // reads of the row-major image (attention.hip: vt_lane)
  const int kf_row = ql * 256, kf_x = lane & 15;
  const int vt_lane = (((lane & 15) >> 2) + 4 * hi) * PF_PITCH + ((((lane >> 2) & 3) * 4) << 4) + (((lane >> 4) & 1) * 16 + 4 * (lane & 3)) * 2;
  // the wave's first query sees keys 0 .. L0 + qw0: tiles wholly inside that range need no mask
  const int qw0 = qb * PF_QB + wave * 32;
  const int n_row = L0 + q_eff + 1;                                   // keys the lane's query sees

  f32x16_t oacc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  PF_WAIT_VM0();                                                      // first tile + Q rows
  for (int t = 0; t < ntiles; ++t) {
    if (t > 0) PF_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // behind the last tile the pieces re-stage it into the idle stage (nobody reads it; waited for before the stores)
    const int st_t = (t + 1 < ntiles) ? t + 1 : t, st_buf = (t + 1) & 1;
    const char* k_lds = smem + (t & 1) * PF_STAGE;
    const char* v_lds = k_lds + PF_K_LDS;
    uint64_t word = ~0ull;
    bool fast = true;
    if (t * PF_KB + PF_KB - 1 > L0 + qw0) {                           // the tile reaches past what the wave's first query sees
      const int n = n_row - t * PF_KB;
      word = n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull));
      fast = false;
    }

    // ---- S^T = K Q^T: two independent 32-key accumulation chains; K fragments two k-slices ahead (counted lgkmcnt); one LDS-DMA piece
    //      of the next tile behind every product pair
    f32x16_t sacc[2];
    {
      const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const uint32_t kbase = ((uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)k_lds) + (uint32_t)kf_row) | (uint32_t)((hi ^ kf_x) << 4);
      frag_t kr[8][2];
#define PF_K_READ(KS)                                                                                                               \
  do {                                                                                                                              \
    const uint32_t ka = kbase ^ (uint32_t)((KS) << 5);                                                                              \
    asm volatile("ds_read_b128 %0, %1" : "=v"(kr[KS][0]) : "v"(ka));                                                                \
    asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(kr[KS][1]) : "v"(ka));                                                    \
  } while (0)
#define PF_K_MMA(KS, N)                                                                                                             \
  do {                                                                                                                              \
    asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(kr[KS][0]), "+v"(kr[KS][1]) : : "memory");                                      \
    sacc[0] = pf_mma(kr[KS][0], qf[KS], (KS) == 0 ? zero16 : sacc[0]);                                                              \
    sacc[1] = pf_mma(kr[KS][1], qf[KS], (KS) == 0 ? zero16 : sacc[1]);                                                              \
    stage_piece(st_t, st_buf, (KS) >> 1, (KS) & 1);                                                                                 \
    asm volatile("" ::: "memory");                                                                                                  \
  } while (0)
      __builtin_amdgcn_s_setprio(1);
      PF_K_READ(0); PF_K_READ(1);
      PF_K_READ(2); PF_K_MMA(0, 4);
      PF_K_READ(3); PF_K_MMA(1, 4);
      PF_K_READ(4); PF_K_MMA(2, 4);
      PF_K_READ(5); PF_K_MMA(3, 4);
      PF_K_READ(6); PF_K_MMA(4, 4);
      PF_K_READ(7); PF_K_MMA(5, 4);
      PF_K_MMA(6, 2); PF_K_MMA(7, 0);
      __builtin_amdgcn_s_setprio(0);
#undef PF_K_READ
#undef PF_K_MMA
    }

    // ---- transposing V reads (counted lgkmcnt, four groups of 8; the first two requested in front of the softmax)
    const uint32_t vbase = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)v_lds);
    uint32_t va[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) va[db] = vbase + (uint32_t)(vt_lane ^ (db << 6));
    pf_s16x4_t vr[2][4][2];
#define PF_TR_GROUP(G, BUF)                                                                                                           \
  _Pragma("unroll") for (int db = 0; db < 4; ++db) {                                                                                  \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vr[BUF][db][0]) : "v"(va[db]), "i"(((G) >> 1) * 32 * PF_PITCH + ((G) & 1) * 16 * PF_PITCH));                \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vr[BUF][db][1]) : "v"(va[db]), "i"(((G) >> 1) * 32 * PF_PITCH + ((G) & 1) * 16 * PF_PITCH + 8 * PF_PITCH)); \
  }
    {
      int fast_i = __builtin_amdgcn_readfirstlane(fast ? 1 : 0);
      asm volatile("" : "+s"(fast_i));
      fast = fast_i != 0;
    }
    PF_TR_GROUP(0, 0)
    PF_TR_GROUP(1, 1)

    // ---- mask + online softmax (lane-local except one exchange with lane^32)
    float mx = -INFINITY;
    if (fast) {
      float m4[4];
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        const int kb = c4 >> 1, r0 = (c4 & 1) * 8;
        m4[c4] = fmaxf(fmaxf(sacc[kb][r0], sacc[kb][r0 + 1]), sacc[kb][r0 + 2]);
#pragma unroll
        for (int r = 3; r < 8; ++r) m4[c4] = fmaxf(m4[c4], sacc[kb][r0 + r]);
      }
      mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    } else {
      const uint32_t wlo = (uint32_t)(word >> (4 * hi)), whi = (uint32_t)(word >> (32 + 4 * hi));
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const uint32_t wsel = kb ? whi : wlo;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kbit = (r & 3) + 8 * (r >> 2);
          const float s = ((wsel >> kbit) & 1u) ? sacc[kb][r] : -INFINITY;
          sacc[kb][r] = s;
          mx = fmaxf(mx, s);
        }
      }
    }
    {
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * scale_log2;
    }
    const float m_new = fmaxf(m_run, mx);
    // deferred rescale, decided per row before any P of this tile is formed (the whole of O and l move together)
    const bool grow = !(m_new - m_run <= 8.0f);
    if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {
      const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = grow ? __builtin_amdgcn_exp2f(m_run - m_ref) : 1.0f;
      m_run = grow ? m_new : m_run;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
    }
    const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
    float psum = 0.f;
    frag_t pb[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        uint32_t pk[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][8 * c + 2 * jj], scale_log2, -m_use));
          const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][8 * c + 2 * jj + 1], scale_log2, -m_use));
          psum += p0 + p1;
          pk[jj] = pack2_op<F16>(p0, p1);
        }
        pb[kb][c] = __builtin_bit_cast(frag_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));
      }
    l_run += psum;

    // ---- O^T += V^T P^T (four d-blocks round-robin)
    {
#define PF_TR_WAIT(N, BUF)                                                                                                            \
  asm volatile("s_waitcnt lgkmcnt(" #N ")"                                                                                            \
               : "+v"(vr[BUF][0][0]), "+v"(vr[BUF][0][1]), "+v"(vr[BUF][1][0]), "+v"(vr[BUF][1][1]), "+v"(vr[BUF][2][0]),              \
                 "+v"(vr[BUF][2][1]), "+v"(vr[BUF][3][0]), "+v"(vr[BUF][3][1]))
#define PF_TR_MMA(G, BUF)                                                                                                             \
  _Pragma("unroll") for (int db = 0; db < 4; ++db) {                                                                                  \
    const pf_s16x4_t v0 = vr[BUF][db][0], v1 = vr[BUF][db][1];                                                                        \
    const frag_t vf = __builtin_bit_cast(frag_t, (__attribute__((ext_vector_type(8))) short){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]}); \
    oacc[db] = pf_mma(vf, pb[(G) >> 1][(G) & 1], oacc[db]);                                                                           \
  }
      PF_TR_WAIT(8, 0);
      PF_TR_MMA(0, 0)
      PF_TR_GROUP(2, 0)
      PF_TR_WAIT(8, 1);
      PF_TR_MMA(1, 1)
      PF_TR_GROUP(3, 1)
      PF_TR_WAIT(8, 0);
      PF_TR_MMA(2, 0)
      PF_TR_WAIT(0, 1);
      PF_TR_MMA(3, 1)
#undef PF_TR_GROUP
#undef PF_TR_WAIT
#undef PF_TR_MMA
    }
  }
  PF_WAIT_VM0();                                                      // the re-staged last tile has landed before the workgroup leaves

  // ---- epilogue: lane holds O[q][32db + 8g + 4hi + 0..3] in regs 4g..4g+3 of oacc[db]; full-line stores through the wave's buffer
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv_l = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  int ln = lane;
  asm volatile("" : "+v"(ln));
  const int x_row = ln >> 3, x_unit = ln & 7;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    char* wp = xs + (ln & 31) * 128;
#pragma unroll
    for (int dbl = 0; dbl < 2; ++dbl)
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {
        const int db = half * 2 + dbl;
        float a[4], bq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(oacc[db][8 * gp + e] * inv_l),
                                                           __float_as_uint(oacc[db][8 * gp + 4 + e] * inv_l), false, false);
          a[e] = __uint_as_float(sw[0]); bq[e] = __uint_as_float(sw[1]);
        }
        *reinterpret_cast<uint4*>(wp + (((dbl * 4 + gp * 2 + hi) ^ q_swz) << 4)) =
            make_uint4(pack2_op<F16>(a[0], a[1]), pack2_op<F16>(a[2], a[3]), pack2_op<F16>(bq[0], bq[1]), pack2_op<F16>(bq[2], bq[3]));
      }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);                               // lgkmcnt(0)
    asm volatile("" ::: "memory");
    uint4 piece[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) piece[j] = *reinterpret_cast<const uint4*>(xs + j * 1024 + ln * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 8 * j + x_row;
      const int qr = qw0 + r;
      if (qr < P) {
        const bool valid = qr < pl;
        const pf_u32x4_t pv = {valid ? piece[j].x : 0u, valid ? piece[j].y : 0u, valid ? piece[j].z : 0u, valid ? piece[j].w : 0u};
        *reinterpret_cast<pf_u32x4_t*>(o_base + ((uint32_t)qr * out_stride_b + (uint32_t)((half * 8 + (x_unit ^ ((r >> 1) & 7))) << 4))) = pv;
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);
    asm volatile("" ::: "memory");
  }
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
  const uint16_t* src = qkv + (int64_t)row * qkv_stride + (int64_t)nq * PF_D;
  for (int j = threadIdx.x; j < 2 * nkv * 16; j += blockDim.x) {
    const int head = j >> 4, unit = j & 15;                           // head < nkv: k head; else v head head - nkv
    const bool is_v = head >= nkv;
    const int hk = is_v ? head - nkv : head;
    uint16_t* dst = (is_v ? cache_v : cache_k) + (((int64_t)b * nkv + hk) * Lmax + pos) * PF_D + unit * 8;
    *reinterpret_cast<pf_u32x4_t*>(dst) = *reinterpret_cast<const pf_u32x4_t*>(src + (int64_t)head * PF_D + unit * 8);
  }
}

}  // namespace grit

using namespace grit;

static int prefill_attn(const char* name, bool f16, const void* q, const void* cache_k, const void* cache_v, const int32_t* lens,
                        const int32_t* plen, void* out, int B, int P, int nq, int nkv, int d, int Lmax, int64_t q_stride, int64_t out_stride,
                        float scale, void* stream) {
  GRIT_REQUIRE(q && cache_k && cache_v && lens && plen && out, GRIT_E_BADARG, "%s: null pointer", name);
  GRIT_REQUIRE(d == PF_D, GRIT_E_UNSUPPORTED, "%s: head_dim=%d (only 128 is built)", name, d);
  GRIT_REQUIRE(B > 0 && P >= 1 && Lmax > 0 && nq > 0 && nkv > 0 && nq <= 65535 && nkv <= 65535, GRIT_E_BADARG,
               "%s: bad sizes (B=%d, P=%d, Lmax=%d, nq=%d, nkv=%d)", name, B, P, Lmax, nq, nkv);
  GRIT_REQUIRE(nq % nkv == 0, GRIT_E_BADARG, "%s: nq=%d not a multiple of nkv=%d", name, nq, nkv);
  GRIT_REQUIRE(q_stride % 8 == 0 && q_stride >= (int64_t)nq * d && out_stride % 8 == 0 && out_stride >= (int64_t)nq * d, GRIT_E_BADARG,
               "%s: bad strides", name);
  GRIT_REQUIRE(aligned16(q) && aligned16(cache_k) && aligned16(cache_v) && aligned16(out), GRIT_E_BADARG, "%s: pointers must be 16-byte aligned",
               name);
  GRIT_REQUIRE((int64_t)P * q_stride * 2 < (1ll << 31) && (int64_t)P * out_stride * 2 < (1ll << 31) && (int64_t)Lmax * PF_PITCH < (1ll << 31),
               GRIT_E_UNSUPPORTED, "%s: one sequence spans more than 2 GiB (32-bit row offsets)", name);
  const int nqb = (P + PF_QB - 1) / PF_QB, n_sets = B * nkv;
  const int64_t grid = 8ll * ((n_sets + 7) / 8) * (nq / nkv) * nqb;
  GRIT_REQUIRE(grid < (1ll << 30), GRIT_E_UNSUPPORTED, "%s: grid too large", name);
  static std::atomic<uint64_t> optin[2];
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  const float sl2 = scale * 1.4426950408889634f;
  if (f16) {
    if (!(optin[1].load(std::memory_order_acquire) & bit)) {
      (void)hipFuncSetAttribute((const void*)attn_prefill_cached_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, PF_LDS_BYTES);
      optin[1].fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(attn_prefill_cached_k<true>, dim3((unsigned)grid), dim3(256), PF_LDS_BYTES, (hipStream_t)stream, (const uint16_t*)q,
                       (const uint16_t*)cache_k, (const uint16_t*)cache_v, lens, plen, (uint16_t*)out, P, nq, nkv, Lmax, q_stride, out_stride, sl2,
                       nqb, n_sets);
  } else {
    if (!(optin[0].load(std::memory_order_acquire) & bit)) {
      (void)hipFuncSetAttribute((const void*)attn_prefill_cached_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize, PF_LDS_BYTES);
      optin[0].fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(attn_prefill_cached_k<false>, dim3((unsigned)grid), dim3(256), PF_LDS_BYTES, (hipStream_t)stream, (const uint16_t*)q,
                       (const uint16_t*)cache_k, (const uint16_t*)cache_v, lens, plen, (uint16_t*)out, P, nq, nkv, Lmax, q_stride, out_stride, sl2,
                       nqb, n_sets);
  }
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
  GRIT_REQUIRE(d == PF_D, GRIT_E_UNSUPPORTED, "%s: head_dim=%d (only 128 is built)", name, d);
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
