// The MFMA tile loop of the flash-attention forward kernels for gfx950 (head_dim 128): the LDS layout, the per-tile consumer and the
// output epilogue, shared by attn_bidir_fwd_k (attention.hip) and attn_prefill_cached_k (prefill.hip).  Each kernel keeps its own
// tile ranges, mask words, K/V staging and Q loads.  The tile consumer and the epilogue are statement macros (below: why).
// The backward (attention_bwd.hip) has its own tile loops and takes from here what every attention kernel shares: the wait macros, the
// address-space types, the workgroup prologue (ATT_WG_DECODE, ATT_SEQ_BOUNDS) and the LDS opt-in.
//
// A wave owns 32 query rows.  KV tiles of 64 keys are staged HBM -> LDS by the kernel (LDS-DMA, 16 B per lane, 1 KiB = 4 key rows per
// wave instruction) into a two-stage ring; the eight pieces of tile t+1 are issued BETWEEN the QK products of tile t and land under its
// softmax and PV products.  Every LDS fragment read of the tile is inline asm with counted lgkmcnt (K fragments two k-slices ahead of
// their products, V fragments in four groups of 8 with the first two requested in front of the softmax): hipcc's own lgkmcnt(0) /
// vmcnt(0) in front of builtin LDS reads, scalar loads and ds_bpermute cost 12 %.  Both images are row-major [key][256 B] with the
// 16-byte units XOR-swizzled through the per-lane SOURCE address of the DMA (its LDS image is lane-linear): K unit ^= key & 15
// (conflict-free ds_read_b128 of a 32-key fragment), V unit ^= 4 (key & 3) (conflict-free ds_read_b64_tr_b16: the 16 lanes of a
// transposing read touch 4 keys x 32 B, the XOR puts them -- and the second 16-lane group -- on 16 distinct units of one 256-B bank row).
//   S^T = K Q^T     v_mfma_f32_32x32x16_bf16(A = K rows, B = Q)  -> lane (q = lane&31) holds 32 keys' scores
//   O^T = V^T P^T   v_mfma_f32_32x32x16_bf16(A = V^T rows, B = P) -> lane (q = lane&31) holds 64 of its d's
// Both products are "swapped" so that every softmax statistic (max, sum, rescale) is lane-local: the only cross-lane traffic per tile
// is one v_permlane32_swap for the row max.  The P operand needs no permlane/LDS round trip: the MFMA contraction index is permuted
// identically on the V^T side (key(kb,c,hi,j) = 32kb + 16c + 8(j>>2) + 4hi + (j&3)): two transposing 8-byte LDS reads whose per-lane
// addresses select exactly those keys.
// F16 (the encoder's "f16_operands" precision policy): operands and output are IEEE fp16 and P is rounded to fp16 --
// v_mfma_f32_32x32x16_f16 runs at the bf16 rate and the LDS-DMA staging and the transposing reads are 16-bit-format-agnostic, so the
// instruction stream is the bf16 one with the two MFMA opcodes and the two pack instructions exchanged.  The deferred rescale keeps
// P <= 2^8, far inside the fp16 range; the output is a convex combination of V rows: nothing here can overflow.
#pragma once
#include <atomic>

#include "common.h"

// s_waitcnt vmcnt(0) through the builtin (gfx9 encoding: expcnt 7, lgkmcnt 15 = "don't wait"): unlike an asm statement the waitcnt
// insertion pass SEES it, so it does not add its own vmcnt(0) in front of the first MFMA that reads re-fetched Q registers -- that
// wait would sit behind the freshly issued DMA of the next tile and serialise it
#define ATT_WAIT_VM0()                      \
  do {                                      \
    asm volatile("" ::: "memory");          \
    __builtin_amdgcn_s_waitcnt(0x0F70);     \
    asm volatile("" ::: "memory");          \
  } while (0)
// s_waitcnt lgkmcnt(0): the wave's own LDS reads / writes have completed
#define ATT_WAIT_LGKM0()                    \
  do {                                      \
    asm volatile("" ::: "memory");          \
    __builtin_amdgcn_s_waitcnt(0xC07F);     \
    asm volatile("" ::: "memory");          \
  } while (0)

// ATT_DEFER_MAX=0 (A/B knob of tools/ubench/attn_ab.cpp): rescale O and l on every tile instead of deferring it
#ifndef ATT_DEFER_MAX
#define ATT_DEFER_MAX 1
#endif

namespace grit {

constexpr int ATT_D = 128;
constexpr int ATT_QB = 128;   // query rows per workgroup (block)
constexpr int ATT_KB = 64;    // keys per tile
constexpr int V_PITCH = 256;  // bytes per key row of the row-major V image
constexpr int K_LDS_BYTES = ATT_KB * ATT_D * 2;  // 16384
constexpr int V_LDS_BYTES = ATT_KB * V_PITCH;    // 16384
constexpr int ATT_STAGE_BYTES = K_LDS_BYTES + V_LDS_BYTES;   // 32 KiB per stage, two stages
constexpr int ATT_XPOSE_BYTES = 4096;                         // per wave: 32 rows x 128 B, the Q-in / O-out transposition buffer
constexpr int ATT_LDS_BYTES = 2 * ATT_STAGE_BYTES + 4 * ATT_XPOSE_BYTES;   // 80 KiB: two workgroups fill the CU's 160 KiB exactly
typedef const __attribute__((address_space(1))) void* att_gptr_t;
typedef __attribute__((address_space(3))) void* att_lptr_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

// ---- The prologue every attention kernel (forward, cached prefill, backward) starts with.
// XCD-aware decode of the 1-D grid (block v runs on XCD v % 8): the k-th workgroup of XCD x belongs to K/V set (k / U) * 8 + x, U = the
// workgroups that share one set's streamed operands.  Declares `member` (the workgroup's index inside its set), b and hk (the set's
// batch and kv head) from n_sets and nkv in scope, and RETURNS from the kernel for the grid's padding (sets are rounded up to 8).
// A statement macro like the tile consumer below, for the same reason: as a __forceinline__ function (every form tried: the exit test
// in the caller, in the callee, the results as references or as a struct) hipcc leaves set / nkv in front of the exit branch or tests
// the exit twice, and the kernels whose first use of nkv lies behind that branch (attn_bwd_dkdv_k) compile to a different stream.
#define ATT_WG_DECODE(U, member)                                                                                                             \
  const int att_u = (U), att_kx = (int)blockIdx.x >> 3;                                                                                      \
  const int att_set = (att_kx / att_u) * 8 + ((int)blockIdx.x & 7), member = att_kx % att_u;                                                 \
  if (att_set >= n_sets) return;                                                                                                             \
  const int b = att_set / nkv, hk = att_set - b * nkv;
// Declares the first row (row0) and the length (S) of sequence b, from b, S_arg, cu_seqlens and VARLEN in scope: padded batches hold
// S_arg rows per sequence, packed ones (VARLEN) the rows cu_seqlens[b] .. cu_seqlens[b + 1] - 1.  (A macro too: as a function the padded
// forward instantiations allocate their registers differently.)
#define ATT_SEQ_BOUNDS()                                                                                                                     \
  int S = S_arg;                                                                                                                             \
  int64_t row0 = (int64_t)b * S_arg;                                                                                                         \
  if constexpr (VARLEN) {                                                                                                                    \
    row0 = cu_seqlens[b];                                                                                                                    \
    S = cu_seqlens[b + 1] - cu_seqlens[b];                                                                                                   \
  }

__device__ __forceinline__ f32x16_t mma32(bf16x8_t a, bf16x8_t b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16_t mma32(f16x8_t a, f16x8_t b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
template <bool F16> struct att_frag { typedef bf16x8_t type; };
template <> struct att_frag<true> { typedef f16x8_t type; };

// ---- Per-lane constants of the fragment reads, computed once in front of the tile loop (hi = lane >> 5):
//   K fragment: row = 32kb + (lane&31), d-slot = 2ks + hi, swizzle by row&15 == lane&15 -- kf_row = (lane&31) * 256, kf_x = lane & 15.
//   V fragment (A operand of O^T += V^T P^T) straight from the ROW-MAJOR V image with ds_read_b64_tr_b16: in every 16-lane group lane j
//   points at V[k0 + j/4][d0 + 4 (j%4)] and lane c receives V[k0 .. k0+3][d0 + c] (the hardware transposes the group's 4 x 16 block);
//   d0 = 32db + 16 ((lane>>4)&1) makes c <-> the MFMA row lane&31, k0 = 32kb + 16c + 4hi (+8 for the second half of the k-slice).
//   (key & 3) of every key a lane addresses is (lane>>2)&3, so the V swizzle turns the d-block offset db*64 into (db ^ r)*64,
//   r = (lane>>2)&3: vt_lane carries r in byte bits 7:6 and the read address of d-block db is vt_lane ^ (db << 6).
#define ATT_VT_LANE(lane, hi)                                                                                                                \
  (((((lane) & 15) >> 2) + 4 * (hi)) * V_PITCH + (((((lane) >> 2) & 3) * 4) << 4) + ((((lane) >> 4) & 1) * 16 + 4 * ((lane) & 3)) * 2)

// ---- The per-tile consumer and the output epilogue, as statement macros over the calling kernel's variables: each kernel then
//      compiles to the instruction stream it had with this code written out in place (__forceinline__ templates taking the DMA stager
//      and the hook as lambdas did not -- hipcc simplifies a callee on its own before inlining it).  In scope at the expansion:
//        F16, frag_t                      the operand format, att_frag<F16>::type
//        lane, hi, kf_row, kf_x, vt_lane  the lane's constants (above)
//        qf[8]                            Q fragments (B operand): lane holds Q[q][16ks + 8hi .. +8]
//        sacc[2]                          the tile's scores S^T, two 32-key halves
//        oacc[4], m_run, l_run            O^T and the online-softmax state of the lane's row
//        word, fast                       the lane's key mask of the tile (bit k: key k visible; read only when !fast) and "every key
//                                         of the tile is visible to every row of the wave"
//        scale_log2                       softmax scale * log2(e)
//        stage_piece(t, buf, i, is_v), st_t, st_buf
//                                         issues LDS-DMA piece i (K: is_v = 0, V: 1) of tile t into stage buf
//        xs, q_swz, o_base, out_stride_b  (ATT_STORE_OUT) the wave's transposition buffer, the lane's row swizzle (lane&31 >> 1) & 7,
//                                         the output's column base and row pitch in bytes
//   ATT_TILE_QK(k_lds)   S^T = K Q^T from the tile's K image; the next tile's eight DMA pieces go out between the products
//   ATT_TILE_PV(v_lds)   V reads, mask + online softmax, O^T += V^T P^T
//   Between the two, qf is free: the forward kernel refills it there for its next query block.
//
// S^T = K Q^T: the two 32-key halves are two INDEPENDENT accumulation chains, issued alternately (a v_mfma_f32_32x32x16_bf16 occupies
// the pipe for 32 cycles but its result is ready after 64, so a product that accumulates onto the one issued just before it has to
// wait; hipcc keeps MFMA source order; A/B against "8 products on one half, then 8 on the other": +2.5-4.5 %, bit-identical).
// K fragments are inline-asm ds_read_b128 with counted lgkmcnt, requested two k-slices (2 reads each) ahead of the products that
// consume them (three ahead: no gain; hipcc issues builtin reads in small batches and waits lgkmcnt(0) seven times per tile);
// (2 ks + hi) ^ kf_x == (2 ks) ^ (hi ^ kf_x): one per-tile base with the lane's constant in address bits 7:4, one v_xor per k-slice.
// One LDS-DMA piece of the next tile goes out behind every product pair: an LDS-DMA instruction costs 60-185 issue cycles, eight of
// them in front of the first K read held the whole tile back; between MFMAs the cost sits under the matrix pipe.  s_setprio 1 over
// the section: 0 .. +2 % (over the PV section as well: -1.5 %).
#define ATT_K_READ(KS)                                                                                                                       \
  do {                                                                                                                                       \
    const uint32_t ka = kbase ^ (uint32_t)((KS) << 5);                                                                                       \
    asm volatile("ds_read_b128 %0, %1" : "=v"(kr[KS][0]) : "v"(ka));                                                                         \
    asm volatile("ds_read_b128 %0, %1 offset:8192" : "=v"(kr[KS][1]) : "v"(ka));                                                             \
  } while (0)
#define ATT_K_MMA(KS, N)                                                                                                                     \
  do {                                                                                                                                       \
    asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(kr[KS][0]), "+v"(kr[KS][1]) : : "memory");                                               \
    sacc[0] = mma32(kr[KS][0], qf[KS], (KS) == 0 ? zero16 : sacc[0]);                                                                        \
    sacc[1] = mma32(kr[KS][1], qf[KS], (KS) == 0 ? zero16 : sacc[1]);                                                                        \
    stage_piece(st_t, st_buf, (KS) >> 1, (KS) & 1);                                                                                          \
    asm volatile("" ::: "memory");                                                                                                           \
  } while (0)
#define ATT_TILE_QK(k_lds)                                                                                                                   \
  {                                                                                                                                          \
    const f32x16_t zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                                \
    const uint32_t kbase = ((uint32_t)(uintptr_t)((__attribute__((address_space(3))) const char*)(k_lds)) + (uint32_t)kf_row) | (uint32_t)((hi ^ kf_x) << 4); \
    frag_t kr[8][2];                                                                                                                         \
    __builtin_amdgcn_s_setprio(1);                                                                                                           \
    ATT_K_READ(0); ATT_K_READ(1);                                                                                                            \
    ATT_K_READ(2); ATT_K_MMA(0, 4);                                                                                                          \
    ATT_K_READ(3); ATT_K_MMA(1, 4);                                                                                                          \
    ATT_K_READ(4); ATT_K_MMA(2, 4);                                                                                                          \
    ATT_K_READ(5); ATT_K_MMA(3, 4);                                                                                                          \
    ATT_K_READ(6); ATT_K_MMA(4, 4);                                                                                                          \
    ATT_K_READ(7); ATT_K_MMA(5, 4);                                                                                                          \
    ATT_K_MMA(6, 2); ATT_K_MMA(7, 0);                                                                                                        \
    __builtin_amdgcn_s_setprio(0);                                                                                                           \
  }
// The transposing V reads as inline asm with COUNTED lgkmcnt: hipcc's wait-count pass treats a ds_read_b64_tr_b16 builtin as aliasing
// the pending LDS-DMA and puts an s_waitcnt vmcnt(0) in front of the first one -- the NEXT tile's DMA then had to land before this
// tile's PV products could start.  Four groups (kb, c) of 8 reads feed 4 MFMAs each; group g + 1 is requested before group g is
// waited for (lgkmcnt(8): LDS returns in order), two register sets of 16.  The first two groups are requested in front of the
// softmax (the V tile has been in LDS since the barrier at the top of the tile; the K fragments' registers are free).  The four
// d-blocks of O^T are four independent accumulators: round-robin, never the same one twice in a row.
#define ATT_TR_GROUP(G, BUF)                                                                                                                 \
  _Pragma("unroll") for (int db = 0; db < 4; ++db) {                                                                                         \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vr[BUF][db][0]) : "v"(va[db]), "i"(((G) >> 1) * 32 * V_PITCH + ((G) & 1) * 16 * V_PITCH)); \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(vr[BUF][db][1]) : "v"(va[db]), "i"(((G) >> 1) * 32 * V_PITCH + ((G) & 1) * 16 * V_PITCH + 8 * V_PITCH)); \
  }
#define ATT_TR_WAIT(N, BUF)                                                                                                                  \
  asm volatile("s_waitcnt lgkmcnt(" #N ")"                                                                                                   \
               : "+v"(vr[BUF][0][0]), "+v"(vr[BUF][0][1]), "+v"(vr[BUF][1][0]), "+v"(vr[BUF][1][1]), "+v"(vr[BUF][2][0]),                    \
                 "+v"(vr[BUF][2][1]), "+v"(vr[BUF][3][0]), "+v"(vr[BUF][3][1]))
#define ATT_TR_MMA(G, BUF)                                                                                                                   \
  _Pragma("unroll") for (int db = 0; db < 4; ++db) {                                                                                         \
    const s16x4_t v0 = vr[BUF][db][0], v1 = vr[BUF][db][1];                                                                                  \
    const frag_t vf = __builtin_bit_cast(frag_t, (__attribute__((ext_vector_type(8))) short){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]}); \
    oacc[db] = mma32(vf, pb[(G) >> 1][(G) & 1], oacc[db]);                                                                                   \
  }
#if ATT_DEFER_MAX
// deferred rescale: a row keeps its old reference maximum as long as its maximum grows by less than 2^8 (P <= 256, exact in the bf16
// exponent range; l and O stay consistent with m_run); when NO row of the wave has to move, the 64 accumulator multiplies + exp2 of the
// rescale are skipped.  The decision is per row (rows that stay multiply by exactly 1), so a row's result never depends on which other
// rows share its wave -- the packed and the padded layout stay bit-identical.  (grow is also true for m_run = -inf: first tile, or all
// keys masked so far.)
#define ATT_RESCALE()                                                                                                                        \
  const bool grow = !(m_new - m_run <= 8.0f);                                                                                                \
  if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {                                                                                           \
    const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;                                                                                  \
    const float alpha = grow ? __builtin_amdgcn_exp2f(m_run - m_ref) : 1.0f;                                                                 \
    m_run = grow ? m_new : m_run;                                                                                                            \
    l_run *= alpha;                                                                                                                          \
    _Pragma("unroll") for (int db = 0; db < 4; ++db)                                                                                         \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;                                                                   \
  }                                                                                                                                          \
  const float m_use = (m_run == -INFINITY) ? 0.f : m_run;
#define ATT_ACCUMULATE_L()                                                                                                                   \
  l_run += psum;
#else
#define ATT_RESCALE()                                                                                                                        \
  const float m_use = (m_new == -INFINITY) ? 0.f : m_new;                                                                                    \
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);                                                                                 \
  m_run = m_new;
#define ATT_ACCUMULATE_L()                                                                                                                   \
  l_run = l_run * alpha + psum;                                                                                                              \
  _Pragma("unroll") for (int db = 0; db < 4; ++db)                                                                                           \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
#endif
// ATT_TILE_PV: `fast` is made wave-uniform and opaque in front of the V reads, so that the compare -- and with it hipcc's wait for a
// mask word's scalar load -- sits in front of them, not behind.  Unmasked, the row maximum runs as four independent chains (max is
// exact: any order gives the same bits; one chain of 16 dependent v_max3 is a latency chain).  Masked scores become -inf; the words
// wlo / whi are pre-shifted by 4 hi, so bit (r & 3) + 8 (r >> 2) is the key of accumulator register r.  The maximum over the two
// 32-lane halves goes through v_permlane32_swap (a VALU instruction): __shfl_xor is a ds_bpermute, an LDS-queue instruction whose
// lgkmcnt(0) also waits for the V reads requested in front of the softmax.  scale > 0: max commutes with the scaling.
// P = exp2(s * scale - m): one fma + one v_exp per score (masked scores are -inf -> 0).
#define ATT_TILE_PV(v_lds)                                                                                                                   \
  {                                                                                                                                          \
    const uint32_t vbase = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)(v_lds));                                          \
    uint32_t va[4];                                                                                                                          \
    _Pragma("unroll") for (int db = 0; db < 4; ++db) va[db] = vbase + (uint32_t)(vt_lane ^ (db << 6));                                       \
    s16x4_t vr[2][4][2];                                                                                                                     \
    {                                                                                                                                        \
      int fast_i = __builtin_amdgcn_readfirstlane(fast ? 1 : 0);                                                                             \
      asm volatile("" : "+s"(fast_i));                                                                                                       \
      fast = fast_i != 0;                                                                                                                    \
    }                                                                                                                                        \
    ATT_TR_GROUP(0, 0)                                                                                                                       \
    ATT_TR_GROUP(1, 1)                                                                                                                       \
    float mx = -INFINITY;                                                                                                                    \
    if (fast) {                                                                                                                              \
      float m4[4];                                                                                                                           \
      _Pragma("unroll") for (int c4 = 0; c4 < 4; ++c4) {                                                                                     \
        const int kb = c4 >> 1, r0 = (c4 & 1) * 8;                                                                                           \
        m4[c4] = fmaxf(fmaxf(sacc[kb][r0], sacc[kb][r0 + 1]), sacc[kb][r0 + 2]);                                                             \
        _Pragma("unroll") for (int r = 3; r < 8; ++r) m4[c4] = fmaxf(m4[c4], sacc[kb][r0 + r]);                                              \
      }                                                                                                                                      \
      mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));                                                                                  \
    } else {                                                                                                                                 \
      const uint32_t wlo = (uint32_t)(word >> (4 * hi)), whi = (uint32_t)(word >> (32 + 4 * hi));                                            \
      _Pragma("unroll") for (int kb = 0; kb < 2; ++kb) {                                                                                     \
        const uint32_t wsel = kb ? whi : wlo;                                                                                                \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                                                     \
          const int kbit = (r & 3) + 8 * (r >> 2);                                                                                           \
          const float s = ((wsel >> kbit) & 1u) ? sacc[kb][r] : -INFINITY;                                                                   \
          sacc[kb][r] = s;                                                                                                                   \
          mx = fmaxf(mx, s);                                                                                                                 \
        }                                                                                                                                    \
      }                                                                                                                                      \
    }                                                                                                                                        \
    {                                                                                                                                        \
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);                              \
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * scale_log2;                                                               \
    }                                                                                                                                        \
    const float m_new = fmaxf(m_run, mx);                                                                                                    \
    ATT_RESCALE()                                                                                                                            \
    float psum = 0.f;                                                                                                                        \
    frag_t pb[2][2];                                                                                                                         \
    _Pragma("unroll") for (int kb = 0; kb < 2; ++kb)                                                                                         \
      _Pragma("unroll") for (int c = 0; c < 2; ++c) {                                                                                        \
        uint32_t pk[4];                                                                                                                      \
        _Pragma("unroll") for (int jj = 0; jj < 4; ++jj) {                                                                                   \
          const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][8 * c + 2 * jj], scale_log2, -m_use));                                       \
          const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][8 * c + 2 * jj + 1], scale_log2, -m_use));                                   \
          psum += p0 + p1;                                                                                                                   \
          pk[jj] = pack2_op<F16>(p0, p1);                                                                                                    \
        }                                                                                                                                    \
        pb[kb][c] = __builtin_bit_cast(frag_t, make_uint4(pk[0], pk[1], pk[2], pk[3]));                                                      \
      }                                                                                                                                      \
    ATT_ACCUMULATE_L()                                                                                                                       \
    ATT_TR_WAIT(8, 0);                                                                                                                       \
    ATT_TR_MMA(0, 0)                                                                                                                         \
    ATT_TR_GROUP(2, 0)                                                                                                                       \
    ATT_TR_WAIT(8, 1);                                                                                                                       \
    ATT_TR_MMA(1, 1)                                                                                                                         \
    ATT_TR_GROUP(3, 1)                                                                                                                       \
    ATT_TR_WAIT(8, 0);                                                                                                                       \
    ATT_TR_MMA(2, 0)                                                                                                                         \
    ATT_TR_WAIT(0, 1);                                                                                                                       \
    ATT_TR_MMA(3, 1)                                                                                                                         \
  }
// ATT_STORE_OUT: the wave's 32 rows q_wave0 .. q_wave0 + 31 (lane holds O[q][32db + 8g + 4hi + 0..3] in regs 4g..4g+3 of oacc[db]),
// normalised by l, go out as full-line stores through the transposition buffer xs (a row-per-lane store touches 32 lines x 32 B per
// instruction): one 64-column half at a time, every lane writes its 4 pieces of the half (unit ^= (row>>1)&7), then stores 16 B of an
// 8-row x 128-B piece.  v_permlane32_swap exchanges the two 32-lane halves of the register groups g and g+1, so that a lane ends up
// with 8 CONSECUTIVE dims of its row (half 0: group g, half 1: group g+1): one 16-byte piece.  Row qr is stored if ROW_STORED, as
// zeros unless ROW_VALID (both expressions in qr).  l over the two lane halves through __shfl_xor once per block (through
// v_permlane32_swap like the tile maximum: measured 2 % slower at S >= 2048); leaves l_tot, the row's l, in scope.
#define ATT_STORE_OUT(Q_WAVE0, ROW_STORED, ROW_VALID)                                                                                        \
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);                                                                                     \
  const float inv_l = l_tot > 0.f ? 1.0f / l_tot : 0.f;                                                                                      \
  const int q_wave0 = (Q_WAVE0);                                                                                                             \
  int ln = lane;                                                                                                                             \
  asm volatile("" : "+v"(ln));                                                                                                               \
  const int x_row = ln >> 3, x_unit = ln & 7;                                                                                                \
  _Pragma("unroll") for (int half = 0; half < 2; ++half) {                                                                                   \
    char* wp = xs + (ln & 31) * 128;                                                                                                         \
    _Pragma("unroll") for (int dbl = 0; dbl < 2; ++dbl)                                                                                      \
      _Pragma("unroll") for (int gp = 0; gp < 2; ++gp) {                                                                                     \
        const int db = half * 2 + dbl;                                                                                                       \
        float a[4], bq[4];                                                                                                                   \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                                      \
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(oacc[db][8 * gp + e] * inv_l),                                    \
                                                           __float_as_uint(oacc[db][8 * gp + 4 + e] * inv_l), false, false);                 \
          a[e] = __uint_as_float(sw[0]); bq[e] = __uint_as_float(sw[1]);                                                                     \
        }                                                                                                                                    \
        *reinterpret_cast<uint4*>(wp + (((dbl * 4 + gp * 2 + hi) ^ q_swz) << 4)) =                                                           \
            make_uint4(pack2_op<F16>(a[0], a[1]), pack2_op<F16>(a[2], a[3]), pack2_op<F16>(bq[0], bq[1]), pack2_op<F16>(bq[2], bq[3]));      \
      }                                                                                                                                      \
    ATT_WAIT_LGKM0();                                                                                                                        \
    uint4 piece[4];                                                                                                                          \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) piece[j] = *reinterpret_cast<const uint4*>(xs + j * 1024 + ln * 16);                       \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                                          \
      const int r = 8 * j + x_row;                                                                                                           \
      const int qr = q_wave0 + r;                                                                                                            \
      if (ROW_STORED) {                                                                                                                      \
        const bool valid = (ROW_VALID);                                                                                                      \
        const u32x4_t pv = {valid ? piece[j].x : 0u, valid ? piece[j].y : 0u, valid ? piece[j].z : 0u, valid ? piece[j].w : 0u};             \
        *reinterpret_cast<u32x4_t*>(o_base + ((uint32_t)qr * out_stride_b + (uint32_t)((half * 8 + (x_unit ^ ((r >> 1) & 7))) << 4))) = pv;  \
      }                                                                                                                                      \
    }                                                                                                                                        \
    ATT_WAIT_LGKM0();                                                                                                                        \
  }

}  // namespace grit

// the dynamic-LDS opt-in (the forward's 80 KiB unless `bytes` says otherwise) is a per-device function attribute: set it once per
// (instantiation, device)
template <typename KernelT>
static void attn_lds_optin(KernelT kernel, std::atomic<uint64_t>& done, int bytes = grit::ATT_LDS_BYTES) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (!(done.load(std::memory_order_acquire) & bit)) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    done.fetch_or(bit, std::memory_order_release);
  }
}
