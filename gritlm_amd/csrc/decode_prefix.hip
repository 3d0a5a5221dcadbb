// Decode attention over ONE shared copy of a prefix for gfx950 (include/gritlm_hip_prefix.h): n sampled continuations of a sequence
// (MistralDecoder.generate(num_return_sequences=n, share_prefix=True)) attend to the sequence's prefix K/V [B0, nkv, Lpre, 128], stored
// once, and to a short per-row tail [B0 n, nkv, Ltail, 128] of their own generated tokens.  The expanded path (decode.hip) reads the
// same prefix keys once per row and query head with scalar FMAs; here the n gq query rows of a (sequence, kv head) are the M side of
// the MFMA tile loop of attn_tile.h, in the shape of attn_prefill_cached_k (prefill.hip).  Four launches per layer and step:
//
//   rope_kv_append_tail_k         RoPE of the new token's q and k at position lens[r]; k / v -> tail slot lens[r] - plen[r / n]
//   attn_decode_prefix_k          (sequence, kv head) x query block x key chunk: flash attention of 128 query slots over KC prefix keys,
//                                 partial (m, l, O) records instead of normalised rows
//   attn_decode_tail_k            (64-key split, query head, row): the row's own tail keys, the fp32 arithmetic of attn_decode_k
//   attn_decode_prefix_combine_k  (query head, row): the records of the prefix chunks and the tail splits -> ctx
//
// Nothing waits on another workgroup inside a launch: the kernel boundary is the hand-over.
#include "attn_tile.h"
#include "../../include/gritlm_hip_prefix.h"

namespace grit {

// keys per prefix chunk: ONE compile-time constant (a row's bits must not depend on n, B0 or the prefix length).  Chosen by measurement:
// libraries that differ in this line alone, tools/shared_prefix_bench.py at n = 64, prefix 2048, bf16, one box -- 128: 8.39, 256: 8.19,
// 512: 8.33 ms per step (profiles/shared_prefix_kc_ab.jsonl).  Fewer keys per chunk are more workgroups (8 sets x 2 query
// blocks x 2048 / KC chunks on 256 CUs) and more partial records (520 B per row, head and chunk) for the combine to read.
constexpr int PX_KC = 256;
static_assert(PX_KC % ATT_KB == 0 && PX_KC >= ATT_KB, "a chunk is whole tiles");
constexpr int PX_REC = ATT_D + 2;            // floats per record: m, l, O[128]
constexpr int PX_CH = 64;                    // keys per tail split
constexpr int PX_MAX_SLOTS = 512;            // records per (row, head) the combine handles
constexpr int PX_LDS_BYTES = 2 * ATT_STAGE_BYTES;
constexpr float PX_LN2 = 0.6931471805599453f;

// (px_unpack8, px_pack2 and px_allreduce below restate unpack8, pack2_rne and wave_allreduce of decode.hip, and launches 1 and 3 restate
//  rope_kv_append_k and the branch of attn_decode_k without RoPE: decode.hip's kernel set is pinned by test_kernel_resources.py, so the
//  helpers cannot move to a shared header from here; they fold into one when that file is next opened.)
template <bool F16>
__device__ __forceinline__ void px_unpack8(const uint4 v, float (&f)[8]) {
  f[0] = lo16_op<F16>(v.x); f[1] = hi16_op<F16>(v.x); f[2] = lo16_op<F16>(v.y); f[3] = hi16_op<F16>(v.y);
  f[4] = lo16_op<F16>(v.z); f[5] = hi16_op<F16>(v.z); f[6] = lo16_op<F16>(v.w); f[7] = hi16_op<F16>(v.w);
}
template <bool F16>
__device__ __forceinline__ uint32_t px_pack2(float lo, float hi) {
  if constexpr (F16) return pack2h_hw(lo, hi);
  else return pack2bf(lo, hi);                 // the bit-trick RNE pack every RoPE kernel of the library uses
}

// ---- 1. RoPE + tail append.  One workgroup per row, as rope_kv_append_k (decode.hip) with the slot and the position apart:
//      position lens[r] (the tables' row), slot lens[r] - plen[r / n] (the tail's row).  F16: q rotated in place in fp32 AND rounded to q16.
template <bool F16>
__global__ void __launch_bounds__(256)
rope_kv_append_tail_k(uint16_t* __restrict__ qkv, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, uint16_t* __restrict__ tk,
                      uint16_t* __restrict__ tv, const int32_t* __restrict__ lens, const int32_t* __restrict__ plen, uint16_t* __restrict__ q16,
                      int n, int nq, int nkv, int Ltail, int Lpos, int64_t qkv_stride, int64_t q16_stride, unsigned int* __restrict__ flag) {
  constexpr int d = ATT_D, half = d >> 1, jc_n = d >> 4;
  const int b = blockIdx.x;
  const int pos = lens[b];
  const int slot = pos - plen[b / n];
  if (pos < 0 || pos >= Lpos || slot < 0 || slot >= Ltail) return;
  uint16_t* row = qkv + (int64_t)b * qkv_stride;
  float* rowf = reinterpret_cast<float*>(qkv) + (int64_t)b * qkv_stride;
  const int rot_items = (nq + nkv) * jc_n, cp_items = nkv * (d >> 3);
  uint32_t bad = 0;
  for (int i = threadIdx.x; i < rot_items + cp_items; i += 256) {
    if (i < rot_items) {
      const int head = i / jc_n, jc = i - head * jc_n;
      const int64_t off = (int64_t)head * d + jc * 8;
      const float* ct = cos_tab + (int64_t)pos * half + jc * 8;
      const float* stb = sin_tab + (int64_t)pos * half + jc * 8;
      float a[8], bb[8], lo[8], hi[8];
      if constexpr (F16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] = rowf[off + e]; bb[e] = rowf[off + half + e]; }
      } else {
        px_unpack8<false>(*reinterpret_cast<const uint4*>(row + off), a);
        px_unpack8<false>(*reinterpret_cast<const uint4*>(row + off + half), bb);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        lo[e] = rope_lo(a[e], bb[e], ct[e], stb[e]);
        hi[e] = rope_hi(a[e], bb[e], ct[e], stb[e]);
      }
      const uint4 r1 = make_uint4(px_pack2<F16>(lo[0], lo[1]), px_pack2<F16>(lo[2], lo[3]), px_pack2<F16>(lo[4], lo[5]), px_pack2<F16>(lo[6], lo[7]));
      const uint4 r2 = make_uint4(px_pack2<F16>(hi[0], hi[1]), px_pack2<F16>(hi[2], hi[3]), px_pack2<F16>(hi[4], hi[5]), px_pack2<F16>(hi[6], hi[7]));
      if constexpr (F16) bad |= h2_nonfinite(r1.x) | h2_nonfinite(r1.y) | h2_nonfinite(r1.z) | h2_nonfinite(r1.w) | h2_nonfinite(r2.x) |
                                h2_nonfinite(r2.y) | h2_nonfinite(r2.z) | h2_nonfinite(r2.w);
      if (head < nq) {
        if constexpr (F16) {                               // q: fp32 in place (the tail launch), fp16 beside it (the MFMA operand)
#pragma unroll
          for (int e = 0; e < 8; ++e) { rowf[off + e] = lo[e]; rowf[off + half + e] = hi[e]; }
          uint16_t* qd = q16 + (int64_t)b * q16_stride + off;
          *reinterpret_cast<uint4*>(qd) = r1; *reinterpret_cast<uint4*>(qd + half) = r2;
        } else {
          *reinterpret_cast<uint4*>(row + off) = r1; *reinterpret_cast<uint4*>(row + off + half) = r2;
        }
      } else {
        uint16_t* dst = tk + (((int64_t)b * nkv + (head - nq)) * Ltail + slot) * d + jc * 8;
        *reinterpret_cast<uint4*>(dst) = r1; *reinterpret_cast<uint4*>(dst + half) = r2;
      }
    } else {
      const int j = i - rot_items, h = j / (d >> 3), c = j - h * (d >> 3);
      uint4 v;
      if constexpr (F16) {
        const float* vs = rowf + (int64_t)(nq + nkv + h) * d + c * 8;
        v = make_uint4(pack2h_hw(vs[0], vs[1]), pack2h_hw(vs[2], vs[3]), pack2h_hw(vs[4], vs[5]), pack2h_hw(vs[6], vs[7]));
        bad |= h2_nonfinite(v.x) | h2_nonfinite(v.y) | h2_nonfinite(v.z) | h2_nonfinite(v.w);
      } else {
        v = reinterpret_cast<const uint4*>(row + (int64_t)(nq + nkv + h) * d)[c];
      }
      reinterpret_cast<uint4*>(tv + (((int64_t)b * nkv + h) * Ltail + slot) * d)[c] = v;
    }
  }
  if constexpr (F16) {
    if (bad) atomicOr(flag, 1u);
  }
}

// ---- 2. The prefix launch.  A K/V set is a (sequence s, kv head hk); its query slots are the n gq (row, head) pairs of rows s n .. s n + n - 1
//      (slot j: row s n + j / gq, head hk gq + j % gq), in blocks of ATT_QB; slots past n gq read the last valid slot and store nothing.
//      Workgroup = (set, query block, chunk of PX_KC keys), the workgroups of a set grouped by XCD.  What differs from attn_prefill_cached_k:
//      no causal mask -- every slot sees keys 0 .. plen[s] - 1, so only the tile that holds key plen[s] - 1 is masked (one word for the
//      whole wave), tiles past it are not loaded and source rows are clamped to the chunk's last key; the epilogue writes the lane's
//      (m, l, O) as they are.
template <bool F16>
__global__ void __launch_bounds__(256, 2)
attn_decode_prefix_k(const uint16_t* __restrict__ q, const uint16_t* __restrict__ pk, const uint16_t* __restrict__ pv, const int32_t* __restrict__ plen,
                     float* __restrict__ part, int n, int nq, int nkv, int Lpre, int64_t q_stride, float scale_log2, int nqb, int nchunks, int nslot,
                     int n_sets) {
  extern __shared__ __attribute__((aligned(256))) char smem[];
  typedef typename att_frag<F16>::type frag_t;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int gq = nq / nkv;
  ATT_WG_DECODE(nqb * nchunks, member)              // b: the sequence, hk: its kv head
  const int chunk = member % nchunks, qb = member / nchunks;
  const int nslots_q = n * gq;                      // the set's query slots
  int pl = plen[b];
  pl = pl < 0 ? 0 : (pl > Lpre ? Lpre : pl);
  const int key0 = chunk * PX_KC;

  if (key0 >= pl) {
    // a chunk at or past the prefix: the neutral element for every valid slot of the block (uniform per workgroup)
    for (int i = tid; i < ATT_QB * PX_REC; i += 256) {
      const int sl = i / PX_REC, e = i - sl * PX_REC, slot = qb * ATT_QB + sl;
      if (slot < nslots_q) {
        const int r = slot / gq, g = slot - r * gq;
        part[(((int64_t)(b * n + r) * nq + hk * gq + g) * nslot + chunk) * PX_REC + e] = e == 0 ? -INFINITY : 0.f;
      }
    }
    return;
  }
  const int kend = (key0 + PX_KC) < pl ? (key0 + PX_KC) : pl;          // keys key0 .. kend-1
  const int t0 = key0 / ATT_KB, nt = (kend - key0 + ATT_KB - 1) / ATT_KB;

  const char* k_base = reinterpret_cast<const char*>(pk + ((int64_t)b * nkv + hk) * Lpre * ATT_D);
  const char* v_base = reinterpret_cast<const char*>(pv + ((int64_t)b * nkv + hk) * Lpre * ATT_D);
  const int ql = lane & 31, hi = lane >> 5;

  // ---- LDS-DMA roles as in prefill.hip: wave w stages keys 16w .. 16w+15 of a tile, four 1-KiB pieces for K and four for V; the SOURCE
  //      row is clamped to kend - 1 (finite copies, masked), the swizzle follows the LDS row
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
  for (int i = 0; i < 4; ++i) { stage_piece(t0, 0, i, 0); stage_piece(t0, 0, i, 1); }

  // ---- Q fragments (B operand), slot per lane: Q[slot][16ks + 8hi .. +8]
  const int slot = qb * ATT_QB + wave * 32 + ql;
  const int slot_eff = slot < nslots_q ? slot : nslots_q - 1;
  const int row = b * n + slot_eff / gq, head = hk * gq + slot_eff % gq;
  frag_t qf[8];
  {
    const char* qp = reinterpret_cast<const char*>(q + (int64_t)row * q_stride + (int64_t)head * ATT_D) + hi * 16;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const frag_t*>(qp + ks * 32);
  }

  const int kf_row = ql * 256, kf_x = lane & 15;   // K / V fragment addresses (attn_tile.h)
  const int vt_lane = ATT_VT_LANE(lane, hi);

  f32x16_t oacc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  ATT_WAIT_VM0();                                                      // first tile + Q rows
  for (int i = 0; i < nt; ++i) {
    if (i > 0) ATT_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // behind the last tile the pieces re-stage it into the idle stage (nobody reads it; waited for before the workgroup leaves)
    const int st_t = t0 + ((i + 1 < nt) ? i + 1 : i), st_buf = (i + 1) & 1;
    const char* k_lds = smem + (i & 1) * ATT_STAGE_BYTES;
    const char* v_lds = k_lds + K_LDS_BYTES;
    uint64_t word = ~0ull;
    bool fast = true;
    const int nvis = kend - (t0 + i) * ATT_KB;                         // >= 1; < 64 only in the tile that holds the prefix's last key
    if (nvis < ATT_KB) {
      word = (1ull << nvis) - 1ull;
      fast = false;
    }

    f32x16_t sacc[2];
    ATT_TILE_QK(k_lds)
    ATT_TILE_PV(v_lds)
  }
  ATT_WAIT_VM0();                                                      // the re-staged last tile has landed before the workgroup leaves

  // ---- the lane's record: l over the two lane halves (each summed its own keys); m is the same in both.  Lane (q = lane&31, hi) holds
  //      O[q][32db + 8g + 4hi + 0..3] in registers 4g .. 4g+3 of oacc[db].  (m, l) put the O part on an 8-byte boundary: float2 stores.
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  if (slot < nslots_q) {
    float* pb = part + (((int64_t)row * nq + head) * nslot + chunk) * PX_REC;
    if (hi == 0) *reinterpret_cast<float2*>(pb) = make_float2(m_run * PX_LN2, l_tot);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float* o = pb + 2 + 32 * db + 8 * g + 4 * hi;
        *reinterpret_cast<float2*>(o) = make_float2(oacc[db][4 * g], oacc[db][4 * g + 1]);
        *reinterpret_cast<float2*>(o + 2) = make_float2(oacc[db][4 * g + 2], oacc[db][4 * g + 3]);
      }
  }
}

// All-reduce of one value over the 64 lanes in registers (the form of decode.hip's wave_allreduce): DPP row rotations, then the row swaps.
template <bool IS_MAX>
__device__ __forceinline__ float px_allreduce(float v) {
  auto op = [](float a, float b) { return IS_MAX ? fmaxf(a, b) : a + b; };
#define GRIT_PX_DPP(CTRL) v = op(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), (CTRL), 0xf, 0xf, false)));
  GRIT_PX_DPP(0x121) GRIT_PX_DPP(0x122) GRIT_PX_DPP(0x124) GRIT_PX_DPP(0x128)      // row_ror 1, 2, 4, 8
#undef GRIT_PX_DPP
  const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = op(__uint_as_float(s16[0]), __uint_as_float(s16[1]));
  const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return op(__uint_as_float(s32[0]), __uint_as_float(s32[1]));
}

// ---- 3. The tail launch: grid (splits of 64 tail keys, nq, B), one wave per workgroup -- the arithmetic of attn_decode_k's branch without
//      RoPE (fp32 q pre-scaled, scalar FMAs, natural exponent) over tail keys 0 .. lens[b] - plen[b / n]; records behind the prefix chunks'.
template <bool F16>
__global__ void __launch_bounds__(64)
attn_decode_tail_k(const uint16_t* __restrict__ q, const uint16_t* __restrict__ tk, const uint16_t* __restrict__ tv, const int32_t* __restrict__ lens,
                   const int32_t* __restrict__ plen, float* __restrict__ part, int n, int nq, int nkv, int Ltail, int64_t q_stride, float scale,
                   int nchunks, int nslot) {
  __shared__ __attribute__((aligned(16))) float qs[ATT_D];      // the query head, pre-scaled
  __shared__ float ps[64];                                      // probabilities of the 64 keys
  const int gq = nq / nkv;
  const int split = blockIdx.x, hq = blockIdx.y, hk = hq / gq, b = blockIdx.z;
  const int lane = threadIdx.x;
  int L = lens[b] - plen[b / n] + 1;                            // tail keys 0 .. L-1 (the new token was appended)
  L = L > Ltail ? Ltail : L;
  const int k0 = split * PX_CH;
  float* pbase = part + (((int64_t)b * nq + hq) * nslot + nchunks + split) * PX_REC;
  if (k0 >= L) {                                                // empty split: neutral element
    for (int i = lane; i < PX_REC; i += 64) pbase[i] = i == 0 ? -INFINITY : 0.f;
    return;
  }
  const int key = k0 + lane;
  const bool live = key < L;
  const int kg = lane >> 4, dc = lane & 15;                     // PV layout: key group kg (16 keys), dim chunk dc (8 dims)
  const int nk = min(64, L - k0);
  uint4 kreg[ATT_D / 8], vreg[16];
  {
    const uint4* kr = reinterpret_cast<const uint4*>(tk + (((int64_t)b * nkv + hk) * Ltail + (live ? key : L - 1)) * ATT_D);
#pragma unroll
    for (int c = 0; c < ATT_D / 8; ++c) kreg[c] = kr[c];
    const uint16_t* vbase = tv + (((int64_t)b * nkv + hk) * Ltail + k0) * ATT_D;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int kk = kg * 16 + j;
      vreg[j] = reinterpret_cast<const uint4*>(vbase + (int64_t)(kk < nk ? kk : nk - 1) * ATT_D)[dc];
    }
  }
  for (int e = lane; e < ATT_D; e += 64) {
    const int64_t qi = (int64_t)b * q_stride + (int64_t)hq * ATT_D + e;
    qs[e] = (F16 ? reinterpret_cast<const float*>(q)[qi] : bf2f(q[qi])) * scale;
  }
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < ATT_D / 8; ++c) {
    float kf[8];
    px_unpack8<F16>(kreg[c], kf);
    const float4 qa = *reinterpret_cast<const float4*>(&qs[c * 8]), qb = *reinterpret_cast<const float4*>(&qs[c * 8 + 4]);
    s += kf[0] * qa.x + kf[1] * qa.y + kf[2] * qa.z + kf[3] * qa.w + kf[4] * qb.x + kf[5] * qb.y + kf[6] * qb.z + kf[7] * qb.w;
  }
  const float m = px_allreduce<true>(live ? s : -INFINITY);
  const float p = live ? __expf(s - m) : 0.f;
  ps[lane] = p;
  const float l = px_allreduce<false>(p);
  __syncthreads();
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float vf[8];
    px_unpack8<F16>(vreg[j], vf);
    const float pj = ps[kg * 16 + j];                            // 0 for keys past the tail
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] += pj * vf[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {                                  // fold the four key groups: same dims sit 16 / 32 lanes apart
    const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(o[e]), __float_as_uint(o[e]), false, false);
    const float t = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
    const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t), __float_as_uint(t), false, false);
    o[e] = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
  }
  if (kg == 0) {
    float* od = pbase + 2 + 8 * dc;
#pragma unroll
    for (int e = 0; e < 8; e += 2) *reinterpret_cast<float2*>(od + e) = make_float2(o[e], o[e + 1]);
  }
  if (lane == 0) { pbase[0] = m; pbase[1] = l; }
}

// ---- 4. The combine: grid (nq, B), 128 threads (thread e owns output dim e); every wave derives the global maximum and the denominator
//      for itself from the (m, l) pairs of all nslot <= 512 records, as attn_decode_combine_k does.
template <bool F16>
__global__ void __launch_bounds__(128)
attn_decode_prefix_combine_k(const float* __restrict__ part, uint16_t* __restrict__ out, int nq, int nslot, int64_t out_stride) {
  __shared__ float fs[2][PX_MAX_SLOTS];      // per wave: exp(m_s - m) of every record
  const int h = blockIdx.x, b = blockIdx.y, e = threadIdx.x, lane = e & 63, wave = e >> 6;
  const float* base = part + ((int64_t)b * nq + h) * nslot * PX_REC;
  float ms[PX_MAX_SLOTS / 64], ls[PX_MAX_SLOTS / 64];
  // the first 16 records' outputs are requested beside the (m, l) pairs (prefix 2048 at KC 256 and a 128-token tail: all of them)
  float pv[16];
#pragma unroll
  for (int sp = 0; sp < 16; ++sp) pv[sp] = sp < nslot ? base[sp * PX_REC + 2 + e] : 0.f;
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < PX_MAX_SLOTS / 64; ++i) {
    const int sp = lane + 64 * i;
    ms[i] = sp < nslot ? base[sp * PX_REC] : -INFINITY;
    ls[i] = sp < nslot ? base[sp * PX_REC + 1] : 0.f;
    m = fmaxf(m, ms[i]);
  }
  m = px_allreduce<true>(m);
  float l = 0.f;
#pragma unroll
  for (int i = 0; i < PX_MAX_SLOTS / 64; ++i) {
    const int sp = lane + 64 * i;
    const float f = ms[i] == -INFINITY ? 0.f : __expf(ms[i] - m);
    if (sp < nslot) fs[wave][sp] = f;
    l += ls[i] * f;
  }
  l = px_allreduce<false>(l);
  __syncthreads();
  float acc = 0.f;
#pragma unroll
  for (int sp = 0; sp < 16; ++sp) acc += pv[sp] * (sp < nslot ? fs[wave][sp] : 0.f);
#pragma unroll 8
  for (int sp = 16; sp < nslot; ++sp) acc += base[sp * PX_REC + 2 + e] * fs[wave][sp];
  const float o = l > 0.f ? acc / l : 0.f;                      // a convex combination of cached values: inside their range
  uint16_t r;
  if constexpr (F16) r = (uint16_t)(pack2h_hw(o, 0.f) & 0xffffu);
  else r = (uint16_t)f2bf(o);
  out[(int64_t)b * out_stride + (int64_t)h * ATT_D + e] = r;
}

}  // namespace grit

using namespace grit;

// records per (row, head): prefix chunks, then tail splits; 0 for sizes the launches reject
static int px_slots(int Lpre, int Ltail, int* nchunks) {
  if (Lpre <= 0 || Ltail <= 0 || Ltail % PX_CH != 0) return 0;
  const int64_t nc = ((int64_t)Lpre + PX_KC - 1) / PX_KC, total = nc + Ltail / PX_CH;
  if (total > PX_MAX_SLOTS) return 0;
  if (nchunks) *nchunks = (int)nc;
  return (int)total;
}

static int px_sizes(const char* name, int B, int n, int nq, int nkv, int d, int Lpre, int Ltail, int* nchunks, int* nslot) {
  GRIT_REQUIRE(d == ATT_D, GRIT_E_UNSUPPORTED, "%s: head_dim=%d (only 128 is built)", name, d);
  GRIT_REQUIRE(B > 0 && n > 0 && B % n == 0 && nq > 0 && nkv > 0 && B <= 65535 && nq <= 65535 && nkv <= 65535, GRIT_E_BADARG,
               "%s: bad sizes (B=%d, n=%d, nq=%d, nkv=%d)", name, B, n, nq, nkv);
  GRIT_REQUIRE(nq % nkv == 0 && nq / nkv <= 8, GRIT_E_UNSUPPORTED, "%s: %d query heads per %d kv heads (whole groups of at most 8)", name, nq, nkv);
  GRIT_REQUIRE(Lpre > 0 && Ltail > 0 && Ltail % PX_CH == 0, GRIT_E_BADARG, "%s: Lpre=%d, Ltail=%d (positive, Ltail a multiple of %d)", name, Lpre,
               Ltail, PX_CH);
  GRIT_REQUIRE((int64_t)Lpre * V_PITCH < (1ll << 31), GRIT_E_UNSUPPORTED, "%s: one prefix spans more than 2 GiB (32-bit row offsets)", name);
  *nslot = px_slots(Lpre, Ltail, nchunks);
  GRIT_REQUIRE(*nslot > 0, GRIT_E_UNSUPPORTED, "%s: more than %d records per row and head (Lpre=%d in chunks of %d, Ltail=%d in splits of %d)", name,
               PX_MAX_SLOTS, Lpre, PX_KC, Ltail, PX_CH);
  return GRIT_OK;
}

extern "C" int grit_attn_decode_prefix_kc(void) { return PX_KC; }

extern "C" int64_t grit_attn_decode_prefix_workspace_floats(int B, int nq, int nkv, int Lpre, int Ltail) {
  if (B <= 0 || nq <= 0 || nkv <= 0 || B > 65535 || nq > 65535 || nkv > 65535 || nq % nkv != 0) return 0;
  return (int64_t)B * nq * px_slots(Lpre, Ltail, nullptr) * PX_REC;
}

template <bool F16>
static void px_append_launch(hipStream_t st, void* qkv, const float* cos_tab, const float* sin_tab, void* tk, void* tv, const int32_t* lens,
                             const int32_t* plen, void* q16, int B, int n, int nq, int nkv, int Ltail, int Lpos, int64_t qkv_stride,
                             int64_t q16_stride, unsigned int* flag) {
  hipLaunchKernelGGL(rope_kv_append_tail_k<F16>, dim3((unsigned)B), dim3(256), 0, st, (uint16_t*)qkv, cos_tab, sin_tab, (uint16_t*)tk, (uint16_t*)tv, lens,
                     plen, (uint16_t*)q16, n, nq, nkv, Ltail, Lpos, qkv_stride, q16_stride, flag);
}

extern "C" int grit_rope_kv_append_tail(void* qkv, const float* cos_tab, const float* sin_tab, void* tail_k, void* tail_v, const int32_t* lens,
                                        const int32_t* plen, void* q16, int B, int n, int nq, int nkv, int d, int Ltail, int Lpos,
                                        int64_t qkv_stride, int64_t q16_stride, int f16, void* stream) {
  const char* name = "grit_rope_kv_append_tail";
  GRIT_REQUIRE(qkv && cos_tab && sin_tab && tail_k && tail_v && lens && plen && (!f16 || q16), GRIT_E_BADARG, "%s: null pointer", name);
  GRIT_REQUIRE(d == ATT_D, GRIT_E_UNSUPPORTED, "%s: head_dim=%d (only 128 is built)", name, d);
  GRIT_REQUIRE(B > 0 && n > 0 && B % n == 0 && nq > 0 && nkv > 0 && B <= 65535 && nq <= 65535 && nkv <= 65535 && Ltail > 0 && Lpos > 0, GRIT_E_BADARG,
               "%s: bad sizes (B=%d, n=%d, nq=%d, nkv=%d, Ltail=%d, Lpos=%d)", name, B, n, nq, nkv, Ltail, Lpos);
  GRIT_REQUIRE(qkv_stride % 8 == 0 && qkv_stride >= ((int64_t)nq + 2 * (int64_t)nkv) * d, GRIT_E_BADARG, "%s: bad qkv_stride", name);
  GRIT_REQUIRE(!f16 || (q16_stride % 8 == 0 && q16_stride >= (int64_t)nq * d), GRIT_E_BADARG, "%s: bad q16_stride", name);
  GRIT_REQUIRE(aligned16(qkv) && aligned16(tail_k) && aligned16(tail_v) && aligned16(q16), GRIT_E_BADARG, "%s: pointers must be 16-byte aligned", name);
  unsigned int* flag = f16 ? f16_flag_ptr() : nullptr;
  if (f16 && !flag) return GRIT_E_LAUNCH;
  (f16 ? px_append_launch<true> : px_append_launch<false>)((hipStream_t)stream, qkv, cos_tab, sin_tab, tail_k, tail_v, lens, plen, q16, B, n, nq, nkv,
                                                           Ltail, Lpos, qkv_stride, q16_stride, flag);
  GRIT_CHECK_LAUNCH(name);
  return GRIT_OK;
}

template <bool F16>
static void px_prefix_launch(dim3 grid, hipStream_t st, const void* q, const void* pk, const void* pv, const int32_t* plen, float* ws, int n, int nq,
                             int nkv, int Lpre, int64_t q_stride, float scale_log2, int nqb, int nchunks, int nslot, int n_sets) {
  static std::atomic<uint64_t> optin{0};
  attn_lds_optin(attn_decode_prefix_k<F16>, optin, PX_LDS_BYTES);
  hipLaunchKernelGGL(attn_decode_prefix_k<F16>, grid, dim3(256), PX_LDS_BYTES, st, (const uint16_t*)q, (const uint16_t*)pk, (const uint16_t*)pv, plen, ws, n,
                     nq, nkv, Lpre, q_stride, scale_log2, nqb, nchunks, nslot, n_sets);
}

extern "C" int grit_attn_decode_prefix(const void* q, const void* prefix_k, const void* prefix_v, const int32_t* plen, float* workspace, int B0,
                                       int n, int nq, int nkv, int d, int Lpre, int Ltail, int64_t q_stride, float scale, int f16, void* stream) {
  const char* name = "grit_attn_decode_prefix";
  GRIT_REQUIRE(q && prefix_k && prefix_v && plen && workspace, GRIT_E_BADARG, "%s: null pointer", name);
  GRIT_REQUIRE(B0 > 0 && n > 0 && (int64_t)B0 * n <= 65535, GRIT_E_BADARG, "%s: bad sizes (B0=%d, n=%d)", name, B0, n);
  int nchunks = 0, nslot = 0;
  if (const int rc = px_sizes(name, B0 * n, n, nq, nkv, d, Lpre, Ltail, &nchunks, &nslot)) return rc;
  GRIT_REQUIRE(q_stride % 8 == 0 && q_stride >= (int64_t)nq * d, GRIT_E_BADARG, "%s: bad q_stride", name);
  GRIT_REQUIRE(aligned16(q) && aligned16(prefix_k) && aligned16(prefix_v) && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, GRIT_E_BADARG,
               "%s: q / prefix pointers must be 16-byte aligned, the workspace 8-byte", name);
  const int n_sets = B0 * nkv, nqb = (n * (nq / nkv) + ATT_QB - 1) / ATT_QB;
  const int64_t grid = 8ll * ((n_sets + 7) / 8) * nqb * nchunks;
  GRIT_REQUIRE(grid < (1ll << 30), GRIT_E_UNSUPPORTED, "%s: grid too large", name);
  (f16 ? px_prefix_launch<true> : px_prefix_launch<false>)(dim3((unsigned)grid), (hipStream_t)stream, q, prefix_k, prefix_v, plen, workspace, n, nq, nkv,
                                                           Lpre, q_stride, scale * 1.4426950408889634f, nqb, nchunks, nslot, n_sets);
  GRIT_CHECK_LAUNCH(name);
  return GRIT_OK;
}

template <bool F16>
static void px_tail_launch(dim3 grid, hipStream_t st, const void* q, const void* tk, const void* tv, const int32_t* lens, const int32_t* plen, float* ws,
                           int n, int nq, int nkv, int Ltail, int64_t q_stride, float scale, int nchunks, int nslot) {
  hipLaunchKernelGGL(attn_decode_tail_k<F16>, grid, dim3(64), 0, st, (const uint16_t*)q, (const uint16_t*)tk, (const uint16_t*)tv, lens, plen, ws, n, nq,
                     nkv, Ltail, q_stride, scale, nchunks, nslot);
}

extern "C" int grit_attn_decode_tail(const void* q, const void* tail_k, const void* tail_v, const int32_t* lens, const int32_t* plen,
                                     float* workspace, int B, int n, int nq, int nkv, int d, int Lpre, int Ltail, int64_t q_stride, float scale,
                                     int f16, void* stream) {
  const char* name = "grit_attn_decode_tail";
  GRIT_REQUIRE(q && tail_k && tail_v && lens && plen && workspace, GRIT_E_BADARG, "%s: null pointer", name);
  int nchunks = 0, nslot = 0;
  if (const int rc = px_sizes(name, B, n, nq, nkv, d, Lpre, Ltail, &nchunks, &nslot)) return rc;
  GRIT_REQUIRE(q_stride >= (int64_t)nq * d, GRIT_E_BADARG, "%s: bad q_stride", name);
  GRIT_REQUIRE(aligned16(tail_k) && aligned16(tail_v) && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, GRIT_E_BADARG,
               "%s: tail pointers must be 16-byte aligned, the workspace 8-byte", name);
  const dim3 grid((unsigned)(Ltail / PX_CH), (unsigned)nq, (unsigned)B);
  (f16 ? px_tail_launch<true> : px_tail_launch<false>)(grid, (hipStream_t)stream, q, tail_k, tail_v, lens, plen, workspace, n, nq, nkv, Ltail, q_stride,
                                                       scale, nchunks, nslot);
  GRIT_CHECK_LAUNCH(name);
  return GRIT_OK;
}

extern "C" int grit_attn_decode_prefix_combine(const float* workspace, void* out, int B, int nq, int nkv, int d, int Lpre, int Ltail,
                                               int64_t out_stride, int f16, void* stream) {
  const char* name = "grit_attn_decode_prefix_combine";
  GRIT_REQUIRE(workspace && out, GRIT_E_BADARG, "%s: null pointer", name);
  int nchunks = 0, nslot = 0;
  if (const int rc = px_sizes(name, B, 1, nq, nkv, d, Lpre, Ltail, &nchunks, &nslot)) return rc;
  GRIT_REQUIRE(out_stride >= (int64_t)nq * d, GRIT_E_BADARG, "%s: bad out_stride", name);
  const dim3 grid((unsigned)nq, (unsigned)B);
  if (f16) hipLaunchKernelGGL(attn_decode_prefix_combine_k<true>, grid, dim3(ATT_D), 0, (hipStream_t)stream, workspace, (uint16_t*)out, nq, nslot, out_stride);
  else hipLaunchKernelGGL(attn_decode_prefix_combine_k<false>, grid, dim3(ATT_D), 0, (hipStream_t)stream, workspace, (uint16_t*)out, nq, nslot, out_stride);
  GRIT_CHECK_LAUNCH(name);
  return GRIT_OK;
}
