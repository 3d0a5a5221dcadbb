// Exhaustive inner-product search of fp32 queries against a bf16 / fp16 index in the reference's [H, N] layout, as it lies
// (rag/index.py:97-104 with --idxdtype bfloat16|float16), with the top-k selection fused into the scan: no [Q, N] score matrix.
//
// Arithmetic.  A query is not rounded to the index format: knn16_split_k writes it as three 16-bit pieces q = p0 + p1 + p2 (successive
// round-to-nearest residuals; exact for bf16 as it stands, for fp16 after scaling the row by a power of two that puts its largest
// magnitude into [2^14, 2^15), so the low pieces stay inside fp16's range; the score is scaled back exactly).  The products run on
// v_mfma_f32_16x16x32_{bf16,f16}, three per index fragment (A = query pieces, B = index): every product is exact in fp32, only the fp32
// accumulation rounds, in a fixed order (k ascending, p0 p1 p2 inside a 32-step).
//
// Geometry.  A workgroup (4 waves) owns a tile of K16_QT = 32 queries and a strip of columns, walked in chunks of K16_CW = 256 columns
// (64 per wave).  Per chunk the K loop stages [64 k][256 columns] tiles HBM -> registers -> LDS (two buffers, the loads of tile t + 1
// in flight under the products of tile t); the contraction runs over the ROW index of the tile, so the B fragments are read from the
// row-major image with ds_read_b64_tr_b16 (the idiom of the V operand in attn_tile.h).  That read needs 8-byte-aligned addresses, and
// rows of an index with arbitrary N start at arbitrary 2-byte offsets: the ALIGNED path (ld % 8 == 0, 16-byte-aligned base) loads each
// 16-byte unit once, the general path loads the two aligned 16-byte words it straddles and realigns in registers before the LDS
// write -- the LDS image, and with it every result bit, is the same.  16-byte units of the image are XOR-swizzled by the row
// (unit ^= 2 ((row & 3) | ((row >> 3) & 1) << 2)) so that the 8 rows a 32-lane half of a transposing read touches lie on distinct banks.
// The query pieces are streamed per K-tile from the (L2-resident) workspace straight into A fragments.
//
// Selection.  After a chunk's K loop the 32 x 256 scores go to LDS (over the tile buffers).  Each wave takes queries wave, wave + 4, ...:
// the chunk's columns that come before (tk_before) the strip's current k-th best are appended to the strip's running k best (kept, sorted,
// in the candidate buffer [Q, strips, k] the final reduction reads) and a bitonic sort in LDS keeps the k best; a chunk without such a
// column -- nearly all of them once the list has settled -- costs four compares per lane.  The reduction over the <= 1024 strips is
// topk_chunk_k of knn.hip.  No atomics, fixed orders: bit-reproducible, and a query's bits do not depend on Q or its neighbours.
#include "common.h"
#include "../../include/gritlm_hip_index.h"

namespace grit {

constexpr int K16_QT = 32;                        // queries per workgroup
constexpr int K16_CW = 256;                       // columns per chunk
constexpr int K16_KT = 64;                        // index rows per K-tile
constexpr int K16_T = 256;
constexpr int K16_ROW_BYTES = K16_CW * 2;         // 512
constexpr int K16_TILE_BYTES = K16_KT * K16_ROW_BYTES;   // 32 KiB
constexpr int K16_MAX_STRIPS = 1024;
constexpr int K16_MAX_K = 1024;

typedef __attribute__((ext_vector_type(4))) short k16_s4_t;
typedef __attribute__((ext_vector_type(8))) short k16_s8_t;
typedef __attribute__((address_space(3))) k16_s4_t* k16_lds_s4_ptr;
typedef __attribute__((ext_vector_type(4))) unsigned int k16_u4_t;
typedef const __attribute__((address_space(1))) k16_u4_t* k16_gptr_t;      // global_load, not flat_load (which would also count on lgkmcnt)

template <bool F16> struct k16_frag { typedef bf16x8_t type; };
template <> struct k16_frag<true> { typedef f16x8_t type; };
__device__ __forceinline__ f32x4_t mma16(bf16x8_t a, bf16x8_t b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4_t mma16(f16x8_t a, f16x8_t b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// host + device: the strip geometry of an N-column index: chunks of K16_CW columns, at most K16_MAX_STRIPS strips of `cps` chunks
struct k16_geom { int nchunks, cps, nstrips; };
static inline k16_geom k16_geometry(int64_t N) {
  k16_geom g;
  g.nchunks = (int)((N + K16_CW - 1) / K16_CW);
  g.cps = (g.nchunks + K16_MAX_STRIPS - 1) / K16_MAX_STRIPS;
  g.nstrips = (g.nchunks + g.cps - 1) / g.cps;
  return g;
}
static inline int k16_pow2ceil(int v) { int p = 2; while (p < v) p <<= 1; return p; }
static inline int64_t k16_round256(int64_t b) { return (b + 255) / 256 * 256; }

// ---- query preparation: pieces [3][Q][Hpad] (16-bit, zero for h >= H), inv_scale [Q] (1 for bf16)
template <bool F16>
__device__ __forceinline__ uint16_t k16_round(float v, float& back) {
  if constexpr (F16) {
    const _Float16 h = (_Float16)v;
    back = (float)h;
    return __builtin_bit_cast(uint16_t, h);
  } else {
    const uint32_t u = f2bf(v);
    back = __uint_as_float(u << 16);
    return (uint16_t)u;
  }
}

template <bool F16>
__global__ void __launch_bounds__(K16_T) knn16_split_k(const float* __restrict__ queries, int Q, int H, int Hpad, uint16_t* __restrict__ pieces,
                                                      float* __restrict__ inv_scale) {
#pragma clang fp contract(off)
  __shared__ float red[K16_T / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = queries + (int64_t)row * H;
  float scale = 1.f, inv = 1.f;
  if constexpr (F16) {
    float m = 0.f;
    for (int h = tid; h < H; h += K16_T) m = fmaxf(m, fabsf(x[h]));
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m > 0.f && m < INFINITY) {             // m = f 2^e, f in [0.5, 1): scale 2^(15 - e) puts it into [2^14, 2^15)
      int e;
      (void)frexpf(m, &e);
      const int sh = min(15 - e, 126);
      scale = ldexpf(1.f, sh);
      inv = ldexpf(1.f, -sh);
    }
  }
  if (tid == 0) inv_scale[row] = inv;
  const int64_t plane = (int64_t)Q * Hpad;
  uint16_t* out = pieces + (int64_t)row * Hpad;
  for (int h = tid; h < Hpad; h += K16_T) {
    const float v = h < H ? x[h] * scale : 0.f;
    float b0, b1, b2;
    const uint16_t p0 = k16_round<F16>(v, b0);
    const float r1 = v - b0;
    const uint16_t p1 = k16_round<F16>(r1, b1);
    const float r2 = r1 - b1;
    const uint16_t p2 = k16_round<F16>(r2, b2);
    out[h] = p0;
    out[plane + h] = p1;
    out[2 * plane + h] = p2;
  }
}

// ---- index tile staging
// lane's share of a K-tile: rows 8 i + (tid >> 5), i = 0 .. 7, the 16-byte unit tid & 31 (8 columns) of each
template <bool ALIGNED>
struct k16_stage {
  k16_u4_t w0[8];
  k16_u4_t w1[ALIGNED ? 1 : 8];
};

__device__ __forceinline__ uint32_t k16_sel4(uint32_t s, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return s == 0 ? a : (s == 1 ? b : (s == 2 ? c : d));
}

// issue the global loads of the tile at rows k0 .., columns c0 ..: a unit is loaded iff its row is < H and its first column < N (zeros
// otherwise: a row >= H must contribute nothing; columns >= N only feed scores that the selection leaves out).  Every load is a
// 16-byte-aligned word that contains at least one byte of the index, so none crosses into memory the index does not own a part of.
template <bool ALIGNED>
__device__ __forceinline__ void k16_load_tile(k16_stage<ALIGNED>& st, uintptr_t base, uintptr_t end, int64_t ld, int H, int N, int k0, int c0, int tid) {
  const int col = c0 + 8 * (tid & 31);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int h = k0 + 8 * i + (tid >> 5);
    st.w0[i] = (k16_u4_t){0u, 0u, 0u, 0u};
    if constexpr (!ALIGNED) st.w1[i] = (k16_u4_t){0u, 0u, 0u, 0u};
    if (h < H && col < N) {
      const uintptr_t a = base + 2 * (uintptr_t)((int64_t)h * ld + col);
      if constexpr (ALIGNED) {
        st.w0[i] = *(k16_gptr_t)a;
      } else {
        const uintptr_t wa = a & ~(uintptr_t)15;
        st.w0[i] = *(k16_gptr_t)wa;
        if ((a & 15) != 0 && wa + 16 < end) st.w1[i] = *(k16_gptr_t)(wa + 16);
      }
    }
  }
}

// write the staged tile into the (swizzled) LDS image; the general path first shifts the lane's 16 bytes out of the two words
template <bool ALIGNED>
__device__ __forceinline__ void k16_store_tile(const k16_stage<ALIGNED>& st, char* buf, uintptr_t base, int64_t ld, int k0, int c0, int tid) {
  const int u = tid & 31, col = c0 + 8 * u;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = 8 * i + (tid >> 5);
    const int sw = (r & 3) | (((r >> 3) & 1) << 2);
    k16_u4_t v = st.w0[i];
    if constexpr (!ALIGNED) {
      const uint32_t m = (uint32_t)(((base >> 1) + (uintptr_t)((int64_t)(k0 + r) * ld + col)) & 7);   // elements past the aligned word
      const uint32_t ds = m >> 1, hs = (m & 1) * 16;
      const k16_u4_t a = st.w0[i], b = st.w1[i];
      const uint32_t e0 = k16_sel4(ds, a.x, a.y, a.z, a.w), e1 = k16_sel4(ds, a.y, a.z, a.w, b.x), e2 = k16_sel4(ds, a.z, a.w, b.x, b.y),
                     e3 = k16_sel4(ds, a.w, b.x, b.y, b.z), e4 = k16_sel4(ds, b.x, b.y, b.z, b.w);
      v = (k16_u4_t){__builtin_amdgcn_alignbit(e1, e0, hs), __builtin_amdgcn_alignbit(e2, e1, hs), __builtin_amdgcn_alignbit(e3, e2, hs),
                     __builtin_amdgcn_alignbit(e4, e3, hs)};
    }
    *reinterpret_cast<k16_u4_t*>(buf + r * K16_ROW_BYTES + ((u ^ (2 * sw)) << 4)) = v;
  }
}

// the wave's own LDS traffic has completed (the lanes of a wave sort one query's candidates without workgroup barriers)
__device__ __forceinline__ void k16_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// dynamic LDS: [0, 32 K) tile buffer 0 / the chunk's scores [32][256] fp32; [32 K, ..) tile buffer 1 / the four waves' sort regions
// (sb_cap values fp32 + sb_cap columns int32 each); the last 256 bytes: the k-th best (score, column) of each query's running list
template <bool F16, bool ALIGNED>
__global__ void __launch_bounds__(K16_T, 2)
knn16_scan_k(const uint16_t* __restrict__ pieces, const float* __restrict__ inv_scale, const char* __restrict__ emb, int Q, int N, int H, int Hpad,
             int64_t ld, int k, int sb_cap, int thr_off, int cps, int nchunks, float* __restrict__ cand_v, int64_t* __restrict__ cand_i) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename k16_frag<F16>::type frag_t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int strip = blockIdx.x, nstrips = gridDim.x, q0 = blockIdx.y * K16_QT;
  float* sc = reinterpret_cast<float*>(smem);
  float* sort_v = reinterpret_cast<float*>(smem + K16_TILE_BYTES + (size_t)wave * sb_cap * 8);
  int* sort_i = reinterpret_cast<int*>(sort_v + sb_cap);
  float* thr_v = reinterpret_cast<float*>(smem + thr_off);
  int* thr_i = reinterpret_cast<int*>(thr_v + K16_QT);
  const uintptr_t base = reinterpret_cast<uintptr_t>(emb);
  const uintptr_t end = base + 2 * (uintptr_t)((int64_t)(H - 1) * ld + N);
  const int64_t plane = (int64_t)Q * Hpad;
  const int nt = Hpad / K16_KT;

  // transposing B-fragment reads: lane 4 qr + p of a 16-lane group addresses row qr, columns 4 p .. 4 p + 3 of a [4 k][16 columns] block and
  // receives column (lane & 15) of the four rows; group g = lane >> 4 takes k = 8 g .. 8 g + 7 of the 32-step in two reads (rows +0, +4)
  const int g = lane >> 4, qr = (lane & 15) >> 2, p = lane & 3;
  uint32_t b_off[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int sw = qr | ((g & 1) << 2);          // (row & 3) | ((row >> 3) & 1) << 2 of rows 32 ks + 8 g + qr (+ 4)
    b_off[nb] = (uint32_t)((8 * g + qr) * K16_ROW_BYTES + (((wave * 8 + 2 * nb + (p >> 1)) ^ (2 * sw)) << 4) + 8 * (p & 1));
  }
  // A fragments: lane holds pieces[piece][q0 + 16 mb + (lane & 15)][k0 + 32 ks + 8 g .. + 8]; rows >= Q are zero
  uint4 af[2][3][2];
  auto load_a = [&](int k0) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int q = q0 + 16 * mb + (lane & 15);
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          af[mb][pc][ks] = make_uint4(0u, 0u, 0u, 0u);
          if (q < Q) af[mb][pc][ks] = *reinterpret_cast<const uint4*>(pieces + pc * plane + (int64_t)q * Hpad + k0 + 32 * ks + 8 * g);
        }
    }
  };

  for (int ci = 0; ci < cps; ++ci) {
    const int chunk = strip * cps + ci;
    if (chunk >= nchunks) break;
    const int c0 = chunk * K16_CW;
    f32x4_t acc[2][4];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    k16_stage<ALIGNED> st;
    k16_load_tile<ALIGNED>(st, base, end, ld, H, N, 0, c0, tid);
    load_a(0);
    k16_store_tile<ALIGNED>(st, smem, base, ld, 0, c0, tid);
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      char* cur = smem + (t & 1) * K16_TILE_BYTES;
      const bool more = t + 1 < nt;
      if (more) k16_load_tile<ALIGNED>(st, base, end, ld, H, N, (t + 1) * K16_KT, c0, tid);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        frag_t bf[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          const k16_s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((k16_lds_s4_ptr)(cur + b_off[nb] + (32 * ks) * K16_ROW_BYTES));
          const k16_s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((k16_lds_s4_ptr)(cur + b_off[nb] + (32 * ks + 4) * K16_ROW_BYTES));
          bf[nb] = __builtin_bit_cast(frag_t, (k16_s8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
        }
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = mma16(__builtin_bit_cast(frag_t, af[mb][pc][ks]), bf[nb], acc[mb][nb]);
      }
      if (more) {
        load_a((t + 1) * K16_KT);
        k16_store_tile<ALIGNED>(st, smem + ((t + 1) & 1) * K16_TILE_BYTES, base, ld, (t + 1) * K16_KT, c0, tid);
      }
      __syncthreads();
    }

    // scores -> LDS: accumulator register r of (mb, nb) is query 16 mb + 4 g + r, column 64 wave + 16 nb + (lane & 15)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[(16 * mb + 4 * g + r) * K16_CW + 64 * wave + 16 * nb + (lane & 15)] = acc[mb][nb][r];
    if (ci == 0 && tid < K16_QT) { thr_v[tid] = -INFINITY; thr_i[tid] = INT32_MAX; }
    __syncthreads();

    for (int qi = wave; qi < K16_QT && q0 + qi < Q; qi += K16_T / 64) {
      const int q = q0 + qi;
      const float tv = thr_v[qi];
      const int ti = thr_i[qi];
      float inv = 1.f;
      if constexpr (F16) inv = inv_scale[q];
      float s[4];
      bool cand[4];
      bool any = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = c0 + 64 * j + lane;
        float v = sc[qi * K16_CW + 64 * j + lane] * inv;
        v = (v != v) ? -INFINITY : v;
        s[j] = v;
        cand[j] = col < N && tk_before(v, col, tv, ti);
        any = any || cand[j];
      }
      if (__builtin_amdgcn_ballot_w64(any) == 0ull) continue;
      float* lv = cand_v + ((int64_t)q * nstrips + strip) * k;
      int64_t* li = cand_i + ((int64_t)q * nstrips + strip) * k;
      for (int j = lane; j < k; j += 64) {
        float v = -INFINITY;
        int c = INT32_MAX;
        if (ci != 0) {
          v = lv[j];
          const int64_t c64 = li[j];
          c = c64 > (int64_t)INT32_MAX ? INT32_MAX : (int)c64;
        }
        sort_v[j] = v;
        sort_i[j] = c;
      }
      int total = k;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t b = __builtin_amdgcn_ballot_w64(cand[j]);
        if (cand[j]) {
          const int o = total + __popcll(b & ((1ull << lane) - 1ull));
          sort_v[o] = s[j];
          sort_i[o] = c0 + 64 * j + lane;
        }
        total += __popcll(b);
      }
      int sb = 2;
      while (sb < total) sb <<= 1;
      for (int j = total + lane; j < sb; j += 64) { sort_v[j] = -INFINITY; sort_i[j] = INT32_MAX; }
      k16_wave_sync();
      // bitonic sort of sb <= sb_cap entries by one wave, "tk_before" order first (as topk_chunk_k)
      for (int size = 2; size <= sb; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          for (int t = lane; t < sb / 2; t += 64) {
            const int lo = 2 * t - (t & (stride - 1));
            const int hi = lo + stride;
            const bool up = ((lo & size) == 0);
            const float va = sort_v[lo], vb = sort_v[hi];
            const int ia = sort_i[lo], ib = sort_i[hi];
            const bool swap = up ? tk_before(vb, ib, va, ia) : tk_before(va, ia, vb, ib);
            if (swap) { sort_v[lo] = vb; sort_v[hi] = va; sort_i[lo] = ib; sort_i[hi] = ia; }
          }
          k16_wave_sync();
        }
      }
      for (int j = lane; j < k; j += 64) {
        const int c = sort_i[j];
        lv[j] = sort_v[j];
        li[j] = c == INT32_MAX ? INT64_MAX : (int64_t)c;
      }
      if (lane == 0) { thr_v[qi] = sort_v[k - 1]; thr_i[qi] = sort_i[k - 1]; }
    }
    __syncthreads();
  }
}

struct k16_plan {
  k16_geom g;
  int Hpad, sb_cap, lds_bytes;
  int64_t off_scale, off_a, off_b, total;      // workspace: pieces at 0, then inv_scale, candidate buffers A and B (values, then columns)
  int64_t na, nb;                              // candidate entries of A and B
};
static k16_plan k16_make_plan(int Q, int64_t N, int H, int k) {
  k16_plan p;
  p.g = k16_geometry(N);
  p.Hpad = (H + K16_KT - 1) / K16_KT * K16_KT;
  p.sb_cap = k16_pow2ceil(k + K16_CW);
  const int sort_bytes = 4 * p.sb_cap * 8;
  p.lds_bytes = K16_TILE_BYTES + (sort_bytes > K16_TILE_BYTES ? sort_bytes : K16_TILE_BYTES) + 256;
  // A: the strips' lists [Q, nstrips, k] (not needed when one strip writes the result itself); B: the first reduction level's output
  p.na = p.g.nstrips > 1 ? (int64_t)Q * p.g.nstrips * k : 0;
  const int64_t n1 = (int64_t)p.g.nstrips * k, c1 = (n1 + TK_C - 1) / TK_C;
  p.nb = c1 > 1 ? (int64_t)Q * c1 * k : 0;
  p.off_scale = k16_round256(6ll * Q * p.Hpad);
  p.off_a = p.off_scale + k16_round256(4ll * Q);
  p.off_b = p.off_a + k16_round256(p.na * 4) + k16_round256(p.na * 8);
  p.total = p.off_b + k16_round256(p.nb * 4) + k16_round256(p.nb * 8);
  return p;
}

template <bool F16>
static int k16_launch(const float* queries, const void* emb, int Q, int N, int H, int64_t ld, int k, const k16_plan& p, char* ws, float* out_scores,
                      int64_t* out_index, hipStream_t st) {
  uint16_t* pieces = reinterpret_cast<uint16_t*>(ws);
  float* inv_scale = reinterpret_cast<float*>(ws + p.off_scale);
  float* cv[2] = {reinterpret_cast<float*>(ws + p.off_a), reinterpret_cast<float*>(ws + p.off_b)};
  int64_t* ci[2] = {reinterpret_cast<int64_t*>(ws + p.off_a + k16_round256(p.na * 4)), reinterpret_cast<int64_t*>(ws + p.off_b + k16_round256(p.nb * 4))};
  hipLaunchKernelGGL(knn16_split_k<F16>, dim3((unsigned)Q), dim3(K16_T), 0, st, queries, Q, H, p.Hpad, pieces, inv_scale);
  GRIT_CHECK_LAUNCH("grit_knn16_topk: query split");
  const bool one = p.g.nstrips == 1;
  float* sv = one ? out_scores : cv[0];
  int64_t* si = one ? out_index : ci[0];
  const dim3 grid((unsigned)p.g.nstrips, (unsigned)((Q + K16_QT - 1) / K16_QT));
  const bool aligned = (ld % 8 == 0) && aligned16(emb);
  auto scan = [&](auto al) {
    constexpr bool AL = decltype(al)::value;
    lds_optin_once<knn16_scan_k<F16, AL>>(K16_TILE_BYTES + 4 * k16_pow2ceil(K16_MAX_K + K16_CW) * 8 + 256);
    hipLaunchKernelGGL((knn16_scan_k<F16, AL>), grid, dim3(K16_T), p.lds_bytes, st, pieces, inv_scale, (const char*)emb, Q, N, H, p.Hpad, ld, k,
                       p.sb_cap, p.lds_bytes - 256, p.g.cps, p.g.nchunks, sv, si);
  };
  if (aligned) scan(std::true_type{});
  else scan(std::false_type{});
  GRIT_CHECK_LAUNCH("grit_knn16_topk: scan");
  if (one) return GRIT_OK;
  // the strips' lists -> the k best: topk_chunk_k levels, as grit_knn_topk reduces its first level
  const float* in_v = cv[0];
  const int64_t* in_i = ci[0];
  int64_t n = (int64_t)p.g.nstrips * k;
  int cur = 1;
  for (;;) {
    const int64_t nch = (n + TK_C - 1) / TK_C;
    const bool last = nch == 1;
    float* ov = last ? out_scores : cv[cur];
    int64_t* oi = last ? out_index : ci[cur];
    hipLaunchKernelGGL(topk_chunk_k, dim3((unsigned)nch, (unsigned)Q), dim3(TK_T), 0, st, in_v, in_i, n, n, n, k, ov, oi, (int)nch);
    GRIT_CHECK_LAUNCH("grit_knn16_topk: top-k");
    if (last) break;
    in_v = ov; in_i = oi; n = nch * k;
    cur ^= 1;
  }
  return GRIT_OK;
}

static bool k16_sizes_ok(int Q, int64_t N, int H, int k) {
  return Q > 0 && N > 0 && H > 0 && k > 0 && Q <= 65535 && N < (1ll << 31) && k <= K16_MAX_K && k <= N;
}

}  // namespace grit

using namespace grit;

extern "C" int64_t grit_knn16_workspace_bytes(int Q, int64_t N, int H, int k) {
  if (!k16_sizes_ok(Q, N, H, k)) return 0;   // 0 for sizes grit_knn16_topk rejects
  return k16_make_plan(Q, N, H, k).total;
}

extern "C" int grit_knn16_topk(const float* queries, const void* embeddings, int is_f16, int Q, int64_t N, int H, int64_t ld, int k, void* workspace,
                               float* out_scores, int64_t* out_index, void* stream) {
  if (Q == 0) return GRIT_OK;
  GRIT_REQUIRE(queries && embeddings && workspace && out_scores && out_index, GRIT_E_BADARG, "grit_knn16_topk: null pointer");
  GRIT_REQUIRE(Q > 0 && N > 0 && H > 0, GRIT_E_BADARG, "grit_knn16_topk: bad sizes Q=%d N=%lld H=%d", Q, (long long)N, H);
  GRIT_REQUIRE(ld >= N, GRIT_E_BADARG, "grit_knn16_topk: ld=%lld < N=%lld", (long long)ld, (long long)N);
  GRIT_REQUIRE((reinterpret_cast<uintptr_t>(embeddings) & 1u) == 0, GRIT_E_BADARG, "grit_knn16_topk: embeddings at an odd address");
  GRIT_REQUIRE(N < (1ll << 31), GRIT_E_UNSUPPORTED, "grit_knn16_topk: N=%lld >= 2^31 (shard the index)", (long long)N);
  GRIT_REQUIRE(k > 0 && k <= K16_MAX_K && k <= N, GRIT_E_UNSUPPORTED, "grit_knn16_topk: k=%d (1..min(N, %d))", k, K16_MAX_K);
  GRIT_REQUIRE(Q <= 65535, GRIT_E_UNSUPPORTED, "grit_knn16_topk: Q=%d > 65535 (batch the queries)", Q);
  const k16_plan p = k16_make_plan(Q, N, H, k);
  hipStream_t st = (hipStream_t)stream;
  if (is_f16) return k16_launch<true>(queries, embeddings, Q, (int)N, H, ld, k, p, (char*)workspace, out_scores, out_index, st);
  return k16_launch<false>(queries, embeddings, Q, (int)N, H, ld, k, p, (char*)workspace, out_scores, out_index, st);
}
