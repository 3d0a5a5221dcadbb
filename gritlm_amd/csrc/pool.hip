// Masked mean / weighted-mean / cls / last-token pooling fused with L2-normalise, and its backward.
//
// Replaces GritLM.pooling + F.normalize (gritlm/gritlm.py:178-218, :156-158; training/model.py:151-165).
// The reference materialises hidden * mask.float() as a [B,S,H] fp32 temporary (2.1 GB at 256x512x4096)
// and reduces it; here one 512-thread workgroup per document streams the bf16 rows once (16 B per lane,
// 1 KiB per wave-instruction), skips rows whose pooling weight is zero (padding / instruction tokens are
// never read), accumulates in fp32 registers and normalises in the same launch.  HBM-bound:
// algorithmic bytes = B*S*H*2 read + B*H*4 written.
#include "common.h"

namespace grit {

constexpr int POOL_THREADS = 512;

// Pooling weights for one document, computed by wave 0 into LDS:
//   cw[k] = (position s_k, weight w_k) for the nz positions with non-zero weight, *den = denominator.
// mean: w = mask value; weightedmean: w = mask * cumsum(mask) (gritlm.py:211); cls: w[0] = 1;
// lasttoken: w[last s with mask != 0] = mask there (index clamped to 0 when the row is empty, :190-208).
__device__ void pool_weights(const int64_t* __restrict__ mrow, int instr, int S, int mode, int* cs, float* cw, int* nz_out,
                             float* den_out) {
  const int lane = threadIdx.x & 63;
  int nz = 0;
  if (mode == GRIT_POOL_CLS) {
    if (lane == 0) { cs[0] = 0; cw[0] = 1.f; *nz_out = 1; *den_out = 1.f; }
    return;
  }
  if (mode == GRIT_POOL_LASTTOKEN) {
    int last = -1;
    for (int base = 0; base < S; base += 64) {
      const int s = base + lane;
      const bool on = s < S && s >= instr && mrow[s] != 0;
      const unsigned long long b = __ballot(on);
      if (b) last = base + 63 - __builtin_clzll(b);
    }
    if (lane == 0) {
      const int idx = last < 0 ? 0 : last;
      const float w = (last < 0) ? 0.f : (float)mrow[idx];
      cs[0] = idx; cw[0] = w; *nz_out = 1; *den_out = 1.f;  // empty row: one zero-weight entry == hidden*0
    }
    return;
  }
  long long carry = 0, den = 0;
  for (int base = 0; base < S; base += 64) {
    const int s = base + lane;
    long long m = (s < S && s >= instr) ? (long long)mrow[s] : 0;
    long long w = m;
    if (mode == GRIT_POOL_WEIGHTEDMEAN) {
      long long inc = m;  // inclusive scan over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      w = m * (carry + inc);
      carry += __shfl(inc, 63, 64);
    }
    long long ws = w;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o, 64);
    den += ws;
    const bool on = w != 0;
    const unsigned long long b = __ballot(on);
    if (on) {
      const int pos = nz + __popcll(b & ((1ull << lane) - 1ull));
      cs[pos] = s; cw[pos] = (float)w;
    }
    nz += __popcll(b);
  }
  if (lane == 0) { *nz_out = nz; *den_out = (float)den; }
}

__device__ __forceinline__ void fma8(float (&a)[8], const uint4& v, float w) {
  a[0] += w * bflo(v.x); a[1] += w * bfhi(v.x); a[2] += w * bflo(v.y); a[3] += w * bfhi(v.y);
  a[4] += w * bflo(v.z); a[5] += w * bfhi(v.z); a[6] += w * bflo(v.w); a[7] += w * bfhi(v.w);
}

// a += sum over k in [k0, k1) of wt(k) * (16-byte piece cc of row row(k)); the caller says which row and which weight entry k has
template <typename RowF, typename WtF>
__device__ __forceinline__ void pool_accumulate(float (&a)[8], const uint4* __restrict__ hb, int HC, int cc, int k0, int k1, RowF row, WtF wt) {
  int k = k0;
  for (; k + 8 <= k1; k += 8) {  // 8 row loads (128 B) in flight per lane: one workgroup per CU has to cover the HBM latency alone
    uint4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = hb[(int64_t)row(k + u) * HC + cc];
#pragma unroll
    for (int u = 0; u < 8; ++u) fma8(a, v[u], wt(k + u));       // same accumulation order as one row at a time
  }
  for (; k + 4 <= k1; k += 4) {
    const uint4 v0 = hb[(int64_t)row(k) * HC + cc], v1 = hb[(int64_t)row(k + 1) * HC + cc];
    const uint4 v2 = hb[(int64_t)row(k + 2) * HC + cc], v3 = hb[(int64_t)row(k + 3) * HC + cc];
    fma8(a, v0, wt(k)); fma8(a, v1, wt(k + 1)); fma8(a, v2, wt(k + 2)); fma8(a, v3, wt(k + 3));
  }
  for (; k < k1; ++k) fma8(a, hb[(int64_t)row(k) * HC + cc], wt(k));
}

// One document of the forward, both layouts: ob[:] = (weighted row sum) / den, then L2-normalised in place when `normalize`.
// red: POOL_THREADS / 64 floats of LDS.
template <typename RowF, typename WtF>
__device__ __forceinline__ void pool_reduce_normalize(const uint4* __restrict__ hb, int H, int k0, int k1, RowF row, WtF wt, float den,
                                                      float* __restrict__ ob, float* __restrict__ inv_norm_b, int normalize, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HC = H >> 3;
  float ssq = 0.f;
  for (int cc = tid; cc < HC; cc += POOL_THREADS) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    pool_accumulate(a, hb, HC, cc, k0, k1, row, wt);
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = a[e] / den; ssq += a[e] * a[e]; }
    float4* o4 = reinterpret_cast<float4*>(ob + cc * 8);
    o4[0] = make_float4(a[0], a[1], a[2], a[3]);
    o4[1] = make_float4(a[4], a[5], a[6], a[7]);
  }
  if (!normalize) {
    if (inv_norm_b && tid == 0) *inv_norm_b = 1.f;
    return;
  }
  ssq = wave_sum(ssq);
  if (lane == 0) red[wave] = ssq;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < POOL_THREADS / 64; ++w) tot += red[w];
  const float inv = 1.0f / fmaxf(sqrtf(tot), 1e-12f);  // F.normalize eps
  if (inv_norm_b && tid == 0) *inv_norm_b = inv;
  for (int cc = tid; cc < HC; cc += POOL_THREADS) {  // each thread rescales what it wrote itself
    float4* o4 = reinterpret_cast<float4*>(ob + cc * 8);
    float4 x = o4[0], y = o4[1];
    x.x *= inv; x.y *= inv; x.z *= inv; x.w *= inv; y.x *= inv; y.y *= inv; y.z *= inv; y.w *= inv;
    o4[0] = x; o4[1] = y;
  }
}

// Pooled rows [s0, s1) of a packed document of `len` rows whose first `instr` are not pooled, and the denominator (both directions)
struct PackedSpan { int s0, s1; float den; };
__device__ __forceinline__ PackedSpan packed_span(int len, int instr, int mode) {
  PackedSpan p = {instr, len, (float)(len - instr)};
  if (mode == GRIT_POOL_WEIGHTEDMEAN) { const float n = (float)(len - instr); p.den = 0.5f * n * (n + 1.f); }
  if (mode == GRIT_POOL_CLS) { p.s0 = 0; p.s1 = len > 0 ? 1 : 0; p.den = 1.f; }
  if (mode == GRIT_POOL_LASTTOKEN) { p.s0 = len > 0 ? len - 1 : 0; p.s1 = len; p.den = 1.f; }
  return p;
}

__global__ void __launch_bounds__(POOL_THREADS) pool_norm_fwd_k(const uint16_t* __restrict__ hidden, const int64_t* __restrict__ mask,
                                                                const int32_t* __restrict__ instr_len, float* __restrict__ out,
                                                                float* __restrict__ inv_norm, int S, int H, int mode, int normalize) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* cs = reinterpret_cast<int*>(smem);                   // [S]
  float* cw = reinterpret_cast<float*>(smem + 4 * S);       // [S]
  float* red = reinterpret_cast<float*>(smem + 8 * S);      // [8] + nz + den
  int* nzp = reinterpret_cast<int*>(red + 8);
  float* denp = red + 9;

  const int b = blockIdx.x;
  if ((threadIdx.x >> 6) == 0) pool_weights(mask + (int64_t)b * S, instr_len ? instr_len[b] : 0, S, mode, cs, cw, nzp, denp);
  __syncthreads();
  // den == 0 -> NaN/inf rows exactly like the unguarded reference (:213-214)
  pool_reduce_normalize(reinterpret_cast<const uint4*>(hidden + (int64_t)b * S * H), H, 0, *nzp, [cs](int k) { return cs[k]; },
                        [cw](int k) { return cw[k]; }, *denp, out + (int64_t)b * H, inv_norm ? inv_norm + b : nullptr, normalize, red);
}

// Packed (un-padded) batches: document b occupies rows [cu[b], cu[b+1]) of hidden [T,H]; every row is a real token, the first
// instr_len[b] of them are attended to but not pooled.  Same arithmetic as pool_norm_fwd_k with mask == 1 on [instr, len).
__global__ void __launch_bounds__(POOL_THREADS) pool_norm_varlen_fwd_k(const uint16_t* __restrict__ hidden, const int32_t* __restrict__ cu,
                                                                       const int32_t* __restrict__ instr_len, float* __restrict__ out,
                                                                       float* __restrict__ inv_norm, int H, int mode, int normalize) {
  __shared__ float red[POOL_THREADS / 64];
  const int b = blockIdx.x;
  const int64_t start = cu[b];
  const int len = cu[b + 1] - cu[b];
  int instr = instr_len ? instr_len[b] : 0;
  instr = instr < len ? instr : len;
  const PackedSpan p = packed_span(len, instr, mode);
  const bool ramp = (mode == GRIT_POOL_WEIGHTEDMEAN);
  pool_reduce_normalize(reinterpret_cast<const uint4*>(hidden) + start * (H >> 3), H, p.s0, p.s1, [](int s) { return s; },
                        [ramp, instr](int s) { return ramp ? (float)(s - instr + 1) : 1.f; }, p.den, out + (int64_t)b * H,
                        inv_norm ? inv_norm + b : nullptr, normalize, red);
}

// Backward, both layouts: g[0..H) (LDS) = (dy - y (y.dy)) * inv  (normalize)  or dy.  red: POOL_THREADS / 64 floats of LDS.  The
// barrier inside also publishes what the caller wrote to LDS before the call; the caller adds the barrier that publishes g.
__device__ __forceinline__ void pool_bwd_g(const float* __restrict__ yb, const float* __restrict__ dyb, float inv, int H, int normalize,
                                           float* g, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float dot = 0.f;
  if (normalize)
    for (int i = tid; i < H; i += POOL_THREADS) dot += yb[i] * dyb[i];
  dot = wave_sum(dot);
  if (lane == 0) red[wave] = dot;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < POOL_THREADS / 64; ++w) tot += red[w];
  for (int i = tid; i < H; i += POOL_THREADS) g[i] = normalize ? (dyb[i] - yb[i] * tot) * inv : dyb[i];
}

// one wave writes one row of dhidden: w * g, or zeros where the row has no pooling weight
__device__ __forceinline__ void pool_bwd_write_row(uint4* __restrict__ drow, const float* g, int HC, float w) {
  for (int cc = threadIdx.x & 63; cc < HC; cc += 64) {
    uint4 o = make_uint4(0, 0, 0, 0);
    if (w != 0.f) {
      const float4 g0 = *reinterpret_cast<const float4*>(g + cc * 8), g1 = *reinterpret_cast<const float4*>(g + cc * 8 + 4);
      o.x = pack2bf(w * g0.x, w * g0.y); o.y = pack2bf(w * g0.z, w * g0.w);
      o.z = pack2bf(w * g1.x, w * g1.y); o.w = pack2bf(w * g1.z, w * g1.w);
    }
    drow[cc] = o;
  }
}

// dhidden[b,s,:] = (w[s]/den) * g,  g = (dy - y (y.dy)) * inv_norm  (normalize)  or dy
__global__ void __launch_bounds__(POOL_THREADS) pool_norm_bwd_k(const float* __restrict__ y, const float* __restrict__ dy,
                                                                const float* __restrict__ inv_norm, const int64_t* __restrict__ mask,
                                                                const int32_t* __restrict__ instr_len, uint16_t* __restrict__ dhidden,
                                                                int S, int H, int mode, int normalize) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* g = reinterpret_cast<float*>(smem);                        // [H]
  int* cs = reinterpret_cast<int*>(smem + 4 * (size_t)H);           // [S]
  float* cw = reinterpret_cast<float*>(smem + 4 * (size_t)H + 4 * S);
  float* ws = reinterpret_cast<float*>(smem + 4 * (size_t)H + 8 * S);  // [S] dense weights
  float* red = ws + S;                                              // [8] + nz + den
  int* nzp = reinterpret_cast<int*>(red + 8);
  float* denp = red + 9;

  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  if (wave == 0) pool_weights(mask + (int64_t)b * S, instr_len ? instr_len[b] : 0, S, mode, cs, cw, nzp, denp);
  for (int s = tid; s < S; s += POOL_THREADS) ws[s] = 0.f;
  pool_bwd_g(y + (int64_t)b * H, dy + (int64_t)b * H, normalize ? inv_norm[b] : 1.f, H, normalize, g, red);
  const int nz = *nzp;
  const float inv_den = 1.0f / *denp;
  for (int k = tid; k < nz; k += POOL_THREADS) ws[cs[k]] = cw[k] * inv_den;
  __syncthreads();
  const int HC = H >> 3;
  uint4* db = reinterpret_cast<uint4*>(dhidden + (int64_t)b * S * H);
  for (int s = wave; s < S; s += POOL_THREADS / 64) pool_bwd_write_row(db + (int64_t)s * HC, g, HC, ws[s]);
}

// packed rows: dhidden[cu[b]+s, :] = w(s) * g with the weights of pool_norm_varlen_fwd_k (no mask: every packed row is a token)
__global__ void __launch_bounds__(POOL_THREADS) pool_norm_varlen_bwd_k(const float* __restrict__ y, const float* __restrict__ dy,
                                                                       const float* __restrict__ inv_norm, const int32_t* __restrict__ cu,
                                                                       const int32_t* __restrict__ instr_len,
                                                                       uint16_t* __restrict__ dhidden, int H, int mode, int normalize) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* g = reinterpret_cast<float*>(smem);  // [H]
  float* red = g + H;                         // [POOL_THREADS/64]
  const int b = blockIdx.x, wave = threadIdx.x >> 6;
  const int64_t start = cu[b];
  const int len = cu[b + 1] - cu[b];
  int instr = instr_len ? instr_len[b] : 0;
  instr = instr < len ? instr : len;
  const PackedSpan p = packed_span(len, instr, mode);
  const bool ramp = (mode == GRIT_POOL_WEIGHTEDMEAN);
  pool_bwd_g(y + (int64_t)b * H, dy + (int64_t)b * H, normalize ? inv_norm[b] : 1.f, H, normalize, g, red);
  __syncthreads();
  const float inv_den = 1.0f / p.den;
  const int HC = H >> 3;
  uint4* db = reinterpret_cast<uint4*>(dhidden) + start * HC;
  for (int s = wave; s < len; s += POOL_THREADS / 64) {
    float w = 0.f;
    if (s >= p.s0 && s < p.s1) w = (ramp ? (float)(s - instr + 1) : 1.f) * inv_den;
    pool_bwd_write_row(db + (int64_t)s * HC, g, HC, w);
  }
}

}  // namespace grit

using namespace grit;

// The argument checks that the four entry points share, in the caller's name (S = 1 for the packed layouts, inv_ok = true for the forward;
// h_max > 0: H is bounded by the LDS row of the packed backward).  The checks that only one entry point has follow it there.
static int pool_check(const char* fn, bool ptrs_ok, bool inv_ok, int B, int S, int H, int mode, int h_max) {
  GRIT_REQUIRE(ptrs_ok, GRIT_E_BADARG, "%s: null pointer", fn);
  GRIT_REQUIRE(inv_ok, GRIT_E_BADARG, "%s: inv_norm required when normalize", fn);
  GRIT_REQUIRE(B >= 0 && S > 0 && H > 0, GRIT_E_BADARG, "%s: bad sizes", fn);
  GRIT_REQUIRE(mode >= GRIT_POOL_MEAN && mode <= GRIT_POOL_LASTTOKEN, GRIT_E_BADARG, "%s: unknown pooling mode %d", fn, mode);
  if (h_max > 0) GRIT_REQUIRE(H % 8 == 0 && H <= h_max, GRIT_E_UNSUPPORTED, "%s: H=%d must be a multiple of 8, <= %d", fn, H, h_max);
  else GRIT_REQUIRE(H % 8 == 0, GRIT_E_UNSUPPORTED, "%s: H=%d must be a multiple of 8", fn, H);
  return GRIT_OK;
}

extern "C" {

int grit_pool_norm_fwd(const void* hidden, const int64_t* mask, const int32_t* instr_len, float* out, float* inv_norm, int B, int S,
                       int H, int mode, int normalize, void* stream) {
  if (B == 0) return GRIT_OK;
  if (const int rc = pool_check("grit_pool_norm_fwd", hidden && mask && out, true, B, S, H, mode, 0)) return rc;
  GRIT_REQUIRE(S <= 16384, GRIT_E_UNSUPPORTED, "grit_pool_norm_fwd: S=%d > 16384", S);
  GRIT_REQUIRE(aligned16(hidden) && aligned16(out), GRIT_E_BADARG, "grit_pool_norm_fwd: pointers must be 16-byte aligned");
  const size_t lds = 8 * (size_t)S + 64;
  lds_optin_once<pool_norm_fwd_k>(160 * 1024);
  hipLaunchKernelGGL(pool_norm_fwd_k, dim3(B), dim3(POOL_THREADS), lds, (hipStream_t)stream, (const uint16_t*)hidden, mask, instr_len,
                     out, inv_norm, S, H, mode, normalize);
  GRIT_CHECK_LAUNCH("grit_pool_norm_fwd");
  return GRIT_OK;
}

int grit_pool_norm_varlen_fwd(const void* hidden, const int32_t* cu_seqlens, const int32_t* instr_len, float* out, float* inv_norm, int B,
                              int H, int mode, int normalize, void* stream) {
  if (B == 0) return GRIT_OK;
  if (const int rc = pool_check("grit_pool_norm_varlen_fwd", hidden && cu_seqlens && out, true, B, 1, H, mode, 0)) return rc;
  GRIT_REQUIRE(aligned16(hidden) && aligned16(out), GRIT_E_BADARG, "grit_pool_norm_varlen_fwd: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(pool_norm_varlen_fwd_k, dim3(B), dim3(POOL_THREADS), 0, (hipStream_t)stream, (const uint16_t*)hidden, cu_seqlens,
                     instr_len, out, inv_norm, H, mode, normalize);
  GRIT_CHECK_LAUNCH("grit_pool_norm_varlen_fwd");
  return GRIT_OK;
}

int grit_pool_norm_bwd(const float* y, const float* dy, const float* inv_norm, const int64_t* mask, const int32_t* instr_len,
                       void* dhidden, int B, int S, int H, int mode, int normalize, void* stream) {
  if (const int rc = pool_check("grit_pool_norm_bwd", y && dy && mask && dhidden, !normalize || inv_norm, B, S, H, mode, 0)) return rc;
  const size_t lds = 4 * (size_t)H + 12 * (size_t)S + 64;
  GRIT_REQUIRE(lds <= 160 * 1024, GRIT_E_UNSUPPORTED, "grit_pool_norm_bwd: H=%d S=%d exceed LDS", H, S);
  GRIT_REQUIRE(aligned16(dhidden), GRIT_E_BADARG, "grit_pool_norm_bwd: pointers must be 16-byte aligned");
  if (B == 0) return GRIT_OK;
  lds_optin_once<pool_norm_bwd_k>(160 * 1024);
  hipLaunchKernelGGL(pool_norm_bwd_k, dim3(B), dim3(POOL_THREADS), lds, (hipStream_t)stream, y, dy, inv_norm, mask, instr_len,
                     (uint16_t*)dhidden, S, H, mode, normalize);
  GRIT_CHECK_LAUNCH("grit_pool_norm_bwd");
  return GRIT_OK;
}

int grit_pool_norm_varlen_bwd(const float* y, const float* dy, const float* inv_norm, const int32_t* cu_seqlens, const int32_t* instr_len,
                              void* dhidden, int B, int H, int mode, int normalize, void* stream) {
  if (B == 0) return GRIT_OK;
  if (const int rc = pool_check("grit_pool_norm_varlen_bwd", y && dy && cu_seqlens && dhidden, !normalize || inv_norm, B, 1, H, mode, 32768))
    return rc;
  GRIT_REQUIRE(aligned16(dhidden), GRIT_E_BADARG, "grit_pool_norm_varlen_bwd: pointers must be 16-byte aligned");
  const size_t lds = 4 * (size_t)H + 64;
  lds_optin_once<pool_norm_varlen_bwd_k>(160 * 1024);
  hipLaunchKernelGGL(pool_norm_varlen_bwd_k, dim3(B), dim3(POOL_THREADS), lds, (hipStream_t)stream, y, dy, inv_norm, cu_seqlens, instr_len,
                     (uint16_t*)dhidden, H, mode, normalize);
  GRIT_CHECK_LAUNCH("grit_pool_norm_varlen_bwd");
  return GRIT_OK;
}
}  // extern "C"
