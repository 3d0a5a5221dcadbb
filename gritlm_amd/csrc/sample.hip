// Sampled next token on the device (include/gritlm_hip.h, grit_sample_advance): temperature, top-k and top-p as Hugging Face's
// multinomial sampling applies them (generation/utils.py _get_logits_processor + _sample: TemperatureLogitsWarper -> TopKLogitsWarper ->
// TopPLogitsWarper -> one draw), the draw by Gumbel-max on counter-based Philox4x32-10 noise -- the reference's sampled evaluation,
// scripts/generative_eval.sh (--do_sample True --temperature 0.2 --n_samples 20).
//
// One workgroup of 1024 threads per row.  The row's scaled fp32 scores of the first 32768 columns are staged once in LDS (128 KiB of the
// CU's 160), every pass reads them from there; columns beyond are read again from the logits in every pass.  The two thresholds are
// radix walks over the order-preserving uint32 keys of the scores, 11 + 11 + 10 bits, with integer weights summed by integer LDS
// atomics: the result does not depend on arrival order.  The draw is an argmax: no prefix sum, and the token does not depend on how
// the vocabulary is split.
#include <cfloat>

#include "common.h"
#include "next_token.h"

namespace grit {
namespace {

constexpr int ST = 1024;            // threads per row
constexpr int SW = ST / 64;         // waves per row
constexpr int LC = 4096;            // chunks of 8 scores staged in LDS (V <= 32768)
constexpr int NB = 2048;            // radix bins of a level

// the scaled score of one logit: x / T (fp32 division); +inf -> FLT_MAX; NaN and -inf stay as they are and are excluded (key 0)
__device__ __forceinline__ float scale_logit(float x, float T) {
  const float s = x / T;
  return s == INFINITY ? FLT_MAX : s;
}
// order-preserving key of a score; 0 for an excluded score (NaN, -inf): every finite score has a key >= 0x00800000
__device__ __forceinline__ uint32_t skey(float s) {
  const uint32_t b = __float_as_uint(s);
  return s > -INFINITY ? (b ^ ((b & 0x80000000u) ? 0xffffffffu : 0x80000000u)) : 0u;
}
// fixed-point softmax mass of a score: exp(s - M) in fp32, times 2^32, truncated (the maximum weighs exactly 2^32)
__device__ __forceinline__ unsigned long long smass(float s, float M) { return (unsigned long long)(expf(s - M) * 4294967296.0f); }

// the scaled scores of logits 8c .. 8c+7 (columns >= V: -inf, excluded)
template <bool L32>
__device__ __forceinline__ void load8(const void* row, int c, int V, float T, float (&s)[8]) {
  float x[8];
  load8_logits<L32>(row, c, V, x);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = scale_logit(x[e], T);
}

struct Smem {
  float4 sc[2 * LC];                    // the scaled scores of chunks 0 .. LC-1
  unsigned int hc[NB];                  // tokens per bin
  unsigned long long hw[NB];            // mass per bin (top-p walk)
  unsigned long long wu[SW];
  float wf[SW];
  int wi[SW];
};

// f(c, s[8]) for every chunk c of this thread, ascending
template <bool L32, class F>
__device__ __forceinline__ void for_chunks(const Smem& sm, const void* row, int NC, int V, float T, int tid, F&& f) {
  for (int c = tid; c < NC; c += ST) {
    float s[8];
    if (c < LC) {
      const float4 a = sm.sc[2 * c], b = sm.sc[2 * c + 1];
      s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    } else {
      load8<L32>(row, c, V, T, s);
    }
    f(c, s);
  }
}

template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* sh, int lane, int wave) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  v = sh[0];
  for (int w = 1; w < SW; ++w) v = op(v, sh[w]);
  __syncthreads();
  return v;
}

// The lowest key K present among the walk's tokens such that the weight of the walk's tokens with a key > K is < thr (thr >= 1; the
// walk's largest key always qualifies).  The walk's tokens: key >= lo; MASS: also a nonzero mass (weight = mass), else weight 1.
template <bool MASS, bool L32>
__device__ uint32_t radix_walk(Smem& sm, const void* row, int NC, int V, float T, float M, uint32_t lo,
                               unsigned long long thr, int tid, int lane, int wave) {
  uint32_t prefix = 0, pmask = 0;
  unsigned long long above = 0;
  for (int lvl = 0; lvl < 3; ++lvl) {
    const int shift = lvl == 0 ? 21 : (lvl == 1 ? 10 : 0);
    const uint32_t bmask = lvl == 2 ? 1023u : 2047u;
    for (int j = tid; j < NB; j += ST) {
      sm.hc[j] = 0;
      if (MASS) sm.hw[j] = 0;
    }
    __syncthreads();
    for_chunks<L32>(sm, row, NC, V, T, tid, [&](int, const float (&s)[8]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t k = skey(s[e]);
        if (k >= lo && (k & pmask) == prefix) {
          const unsigned long long m = MASS ? smass(s[e], M) : 1ull;
          if (m) {
            const uint32_t bin = (k >> shift) & bmask;
            atomicAdd(&sm.hc[bin], 1u);
            if (MASS) atomicAdd(&sm.hw[bin], m);
          }
        }
      }
    });
    __syncthreads();
    // suffix sums: thread t owns bins 2t, 2t+1
    const int j0 = 2 * tid, j1 = j0 + 1;
    const unsigned long long w0 = MASS ? sm.hw[j0] : sm.hc[j0], w1 = MASS ? sm.hw[j1] : sm.hc[j1];
    const bool p0 = sm.hc[j0] != 0, p1 = sm.hc[j1] != 0;
    unsigned long long incl = w0 + w1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_down(incl, o, 64);
      if (lane + o < 64) incl += y;
    }
    if (lane == 0) sm.wu[wave] = incl;
    __syncthreads();
    unsigned long long after = incl - (w0 + w1);                // weight in bins > j1
    for (int w = wave + 1; w < SW; ++w) after += sm.wu[w];
    int best = 0x7fffffff;
    unsigned long long best_above = 0;
    if (p1 && above + after < thr) { best = j1; best_above = above + after; }
    if (p0 && above + after + w1 < thr) { best = j0; best_above = above + after + w1; }
    __syncthreads();                                            // (sm.wu is reused below)
    const int jb = block_reduce(best, [](int a, int b) { return a < b ? a : b; }, sm.wi, lane, wave);
    if (jb == 0x7fffffff) return lo;                            // (no token: not reached, the caller checks that one exists)
    if (best == jb) sm.wu[0] = best_above;
    __syncthreads();
    above = sm.wu[0];
    prefix |= (uint32_t)jb << shift;
    pmask |= bmask << shift;
    __syncthreads();
  }
  return prefix;
}

// Philox4x32-10 (Random123): counter c, key k
__device__ __forceinline__ void philox(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
  }
}
// Gumbel noise of one Philox word: u = ((x >> 8) + 1/2) 2^-24, E = -log(u) with an exact argument (-log1p(-(1 - u)) for u >= 1/2),
// g = -log(E)
__device__ __forceinline__ float gumbel(uint32_t x) {
  const uint32_t m = x >> 8;
  const float E = m < (1u << 23) ? -logf(((float)m + 0.5f) * 0x1p-24f) : -log1pf(-(((float)((1u << 24) - m) - 0.5f) * 0x1p-24f));
  return -logf(E);
}

template <bool L32>
__global__ void __launch_bounds__(ST) sample_advance_k(const void* __restrict__ logits, int64_t ld, int V, int64_t* __restrict__ next,
                                                       int32_t* __restrict__ lens, int64_t* __restrict__ history, int64_t hist_stride,
                                                       const int32_t* __restrict__ step, float T, int top_k, float top_p,
                                                       const unsigned long long* __restrict__ keys) {
  __shared__ Smem sm;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const void* row = L32 ? (const void*)(reinterpret_cast<const float*>(logits) + (int64_t)b * ld)
                        : (const void*)(reinterpret_cast<const uint16_t*>(logits) + (int64_t)b * ld);
  const int NC = (V >> 3) + ((V & 7) != 0);
  for (int c = tid; c < NC && c < LC; c += ST) {
    float s[8];
    load8<L32>(row, c, V, T, s);
    sm.sc[2 * c] = make_float4(s[0], s[1], s[2], s[3]);
    sm.sc[2 * c + 1] = make_float4(s[4], s[5], s[6], s[7]);
  }
  __syncthreads();
  // the maximum score (keys order the scores; key 0: no finite score in the row)
  uint32_t kmax = 0;
  for_chunks<L32>(sm, row, NC, V, T, tid, [&](int, const float (&s)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) kmax = max(kmax, skey(s[e]));
  });
  kmax = block_reduce(kmax, [](uint32_t a, uint32_t c) { return a > c ? a : c; }, (uint32_t*)sm.wi, lane, wave);
  int tok = 0;                                                  // a row without a finite logit draws token 0
  if (kmax != 0) {
    const uint32_t mb = (kmax & 0x80000000u) ? (kmax ^ 0x80000000u) : ~kmax;
    const float M = __uint_as_float(mb);
    uint32_t lo = 1;
    if (top_k > 0 && top_k < V) lo = radix_walk<false, L32>(sm, row, NC, V, T, M, 1, (unsigned long long)top_k, tid, lane, wave);
    if (top_p < 1.0f) {
      unsigned long long z = 0;
      for_chunks<L32>(sm, row, NC, V, T, tid, [&](int, const float (&s)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (skey(s[e]) >= lo) z += smass(s[e], M);
      });
      z = block_reduce(z, [](unsigned long long a, unsigned long long c) { return a + c; }, sm.wu, lane, wave);
      const double t = ceil((double)top_p * (double)z);
      const unsigned long long thr = t < 1.0 ? 1ull : (unsigned long long)t;
      lo = radix_walk<true, L32>(sm, row, NC, V, T, M, lo, thr, tid, lane, wave);
    }
    // Gumbel-max over the kept tokens: counter (v >> 2, t, 0, 0), key (lo, hi) of the row's 64-bit key, word v & 3
    const uint32_t pos = step ? (uint32_t)step[0] : 0u;
    const unsigned long long key = keys[b];
    float bz = -INFINITY;
    int bi = 0x7fffffff;
    for_chunks<L32>(sm, row, NC, V, T, tid, [&](int c, const float (&s)[8]) {
      bool any = false;
#pragma unroll
      for (int e = 0; e < 8; ++e) any |= skey(s[e]) >= lo;
      if (!any) return;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        uint32_t ctr[4] = {(uint32_t)(2 * c + h), pos, 0u, 0u};
        philox(ctr, (uint32_t)key, (uint32_t)(key >> 32));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = 4 * h + q;
          if (skey(s[e]) >= lo) take_better(bz, bi, s[e] + gumbel(ctr[q]), c * 8 + e);
        }
      }
    });
    block_best<SW>(bz, bi, sm.wf, sm.wi, tid);
    tok = bi;                                                   // (thread 0's is the row's)
  }
  if (tid == 0) commit_token(b, tok, next, lens, history, hist_stride, step);
}

}  // namespace
}  // namespace grit

using namespace grit;

template <bool L32>
static int sample_launch(const char* name, const void* logits, int64_t ld, int V, int64_t* next, int32_t* lens, int64_t* history,
                         int64_t hist_stride, int32_t* step, int B, float temperature, int top_k, float top_p, const uint64_t* keys,
                         void* stream) {
  GRIT_REQUIRE(std::isfinite(temperature) && temperature > 0.f, GRIT_E_BADARG, "%s: temperature must be > 0 and finite", name);
  GRIT_REQUIRE(top_p >= 0.f && top_p <= 1.f, GRIT_E_BADARG, "%s: top_p must lie in [0, 1]", name);
  GRIT_REQUIRE(top_k >= 0, GRIT_E_BADARG, "%s: top_k must be >= 0", name);
  if (B == 0) return GRIT_OK;
  if (const int rc = next_token_check(name, logits && next && keys, logits, ld, V, history, step, B)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sample_advance_k<L32>, dim3((unsigned)B), dim3(ST), 0, st, logits, ld, V, next, lens, history, hist_stride, step,
                     temperature, top_k, top_p, (const unsigned long long*)keys);
  return next_token_finish(name, step, st);
}

extern "C" int grit_sample_advance(const void* logits, int64_t ld, int V, int64_t* next, int32_t* lens, int64_t* history, int64_t hist_stride,
                                   int32_t* step, int B, void* stream, float temperature, int top_k, float top_p, const uint64_t* keys) {
  return sample_launch<false>("grit_sample_advance", logits, ld, V, next, lens, history, hist_stride, step, B, temperature, top_k, top_p,
                              keys, stream);
}

extern "C" int grit_sample_advance_f32(const void* logits, int64_t ld, int V, int64_t* next, int32_t* lens, int64_t* history,
                                       int64_t hist_stride, int32_t* step, int B, void* stream, float temperature, int top_k, float top_p,
                                       const uint64_t* keys) {
  return sample_launch<true>("grit_sample_advance_f32", logits, ld, V, next, lens, history, hist_stride, step, B, temperature, top_k, top_p,
                             keys, stream);
}
