// The pieces the two next-token kernels share -- the greedy argmax_advance_k (decode.hip, 256 threads per row) and the sampling
// sample_advance_k (sample.hip, 1024 threads per row): the load of eight logits, the (value, index) reduction in which the lowest index
// wins, the commit of the chosen token, the step bump and the host checks.
#pragma once
#include "common.h"

namespace grit {

// Logits 8c .. 8c+7 of a bf16 (L32: fp32) row as fp32, one or two 16-byte loads (rows are 16-byte aligned and ld % 8 == 0)
template <bool L32>
__device__ __forceinline__ void load8_full(const void* row, int c, float (&x)[8]) {
  if constexpr (L32) {
    const float4 u = reinterpret_cast<const float4*>(row)[2 * c], w = reinterpret_cast<const float4*>(row)[2 * c + 1];
    x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = w.x; x[5] = w.y; x[6] = w.z; x[7] = w.w;
  } else {
    const uint4 u = reinterpret_cast<const uint4*>(row)[c];
    x[0] = bflo(u.x); x[1] = bfhi(u.x); x[2] = bflo(u.y); x[3] = bfhi(u.y); x[4] = bflo(u.z); x[5] = bfhi(u.z); x[6] = bflo(u.w); x[7] = bfhi(u.w);
  }
}
// ... of a row of V columns whose last chunk may be partial: columns >= V are never read and come back as -inf
template <bool L32>
__device__ __forceinline__ void load8_logits(const void* row, int c, int V, float (&x)[8]) {
  if (c * 8 + 8 <= V) {
    load8_full<L32>(row, c, x);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int v = c * 8 + e;
      x[e] = v < V ? (L32 ? reinterpret_cast<const float*>(row)[v] : bf2f(reinterpret_cast<const uint16_t*>(row)[v])) : -INFINITY;
    }
  }
}

// (value, index) <- the better of two candidates: the larger value, the lower index on equal values
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// The best (value, index) of the workgroup's NW waves: over the wave by shuffles, then over the waves through shv / shi (NW slots).
// Thread 0 holds the result; the order of the steps does not matter (a total order: value descending, index ascending).
template <int NW>
__device__ __forceinline__ void block_best(float& v, int& i, float* shv, int* shi, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    take_better(v, i, ov, oi);
  }
  if ((tid & 63) == 0) { shv[tid >> 6] = v; shi[tid >> 6] = i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NW; ++w) take_better(v, i, shv[w], shi[w]);
  }
}

// one thread per row: the token becomes the next input id and an entry of the history, and the sequence grows by it
__device__ __forceinline__ void commit_token(int b, int tok, int64_t* next, int32_t* lens, int64_t* history, int64_t hist_stride,
                                             const int32_t* step) {
  next[b] = tok;
  if (history) history[(int64_t)b * hist_stride + step[0]] = tok;
  if (lens) lens[b] += 1;
}

// the step counter advances BEHIND the rows' kernel (every row reads step[0]): a launch of its own, in stream order
static __global__ void step_bump_k(int32_t* v) { v[0] += 1; }

// host: the checks of a next-token entry point behind `if (B == 0) return GRIT_OK` (pointers: logits, next and whatever else it needs)
static inline int next_token_check(const char* name, bool pointers, const void* logits, int64_t ld, int V, const void* history, const void* step,
                                   int B) {
  GRIT_REQUIRE(pointers, GRIT_E_BADARG, "%s: null pointer", name);
  GRIT_REQUIRE(V > 0 && ld >= V && ld % 8 == 0 && B > 0 && (!history || step), GRIT_E_BADARG, "%s: bad sizes", name);
  GRIT_REQUIRE(aligned16(logits), GRIT_E_BADARG, "%s: logits must be 16-byte aligned", name);
  return GRIT_OK;
}

// host: behind the rows' launch -- its error check, then the step bump
static inline int next_token_finish(const char* name, int32_t* step, hipStream_t st) {
  GRIT_CHECK_LAUNCH(name);
  if (step) {
    hipLaunchKernelGGL(step_bump_k, dim3(1), dim3(1), 0, st, step);
    GRIT_CHECK_LAUNCH(name);
  }
  return GRIT_OK;
}

}  // namespace grit
