// Skinny MFMA GEMMs for the decode step at 9..64 rows (the batched native decoder): out[b,n] = x[b,:] . W[n,:] for B <= 64 rows and
// the 7B projections (N = 4096 .. 32000, K = 4096 / 14336).  The GEMV of decode.hip does per-row work for every weight element (its cost
// grows with the rows); the 256 x 256 tiles of gemm_bf16.hip would put 16 workgroups on 256 CUs at N = 4096.  Here one workgroup owns
// 16 (or 32) weight rows -- every weight element is read from HBM once per launch -- and ALL the B rows of x, which stay in L2 and are
// re-read by every column tile.  v_mfma_f32_16x16x32_{bf16,f16}: A = 16 weight rows, B = 16 x rows (one "row block"; up to 4 of them).
//
// Decomposition: the K dimension is split over the workgroup's waves (chunks of 64 k, chunk c to wave c % WV) and the waves' fp32
// partial tiles are summed through LDS in wave order -- no split over workgroups, so no atomics and no cross-workgroup hand-off: the
// results are bit-reproducible, and the sum order of an output depends on K and on the launch form, which depends on N only.  A row's
// MFMA products do not depend on the other columns of the B operand, so a row's output is the same bits whatever B is and wherever the
// row sits (batch invariance; rows >= B are zero operands and never written).
//   N < 16384 and every RESIDUAL (q|k|v, o_proj, down at the 7B shape): 16 weight rows and 8 waves per workgroup -- N = 4096 gives 256
//   workgroups, one per CU; SWIGLU and a STORE at N >= 16384 (gate|up, lm_head): 32 weight rows (for SWIGLU one gate and one up block of
//   the interleaved layout) and 4 waves; the deferred-norm forms of these need 184 VGPR + AGPR = 2 waves per SIMD, so 2 workgroups per
//   CU and the 896 gate|up workgroups run in 1.75 rounds.
// Weights go through non-temporal loads straight into VGPRs (the GEMV's measured choice: streamed once, shared with nobody); x
// fragments are plain loads straight into VGPRs (16 rows x 64 B per instruction; L2 hits after the first column tiles).
// KNOWN LIMIT (measured, profiles/batched_decode_bench.json and the kernel trace in profiles/README.md): every workgroup re-reads all B
// rows of x over the whole K, so at B = 64 the L2 -> CU x traffic is 4x the weight bytes in the 16-row form and 2x in the 32-row form
// (about 41 GB of x re-reads per 7B step against 14.5 GB of weights).  That stream, not HBM, is the likely bound at 64 rows (no PMC
// counters taken yet): the step runs at 0.21 of its roofline, and the launches at 0.13 (q|k|v) .. 0.30 (lm_head) of the HBM bound of
// their weight bytes.  cdna_hip_programming.md §5 measured fragment-shaped x loads at +18-45 % against full-line LDS staging; staging
// alone would not remove the re-reads -- the fix is a decomposition where the waves of a workgroup share one x chunk through LDS across
// more weight rows (and a split over workgroups to keep 256 CUs busy at N = 4096), which this file does not have yet.
// Epilogues and rounding points: grit_gemv_bf16 / grit_gemv_f16
// (include/gritlm_hip.h).  The deferred norm accumulates the row's sum of squares from the x fragments the waves load for the product
// (every x element is loaded by exactly one lane of one wave) and multiplies the finished sums by rsqrt(mean x^2 + eps); the MFMA needs a
// 16-bit operand, so x * ln_weight is rounded ONCE to the operand format (the GEMV keeps it in fp32).
#include "decode_epi.h"

namespace grit {

__device__ __forceinline__ f32x4_t dg_mma(bf16x8_t a, bf16x8_t b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4_t dg_mma(f16x8_t a, f16x8_t b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

__device__ __forceinline__ uint4 dg_wload(const uint16_t* p) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}

constexpr int DG_MAX_MB = 4;      // row blocks of 16: B <= 64

// MODE 0: store, 1: + residual, 2: SwiGLU (NT = 2: column tile 0 = the 16 gate rows, 1 = the 16 up rows of one interleaved block).
// PRENORM: the deferred RMSNorm (x = the raw stream, or its fp16 copy under F16).  F16: fp16 operands, formats of grit_gemv_f16.
// Lane l of a wave: A operand = weight row (l & 15) of a column tile, B operand = x row (l & 15) of a row block, both at k pieces
// 8 (l >> 4) .. + 7 of each 32-k step; the accumulator holds out[b = 16 mb + (l & 15)][n = 16 nt + 4 (l >> 4) + i], i < 4.
template <int MODE, bool PRENORM, bool F16, int NT, int WV>
__global__ void __launch_bounds__(64 * WV) decode_gemm_k(const uint16_t* __restrict__ x, const uint16_t* __restrict__ W, void* out,
                                                         const void* res, const uint16_t* __restrict__ ln_w, float eps, int B, int N, int K,
                                                         int64_t ldx, int64_t ldw, int64_t ldo, int64_t ldr, unsigned int* __restrict__ flag,
                                                         uint16_t* __restrict__ out16, int64_t ldo16) {
  static_assert(MODE != 2 || NT == 2, "SWIGLU pairs a gate and an up tile");
  using frag_t = std::conditional_t<F16, f16x8_t, bf16x8_t>;
  __shared__ f32x4_t red[WV][DG_MAX_MB][NT][64];
  __shared__ float red_ss[PRENORM ? WV : 1][DG_MAX_MB][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int MB = (B + 15) >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * (16 * NT);
  const uint16_t* wp[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wp[nt] = W + (n0 + nt * 16 + r) * ldw + g * 8;
  const uint16_t* xp[DG_MAX_MB];
  bool xin[DG_MAX_MB];
#pragma unroll
  for (int mb = 0; mb < DG_MAX_MB; ++mb) {
    const int b = mb * 16 + r;
    xin[mb] = b < B;
    xp[mb] = x + (int64_t)(xin[mb] ? b : 0) * ldx + g * 8;
  }
  f32x4_t acc[DG_MAX_MB][NT];
#pragma unroll
  for (int mb = 0; mb < DG_MAX_MB; ++mb)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mb][nt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float ss[DG_MAX_MB] = {0.f, 0.f, 0.f, 0.f};
  uint32_t bad = 0;                                           // F16 + PRENORM: OR of h2_nonfinite() over the rounded operands
  const int nch = K >> 6;
  // two chunks per iteration: every weight and x piece of both is requested before the first product
  for (int c0 = wave; c0 < nch; c0 += 2 * WV) {
    const bool two = c0 + WV < nch;
    uint4 wv[2][NT][2], xv[2][DG_MAX_MB][2], lw[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      const int k = (c0 + u * WV) * 64;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 2; ++j) wv[u][nt][j] = dg_wload(wp[nt] + k + j * 32);
#pragma unroll
      for (int mb = 0; mb < DG_MAX_MB; ++mb)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          xv[u][mb][j] = make_uint4(0, 0, 0, 0);
          if (mb < MB && xin[mb]) xv[u][mb][j] = *reinterpret_cast<const uint4*>(xp[mb] + k + j * 32);
        }
      if (PRENORM) {
#pragma unroll
        for (int j = 0; j < 2; ++j) lw[u][j] = *reinterpret_cast<const uint4*>(ln_w + k + j * 32 + g * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int mb = 0; mb < DG_MAX_MB; ++mb) {
          if (mb >= MB) break;
          uint4 xb = xv[u][mb][j];
          if (PRENORM) {
#pragma clang fp contract(off)
            const uint4 l4 = lw[u][j];
            const float xf[8] = {lo16_op<F16>(xb.x), hi16_op<F16>(xb.x), lo16_op<F16>(xb.y), hi16_op<F16>(xb.y),
                                 lo16_op<F16>(xb.z), hi16_op<F16>(xb.z), lo16_op<F16>(xb.w), hi16_op<F16>(xb.w)};
            const float lf[8] = {bflo(l4.x), bfhi(l4.x), bflo(l4.y), bfhi(l4.y), bflo(l4.z), bfhi(l4.z), bflo(l4.w), bfhi(l4.w)};   // (norm weights stay bf16)
#pragma unroll
            for (int e = 0; e < 8; ++e) ss[mb] = __builtin_fmaf(xf[e], xf[e], ss[mb]);
            xb.x = pack2_op<F16>(xf[0] * lf[0], xf[1] * lf[1]);
            xb.y = pack2_op<F16>(xf[2] * lf[2], xf[3] * lf[3]);
            xb.z = pack2_op<F16>(xf[4] * lf[4], xf[5] * lf[5]);
            xb.w = pack2_op<F16>(xf[6] * lf[6], xf[7] * lf[7]);
            if (F16) bad |= h2_nonfinite(xb.x) | h2_nonfinite(xb.y) | h2_nonfinite(xb.z) | h2_nonfinite(xb.w);
          }
          const frag_t bfr = __builtin_bit_cast(frag_t, xb);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) acc[mb][nt] = dg_mma(__builtin_bit_cast(frag_t, wv[u][nt][j]), bfr, acc[mb][nt]);
        }
      }
    }
  }
  // the waves' partial tiles, summed in wave order by the epilogue threads
#pragma unroll
  for (int mb = 0; mb < DG_MAX_MB; ++mb) {
    if (mb >= MB) break;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) red[wave][mb][nt][lane] = acc[mb][nt];
    if (PRENORM) red_ss[PRENORM ? wave : 0][mb][lane] = ss[mb];
  }
  __syncthreads();
  if (F16 && PRENORM && bad) atomicOr(flag, 1u);
  const int slots = MB * (MODE == 2 ? 1 : NT) * 64;
  for (int s = threadIdx.x; s < slots; s += 64 * WV) {
    const int l = s & 63, t = s >> 6;
    const int mb = MODE == 2 ? t : t / NT, nt = MODE == 2 ? 0 : t - mb * NT;
    const int b = mb * 16 + (l & 15);
    if (b >= B) continue;
    float rs = 1.f;
    if (PRENORM) {
      float q = 0.f;
#pragma unroll
      for (int w = 0; w < WV; ++w)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) q += red_ss[PRENORM ? w : 0][mb][gg * 16 + (l & 15)];
      rs = rsqrtf(q / (float)K + eps);
    }
    auto total = [&](int ntile) -> f32x4_t {
      f32x4_t v = red[0][mb][ntile][l];
#pragma unroll
      for (int w = 1; w < WV; ++w) v += red[w][mb][ntile][l];
      return v * rs;
    };
    // this thread's four elements (decode_epi.h holds the rounding points): RESIDUAL reads all four residual elements before it writes
    // the first (out may be the residual: in place)
    const int q4 = 4 * (l >> 4);
    const int64_t n = n0 + nt * 16 + q4;
    const f32x4_t v = total(nt);
    f32x4_t r = v;                                            // SWIGLU: the up sums; RESIDUAL: the residual; STORE: unused
    int64_t o = (int64_t)b * ldo + n;
    if (MODE == 2) {
      r = total(1 % NT);
      o = (int64_t)b * ldo + n0 / 2 + q4;                     // pair p: gate row (p / 16) * 32 + p % 16, up row + 16
    }
    if (MODE == 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = decode_epi_residual<F16>(res, (int64_t)b * ldr + n + i);
    }
    uint32_t ob = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) ob |= decode_epi<MODE, F16>(v[i], r[i], out, o + i, out16, (int64_t)b * ldo16 + n + i);
    if (F16 && ob) atomicOr(flag, 1u);
  }
}

}  // namespace grit

using namespace grit;

namespace {

template <int MODE, bool PRENORM, bool F16, int NT, int WV>
void dg_launch(const void* x, const void* W, void* out, const void* res, const void* ln_w, float eps, int B, int N, int K, int64_t ldx,
               int64_t ldw, int64_t ldo, int64_t ldr, unsigned int* flag, void* out16, int64_t ldo16, hipStream_t st) {
  hipLaunchKernelGGL((decode_gemm_k<MODE, PRENORM, F16, NT, WV>), dim3((unsigned)(N / (16 * NT))), dim3(64 * WV), 0, st, (const uint16_t*)x,
                     (const uint16_t*)W, out, res, (const uint16_t*)ln_w, eps, B, N, K, ldx, ldw, ldo, ldr, flag, (uint16_t*)out16, ldo16);
}

// the launch form depends on N (and the epilogue) only, never on B: 32 weight rows and 4 waves per workgroup for SWIGLU and for a STORE
// at N >= 16384 with N % 32 == 0 (lm_head), else 16 rows and 8 waves (RESIDUAL always: the decoder's o_proj / down, N = hidden size)
template <int MODE, bool PRENORM, bool F16, class... Args>
void dg_run(int N, Args... args) {
  if constexpr (MODE == 2) dg_launch<MODE, PRENORM, F16, 2, 4>(args...);
  else if constexpr (MODE == 1) dg_launch<MODE, PRENORM, F16, 1, 8>(args...);
  else if (N >= 16384 && N % 32 == 0) dg_launch<MODE, PRENORM, F16, 2, 4>(args...);
  else dg_launch<MODE, PRENORM, F16, 1, 8>(args...);
}

// ln_w: the deferred norm in front (STORE / SWIGLU)
template <bool F16>
int dg_entry(const char* name, const void* x, const void* W, void* out, const void* ln_w, float eps, int B, int N, int K,
             int64_t ldx, int64_t ldw, int64_t ldo, int epilogue, const void* residual, int64_t ldr, void* out16, int64_t ldo16, void* stream) {
  if (const int rc = decode_proj_pointers(name, x, W, out)) return rc;
  GRIT_REQUIRE(B >= 1 && B <= 64, GRIT_E_UNSUPPORTED, "%s: B=%d rows (1..64)", name, B);
  GRIT_REQUIRE(N > 0 && K > 0, GRIT_E_BADARG, "%s: bad sizes", name);
  GRIT_REQUIRE(K % 64 == 0, GRIT_E_UNSUPPORTED, "%s: K=%d must be a multiple of 64", name, K);
  GRIT_REQUIRE(N % 16 == 0, GRIT_E_UNSUPPORTED, "%s: N=%d must be a multiple of 16", name, N);
  GRIT_REQUIRE(ldx % 8 == 0 && ldw % 8 == 0 && ldx >= K && ldw >= K, GRIT_E_BADARG, "%s: bad leading dimensions", name);
  if (const int rc = decode_proj_aligned(name, x, W, ln_w)) return rc;
  return decode_proj_epilogue(name, epilogue, ln_w != nullptr, N, ldo, residual, ldr, out16, ldo16, [&](auto mode) -> int {
    constexpr int MODE = decltype(mode)::value;
    unsigned int* flag;
    if (const int rc = decode_proj_flag<F16>(name, &flag)) return rc;
    auto run = [&](auto pn) {
      dg_run<MODE, decltype(pn)::value, F16>(N, x, W, out, residual, ln_w, eps, B, N, K, ldx, ldw, ldo, ldr, flag, out16, ldo16, (hipStream_t)stream);
    };
    if constexpr (MODE == 1) run(std::false_type{});          // (RESIDUAL takes no norm: refused above)
    else if (ln_w) run(std::true_type{});
    else run(std::false_type{});
    GRIT_CHECK_LAUNCH(name);
    return GRIT_OK;
  });
}

}  // namespace

extern "C" int grit_decode_gemm_bf16(const void* x, const void* W, void* out, int B, int N, int K, int64_t ldx, int64_t ldw, int64_t ldo,
                                     int epilogue, const void* residual, int64_t ldr, void* stream) {
  return dg_entry<false>("grit_decode_gemm_bf16", x, W, out, nullptr, 0.f, B, N, K, ldx, ldw, ldo, epilogue, residual, ldr, nullptr, 0, stream);
}

extern "C" int grit_decode_gemm_f16(const void* x, const void* W, void* out, int B, int N, int K, int64_t ldx, int64_t ldw, int64_t ldo,
                                    int epilogue, const void* residual, int64_t ldr, void* out16, int64_t ldo16, void* stream) {
  GRIT_REQUIRE(!out16 || epilogue == GRIT_EPI_RESIDUAL, GRIT_E_BADARG, "grit_decode_gemm_f16: out16 goes with the RESIDUAL epilogue");
  return dg_entry<true>("grit_decode_gemm_f16", x, W, out, nullptr, 0.f, B, N, K, ldx, ldw, ldo, epilogue, residual, ldr, out16, ldo16, stream);
}

extern "C" int grit_rmsnorm_decode_gemm_bf16_deferred(const void* x, const void* ln_weight, float eps, const void* W, void* out, int B, int N,
                                                      int K, int64_t ldx, int64_t ldw, int64_t ldo, int epilogue, void* stream) {
  GRIT_REQUIRE(ln_weight, GRIT_E_BADARG, "grit_rmsnorm_decode_gemm_bf16_deferred: null pointer");
  GRIT_REQUIRE(epilogue != GRIT_EPI_RESIDUAL, GRIT_E_BADARG, "grit_rmsnorm_decode_gemm_bf16_deferred: STORE or SWIGLU");
  return dg_entry<false>("grit_rmsnorm_decode_gemm_bf16_deferred", x, W, out, ln_weight, eps, B, N, K, ldx, ldw, ldo, epilogue, nullptr, 0,
                  nullptr, 0, stream);
}

extern "C" int grit_rmsnorm_decode_gemm_f16_deferred(const void* x, const void* ln_weight, float eps, const void* W, void* out, int B, int N,
                                                     int K, int64_t ldx, int64_t ldw, int64_t ldo, int epilogue, void* stream) {
  GRIT_REQUIRE(ln_weight, GRIT_E_BADARG, "grit_rmsnorm_decode_gemm_f16_deferred: null pointer");
  GRIT_REQUIRE(epilogue != GRIT_EPI_RESIDUAL, GRIT_E_BADARG, "grit_rmsnorm_decode_gemm_f16_deferred: STORE or SWIGLU");
  return dg_entry<true>("grit_rmsnorm_decode_gemm_f16_deferred", x, W, out, ln_weight, eps, B, N, K, ldx, ldw, ldo, epilogue, nullptr, 0,
                  nullptr, 0, stream);
}
