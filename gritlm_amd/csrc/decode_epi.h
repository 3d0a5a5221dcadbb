// What the two decode projections -- the GEMV of decode.hip (1..8 rows) and the MFMA row GEMM of decode_gemm.hip (1..64 rows) -- share:
// the rounding points of one output element and the host checks around the epilogue argument.  The C entry points of the two files have
// the same signatures and must round alike (include/gritlm_hip.h, grit_gemv_bf16 / grit_gemv_f16); a rounding point changes HERE.
#pragma once
#include <type_traits>

#include "common.h"

namespace grit {

// one fp32 value -> the 16 bits of its fp16 rounding (RNE; beyond 65504: inf, reported by the caller)
__device__ __forceinline__ uint16_t f2h_bits(float f) { return (uint16_t)(pack2h_hw(f, 0.f) & 0xffffu); }

// the residual element a RESIDUAL epilogue adds: bf16, or the fp32 stream under F16.  A caller that finishes several elements loads all
// of them before it stores the first (out may be the residual: in place)
template <bool F16>
__device__ __forceinline__ float decode_epi_residual(const void* res, int64_t i) {
  if constexpr (F16) return reinterpret_cast<const float*>(res)[i];
  else return bf2f(reinterpret_cast<const uint16_t*>(res)[i]);
}

// One finished output element.  MODE 0 (STORE): out[o] = v.  MODE 1 (RESIDUAL): out[o] = v + r.  MODE 2 (SWIGLU): out[o] = silu(v) * r,
// v the gate's and r the up row's sum.
// bf16 operands: out is bf16; RESIDUAL rounds the product before the add and the sum after it (two launches' bits), SWIGLU rounds gate, up,
// silu(gate) and the product (the un-fused kernels' bits).
// F16: STORE / RESIDUAL write fp32, nothing rounded; RESIDUAL with out16 also writes out16[o16] = fp16(out), the operand copy of the stream
// the next norm + projection reads; SWIGLU writes the fp16 activation, one rounding of silu(gate) * up.
// Returns non-zero iff an fp16 value it wrote left the fp16 range: the caller raises the device's overflow flag (atomicOr(flag, 1u)).
template <int MODE, bool F16>
__device__ __forceinline__ uint32_t decode_epi(float v, float r, void* out, int64_t o, uint16_t* out16, int64_t o16) {
  if constexpr (MODE == 2) {
    uint16_t* oh = reinterpret_cast<uint16_t*>(out);
    if constexpr (F16) {
      const uint16_t hb = f2h_bits(silu_f(v) * r);
      oh[o] = hb;
      return h2_nonfinite(hb);
    } else {
      oh[o] = (uint16_t)f2bf(round_bf(silu_f(round_bf(v))) * round_bf(r));
      return 0;
    }
  } else if constexpr (F16) {
    if (MODE == 1) v += r;
    reinterpret_cast<float*>(out)[o] = v;
    if (MODE == 1 && out16) {
      const uint16_t hb = f2h_bits(v);
      out16[o16] = hb;
      return h2_nonfinite(hb);
    }
    return 0;
  } else {
    if (MODE == 1) v = round_bf(v) + r;
    reinterpret_cast<uint16_t*>(out)[o] = (uint16_t)f2bf(v);
    return 0;
  }
}

// ---- host: the checks of a projection entry point that do not depend on its shape limits ----
static inline int decode_proj_pointers(const char* name, const void* x, const void* W, const void* out) {
  GRIT_REQUIRE(x && W && out, GRIT_E_BADARG, "%s: null pointer", name);
  return GRIT_OK;
}
static inline int decode_proj_aligned(const char* name, const void* x, const void* W, const void* ln_w) {
  GRIT_REQUIRE(aligned16(x) && aligned16(W) && (!ln_w || aligned16(ln_w)), GRIT_E_BADARG, "%s: pointers must be 16-byte aligned", name);
  return GRIT_OK;
}

// the epilogue's own checks, then launch(std::integral_constant<int, MODE>) -- behind the other checks of an entry point.
// pn: a norm is fused in front (STORE / SWIGLU only)
template <class Launch>
static int decode_proj_epilogue(const char* name, int epilogue, bool pn, int N, int64_t ldo, const void* residual, int64_t ldr, const void* out16,
                                int64_t ldo16, Launch&& launch) {
  switch (epilogue) {
    case GRIT_EPI_STORE: GRIT_REQUIRE(ldo >= N, GRIT_E_BADARG, "%s: ldo < N", name);
      return launch(std::integral_constant<int, 0>{});
    case GRIT_EPI_RESIDUAL: GRIT_REQUIRE(residual && ldo >= N && ldr >= N && !pn, GRIT_E_BADARG, "%s: RESIDUAL needs residual, ldo, ldr >= N (no pre-norm)", name);
      GRIT_REQUIRE(!out16 || ldo16 >= N, GRIT_E_BADARG, "%s: ldo16 < N", name);
      return launch(std::integral_constant<int, 1>{});
    case GRIT_EPI_SWIGLU: GRIT_REQUIRE(N % 32 == 0 && ldo >= N / 2, GRIT_E_UNSUPPORTED, "%s: SWIGLU needs N %% 32 == 0, ldo >= N/2", name);
      return launch(std::integral_constant<int, 2>{});
    default: GRIT_REQUIRE(false, GRIT_E_BADARG, "%s: unknown epilogue %d", name, epilogue);
  }
  return GRIT_OK;
}

// the device's fp16 overflow flag word for an F16 launch (nullptr for bf16 operands, which never raise it)
template <bool F16>
static int decode_proj_flag(const char* name, unsigned int** flag) {
  *flag = F16 ? f16_flag_ptr() : nullptr;
  GRIT_REQUIRE(!F16 || *flag, GRIT_E_LAUNCH, "%s: the overflow flag word of this device is not reachable", name);
  return GRIT_OK;
}

}  // namespace grit
