// Cross-lane operations shared by the integrator (ros3_kernel.hip) and the hand-over kernels (pack.hip): the partner's value inside a lane row comes
// by DPP (quad swaps, half-row mirror, row mirror), across lane rows by v_permlane16/32_swap.  Device code of gfx950, header-only: every unit that
// includes it gets copies of its own (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mistra {

namespace {

template <int CTRL>
__device__ __forceinline__ double dpp_partner(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32));
}

// Maximum over the wave, the same value in every lane: six pairing steps.  Neither operand is a NaN (the callers keep NaNs out of what they hand over).
[[maybe_unused]] __device__ __forceinline__ double max_nn(double a, double b) { return b > a ? b : a; }
[[maybe_unused]] __device__ __forceinline__ double wave_max(double v) {
  v = max_nn(v, dpp_partner<0xB1>(v));       // quad_perm [1,0,3,2]
  v = max_nn(v, dpp_partner<0x4E>(v));       // quad_perm [2,3,0,1]
  v = max_nn(v, dpp_partner<0x141>(v));      // row_half_mirror
  v = max_nn(v, dpp_partner<0x140>(v));      // row_mirror
  {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const auto l = __builtin_amdgcn_permlane16_swap((uint32_t)u, (uint32_t)u, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap((uint32_t)(u >> 32), (uint32_t)(u >> 32), false, false);
    v = max_nn(__builtin_bit_cast(double, (uint64_t)l[0] | ((uint64_t)h[0] << 32)), __builtin_bit_cast(double, (uint64_t)l[1] | ((uint64_t)h[1] << 32)));
  }
  {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const auto l = __builtin_amdgcn_permlane32_swap((uint32_t)u, (uint32_t)u, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap((uint32_t)(u >> 32), (uint32_t)(u >> 32), false, false);
    v = max_nn(__builtin_bit_cast(double, (uint64_t)l[0] | ((uint64_t)h[0] << 32)), __builtin_bit_cast(double, (uint64_t)l[1] | ((uint64_t)h[1] << 32)));
  }
  return v;
}

}  // namespace

}  // namespace mistra
