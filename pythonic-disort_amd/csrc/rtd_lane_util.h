// rtd_lane_util.h -- the few helpers that the eigen kernels (rtd_eig*.hip) and the boundary-condition kernels (rtd_bc*.hip) both
// use, defined once.  Included inside each file's anonymous namespace, after <type_traits> (it includes nothing itself).
// NOT here: xor_lane, which exists in two forms on purpose -- DPP moves in rtd_eig.hip, ds_swizzle in rtd_bc_common.h.
#pragma once

// compiler-only barrier: keeps the scheduler from hoisting a whole unrolled loop's LDS loads
#define RTD_FENCE() asm volatile("" ::: "memory")

// 1/x to full double precision from the hardware seed (x > 0, normal range): two Newton steps
__device__ __forceinline__ double fast_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = y * (2.0 - x * y);
  y = y * (2.0 - x * y);
  return y;
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// value of `v` in the lane `lane` (wave-uniform): v_readlane_b32 per dword, an SGPR pair
__device__ __forceinline__ double readlane_f64(const double v, const int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
