// One kernel per translation unit: ros3_integrate_kernel<MT, NT, VARIANT, METHOD> for one of the options variants the product unit does not hold
// (ros3_kernel.hip: 3 a method kernel, 4 the step-control trace, 5 a series, 6 the reaction flux) on gas, aer or tot, with its launcher; a series unit
// holds the dense-output kernel (VARIANT 7) of its mechanism and method as well, a trace unit the operator kernel (VARIANT 8) and the replay kernel (VARIANT 9) of its mechanism; a method unit
// and (for Ros3) a trace unit the series kernel with rate constants linear in time (VARIANT 10) and the series kernel with the reaction flux (VARIANT 11)
// of its mechanism and method (below).  Compiled
// once per unit of mistra_amd/build.py: VARIANT_UNITS.  Units of their own because the non-inlined device functions the kernels share (vm_run,
// gsum_run*, tail_solve, scale_run, dense_lu, dense_finish) are compiled once per unit, under the register budget of all kernels in it: the product
// kernels' unit (ros3_kernel.hip) must compile as it does without these, and each of these as it does without the others.
#if !defined(MISTRA_UNIT_VARIANT) || !defined(MISTRA_UNIT_MECH) || !defined(MISTRA_UNIT_METHOD)
#error "build with -DMISTRA_UNIT_VARIANT=<3 method | 4 trace | 5 series | 6 flux> -DMISTRA_UNIT_MECH=<0 gas | 1 aer | 2 tot> -DMISTRA_UNIT_METHOD=<1 Ros2 | 2 Ros3 | 3 Ros4 | 4 Rodas3 | 5 Rodas4>"
#endif
#define MISTRA_METHOD_TU 1
#include "ros3_kernel.hip"

namespace mistra {

#if MISTRA_UNIT_MECH == 0
using UnitMT = GasTraits;
constexpr int kUnitNT = kGasNT;
#elif MISTRA_UNIT_MECH == 1
using UnitMT = AerTraits;
constexpr int kUnitNT = kAerNT;
#else
using UnitMT = TotTraits;
constexpr int kUnitNT = kTotNT;
#endif

template <>
hipError_t launch_ros_unit<UnitMT, kUnitNT, MISTRA_UNIT_VARIANT, MISTRA_UNIT_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr int VARIANT = MISTRA_UNIT_VARIANT, METHOD = MISTRA_UNIT_METHOD;
  static_assert(VARIANT >= 3 && VARIANT <= 6, "the options variants: method, trace, series, flux");
  static_assert(METHOD >= kRos2 && METHOD <= kRodas4, "IPAR(4) resolved: 1 .. 5");
  static_assert(VARIANT != 3 || METHOD != kRos3, "Ros3 with options is the product unit's VARIANT 3 kernel");
  static_assert(VARIANT != 4 || METHOD == kRos3, "the step-control trace is a Ros3 instantiation");
  // the cell's state as the product kernels lay it out; the trace keeps the 2*NW cells of its largest-term reduction (value, species per wave) behind it
  constexpr int NW = kUnitNT / 64;
  constexpr size_t lds_bytes = (LdsLayout<UnitMT, kUnitNT>::TOTAL + (VARIANT == 4 ? 2 * NW : 0)) * sizeof(double);
  static_assert(lds_bytes <= 160 * 1024, "cell state and the trace's reduction cells do not fit the 160 KiB LDS of a gfx950 CU");
  auto kern = ros3_integrate_kernel<UnitMT, kUnitNT, VARIANT, METHOD>;
  if (!a.opt) return hipErrorInvalidValue;      // all of these are options instantiations
  if constexpr (VARIANT == 4) {
    if (!a.ntrace || a.trace_cap < 0 || (a.trace_cap > 0 && (!a.trace_d || !a.trace_i))) return hipErrorInvalidValue;
  } else if constexpr (VARIANT == 5) {
    if (!a.times || a.nleg < 1) return hipErrorInvalidValue;
  } else if constexpr (VARIANT == 6) {
    if (!a.flux) return hipErrorInvalidValue;
  }
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kUnitNT), lds_bytes, stream, a);
  return hipGetLastError();
}

#if MISTRA_UNIT_VARIANT == 5
// Dense output (VARIANT 7) is a kernel variant without units of its own: its instantiation lives here, beside the series kernel of the same mechanism and
// method — both are "output at several times" under the same workgroup size and register budget, so the unit's non-inlined device functions compile as
// they do.  Its own argument guard and its own lds_configured flag (capi.cpp: DeviceState, [mechanism][7][method]).
template <>
hipError_t launch_ros_unit<UnitMT, kUnitNT, 7, MISTRA_UNIT_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr size_t lds_bytes = LdsLayout<UnitMT, kUnitNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<UnitMT, kUnitNT, 7, MISTRA_UNIT_METHOD>;
  if (!a.opt) return hipErrorInvalidValue;
  if (!a.times || !a.dense_out || !a.dense_nout || a.dense_ns < 1 || a.nleg != 0) return hipErrorInvalidValue;
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kUnitNT), lds_bytes, stream, a);
  return hipGetLastError();
}
#endif

#if MISTRA_UNIT_VARIANT == 4
// The operators (VARIANT 8) are a kernel variant without units of their own: the instantiation lives here, beside the step-control trace of the same
// mechanism — both are Ros3 diagnostics under the same workgroup size and register budget, so the unit's non-inlined device functions compile as they
// do.  Its own argument guard and its own lds_configured flag (capi.cpp: DeviceState, [mechanism][8][Ros3]); no options block.
template <>
hipError_t launch_ros_unit<UnitMT, kUnitNT, 8, MISTRA_UNIT_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr size_t lds_bytes = LdsLayout<UnitMT, kUnitNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<UnitMT, kUnitNT, 8, MISTRA_UNIT_METHOD>;
  if (!a.var_in || !a.fix || !a.rconst || (!a.ops_vdot && !a.ops_jvs && !a.ops_x)) return hipErrorInvalidValue;
  if (a.ops_x && (!a.ops_shift || !a.ops_ising || (a.ops_shift_stride != 0 && a.ops_shift_stride != 1) || a.ops_nrhs < 0 ||
                  (a.ops_fun_rhs ? 1 : 0) + a.ops_nrhs < 1 || (a.ops_nrhs > 0 && !a.ops_rhs)))
    return hipErrorInvalidValue;
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kUnitNT), lds_bytes, stream, a);
  return hipGetLastError();
}

// The replay (VARIANT 9) likewise: Ros3 along a prescribed step sequence, the counterpart of the trace that hands the sequence out.  Its own argument guard
// and its own lds_configured flag (capi.cpp: DeviceState, [mechanism][9][Ros3]); an options instantiation.
template <>
hipError_t launch_ros_unit<UnitMT, kUnitNT, 9, MISTRA_UNIT_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr size_t lds_bytes = LdsLayout<UnitMT, kUnitNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<UnitMT, kUnitNT, 9, MISTRA_UNIT_METHOD>;
  if (!a.opt) return hipErrorInvalidValue;
  if (!a.replay_n || a.replay_cap < 0 || a.replay_h_stride < 0 || (a.replay_cap > 0 && !a.replay_h) || (a.replay_h_stride != 0 && a.replay_h_stride < a.replay_cap))
    return hipErrorInvalidValue;
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kUnitNT), lds_bytes, stream, a);
  return hipGetLastError();
}
#endif

#if MISTRA_UNIT_VARIANT == 3 || MISTRA_UNIT_VARIANT == 4
// The series with rate constants linear in time (VARIANT 10) is a kernel variant without units of its own: its instantiation lives beside the options
// kernel of the same mechanism and method where that has a unit — the method units (Ros2, Ros4, Rodas3, Rodas4) — and, for Ros3, in the trace unit of the
// mechanism: the same workgroup size and register budget, so the unit's non-inlined device functions compile as they do.  (The series and the flux units
// are pinned to the kernels they hold: tests/test_ros_dense.py, tests/test_ros_flux.py.)  Its own argument guard and its own lds_configured flag
// (capi.cpp: DeviceState, [mechanism][10][method]).  (Behind every other specialisation: the kernels in front of it keep their place in the unit.)
template <>
hipError_t launch_ros_unit<UnitMT, kUnitNT, 10, MISTRA_UNIT_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr size_t lds_bytes = LdsLayout<UnitMT, kUnitNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<UnitMT, kUnitNT, 10, MISTRA_UNIT_METHOD>;
  if (!a.opt) return hipErrorInvalidValue;
  if (!a.times || a.nleg < 1 || !a.lin_rates || a.leg_rconst <= 0 || !a.rconst || a.flux || a.dense_nout) return hipErrorInvalidValue;
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kUnitNT), lds_bytes, stream, a);
  return hipGetLastError();
}

// The series with the reaction flux of every leg (VARIANT 11) likewise, in the same units for the same reasons: the series kernel and the flux kernel of a
// mechanism and method in one.  Its own argument guard and its own lds_configured flag (capi.cpp: DeviceState, [mechanism][11][method]).  (Behind every
// other specialisation: the kernels in front of it keep their place in the unit.)
template <>
hipError_t launch_ros_unit<UnitMT, kUnitNT, 11, MISTRA_UNIT_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr size_t lds_bytes = LdsLayout<UnitMT, kUnitNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<UnitMT, kUnitNT, 11, MISTRA_UNIT_METHOD>;
  if (!a.opt) return hipErrorInvalidValue;
  if (!a.times || a.nleg < 1 || !a.flux || a.leg_flux <= 0 || a.lin_rates || a.dense_nout) return hipErrorInvalidValue;
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kUnitNT), lds_bytes, stream, a);
  return hipGetLastError();
}
#endif

}  // namespace mistra
