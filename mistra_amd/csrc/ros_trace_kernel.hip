// One step-control trace kernel per translation unit: ros3_integrate_kernel<MT, NT, 4> — the options kernel (VARIANT 3, Ros3) plus one record
// per attempt that reaches ros_ErrorNorm_x (kernel_args.hpp: trace_d, trace_i, ntrace, ctrl) — with its launcher.  Compiled three times
// (mistra_amd/build.py: -DMISTRA_TRACE_MECH=0|1|2).  Units of their own for the reason the method kernels have theirs (ros_method_kernel.hip):
// the non-inlined device functions are compiled once per unit under the register budget of all kernels in it, and the product kernels' unit
// (ros3_kernel.hip) must compile as it does without these.
#if !defined(MISTRA_TRACE_MECH)
#error "build with -DMISTRA_TRACE_MECH=<0 gas | 1 aer | 2 tot>"
#endif
#define MISTRA_METHOD_TU 1
#include "ros3_kernel.hip"

namespace mistra {

#if MISTRA_TRACE_MECH == 0
using TraceMT = GasTraits;
constexpr int kTraceNT = kGasNT;
#elif MISTRA_TRACE_MECH == 1
using TraceMT = AerTraits;
constexpr int kTraceNT = kAerNT;
#else
using TraceMT = TotTraits;
constexpr int kTraceNT = kTotNT;
#endif

template <>
hipError_t launch_ros_trace<TraceMT, kTraceNT>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  // the cell's state as the product kernels lay it out, and behind it the 2*NW cells of the largest-term reduction (value, species per wave)
  constexpr int NW = kTraceNT / 64;
  constexpr size_t lds_bytes = (LdsLayout<TraceMT, kTraceNT>::TOTAL + 2 * NW) * sizeof(double);
  static_assert(lds_bytes <= 160 * 1024, "cell state and the trace's reduction cells do not fit the 160 KiB LDS of a gfx950 CU");
  auto kern = ros3_integrate_kernel<TraceMT, kTraceNT, 4>;
  if (!a.opt || !a.ntrace || a.trace_cap < 0 || (a.trace_cap > 0 && (!a.trace_d || !a.trace_i))) return hipErrorInvalidValue;
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kTraceNT), lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace mistra
