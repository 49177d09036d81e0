// One series kernel per translation unit: ros3_integrate_kernel<MT, NT, 5, METHOD> — the options kernel of one of the five methods on one mechanism
// with the loop over the legs of a series (kernel_args.hpp: times, nleg) — with its launcher.  Compiled fifteen times (mistra_amd/build.py:
// -DMISTRA_SERIES_MECH=0|1|2 -DMISTRA_SERIES_METHOD=1..5).  Units of their own for the reason ros_method_kernel.hip gives: the non-inlined device
// functions the kernels share are compiled once per unit, under the register budget of all kernels in it, and no existing unit may compile differently.
#if !defined(MISTRA_SERIES_MECH) || !defined(MISTRA_SERIES_METHOD)
#error "build with -DMISTRA_SERIES_MECH=<0 gas | 1 aer | 2 tot> -DMISTRA_SERIES_METHOD=<1 Ros2 | 2 Ros3 | 3 Ros4 | 4 Rodas3 | 5 Rodas4>"
#endif
#define MISTRA_METHOD_TU 1
#include "ros3_kernel.hip"

namespace mistra {

#if MISTRA_SERIES_MECH == 0
using SeriesMT = GasTraits;
constexpr int kSeriesNT = kGasNT;
#elif MISTRA_SERIES_MECH == 1
using SeriesMT = AerTraits;
constexpr int kSeriesNT = kAerNT;
#else
using SeriesMT = TotTraits;
constexpr int kSeriesNT = kTotNT;
#endif

template <>
hipError_t launch_ros_series<SeriesMT, kSeriesNT, MISTRA_SERIES_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  static_assert(MISTRA_SERIES_METHOD >= kRos2 && MISTRA_SERIES_METHOD <= kRodas4, "IPAR(4) resolved: 1 .. 5");
  constexpr size_t lds_bytes = LdsLayout<SeriesMT, kSeriesNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<SeriesMT, kSeriesNT, 5, MISTRA_SERIES_METHOD>;
  if (!a.opt || !a.times || a.nleg < 1) return hipErrorInvalidValue;      // the series kernels are options instantiations
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kSeriesNT), lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace mistra
