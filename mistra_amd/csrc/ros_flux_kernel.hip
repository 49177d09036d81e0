// One flux kernel per translation unit: ros3_integrate_kernel<MT, NT, 6, METHOD> — the options kernel of one of the five methods on one mechanism that
// also integrates every reaction's rate over the call (kernel_args.hpp: flux) — with its launcher.  Compiled fifteen times (mistra_amd/build.py:
// -DMISTRA_FLUX_MECH=0|1|2 -DMISTRA_FLUX_METHOD=1..5).  Units of their own for the reason ros_method_kernel.hip gives: the non-inlined device
// functions the kernels share are compiled once per unit, under the register budget of all kernels in it, and no existing unit may compile differently.
#if !defined(MISTRA_FLUX_MECH) || !defined(MISTRA_FLUX_METHOD)
#error "build with -DMISTRA_FLUX_MECH=<0 gas | 1 aer | 2 tot> -DMISTRA_FLUX_METHOD=<1 Ros2 | 2 Ros3 | 3 Ros4 | 4 Rodas3 | 5 Rodas4>"
#endif
#define MISTRA_METHOD_TU 1
#include "ros3_kernel.hip"

namespace mistra {

#if MISTRA_FLUX_MECH == 0
using FluxMT = GasTraits;
constexpr int kFluxNT = kGasNT;
#elif MISTRA_FLUX_MECH == 1
using FluxMT = AerTraits;
constexpr int kFluxNT = kAerNT;
#else
using FluxMT = TotTraits;
constexpr int kFluxNT = kTotNT;
#endif

template <>
hipError_t launch_ros_flux<FluxMT, kFluxNT, MISTRA_FLUX_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  static_assert(MISTRA_FLUX_METHOD >= kRos2 && MISTRA_FLUX_METHOD <= kRodas4, "IPAR(4) resolved: 1 .. 5");
  constexpr size_t lds_bytes = LdsLayout<FluxMT, kFluxNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<FluxMT, kFluxNT, 6, MISTRA_FLUX_METHOD>;
  if (!a.opt || !a.flux) return hipErrorInvalidValue;      // the flux kernels are options instantiations
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kFluxNT), lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace mistra
