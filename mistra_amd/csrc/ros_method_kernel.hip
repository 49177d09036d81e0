// One method kernel per translation unit: ros3_integrate_kernel<MT, NT, 3, METHOD> for Ros2, Ros4, Rodas3 or Rodas4 on one mechanism, with
// its launcher.  Compiled twelve times (mistra_amd/build.py: -DMISTRA_METHOD_MECH=0|1|2 -DMISTRA_METHOD=1|3|4|5).  Units of their own because
// the non-inlined device functions the kernels share (vm_run, gsum_run*, tail_solve, scale_run, dense_lu, dense_finish) are compiled once per
// unit, under the register budget of all kernels in it: the product kernels' unit (ros3_kernel.hip) must compile as it did without these.
#if !defined(MISTRA_METHOD_MECH) || !defined(MISTRA_METHOD)
#error "build with -DMISTRA_METHOD_MECH=<0 gas | 1 aer | 2 tot> -DMISTRA_METHOD=<1 Ros2 | 3 Ros4 | 4 Rodas3 | 5 Rodas4>"
#endif
#define MISTRA_METHOD_TU 1
#include "ros3_kernel.hip"

namespace mistra {

#if MISTRA_METHOD_MECH == 0
using MethodMT = GasTraits;
constexpr int kMethodNT = kGasNT;
#elif MISTRA_METHOD_MECH == 1
using MethodMT = AerTraits;
constexpr int kMethodNT = kAerNT;
#else
using MethodMT = TotTraits;
constexpr int kMethodNT = kTotNT;
#endif

template <>
hipError_t launch_ros_method<MethodMT, kMethodNT, MISTRA_METHOD>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  static_assert(MISTRA_METHOD != kRos3, "Ros3 with options is the product unit's VARIANT 3 kernel");
  constexpr size_t lds_bytes = LdsLayout<MethodMT, kMethodNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<MethodMT, kMethodNT, 3, MISTRA_METHOD>;
  if (!a.opt) return hipErrorInvalidValue;      // the method kernels are options instantiations
  if (!*lds_configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kMethodNT), lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace mistra
