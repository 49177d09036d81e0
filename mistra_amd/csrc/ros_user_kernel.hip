// The kernels of one user mechanism slot per translation unit: ros3_integrate_kernel<UserMT, NT, VARIANT> for VARIANT 0 (product), 2 (first-step
// dump) and 3 (Rosenbrock_x's options, Ros3) on the slot's generated traits (user_mechs.hpp), with their launcher.  Compiled once per slot
// (mistra_amd/build.py: -DMISTRA_USER_SLOT=0|1).  A unit of its own for the reason the method kernels have theirs (ros_unit_kernel.hip): the
// product kernels' unit (ros3_kernel.hip) must compile as it does without the slots.  No phase-timing, method or trace instantiation: a user slot
// has none of those entries (capi.cpp refuses them).
#if !defined(MISTRA_USER_SLOT)
#error "build with -DMISTRA_USER_SLOT=<0 | 1> -DMISTRA_USER_MECHS=<slots>"
#endif
#define MISTRA_METHOD_TU 1
#include "ros3_kernel.hip"
#include "user_mechs.hpp"

namespace mistra {

#if MISTRA_USER_SLOT == 0
using UserMT = User0Traits;
constexpr int kUserNT = kUser0NT, kUserLdsTotal = kUser0LdsTotal, kUserLdsAB = kUser0LdsAB, kUserLdsJB = kUser0LdsJB;
#else
using UserMT = User1Traits;
constexpr int kUserNT = kUser1NT, kUserLdsTotal = kUser1LdsTotal, kUserLdsAB = kUser1LdsAB, kUserLdsJB = kUser1LdsJB;
#endif

// the generator sized and refused the table by its own restatement of LdsLayout: the two agree, or this unit does not compile
static_assert(LdsLayout<UserMT, kUserNT>::TOTAL == kUserLdsTotal && LdsLayout<UserMT, kUserNT>::AB == kUserLdsAB && LdsLayout<UserMT, kUserNT>::JB == kUserLdsJB,
              "user_traits_gen.cpp lays the cell out differently from LdsLayout (ros3_kernel.hpp)");
static_assert(UserMT::DENSE_ND == 0 && UserMT::DENSE_KB == 0, "a user slot runs without the dense tail block");
static_assert((kUserNT == 64 && UserMT::NVAR <= 128 && UserMT::RING_LOW) || (kUserNT == 256 && UserMT::NVAR > 128 && UserMT::NVAR <= 512 && !UserMT::RING_LOW),
              "size class of a user mechanism");

template <>
hipError_t launch_ros3<UserMT, kUserNT>(const KernelArgs& a, hipStream_t stream, bool* lds_configured) {
  constexpr size_t lds_bytes = LdsLayout<UserMT, kUserNT>::TOTAL * sizeof(double);
  auto kern = ros3_integrate_kernel<UserMT, kUserNT, 0>;
  auto kern_dump = ros3_integrate_kernel<UserMT, kUserNT, 2>;      // first-step dump (mistra_chem_debug_first_step)
  auto kern_opt = ros3_integrate_kernel<UserMT, kUserNT, 3>;       // Rosenbrock_x's options (mistra_chem_set_options, mistra_chem_rosenbrock_ex)
  if (a.prof) return hipErrorInvalidValue;                         // (never a quiet run without the timing)
  if (!*lds_configured) {
    for (const void* k : {reinterpret_cast<const void*>(kern), reinterpret_cast<const void*>(kern_dump), reinterpret_cast<const void*>(kern_opt)}) {
      hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) return e;
    }
    *lds_configured = true;
  }
  if (a.ncell <= 0) return hipSuccess;
  if (a.dump) hipLaunchKernelGGL(kern_dump, dim3((unsigned)a.ncell), dim3(kUserNT), lds_bytes, stream, a);
  else if (a.opt) hipLaunchKernelGGL(kern_opt, dim3((unsigned)a.ncell), dim3(kUserNT), lds_bytes, stream, a);
  else hipLaunchKernelGGL(kern, dim3((unsigned)a.ncell), dim3(kUserNT), lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace mistra
