// The user mechanism slots this library is built with (mistra_amd/build.py: MISTRA_USER_MECHS): 0, 1 or 2 generated traits headers, written
// into the build directory by user_traits_gen from the slots' tables.  Included by capi.cpp and ros_user_kernel.hip only: the product kernels'
// unit does not see it.
#pragma once
#include "ros3_kernel.hpp"

#ifndef MISTRA_USER_MECHS
#define MISTRA_USER_MECHS 0
#endif
#if MISTRA_USER_MECHS < 0 || MISTRA_USER_MECHS > 2
#error "there are two user mechanism slots"
#endif
#if MISTRA_USER_MECHS >= 1
#include "user_traits_0.hpp"
#endif
#if MISTRA_USER_MECHS >= 2
#include "user_traits_1.hpp"
#endif
