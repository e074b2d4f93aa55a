/*
 * Device/GlibcLogf.h -- mcmcpp::glibc_logf(float) for host Calculators.
 *
 * An fp32 Calculator that takes a logarithm has a host side (this include path) and a device functor (a plug-in built
 * against mcmcpp_amd/csrc/mcmcpp_hip_plugin.hpp).  The host's logf and the device's are different functions and differ in
 * the last place on about half of all arguments, so such a Calculator's two sides would not agree bit for bit.
 * mcmcpp::glibc_logf is one function for both: the bits of the logf of glibc 2.28 - 2.40 on positive normal floats
 * (checked on every float in [2^-24, 4]), with no libm call.  The sampler's own fp32 logarithms are this function.
 *
 * One text, two include paths: the definition is the kernels' own header.
 */
#ifndef MCMCPP_DEVICE_GLIBC_LOGF_H
#define MCMCPP_DEVICE_GLIBC_LOGF_H

#include "../../../mcmcpp_amd/csrc/glibc_logf.hpp"

#endif
