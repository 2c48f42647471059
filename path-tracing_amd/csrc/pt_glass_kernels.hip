// The dielectric kernels (pt_hip.h: pt_dielectric): pt::integrate_kernel_glass and its launcher, compiled from pt_kernels.hip -- the
// search, the shared integrator body and the waves-per-SIMD rules of the twins are all there -- as a translation unit of its own, the
// way pt_environment_kernels.hip is.  Every flavour of the library but the diagnostic ones (Makefile) builds this file with the flags
// of its pt_kernels object.
#define PT_SURFACE_UNIT 1
#include "pt_kernels.hip"
