// The texture kernels (pt_hip.h: pt_texture): pt::integrate_kernel_texture and its launcher, compiled from pt_kernels.hip -- the
// search, the shared integrator body, the dielectric kernels' set of instantiations and the waves-per-SIMD rules of the twins are all
// there -- as a translation unit of its own, the way pt_glass_kernels.hip is.  Every flavour of the library but the diagnostic ones
// (Makefile) builds this file with the flags of its pt_kernels object.
#define PT_SURFACE_UNIT 2
#include "pt_kernels.hip"
