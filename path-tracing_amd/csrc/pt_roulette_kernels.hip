// The roulette kernels (pt_hip.h: Russian roulette): pt::integrate_kernel_roulette and its launcher, compiled from pt_kernels.hip -- the
// search, the shared integrator body, the direct and the environment-sampling kernels' sets of instantiations and the waves-per-SIMD
// rules of the twins are all there -- as a translation unit of its own, the way pt_direct_kernels.hip is.  Every flavour of the library
// but the diagnostic ones (Makefile) builds this file with the flags of its pt_kernels object.
#define PT_SURFACE_UNIT 7
#include "pt_kernels.hip"
