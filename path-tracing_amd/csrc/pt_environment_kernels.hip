// The environment kernels (pt_hip.h: pt_environment_*): pt::integrate_kernel_environment and its launcher, compiled from
// pt_kernels.hip -- the search, the shared integrator body and the waves-per-SIMD rules of the skybox twins are all there -- as a
// translation unit of its own.  Every flavour of the library (Makefile) builds this file with the flags of its pt_kernels object.
#define PT_ENVIRONMENT_UNIT
#include "pt_kernels.hip"
