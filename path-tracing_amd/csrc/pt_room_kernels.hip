// The room kernels (pt_scene.hpp: CullTables::room): pt::integrate_kernel<false, false, false, false, NARROW, 8>, compiled from
// pt_kernels.hip -- the search, the shared integrator body and the waves-per-SIMD rules are all there -- as a translation unit of its
// own, the way pt_environment_kernels.hip is.  Every flavour of the library (Makefile) builds this file with the flags of its
// pt_kernels object.
#define PT_ROOM_UNIT
#include "pt_kernels.hip"
