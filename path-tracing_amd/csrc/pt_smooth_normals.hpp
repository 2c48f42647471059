// The normal generator of pt_smooth_normals (pt_smooth_normals.cpp).  Host only.
#pragma once
#include <cstdint>

namespace pt {

// out[9 * n_tri]: a unit normal per corner, zeros for the corners of a degenerate triangle.  vertices: 9 floats per triangle.
// crease_degrees in [0, 180]: faces at one vertex whose normals' cosine is >= cos(crease) are smoothed together.
void smooth_normals(int32_t n_tri, const float *vertices, double crease_degrees, float *out);

}  // namespace pt
