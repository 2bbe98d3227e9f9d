// The NeRF placement step (foldingdiff/nerf.py:145-204 place_dihedral) and its small fp64 vector helpers: the one
// device definition, shared by the structure builder (nerf.hip) and the pairwise-distance term of the denoising loss
// (loss_variants.hip), whose chains are nerf_build_batch's (nerf.py:207-292).
#pragma once
#include <hip/hip_runtime.h>

namespace fdmi {

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ D3 unit(D3 a) {
  const double n = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x / n, a.y / n, a.z / n};
}
// float32 sin / cos as numpy computes them on a float32 array (correctly rounded from the double result)
__device__ __forceinline__ float sin32(float v) { return (float)sin((double)v); }
__device__ __forceinline__ float cos32(float v) { return (float)cos((double)v); }

// nerf.py:145-204.  dtype follows numpy's promotion in the reference call: the torsion (and an angle /
// length that is a FEATURE) is a float32 array element, a python-float length is "weak" (stays float32
// against a float32 operand), but a DEFAULT bond angle is a python float whose cos / sin are float64 and
// pull the products to float64.
// the displacement of the new atom in the frame [bc | nbc | n] of the three atoms before it
__device__ __forceinline__ D3 place_local(bool angle_is_feature, float angle_f, double angle_default, bool length_is_feature,
                                          float length_f, double length_default, float torsion) {
  const float bl = length_is_feature ? length_f : (float)length_default;
  const float blc = bl * cos32(torsion), bls = bl * sin32(torsion);        // float32 in every case
  double d0, d1, d2;
  if (angle_is_feature) {
    const float ca = cos32(angle_f), sa = sin32(angle_f);
    d0 = (double)(-bl * ca);
    d1 = (double)(blc * sa);
    d2 = (double)(bls * sa);
  } else {
    const double ca = cos(angle_default), sa = sin(angle_default);
    d0 = -(length_is_feature ? (double)length_f : length_default) * ca;
    d1 = (double)blc * sa;
    d2 = (double)bls * sa;
  }
  return {d0, d1, d2};
}

__device__ __forceinline__ D3 place(D3 a, D3 b, D3 c, bool angle_is_feature, float angle_f, double angle_default,
                                    bool length_is_feature, float length_f, double length_default, float torsion) {
  const D3 ab = sub(b, a);
  const D3 bc = unit(sub(c, b));
  const D3 n = unit(cross(ab, bc));
  const D3 nbc = cross(n, bc);
  const D3 d = place_local(angle_is_feature, angle_f, angle_default, length_is_feature, length_f, length_default, torsion);
  const double d0 = d.x, d1 = d.y, d2 = d.z;
  // m = [bc | nbc | n] (columns);  d = m . (d0, d1, d2) + c
  return {bc.x * d0 + nbc.x * d1 + n.x * d2 + c.x, bc.y * d0 + nbc.y * d1 + n.y * d2 + c.y,
          bc.z * d0 + nbc.z * d1 + n.z * d2 + c.z};
}

}  // namespace fdmi
