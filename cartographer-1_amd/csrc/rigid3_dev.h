// Rigid3f on the device as the range-data front ends apply it
// (range_data2d.hip, range_data3d.hip): (t x y z, q w x y z), float and
// non-contracted (-ffp-contract=off), Eigen's coefficient order, so a moved
// point equals the reference's transform::Rigid3f * point bit for bit.
#ifndef CSM_RIGID3_DEV_H_
#define CSM_RIGID3_DEV_H_

#include <hip/hip_runtime.h>

namespace csm {

struct RdVec3 {
  float x, y, z;
};
struct RdRigid3 {
  float tx, ty, tz, qw, qx, qy, qz;
};

// Eigen MatrixBase::cross, coefficient order kept.
__host__ __device__ __forceinline__ RdVec3 RdCross(float ax, float ay, float az, const RdVec3& b) {
  return RdVec3{ay * b.z - az * b.y, az * b.x - ax * b.z, ax * b.y - ay * b.x};
}

// rigid_transform.h:190-196 with Eigen QuaternionBase::_transformVector:
// uv = 2 (q.vec x v); v + q.w uv + q.vec x uv; then the translation.
__host__ __device__ __forceinline__ RdVec3 RdApply(const RdRigid3& r, const RdVec3& v) {
  RdVec3 uv = RdCross(r.qx, r.qy, r.qz, v);
  uv.x += uv.x;
  uv.y += uv.y;
  uv.z += uv.z;
  const RdVec3 c = RdCross(r.qx, r.qy, r.qz, uv);
  const RdVec3 w{(v.x + r.qw * uv.x) + c.x, (v.y + r.qw * uv.y) + c.y, (v.z + r.qw * uv.z) + c.z};
  return RdVec3{w.x + r.tx, w.y + r.ty, w.z + r.tz};
}

__device__ __forceinline__ RdRigid3 RdLoadRigid(const float* __restrict__ p) {
  return RdRigid3{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}

}  // namespace csm

#endif  // CSM_RIGID3_DEV_H_
