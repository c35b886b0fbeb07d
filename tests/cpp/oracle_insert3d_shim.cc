// Test infrastructure: C entry points over the oracle symbols the 3D insertion
// tests need and oracle_capi3d.cc does not expose (oracle/csm_oracle.h,
// oracle/oracle3d.h): LookupTableToApplyOdds, RotateHistogram, Apply3 /
// Inverse3 / CastF, NormF, and the yaw Submap3D::InsertData rotates the scan
// histogram by. Built by the tests against oracle/_build/liboracle.so.
#include <cmath>
#include <cstdint>
#include <vector>

#include "oracle3d.h"

using namespace oracle;

namespace {
Rigid3f Pose7f(const float* p) {
  return Rigid3f{Vec3f{p[0], p[1], p[2]}, Quatf{p[3], p[4], p[5], p[6]}};
}
void Out7f(const Rigid3f& r, float* out) {
  out[0] = r.t.x;
  out[1] = r.t.y;
  out[2] = r.t.z;
  out[3] = r.q.w;
  out[4] = r.q.x;
  out[5] = r.q.y;
  out[6] = r.q.z;
}
}  // namespace

extern "C" {

// ComputeLookupTableToApplyOdds(Odds(probability)).
void shim3_lookup_table(float probability, uint16_t* out32768) {
  const std::vector<uint16_t> t = LookupTableToApplyOdds(Odds(probability));
  for (int i = 0; i < 32768; ++i) out32768[i] = t[i];
}

void shim3_rotate_histogram(const float* histogram, int32_t size, float angle, float* out) {
  const std::vector<float> r =
      RotateHistogram(std::vector<float>(histogram, histogram + size), angle);
  for (int32_t i = 0; i < size; ++i) out[i] = r[i];
}

// Poses are (tx, ty, tz, qw, qx, qy, qz).
void shim3_apply(const float* pose7, const float* xyz, int64_t n, float* out) {
  const Rigid3f r = Pose7f(pose7);
  for (int64_t i = 0; i < n; ++i) {
    const Vec3f v = Apply3(r, Vec3f{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
    out[3 * i] = v.x;
    out[3 * i + 1] = v.y;
    out[3 * i + 2] = v.z;
  }
}

void shim3_inverse(const float* pose7, float* out7) { Out7f(Inverse3(Pose7f(pose7)), out7); }

// local_pose().inverse().cast<float>() (submap_3d.cc:330-331).
void shim3_cast_inverse(const double* p, float* out7) {
  const Rigid3d r{Vec3d{p[0], p[1], p[2]}, Quatd{p[3], p[4], p[5], p[6]}};
  Out7f(CastF(Inverse(r)), out7);
}

float shim3_norm(const float* v) { return NormF(Vec3f{v[0], v[1], v[2]}); }

// GetYaw(local_pose().inverse().rotation() * local_from_gravity_aligned) in
// double, cast to float (submap_3d.cc:341-342, transform.h:43-47).
float shim3_yaw_in_submap(const double* lq, const double* gq) {
  const Quatd q = QuatMul(QuatConjugate(Quatd{lq[0], lq[1], lq[2], lq[3]}),
                          Quatd{gq[0], gq[1], gq[2], gq[3]});
  const Vec3d d = Rotate(q, Vec3d{1., 0., 0.});
  return static_cast<float>(std::atan2(d.y, d.x));
}

}  // extern "C"
