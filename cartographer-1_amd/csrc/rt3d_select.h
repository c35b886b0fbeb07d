// Which RTCSM3D kernel (kernels3d.hip) scores a match: one pure function of
// the probability brick's dimensions, the padding P the rotation-lane kernels
// need (the translation lattice's reach in cells + 2), the lattice's steps
// per axis nl = 2L + 1, and the best kernel allowed. Plain C++ so that a
// stand-alone program can check it (tests/cpp/rt3d_select_test.cc).
#ifndef CSM_RT3D_SELECT_H_
#define CSM_RT3D_SELECT_H_

#include <algorithm>
#include <cstdint>

namespace csm {

// In ascending order of preference: each kernel is the only one for some
// input.
enum class Rt3dKernel : int {
  kPlain = 0,     // rt3d_score: the unpadded brick, any size; no scoring mode
  kPadded = 1,    // rt3d_score2: the brick padded by one cell
  kRotLanes = 2,  // rt3d_score4: the brick padded by P cells, lanes = rotations
  kColumns = 3,   // rt3d_score5: the same brick z fastest, one wave per z column
};

// `cap` is the best kernel the caller allows (kColumns: no restriction).
inline Rt3dKernel SelectRt3dKernel(int nx, int ny, int nz, int P, int nl, Rt3dKernel cap) {
  auto cells = [&](int pad) {
    return (int64_t{nx} + 2 * pad) * (int64_t{ny} + 2 * pad) * (int64_t{nz} + 2 * pad);
  };
  Rt3dKernel k = Rt3dKernel::kPlain;
  // rt3d_score2 addresses the padded brick with 24-bit row products and a
  // 32-bit byte offset.
  if (cells(1) < (int64_t{1} << 29) && (int64_t{ny} + 2) * (int64_t{nz} + 2) < (int64_t{1} << 24)) {
    k = Rt3dKernel::kPadded;
    // The rotation-lane kernels compute byte offsets into the brick padded by
    // P in float: exact below 2^24.
    if (4 * cells(P) < (int64_t{1} << 24)) {
      k = Rt3dKernel::kRotLanes;
      // One wave per z column of 3 to 15 steps; 1 step and wider windows
      // run rt3d_score4.
      if (nl >= 3 && nl <= 15) k = Rt3dKernel::kColumns;
    }
  }
  return std::min(k, cap);
}

}  // namespace csm

#endif  // CSM_RT3D_SELECT_H_
