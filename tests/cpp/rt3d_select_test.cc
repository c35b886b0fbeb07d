// Which RTCSM3D kernel scores a match (rt3d_select.h SelectRt3dKernel): the
// thresholds between the four kernels, each case derived from them, with
// every dimension product taken in 64-bit. Built with
// -fsanitize=address,undefined (tests/test_rt3d_select.py).
#include <cstdint>
#include <cstdio>

#include "../../cartographer-1_amd/csrc/rt3d_select.h"

namespace {

using csm::Rt3dKernel;
using csm::SelectRt3dKernel;

int failures = 0;

const char* Name(Rt3dKernel k) {
  switch (k) {
    case Rt3dKernel::kPlain: return "plain";
    case Rt3dKernel::kPadded: return "padded";
    case Rt3dKernel::kRotLanes: return "rotation lanes";
    case Rt3dKernel::kColumns: return "columns";
  }
  return "?";
}

void Expect(int nx, int ny, int nz, int P, int nl, Rt3dKernel cap, Rt3dKernel want) {
  const Rt3dKernel got = SelectRt3dKernel(nx, ny, nz, P, nl, cap);
  if (got == want) return;
  std::printf("FAIL %d x %d x %d, P %d, nl %d, cap %s: %s, expected %s\n", nx, ny, nz, P, nl,
              Name(cap), Name(got), Name(want));
  ++failures;
}

int64_t Cells(int64_t nx, int64_t ny, int64_t nz, int64_t pad) {
  return (nx + 2 * pad) * (ny + 2 * pad) * (nz + 2 * pad);
}

}  // namespace

int main() {
  const Rt3dKernel kAny = Rt3dKernel::kColumns;
  constexpr int64_t k22 = int64_t{1} << 22, k24 = int64_t{1} << 24, k29 = int64_t{1} << 29;
  // A small brick: columns for 3 to 15 steps, rotation lanes for 1 and 17.
  Expect(100, 100, 20, 5, 7, kAny, Rt3dKernel::kColumns);
  Expect(100, 100, 20, 5, 3, kAny, Rt3dKernel::kColumns);
  Expect(100, 100, 20, 5, 15, kAny, Rt3dKernel::kColumns);
  Expect(100, 100, 20, 5, 1, kAny, Rt3dKernel::kRotLanes);
  Expect(100, 100, 20, 5, 17, kAny, Rt3dKernel::kRotLanes);
  // 4 bytes x cells padded by P against 2^24: 128 x 128 x 255 is the last
  // brick under it, 128 x 128 x 256 = 2^22 cells the first one at it.
  if (!(Cells(124, 124, 251, 2) < k22 && Cells(124, 124, 252, 2) == k22)) {
    std::printf("FAIL: the 2^22 boundary cases are not at the boundary\n");
    ++failures;
  }
  Expect(124, 124, 251, 2, 7, kAny, Rt3dKernel::kColumns);
  Expect(124, 124, 252, 2, 7, kAny, Rt3dKernel::kPadded);
  // The retired v3 kernel's band, (n + 2)^3 < 2^22 <= (n + 2 P)^3: padded.
  if (!(Cells(159, 159, 159, 1) < k22 && Cells(159, 159, 159, 2) >= k22)) {
    std::printf("FAIL: 159^3 is not in the retired band\n");
    ++failures;
  }
  Expect(159, 159, 159, 2, 5, kAny, Rt3dKernel::kPadded);
  Expect(159, 159, 159, 5, 7, kAny, Rt3dKernel::kPadded);
  Expect(160, 160, 160, 5, 7, kAny, Rt3dKernel::kPadded);
  // Past the padded kernel's addressing: a (ny + 2)(nz + 2) row product at
  // 2^24 or over, or 2^29 padded cells or more.
  if (!(int64_t{4097} * 4097 >= k24 && Cells(2, 4095, 4095, 1) < k29 &&
        Cells(1000, 1000, 600, 1) >= k29 && int64_t{1002} * 602 < k24)) {
    std::printf("FAIL: the plain cases do not isolate one condition each\n");
    ++failures;
  }
  Expect(2, 4095, 4095, 2, 5, kAny, Rt3dKernel::kPlain);
  Expect(1000, 1000, 600, 2, 5, kAny, Rt3dKernel::kPlain);
  // Products past 32 bits (2^11 x 2^11 x 2^11 = 2^33 cells) stay plain.
  Expect(2046, 2046, 2046, 2, 5, kAny, Rt3dKernel::kPlain);
  // Each cap demotes the small brick in turn, and never promotes.
  Expect(100, 100, 20, 5, 7, Rt3dKernel::kRotLanes, Rt3dKernel::kRotLanes);
  Expect(100, 100, 20, 5, 7, Rt3dKernel::kPadded, Rt3dKernel::kPadded);
  Expect(100, 100, 20, 5, 7, Rt3dKernel::kPlain, Rt3dKernel::kPlain);
  Expect(100, 100, 20, 5, 17, Rt3dKernel::kColumns, Rt3dKernel::kRotLanes);
  Expect(159, 159, 159, 2, 5, Rt3dKernel::kRotLanes, Rt3dKernel::kPadded);
  Expect(1000, 1000, 600, 2, 5, Rt3dKernel::kPadded, Rt3dKernel::kPlain);
  if (failures) return 1;
  std::printf("rt3d select OK\n");
  return 0;
}
