// os1_amd/csrc/window_plan.h as a program of its own (no HIP, no GPU): lanes per query and blocks of the window kernel's launch
// at the edges of the four lane classes, for widths that are negative, not a number or infinite, and for query counts around a
// block.  The expected values are written out by hand from the two places the rule used to be spelled (run_search of
// orbfe_frame.hip, candidates() of the host-array search); both spellings are also kept below and swept against the header
// over the widths on which they are defined.  Built plainly and with -fsanitize=address,undefined by tests/test_window_plan.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "window_plan.h"

using namespace orbfe_match;

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

namespace {
int lanes_of(int maxCols) {
  int lpq = 8;
  while (lpq < 64 && lpq < maxCols) lpq <<= 1;
  return lpq;
}
// run_search, as it was: per call, from the call's largest radius.  Defined for widths whose ceiling fits an int.
int old_frame_lanes(float cols) {
  const int maxCols = cols >= 64.f ? 64 : std::max(1, (int)std::ceil(cols));
  return lanes_of(maxCols);
}
// candidates(), as it was: a running maximum over the jobs, from 1
int old_host_lanes(const std::vector<float>& jobCols) {
  int maxCols = 1;
  for (const float cols : jobCols) maxCols = std::max(maxCols, cols >= 64.f ? 64 : (int)std::ceil(cols));
  return lanes_of(maxCols);
}
// what candidates() passes now: the largest width over its jobs
float widest(const std::vector<float>& jobCols) {
  float w = 0.f;
  for (const float cols : jobCols) w = std::max(w, cols);
  return w;
}
unsigned old_blocks(int nq, int lpq) { return (unsigned)((nq + (kWinThreads / lpq) - 1) / (kWinThreads / lpq)); }
}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  auto above = [&](float v) { return std::nextafter(v, inf); };
  CHECK(kWinThreads == 256);
  // the class edges: the last width of a class and the first of the next
  CHECK(window_lanes(8.f) == 8 && window_lanes(above(8.f)) == 16);
  CHECK(window_lanes(16.f) == 16 && window_lanes(above(16.f)) == 32);
  CHECK(window_lanes(32.f) == 32 && window_lanes(above(32.f)) == 64);
  CHECK(window_lanes(63.5f) == 64 && window_lanes(64.f) == 64 && window_lanes(1e9f) == 64 && window_lanes(inf) == 64);
  // the narrowest a caller can pass (radius 0: 3 columns), nothing, and below: a negative width is what every query inactive
  // with rmax < 0 gives (max(1, negative) = 1); NaN failed `cols >= 64` and came out of the int conversion as INT_MIN, 1 again
  CHECK(window_lanes(3.f) == 8 && window_lanes(1.f) == 8 && window_lanes(0.f) == 8);
  CHECK(window_lanes(-17.f) == 8 && window_lanes(-1e30f) == 8 && window_lanes(-inf) == 8 && window_lanes(nan) == 8);
  // the radii of tests/test_gpu_window_lanes.py at invW = 0.1: 2 r / 10 + 3
  CHECK(window_lanes(2.f * 25.f * 0.1f + 3.f) == 8 && window_lanes(2.f * 25.5f * 0.1f + 3.f) == 16);
  CHECK(window_lanes(2.f * 65.f * 0.1f + 3.f) == 16 && window_lanes(2.f * 65.5f * 0.1f + 3.f) == 32);
  CHECK(window_lanes(2.f * 145.f * 0.1f + 3.f) == 32 && window_lanes(2.f * 145.5f * 0.1f + 3.f) == 64);
  CHECK(window_lanes(2.f * 400.f * 0.1f + 3.f) == 64);

  // blocks: 256 / lanes queries each -- 32, 16, 8, 4
  CHECK(window_blocks(1, 8) == 1 && window_blocks(31, 8) == 1 && window_blocks(32, 8) == 1 && window_blocks(33, 8) == 2);
  CHECK(window_blocks(1, 16) == 1 && window_blocks(31, 16) == 2 && window_blocks(32, 16) == 2 && window_blocks(33, 16) == 3);
  CHECK(window_blocks(1, 32) == 1 && window_blocks(31, 32) == 4 && window_blocks(32, 32) == 4 && window_blocks(33, 32) == 5);
  CHECK(window_blocks(1, 64) == 1 && window_blocks(31, 64) == 8 && window_blocks(32, 64) == 8 && window_blocks(33, 64) == 9);
  CHECK(window_blocks((1u << 20) - 2, 64) == 262144u && window_blocks((1u << 20) - 2, 8) == 32768u);   // the most run_search accepts

  // both old spellings against the header, every eighth of a column from -10 to 70 and the neighbours of every whole width
  int n = 0;
  for (int k = -80; k <= 560; k++) {
    const float c = 0.125f * (float)k;
    for (const float v : {c, above(c), std::nextafter(c, -inf)}) {
      CHECK(old_frame_lanes(v) == window_lanes(v));
      CHECK(old_host_lanes({v}) == window_lanes(widest({v})));
      n++;
    }
    for (const int nq : {1, 31, 32, 33, 1000, 10000}) CHECK(old_blocks(nq, window_lanes(c)) == window_blocks((size_t)nq, window_lanes(c)));
  }
  CHECK(n == 3 * 641);
  // several jobs: the class of the widest job, wherever it stands
  const std::vector<std::vector<float>> jobLists = {{3.f, 8.f}, {8.f, 8.5f, 3.f}, {16.f, 3.f, 16.f}, {3.f, 33.f, 9.f}, {70.f, 3.f}, {5.f, 17.f, 64.f}, {}};
  const int classes[7] = {8, 16, 16, 64, 64, 64, 8};
  for (size_t i = 0; i < jobLists.size(); i++) {
    CHECK(old_host_lanes(jobLists[i]) == classes[i]);
    CHECK(window_lanes(widest(jobLists[i])) == classes[i]);
  }
  // a job whose width is not a number counted for nothing (INT_MIN against the running maximum): the others decide
  CHECK(window_lanes(widest({nan, 20.f})) == 32 && window_lanes(widest({20.f, nan})) == 32 && window_lanes(widest({nan})) == 8);
  std::printf("PASS\n");
  return 0;
}
