// window_plan.h -- how wide the window kernel is launched (orbfe_window.hip, launch_window_match): lanes per query from the
// call's widest window, blocks from that.  Free of HIP so that a plain host program can exercise it
// (tests/cpp/window_plan_test.cpp, also under the address and undefined-behaviour sanitizers).
//
// k_window_match gives a query one lane per grid column of its window.  A window of radius r on cells of inverse width invW
// spans floor((x - r) * invW) .. ceil((x + r) * invW): at most 2 * r * invW + 3 columns (+3: floor / ceil slack).  Both callers
// pass that: the resident-frame search (run_search) for its frame and the call's largest radius, the host-array search
// (HostSearch::candidates) its largest value over the call's jobs, each job's largest radius counted from 0.
//
// The rule used to be written out at both places:
//     maxCols = cols >= 64 ? 64 : max(1, (int)ceil(cols));   lpq = 8;   while (lpq < 64 && lpq < maxCols) lpq <<= 1;
// per call in run_search; in candidates() the same clamp and ceil per job, folded into a running integer maximum that started
// at 1.  They agree with each other and with window_lanes() for every input:
//   * the loop gives 8 for maxCols <= 8, 16 for 9..16, 32 for 17..32, 64 above, and below 64 ceil(cols) <= k is cols <= k: the
//     class depends on cols alone -- 8 up to 8.0, 16 up to 16.0, 32 up to 32.0, 64 above (63.5, 64, 1e9, +inf);
//   * max(1, .) and the start at 1 only name the lowest class: every width up to 8, a negative one (rmax < 0) included, is 8;
//   * NaN (0 * inf: bounds so narrow that invW overflows) failed `cols >= 64`, became INT_MIN as an int and lost against the 1:
//     class 8, which `!(cols > 8)` says without the conversion; std::max(widest, NaN) likewise keeps widest;
//   * the class is monotone in cols, so the largest width selects what the largest clamped integer selected.
#pragma once
#include <cstddef>

namespace orbfe_match {

constexpr int kWinThreads = 256;   // a block of k_window_match: 4 waves, kWinThreads / LPQ queries

// lanes per query (the kernel's LPQ) for a call whose widest window spans `widestCols` grid columns
inline int window_lanes(float widestCols) {
  if (!(widestCols > 8.f)) return 8;   // NaN too
  return widestCols <= 16.f ? 16 : widestCols <= 32.f ? 32 : 64;
}
// blocks for nq queries at `lanes` lanes each
inline unsigned window_blocks(size_t nq, int lanes) { return (unsigned)((nq + kWinThreads / lanes - 1) / (kWinThreads / lanes)); }

}  // namespace orbfe_match
