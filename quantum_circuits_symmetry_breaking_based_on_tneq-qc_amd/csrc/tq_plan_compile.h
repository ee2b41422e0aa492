// Compile-time types the plan compiler's three units share (tq_plan.cpp lowers a path into ops
// and sweep chains, tq_sweep2_layout.cpp lays a chain out, tq_plan_finish.cpp finishes the
// lowered plan).  Nothing here survives into a Plan.
#pragma once
#include "tq_plan.h"

#include <vector>

namespace tq {

constexpr int64_t kAlign = 256;   // arena buffers, table blobs

inline std::vector<int64_t> contig_strides(const std::vector<int64_t>& ext) {
  std::vector<int64_t> s(ext.size());
  int64_t p = 1;
  for (int d = (int)ext.size() - 1; d >= 0; --d) { s[d] = p; p *= ext[d]; }
  return s;
}

struct Live {
  std::vector<int> modes;
  std::vector<int64_t> ext;
  std::vector<int64_t> stride;
  BufRef buf;
  bool owned = false;  // arena intermediate that must be freed after use
  bool dep = false;    // depends on a sliced input (otherwise computed once per execute)
  bool vol = true;     // depends on a sliced or a volatile input (otherwise frozen: Plan::frozen_valid)
  int64_t numel() const { return prod(ext); }
  bool contiguous() const {
    auto cs = contig_strides(ext);
    for (size_t d = 0; d < ext.size(); ++d)
      if (ext[d] != 1 && stride[d] != cs[d]) return false;
    return true;
  }
  int pos(int m) const {
    for (size_t i = 0; i < modes.size(); ++i) if (modes[i] == m) return (int)i;
    return -1;
  }
};

// ---- APPLY lowering: big operand S = [O][K1][M][K2][I] (contracted modes in <= 2 runs),
// small operand G[K][N] read through a gather table, C = [O][N][M][I]
struct ApplyDesc {
  bool a_big = true;
  std::vector<int> korder, nfree, order;
  int64_t O = 1, K1 = 1, M = 1, K2 = 1, I = 1, K = 1, N = 1;
  std::vector<int32_t> gtab;   // empty: small operand already contiguous in [K][N] order
};

// ---- sweep chains: consecutive APPLY steps on one tensor
struct Chain {
  struct Gate {
    Live Sm;
    bool release = true;
    int step = -1;
    ApplyDesc d;
  };
  bool active = false;
  bool dep = false;
  bool vol = true;      // Live::vol of its steps (a chain does not cross a tier)
  int br = 0;           // branch of its steps
  int id = -1;          // SSA id of the (pending) chain result
  int flushed_id = -1;
  Live X0;
  bool release_X0 = true;
  std::vector<Gate> gates;
  std::vector<int> out_modes;
};
struct ChainShape {
  bool s2 = false;      // fits the in-place butterfly sweep (tq_sweep2.hip)
  std::vector<int> tin, tout, outer;
  std::vector<std::vector<int>> W;   // working-set mode lists after each gate (W[q-1] = tout)
  int64_t tin_n = 1, tout_n = 1, wmax = 1;
};

// what happens to a lowered plan (tq_plan_finish.cpp): arena bases from the four arena peaks
// (ordinary regions 0 / 1, pinned regions 0 / 1), slice lanes, operand-max words, table layout,
// counters, launch schedule, the describe text
void plan_finish(Plan& P, const int64_t arena_peak[2], const int64_t pinned_peak[2]);

}  // namespace tq
