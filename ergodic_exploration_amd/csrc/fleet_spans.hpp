// Host-side table of the fleet layer (fleet_layer_kernel.hip): the offset set F at which one robot is an obstacle to
// another, as row spans.  Plain C++: no HIP call, no global state -- tests/fleet_spans_check.cpp drives this file alone.
//
// S = ring_offsets(r_bnd, r_col, r_max) is where collisionCheck can see an occupied cell (hit_map_table.hpp); a robot's body
// is the disc D = { d : d.d <= body^2 } of cells around its cell.  A centre c sees the body of the robot at cell p iff
// c + o = p + d for some o in S, d in D, i.e. c - p in D - S = S + D =: F (S is closed under 90-degree rotations and so is D:
// S = -S, D = -D, F = -F).  |o| <= r_col and |d| <= body: F lies within the reach R' = r_col + body.
//
// Row spans: for each dy in [-R', R'] the sorted maximal x-intervals [x0, x1] of F.  One table serves both uses --
//   the stamp:       +1 at p + (x0, dy), -1 behind p + (x1, dy) in a difference map, then a prefix sum along every row;
//   the membership:  (c - own) in F, to take a robot's own body out of the count it reads.
#pragma once

#include <set>
#include <utility>
#include <vector>

#include "hit_map_table.hpp"  // ring_offsets

namespace eea
{
struct FleetSpan
{
  short x0, x1, dy, pad;  // the cells (x0..x1, dy) of F, x0 <= x1; 8 bytes
};

struct FleetSpans
{
  int reach = 0;               // R' = r_col + body
  std::vector<int> row_start;  // [2 R' + 2]: the spans of row dy are spans[row_start[dy + R']] .. spans[row_start[dy + R' + 1] - 1]
  std::vector<FleetSpan> spans;
  size_t cells = 0;            // |F|

  bool contains(int dx, int dy) const
  {
    if (dy < -reach || dy > reach) return false;
    for (int k = row_start[dy + reach]; k < row_start[dy + reach + 1]; ++k) {
      if (spans[k].x0 <= dx && dx <= spans[k].x1) return true;
    }
    return false;
  }
};

// body >= 0; the caller keeps r_col + body within a short (eea_fleet_layer_create: <= 127)
inline FleetSpans fleet_spans(int r_bnd, int r_col, int r_max, int body)
{
  FleetSpans f;
  f.reach = (r_col > 0 ? r_col : 0) + body;
  const int R = f.reach;
  // the disc as one half-width per row
  std::vector<int> half(2 * body + 1, -1);
  for (int dy = -body; dy <= body; ++dy) {
    int hw = 0;
    while ((hw + 1) * (hw + 1) + dy * dy <= body * body) ++hw;
    half[dy + body] = hw;
  }
  // F row by row: every o in S widens row o.y + dy by [o.x - hw, o.x + hw]
  std::vector<std::set<std::pair<int, int>>> rows(2 * R + 1);
  for (const short2& o : ring_offsets(r_bnd, r_col, r_max)) {
    for (int dy = -body; dy <= body; ++dy) {
      const int hw = half[dy + body];
      rows[o.y + dy + R].emplace(o.x - hw, o.x + hw);
    }
  }
  f.row_start.assign(2 * R + 2, 0);
  for (int row = 0; row <= 2 * R; ++row) {
    f.row_start[row] = static_cast<int>(f.spans.size());
    bool open = false;
    int x0 = 0, x1 = 0;
    for (const auto& iv : rows[row]) {  // sorted by start: merge what overlaps or touches
      if (open && iv.first <= x1 + 1) {
        if (iv.second > x1) x1 = iv.second;
        continue;
      }
      if (open) f.spans.push_back(FleetSpan{ static_cast<short>(x0), static_cast<short>(x1), static_cast<short>(row - R), 0 });
      open = true;
      x0 = iv.first;
      x1 = iv.second;
    }
    if (open) f.spans.push_back(FleetSpan{ static_cast<short>(x0), static_cast<short>(x1), static_cast<short>(row - R), 0 });
  }
  f.row_start[2 * R + 1] = static_cast<int>(f.spans.size());
  for (const FleetSpan& s : f.spans) f.cells += static_cast<size_t>(s.x1 - s.x0 + 1);
  return f;
}
}  // namespace eea
