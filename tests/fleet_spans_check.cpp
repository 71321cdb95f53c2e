// Drives csrc/fleet_spans.hpp alone, on the CPU (tests/test_fleet_layer.py builds this with the address and undefined-
// behaviour sanitizers and runs it as a process):
//   fleet_spans_check                           spans == brute-force F for several radii; stops at the first wrong answer
//   fleet_spans_check r_bnd r_col r_max body    prints the cells of F "dx dy", one per line, expanded from the spans
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../ergodic_exploration_amd/csrc/fleet_spans.hpp"

using namespace eea;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (r_bnd %d r_col %d r_max %d body %d)\n", __FILE__, __LINE__, #cond, g_case[0], \
                   g_case[1], g_case[2], g_case[3]);                         \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace
{
int g_case[4];

// F = { o + d : o in S, d.d <= body^2 } cell by cell
std::set<std::pair<int, int>> brute_force(int r_bnd, int r_col, int r_max, int body)
{
  std::set<std::pair<int, int>> f;
  for (const short2& o : ring_offsets(r_bnd, r_col, r_max)) {
    for (int dy = -body; dy <= body; ++dy) {
      for (int dx = -body; dx <= body; ++dx) {
        if (dx * dx + dy * dy <= body * body) f.emplace(o.x + dx, o.y + dy);
      }
    }
  }
  return f;
}

void one_case(int r_bnd, int r_col, int r_max, int body)
{
  g_case[0] = r_bnd, g_case[1] = r_col, g_case[2] = r_max, g_case[3] = body;
  const FleetSpans t = fleet_spans(r_bnd, r_col, r_max, body);
  const std::set<std::pair<int, int>> f = brute_force(r_bnd, r_col, r_max, body);
  const int R = r_col + body;
  CHECK(t.reach == R);
  CHECK(static_cast<int>(t.row_start.size()) == 2 * R + 2);
  CHECK(t.row_start.front() == 0 && t.row_start.back() == static_cast<int>(t.spans.size()));
  CHECK(t.cells == f.size());
  // the rows in order, every span inside the reach, sorted, maximal (a gap of at least one cell between neighbours)
  for (int row = 0; row <= 2 * R; ++row) {
    CHECK(t.row_start[row] <= t.row_start[row + 1]);
    for (int k = t.row_start[row]; k < t.row_start[row + 1]; ++k) {
      const FleetSpan& s = t.spans[k];
      CHECK(s.dy == row - R && s.x0 <= s.x1 && s.x0 >= -R && s.x1 <= R);
      CHECK(k == t.row_start[row] || t.spans[k - 1].x1 + 1 < s.x0);
    }
  }
  // membership == brute force on a window two cells wider than the reach, and F = -F
  int max_x = -1, max_y = -1;
  for (int dy = -R - 2; dy <= R + 2; ++dy) {
    for (int dx = -R - 2; dx <= R + 2; ++dx) {
      const bool in = f.count({ dx, dy }) != 0;
      CHECK(t.contains(dx, dy) == in);
      CHECK(t.contains(-dx, -dy) == in);
      if (in) {
        if (dx > max_x) max_x = dx;
        if (dy > max_y) max_y = dy;
      }
    }
  }
  // the reach is R' whenever the ring of radius r_col is walked: its point (r_col, 0) carries the disc's (body, 0)
  // (the ring of radius 0 visits no cell)
  if (r_col >= 1 && r_bnd <= r_col && r_col <= r_max) CHECK(max_x == R && max_y == R);
  CHECK(max_x <= R && max_y <= R);
  if (body == 0) CHECK(f.size() == ring_offsets(r_bnd, r_col, r_max).size());
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc == 5) {
    const FleetSpans t = fleet_spans(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
    for (const FleetSpan& s : t.spans) {
      for (int x = s.x0; x <= s.x1; ++x) std::printf("%d %d\n", x, s.dy);
    }
    return 0;
  }
  const int cases[][4] = {
    { 4, 6, 8, 4 },      // the small robots of the GPU tests: (0.2, 0.4, 0.1) at 0.05
    { 4, 6, 8, 0 },      // a robot of one cell: F = S, a hollow ring
    { 4, 6, 8, 2 },      // a body smaller than the hollow
    { 4, 6, 8, 9 },      // a body larger than r_col
    { 0, 2, 3, 0 },      // r_bnd = 0: the ring of radius 0 is empty (the walk starts at x = 0)
    { 0, 2, 3, 1 },
    { 0, 0, 0, 3 },      // S empty: F empty, no span
    { 1, 1, 1, 0 },
    { 3, 3, 7, 5 },      // r_col = r_bnd
    { 5, 9, 7, 3 },      // r_col beyond r_max: the reach is not attained
    { 14, 18, 20, 14 },  // the demo robot at 0.05
    { 14, 18, 20, 0 },
    { 7, 9, 10, 7 },
  };
  for (const auto& c : cases) one_case(c[0], c[1], c[2], c[3]);
  std::printf("fleet spans: ok\n");
  return 0;
}
