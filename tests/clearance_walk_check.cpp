// Drives clearance_walk() of csrc/hit_map_table.hpp alone, on the CPU (tests/test_clearance.py builds this with the address
// and undefined-behaviour sanitizers and runs it as a process):
//   clearance_walk_check                  the checks below; stops at the first wrong answer and names the line
//   clearance_walk_check r_bnd r_max      prints the walk's offsets "dx dy" in visit order, one per line ("refused" if the key
//                                         does not fit)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../ergodic_exploration_amd/csrc/hit_map_table.hpp"

using namespace eea;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

namespace
{
struct Set
{
  double resolution, boundary, search, obstacle;
  size_t n_off;  // what the walk of this set visits (counted with the oracle's own search)
};
// the parameter sets of tests/test_gpu_collision_parity.py and one with a long walk
const Set kSets[] = { { 0.05, 0.7, 1.0, 0.2, 744 }, { 0.25, 0.7, 1.0, 0.2, 48 }, { 0.1, 0.3, 0.6, 0.1, 76 },
                      { 0.1, 0.0, 0.5, 0.3, 80 },   { 0.1, 0.4, 0.4, 0.5, 20 },  { 0.1, 0.2, 1.2, 0.1, 360 } };

void one_set(int r_bnd, int r_col, int r_max, size_t n_off)
{
  ClearanceWalk w;
  CHECK(clearance_walk(r_bnd, r_max, w));
  CHECK(w.offsets.size() == n_off && n_off % 4 == 0);
  // the offsets within r_col, as a set, are the dilation of the inflated map
  std::set<std::pair<int, int>> near;
  unsigned long long largest_key = 0;
  int reach = 0;
  unsigned max_sq = 0;
  for (size_t k = 0; k < w.offsets.size(); ++k) {
    const int dx = w.offsets[k].x, dy = w.offsets[k].y;
    const unsigned sq = static_cast<unsigned>(dx * dx + dy * dy);
    if (static_cast<int>(sq) <= r_col * r_col) near.emplace(dx, dy);
    const unsigned long long key = static_cast<unsigned long long>(sq) * w.offsets.size() + k;
    if (key > largest_key) largest_key = key;
    if (std::abs(dx) > reach) reach = std::abs(dx);
    if (std::abs(dy) > reach) reach = std::abs(dy);
    if (sq > max_sq) max_sq = sq;
  }
  std::set<std::pair<int, int>> dilation;
  for (const short2& d : ring_offsets(r_bnd, r_col, r_max)) dilation.emplace(d.x, d.y);
  CHECK(near == dilation);
  CHECK(reach == w.reach && max_sq == w.max_sq && reach <= r_max);
  CHECK(largest_key < kNoClearanceKey);  // every key is a key, none is "no cell"
  // the walk is the rings' walks one after the other, and every ring starts at (r, 0): Q1 of its first step
  std::vector<short2> joined;
  for (int r = r_bnd; r <= r_max; ++r) {
    ClearanceWalk ring;
    CHECK(clearance_walk(r, r, ring));
    if (r <= 0) {
      CHECK(ring.offsets.empty());
      continue;
    }
    CHECK(ring.offsets.size() >= 4u * static_cast<unsigned>(r));
    CHECK(ring.offsets[0].x == r && ring.offsets[0].y == 0);
    CHECK(ring.offsets[1].x == 0 && ring.offsets[1].y == r);    // Q2, Q3, Q4 of that step
    CHECK(ring.offsets[2].x == -r && ring.offsets[2].y == 0);
    CHECK(ring.offsets[3].x == 0 && ring.offsets[3].y == -r);
    joined.insert(joined.end(), ring.offsets.begin(), ring.offsets.end());
  }
  CHECK(joined.size() == w.offsets.size());
  for (size_t k = 0; k < joined.size(); ++k) CHECK(joined[k].x == w.offsets[k].x && joined[k].y == w.offsets[k].y);
}

// the two views of the one walk: the walk's offsets within r_col, as a set, are ring_offsets -- for every r_col up to r_max
// (both are filters over walk_rings: this catches a wrong filter, not a wrong walk -- the walk itself is held to the oracle's
// ring search by tests/test_hit_map_table.py and to the restatement's own enumeration by tests/test_clearance.py)
void views_of_one_walk()
{
  for (int r_bnd = 0; r_bnd <= 6; ++r_bnd) {
    for (int r_max = r_bnd; r_max <= 12; ++r_max) {
      ClearanceWalk w;
      CHECK(clearance_walk(r_bnd, r_max, w));
      for (int r_col = 0; r_col <= r_max; ++r_col) {
        std::set<std::pair<int, int>> near;
        for (const short2& d : w.offsets) {
          if (d.x * d.x + d.y * d.y <= r_col * r_col) near.emplace(d.x, d.y);
        }
        const std::vector<short2> ring = ring_offsets(r_bnd, r_col, r_max);
        std::set<std::pair<int, int>> dilation;
        for (const short2& d : ring) dilation.emplace(d.x, d.y);
        CHECK(dilation.size() == ring.size());  // each offset once
        CHECK(near == dilation);
        CHECK(near.empty() == (r_col < (r_bnd < 1 ? 1 : r_bnd)));  // (ring 0 visits nothing; ring r > 0 starts at (r, 0))
      }
    }
  }
}

void checks()
{
  views_of_one_walk();
  for (const Set& s : kSets) {
    // the radii in cells as csrc/entry_util.hpp derives them (collision.cpp:130-133)
    one_set(static_cast<int>(std::floor(s.boundary / s.resolution)), static_cast<int>(std::floor((s.boundary + s.obstacle) / s.resolution)),
            static_cast<int>(std::floor(s.search / s.resolution)), s.n_off);
  }
  ClearanceWalk w;
  CHECK(clearance_walk(0, 0, w) && w.offsets.empty() && w.reach == 0 && w.max_sq == 0);  // no ring: every answer is "none"
  CHECK(clearance_walk(-3, -1, w) && w.offsets.empty());
  CHECK(clearance_walk(5, 3, w) && w.offsets.empty());
  CHECK(clearance_walk(2000, 1500, w) && w.offsets.empty());  // (r_bnd > r_max: nothing to refuse)
  // the key bound: (max_sq + 1) * n <= 2^32 - 1
  CHECK(clearance_key_fits(0, 0) && clearance_key_fits(0xfffffffeull, 1) && !clearance_key_fits(0xffffffffull, 1));
  CHECK(clearance_key_fits(65534, 65537) && !clearance_key_fits(65535, 65537));  // 2^32 - 1 = 65535 * 65537
  CHECK(clearance_walk(0, 100, w) && clearance_key_fits(w.max_sq, w.offsets.size()));
  CHECK(clearance_walk(100, 100, w) && w.offsets[0].x == 100);
  // r_bnd = 0: the largest r_max whose key fits -- every smaller one fits, the next one does not
  int last = 0;
  while (clearance_walk(0, last + 1, w)) ++last;
  CHECK(last == 196);  // (109196 offsets up to |d|^2 = 196^2)
  for (int r = last + 1; r < last + 40; ++r) CHECK(!clearance_walk(0, r, w));
  CHECK(!clearance_walk(1023, 1023, w));  // one ring: ~5800 offsets of |d|^2 ~ 2^20
  CHECK(!clearance_walk(1024, 1024, w) && !clearance_walk(0, 1024, w) && !clearance_walk(-5, 2000000000, w));  // before any walk
  std::printf("clearance walk: ok\n");
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc == 3) {
    ClearanceWalk w;
    if (!clearance_walk(std::atoi(argv[1]), std::atoi(argv[2]), w)) {
      std::printf("refused\n");
      return 0;
    }
    for (const short2& d : w.offsets) std::printf("%d %d\n", d.x, d.y);
    return 0;
  }
  checks();
  return 0;
}
