// Drives csrc/hit_map_table.hpp alone, on the CPU (tests/test_hit_map_table.py builds this with the address and undefined-
// behaviour sanitizers and runs it as a process):
//   hit_map_table_check                         the policy of the map buffers; stops at the first wrong answer
//   hit_map_table_check r_bnd r_col r_max       prints the dilation's offsets "dx dy", one per line
// Each case is what one test of tests/test_gpu_collision_state.py observes indirectly, through 4096 poses on a GPU.
#include <cstdio>
#include <cstdlib>
#include <set>
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
char g_memory[4096];  // addresses only: streams, grids and "device" buffers are never dereferenced
int g_next = 0;
void* fresh() { return &g_memory[g_next++]; }

const CollisionParams kParams{ -2.0, -1.0, 0.1, 80u, 60u, 6, 8, 10, 0.8 };

// one build as collision_kernel.hip performs it: the plan, its effects (a reallocation "allocates" a fresh address), the
// report -- unless the launch is said to have failed
HitMapPlan build(HitMapTable& t, int device, const void* stream, size_t bytes, const void* grid = nullptr,
                 unsigned long long epoch = 0, const CollisionParams& c = kParams, bool launch_ok = true)
{
  const HitMapPlan p = t.plan(device, stream, bytes, grid, epoch, c);
  if (p.slot < 0) {
    CHECK(!p.reallocate && p.clear && !p.reuse && p.stamp == 1u && p.cells == nullptr && p.cap == bytes);
    return p;
  }
  CHECK(p.stamp >= 1u && p.stamp <= 255u && p.cap >= bytes);
  CHECK(!p.reuse || (!p.reallocate && !p.clear));
  if (p.reallocate) t.allocated(p.slot, fresh(), bytes);
  if (!p.reuse && launch_ok) t.built(p, grid, epoch, c);
  return p;
}

// test_stamps_wrap_without_showing_an_earlier_map: a clear at the build after stamp 255 and at no other
void stamps_wrap()
{
  HitMapTable t;
  const void* s = fresh();
  for (unsigned k = 0; k < 300; ++k) {
    const HitMapPlan p = build(t, 0, s, 1000);
    CHECK(p.slot == 0 && p.reallocate == (k == 0));
    CHECK(p.stamp == k % 255u + 1u);
    CHECK(p.clear == (k % 255u == 0));  // k = 0: the fresh buffer; k = 255: the build after stamp 255
    CHECK(p.cap == 1000);
  }
}

// test_buffer_grows_and_is_reused_by_smaller_maps
void grow_and_shrink()
{
  HitMapTable t;
  const void* s = fresh();
  const HitMapPlan a = build(t, 0, s, 1000);
  CHECK(a.reallocate && a.clear && a.stamp == 1u && a.cells == nullptr && a.cap == 1000);
  const HitMapPlan b = build(t, 0, s, 1000);
  CHECK(!b.reallocate && !b.clear && b.stamp == 2u && b.cells != nullptr);
  const HitMapPlan big = build(t, 0, s, 5000);  // larger: the old buffer is handed back to be freed
  CHECK(big.reallocate && big.clear && big.stamp == 1u && big.cells == b.cells && big.cap == 5000);
  const HitMapPlan small = build(t, 0, s, 800);  // smaller: as it is
  CHECK(!small.reallocate && !small.clear && small.stamp == 2u && small.cells != big.cells && small.cap == 5000);
  const HitMapPlan same = build(t, 0, s, 5000);
  CHECK(!same.reallocate && !same.clear && same.stamp == 3u && same.cells == small.cells);
  // the stamps wrap while a smaller map is asked for: the WHOLE capacity is cleared (stale stamps lie beyond 800 bytes too)
  for (unsigned k = 4; k <= 255; ++k) CHECK(build(t, 0, s, 800).stamp == k);
  const HitMapPlan wrap = build(t, 0, s, 800);
  CHECK(wrap.clear && wrap.stamp == 1u && wrap.cap == 5000 && !wrap.reallocate && wrap.cells == same.cells);
  // a reallocation that failed (no allocated()): the next build reallocates again, with nothing to free
  const HitMapPlan lost = t.plan(0, s, 9000, nullptr, 0, kParams);
  CHECK(lost.reallocate && lost.cells == same.cells);
  const HitMapPlan again = build(t, 0, s, 9000);
  CHECK(again.reallocate && again.clear && again.stamp == 1u && again.cells == nullptr);
  // a clear that failed (no built()) is asked for again
  HitMapTable u;
  for (int k = 0; k < 255; ++k) build(u, 0, s, 100);
  CHECK(u.plan(0, s, 100, nullptr, 0, kParams).clear);
  const HitMapPlan retry = build(u, 0, s, 100);
  CHECK(retry.clear && retry.stamp == 1u);
  CHECK(build(u, 0, s, 100).stamp == 2u);
}

// test_two_streams_keep_their_own_maps (and the same stream handle on another device is another key)
void keys_are_independent()
{
  HitMapTable t;
  const void *s1 = fresh(), *s2 = fresh();
  for (unsigned k = 1; k <= 20; ++k) {
    const HitMapPlan a = build(t, 0, s1, 1000), b = build(t, 0, s2, 700);
    CHECK(a.slot == 0 && b.slot == 1 && a.stamp == k && b.stamp == k);
    if (k > 1) CHECK(!a.clear && !b.clear && a.cells != b.cells);
  }
  for (unsigned k = 21; k <= 30; ++k) CHECK(build(t, 0, s1, 1000).stamp == k);
  CHECK(build(t, 0, s2, 700).stamp == 21u);
  const HitMapPlan other = build(t, 1, s1, 1000);
  CHECK(other.slot == 2 && other.reallocate && other.stamp == 1u);
}

// test_more_streams_than_map_buffers
void table_full()
{
  HitMapTable t;
  std::vector<const void*> ss;
  for (int k = 0; k < 66; ++k) ss.push_back(fresh());
  for (int k = 0; k < 66; ++k) {
    const HitMapPlan p = build(t, 0, ss[k], 1000);
    CHECK(p.slot == (k < 64 ? k : -1));
  }
  for (int k = 65; k >= 0; --k) {  // the 64 earlier keys keep their slots and go on counting; the others still get none
    const HitMapPlan p = build(t, 0, ss[k], 1000);
    CHECK(p.slot == (k < 64 ? k : -1));
    if (k < 64) CHECK(p.stamp == 2u && !p.clear && !p.reallocate);
  }
  std::set<void*> freed;
  t.release([&](int device, void* cells) {
    CHECK(device == 0 && cells != nullptr);
    CHECK(freed.insert(cells).second);
  });
  CHECK(freed.size() == 64);
  const HitMapPlan p = build(t, 0, ss[65], 1000);  // after the release a new key gets a slot
  CHECK(p.slot == 0 && p.reallocate && p.clear && p.stamp == 1u && p.cells == nullptr);
  int n = 0;
  t.release([&](int, void*) { ++n; });
  CHECK(n == 1);
  t.release([&](int, void*) { ++n; });
  CHECK(n == 1);
}

// test_tick_epoch_cache_is_dropped_by_any_other_build
void epoch_reuse()
{
  const void *s = fresh(), *s2 = fresh(), *grid = fresh(), *grid2 = fresh();
  {  // hit: the same (grid, epoch, parameters) again, as often as it comes
    HitMapTable t;
    const HitMapPlan a = build(t, 0, s, 1000, grid, 7);
    CHECK(!a.reuse && a.stamp == 1u);
    for (int k = 0; k < 3; ++k) {
      const HitMapPlan b = build(t, 0, s, 1000, grid, 7);
      CHECK(b.reuse && b.stamp == 1u && b.cells != nullptr && !b.clear && !b.reallocate);
    }
    CHECK(build(t, 0, s, 1000, grid, 8).stamp == 2u);  // and the stamps go on from there
    // another key's builds do not touch this one's record
    build(t, 0, s2, 1000, grid2, 3);
    CHECK(build(t, 0, s, 1000, grid, 8).reuse);
    CHECK(!build(t, 0, s2, 1000, grid, 8).reuse);
  }
  // miss: one thing differs from the recorded build (and the build that missed is the record from then on)
  std::vector<CollisionParams> others(9, kParams);
  others[0].xmin = -2.5;
  others[1].ymin = 0.0;
  others[2].resolution = 0.05;
  others[3].xsize = 81u;
  others[4].ysize = 61u;
  others[5].r_bnd = 7;
  others[6].r_col = 9;
  others[7].r_max = 11;
  others[8].occupied_threshold = 0.5;
  for (const CollisionParams& o : others) {
    HitMapTable t;
    build(t, 0, s, 1000, grid, 7);
    const HitMapPlan p = build(t, 0, s, 1000, grid, 7, o);
    CHECK(!p.reuse && p.stamp == 2u);
    CHECK(build(t, 0, s, 1000, grid, 7, o).reuse);
    CHECK(!build(t, 0, s, 1000, grid, 7).reuse);
  }
  {
    HitMapTable t;
    build(t, 0, s, 1000, grid, 7);
    CHECK(!build(t, 0, s, 1000, grid2, 7).reuse);  // the grid pointer
    CHECK(!build(t, 0, s, 1000, grid2, 8).reuse);  // the epoch
    CHECK(build(t, 0, s, 1000, grid2, 8).reuse);
    CHECK(!build(t, 0, s, 1000, grid2, 0).reuse);  // epoch 0 asks for no reuse ...
    CHECK(!build(t, 0, s, 1000, grid2, 0).reuse);  // ... and records none,
    CHECK(!build(t, 0, s, 1000, grid2, 8).reuse);  // and like any other build on the key it has dropped the record
    CHECK(build(t, 0, s, 1000, grid2, 8).reuse);
    CHECK(!build(t, 0, s, 4000, grid2, 8).reuse);  // a reallocation
    CHECK(build(t, 0, s, 4000, grid2, 8).reuse);
    CHECK(build(t, 0, s, 500, grid2, 8).reuse);    // (a smaller request for the same map: the buffer holds it)
  }
  {  // the previous build was never reported as succeeded
    HitMapTable t;
    build(t, 0, s, 1000, grid, 7, kParams, false);
    const HitMapPlan p = build(t, 0, s, 1000, grid, 7);
    CHECK(!p.reuse && p.clear);  // (the clear of the fresh buffer was not reported either)
    CHECK(build(t, 0, s, 1000, grid, 7).reuse);
    const HitMapPlan q = build(t, 0, s, 1000, grid, 9, kParams, false);  // a failed launch between two ticks of one epoch
    CHECK(!q.reuse && q.stamp == 2u);
    const HitMapPlan r = build(t, 0, s, 1000, grid, 9);
    CHECK(!r.reuse && r.stamp == 3u);  // the map of epoch 9 was never stamped, and the failed build's stamp is spent
    CHECK(build(t, 0, s, 1000, grid, 9).reuse);
    CHECK(build(t, 0, s, 1000, grid, 7, kParams, false).stamp == 4u);
    const HitMapPlan r2 = build(t, 0, s, 1000, grid, 9);
    CHECK(!r2.reuse && r2.stamp == 5u);  // the record of epoch 9 went when the failed build started
  }
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc == 4) {
    for (const short2& o : ring_offsets(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]))) std::printf("%d %d\n", o.x, o.y);
    return 0;
  }
  CHECK(argc == 1);
  stamps_wrap();
  grow_and_shrink();
  keys_are_independent();
  table_full();
  epoch_reuse();
  std::printf("hit map table: ok\n");
  return 0;
}
