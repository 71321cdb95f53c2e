// Host-side bookkeeping of the grid queries: the ring walk of the reference's search with its two views -- the offset set of
// the inflated collision map's dilation (collision_kernel.hip) and the visit-ordered list of the clearance queries
// (clearance_kernel.hip) -- and the policy of the map buffers both keep between calls.  Plain C++: no HIP call, no global
// state, no lock -- the callers own their mutex and grid_buffers.hpp performs the effects; tests/hit_map_table_check.cpp and
// tests/clearance_walk_check.cpp drive this file alone, without a GPU.
#pragma once

#include <set>
#include <utility>
#include <vector>

#include "common.hpp"  // CollisionParams, short2

namespace eea
{
// The reference's ring walk (collision.cpp:166-214), written ONCE on the host: the rings r_bnd..r_max one after the other,
// within a ring the Bresenham steps in order, within a step Q1 Q2 Q3 Q4 (collision.cpp:175-193); visit(dx, dy) per visit,
// (dx, dy) = cell - centre.  A ring of radius <= 0 visits nothing.  (The device's own bresenham_circle, collision_kernel.hip,
// is the reference-literal search; this is its enumeration.)
template <typename Visit>
inline void walk_rings(int r_bnd, int r_max, Visit visit)
{
  for (int r0 = r_bnd < 1 ? 1 : r_bnd; r0 <= r_max; ++r0) {
    int r = r0, x = -r0, y = 0, err = 2 - 2 * r0;
    while (x < 0) {
      visit(-x, y);
      visit(-y, -x);
      visit(x, -y);
      visit(y, x);
      r = err;
      if (r <= y) {
        y++;
        err += 2 * y + 1;
      }
      if (r > x || err > y) {
        x++;
        err += 2 * x + 1;
      }
    }
  }
}

// offsets (cell - centre) the ring search r_bnd..r_max can report a collision at: the set of the walk's visits within r_col
// (collision.cpp:239), sorted, each offset once
inline std::vector<short2> ring_offsets(int r_bnd, int r_col, int r_max)
{
  std::set<std::pair<int, int>> pts;
  walk_rings(r_bnd, r_max, [&](int dx, int dy) {
    if (dx * dx + dy * dy <= r_col * r_col) pts.emplace(dx, dy);
  });
  std::vector<short2> out;
  for (const auto& p : pts) out.push_back(make_short2(static_cast<short>(p.first), static_cast<short>(p.second)));
  return out;
}

// The walk's visits as a list, in VISIT order with duplicates kept (clearance_kernel.hip): offsets[k] is the k-th cell the
// search r_bnd..r_max tests.  Collision::minDistance / minDirection keep the FIRST visited cell of the smallest squared
// distance, i.e. the smallest key (|d_k|^2, k); the device holds that key in one 32-bit word, |d_k|^2 * n + k, with the
// all-ones word for "no cell".
struct ClearanceWalk
{
  std::vector<short2> offsets;
  int reach = 0;        // max |component| of an offset: the key map covers the centres [-reach, size + reach)
  unsigned max_sq = 0;  // max |d_k|^2
};
constexpr unsigned kNoClearanceKey = 0xffffffffu;

// every key of n offsets up to max_sq is below kNoClearanceKey
inline bool clearance_key_fits(unsigned long long max_sq, unsigned long long n)
{
  return (max_sq + 1ull) * n <= 0xffffffffull;  // the largest key is max_sq * n + n - 1
}

// false: the parameter set is refused (its largest key does not fit), `w` is then unspecified
inline bool clearance_walk(int r_bnd, int r_max, ClearanceWalk& w)
{
  w = ClearanceWalk{};
  // The ring r_max alone has at least 4 r_max offsets (x goes from -r_max to 0 by at most 1 per step) of |d|^2 >= r_max^2:
  // 4 r_max^3 >= 2^32 from r_max = 1024 on.  Refused here, before a walk of that size is enumerated.
  if (r_max >= 1024 && r_bnd <= r_max) return false;
  walk_rings(r_bnd, r_max, [&](int dx, int dy) {
    w.offsets.push_back(make_short2(static_cast<short>(dx), static_cast<short>(dy)));
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    if (ax > w.reach) w.reach = ax;
    if (ay > w.reach) w.reach = ay;
    const unsigned sq = static_cast<unsigned>(dx * dx + dy * dy);
    if (sq > w.max_sq) w.max_sq = sq;
  });
  return clearance_key_fits(w.max_sq, w.offsets.size());
}

// What one build of an inflated map has to do, in this order: reallocate, clear, launch the dilation with `stamp`.
struct HitMapPlan
{
  int slot;         // the (device, stream) pair's entry; -1: the table is full, the caller builds in a stream-ordered allocation
  bool reallocate;  // free `cells` (it may be null) and allocate `cap` bytes: then HitMapTable::allocated
  bool clear;       // zero all `cap` bytes
  bool reuse;       // the slot's last build is the map asked for: no launch, `stamp` is that build's
  unsigned stamp;   // 1..255
  void* cells;      // the slot's buffer as it is now
  size_t cap;       // its capacity once the plan is carried out
};

// The map buffer of a (device, stream) pair is kept between calls: launches on one stream are ordered, so a buffer is never
// written while an earlier call still reads it.  Every build marks with a fresh stamp (1..255), which makes the marks of
// earlier builds stale without clearing the buffer; it is cleared when the stamps wrap.  A build is then a single scatter
// kernel.  Use: plan(), the plan's effects, allocated() behind a reallocation, built() behind the launch.
class HitMapTable
{
public:
  static constexpr size_t kMaxSlots = 64;

  // epoch != 0: the caller vouches that (grid, epoch) names one content -- the last build on this key is reused when it was
  // reported as built() from the same (grid, epoch, parameters).  Any other plan forgets that record before the build starts.
  HitMapPlan plan(int device, const void* stream, size_t bytes, const void* grid, unsigned long long epoch, const CollisionParams& c)
  {
    size_t k = 0;
    while (k < slots_.size() && !(slots_[k].device == device && slots_[k].stream == stream)) ++k;
    if (k == slots_.size()) {
      if (k == kMaxSlots) return HitMapPlan{ -1, false, true, false, 1u, nullptr, bytes };
      slots_.push_back(Slot{ device, stream });
    }
    Slot& s = slots_[k];
    HitMapPlan p{ static_cast<int>(k), s.cap < bytes, false, false, s.stamp, s.cells, s.cap };
    if (p.reallocate) {  // (a smaller map lives in the buffer as it is: stale stamps mark nothing, whatever the row pitch)
      s = Slot{ device, stream };
      p.cap = bytes;
    }
    p.reuse = epoch != 0 && s.stamp != 0 && s.built_grid == grid && s.built_epoch == epoch && same_params(s.built_params, c);
    if (p.reuse) return p;
    s.built_epoch = 0;  // (no call's epoch)
    p.clear = s.stamp == 0 || s.stamp >= 255u;  // a fresh buffer, or the stamps wrap
    p.stamp = p.clear ? 1u : s.stamp + 1u;
    // A clear is asked for again until built() reports it: also after a clear whose launch then failed, where a second
    // clear is harmless.  (bytes == 0, which no valid grid gives, asks for a clear of no bytes in a null buffer.)
    s.stamp = p.clear ? 0u : p.stamp;
    return p;
  }

  // the plan's reallocation succeeded
  void allocated(int slot, void* cells, size_t cap)
  {
    slots_[slot].cells = cells;
    slots_[slot].cap = cap;
  }

  // The plan's clear and launch succeeded.  The cache key is recorded only now: after a failed launch the next tick with the
  // same (grid, epoch) must not validate against a map that was never stamped.  It is valid for work ordered behind this
  // launch (the caller's stream contract).
  void built(const HitMapPlan& p, const void* grid, unsigned long long epoch, const CollisionParams& c)
  {
    Slot& s = slots_[p.slot];
    s.stamp = p.stamp;
    s.built_grid = grid;
    s.built_epoch = epoch;
    s.built_params = c;
  }

  // empties the table: free_cells(device, buffer) for every buffer the caller has to free
  template <typename Free>
  void release(Free free_cells)
  {
    for (const Slot& s : slots_) {
      if (s.cells != nullptr) free_cells(s.device, s.cells);
    }
    slots_.clear();
  }

private:
  struct Slot
  {
    int device;
    const void* stream;
    void* cells = nullptr;
    size_t cap = 0;
    unsigned stamp = 0;  // of the last build; 0: the buffer has to be cleared first
    // what that stamp was built from (built_epoch != 0)
    const void* built_grid = nullptr;
    unsigned long long built_epoch = 0;
    CollisionParams built_params{};
  };
  std::vector<Slot> slots_;
};
}  // namespace eea
