// Host-side bookkeeping of the small tables the grid queries upload once per device and keep: the inflated map's ring offsets
// (collision_kernel.hip), the clearance walk (clearance_kernel.hip), the fleet layer's row spans (fleet_layer_kernel.hip).
// Plain C++ like HitMapTable: no HIP call, no global state, no lock -- each kernel file owns its mutex and performs the
// effects (grid_buffers.hpp); tests/device_tables_check.cpp drives this alone.
#pragma once

#include <cstddef>
#include <vector>

namespace eea
{
// One entry per (device, Key): one device allocation (`block`; null for a table without elements), a small trivially
// copyable View of it (pointers into the block, counts) and the number of users that hold it.  Key: anything with ==.
template <typename Key, typename View>
class DeviceTables
{
public:
  struct Entry
  {
    int device;
    Key key;
    void* block;
    View view;
    int users;
  };

  // null: no such entry (the pointer is valid until the next insert or release).  hold: the caller becomes a user of the
  // entry until it gives the block back
  const Entry* find(int device, const Key& key, bool hold = false)
  {
    for (Entry& e : entries_) {
      if (e.device != device || !(e.key == key)) continue;
      if (hold) e.users += 1;
      return &e;
    }
    return nullptr;
  }

  // after a miss: the caller has allocated and filled `block`
  const Entry& insert(int device, const Key& key, void* block, const View& view, bool hold = false)
  {
    entries_.push_back(Entry{ device, key, block, view, hold ? 1 : 0 });
    return entries_.back();
  }

  // a user of `block` is gone; an unknown block, or one nobody holds, changes nothing
  void give_back(int device, const void* block)
  {
    for (Entry& e : entries_) {
      if (e.device == device && e.block == block && e.users > 0) {
        e.users -= 1;
        return;
      }
    }
  }

  // forgets every entry nobody holds: free_block(device, block) for each of their allocations.  Held entries stay.
  template <typename Free>
  void release(Free free_block)
  {
    std::vector<Entry> kept;
    for (const Entry& e : entries_) {
      if (e.users > 0) kept.push_back(e);
      else if (e.block != nullptr) free_block(e.device, e.block);
    }
    entries_.swap(kept);
  }

  size_t size() const { return entries_.size(); }

private:
  std::vector<Entry> entries_;
};
}  // namespace eea
