// Drives csrc/device_tables.hpp alone, on the CPU (tests/test_device_tables.py builds this with the address and undefined-
// behaviour sanitizers and runs it as a process): the cache of the small tables kept per device -- the ring offsets, the
// clearance walk, the fleet layer's spans.  Stops at the first wrong answer and names the line.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "../ergodic_exploration_amd/csrc/device_tables.hpp"

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
char g_memory[4096];  // addresses only: "device" blocks are never dereferenced
int g_next = 0;
void* fresh() { return &g_memory[g_next++]; }

struct Key
{
  int a, b;
  bool operator==(const Key& o) const { return a == o.a && b == o.b; }
};
struct View
{
  const void* at;
  int n;
};
using Tables = DeviceTables<Key, View>;

// what a release hands to `free`: (device, block) -> how often
using Freed = std::map<std::pair<int, const void*>, int>;
Freed release(Tables& t)
{
  Freed freed;
  t.release([&](int device, void* block) { freed[{ device, block }] += 1; });
  return freed;
}

void miss_then_hit()
{
  Tables t;
  CHECK(t.find(0, Key{ 6, 10 }) == nullptr && t.size() == 0);
  void* const b0 = fresh();
  const Tables::Entry& in = t.insert(0, Key{ 6, 10 }, b0, View{ b0, 744 });
  CHECK(in.device == 0 && in.block == b0 && in.view.at == b0 && in.view.n == 744 && in.users == 0);
  const Tables::Entry* hit = t.find(0, Key{ 6, 10 });
  CHECK(hit != nullptr && hit->block == b0 && hit->view.n == 744 && hit->users == 0);
  CHECK(t.find(0, Key{ 6, 11 }) == nullptr && t.find(0, Key{ 10, 6 }) == nullptr);  // another key
  CHECK(t.find(1, Key{ 6, 10 }) == nullptr);                                        // the same key on another device
  void* const b1 = fresh();
  t.insert(1, Key{ 6, 10 }, b1, View{ b1, 744 });
  CHECK(t.find(1, Key{ 6, 10 })->block == b1 && t.find(0, Key{ 6, 10 })->block == b0 && t.size() == 2);
  const Freed freed = release(t);
  CHECK(freed.size() == 2 && freed.at({ 0, b0 }) == 1 && freed.at({ 1, b1 }) == 1 && t.size() == 0);
  CHECK(t.find(0, Key{ 6, 10 }) == nullptr);
}

void held_entries_survive_a_release()
{
  Tables t;
  void *const held = fresh(), *const loose = fresh(), *const twice = fresh();
  t.insert(0, Key{ 1, 1 }, held, View{ held, 1 }, true);  // a layer is created: it holds its table
  t.insert(0, Key{ 2, 2 }, loose, View{ loose, 2 });
  t.insert(1, Key{ 3, 3 }, twice, View{ twice, 3 }, true);
  CHECK(t.find(1, Key{ 3, 3 }, true)->users == 2);  // a second layer on the same table
  Freed freed = release(t);
  CHECK(freed.size() == 1 && freed.at({ 0, loose }) == 1 && t.size() == 2);
  CHECK(t.find(0, Key{ 1, 1 })->block == held && t.find(0, Key{ 1, 1 })->users == 1);  // (a find without hold counts nobody)
  CHECK(t.find(0, Key{ 2, 2 }) == nullptr);
  CHECK(release(t).empty() && t.size() == 2);  // again: nothing is freed twice
  // give-back, then release: freed
  t.give_back(0, held);
  CHECK(t.find(0, Key{ 1, 1 })->users == 0);
  freed = release(t);
  CHECK(freed.size() == 1 && freed.at({ 0, held }) == 1 && t.size() == 1);
  // two holders: one give-back is not enough
  t.give_back(1, twice);
  CHECK(release(t).empty() && t.find(1, Key{ 3, 3 })->users == 1);
  t.give_back(1, twice);
  freed = release(t);
  CHECK(freed.size() == 1 && freed.at({ 1, twice }) == 1 && t.size() == 0);
}

void give_back_of_an_unknown_block_changes_nothing()
{
  Tables t;
  void *const b = fresh(), *const other = fresh();
  t.give_back(0, b);  // an empty cache
  CHECK(t.size() == 0);
  t.insert(0, Key{ 1, 2 }, b, View{ b, 5 }, true);
  t.give_back(0, other);  // no entry's block
  t.give_back(1, b);      // the block, on another device
  CHECK(t.find(0, Key{ 1, 2 })->users == 1 && release(t).empty());
  t.give_back(0, b);
  t.give_back(0, b);  // nobody holds it any more: the count stays at 0
  CHECK(t.find(0, Key{ 1, 2 })->users == 0);
  CHECK(t.find(0, Key{ 1, 2 }, true)->users == 1 && release(t).empty());
  t.give_back(0, b);
  CHECK(release(t).size() == 1);
}

void release_on_an_empty_cache()
{
  Tables t;
  CHECK(release(t).empty() && t.size() == 0);
  CHECK(release(t).empty());
  // a table without elements has no block: found like any other, nothing to free
  t.insert(2, Key{ 0, 0 }, nullptr, View{ nullptr, 0 });
  CHECK(t.find(2, Key{ 0, 0 }) != nullptr && t.find(2, Key{ 0, 0 })->view.n == 0);
  CHECK(release(t).empty() && t.size() == 0);
}

void two_hundred_inserts()
{
  Tables t;
  void* blocks[200];
  for (int k = 0; k < 200; ++k) {
    CHECK(t.find(k % 3, Key{ k, -k }) == nullptr);
    blocks[k] = fresh();
    t.insert(k % 3, Key{ k, -k }, blocks[k], View{ blocks[k], k });
  }
  CHECK(t.size() == 200);
  for (int k = 0; k < 200; ++k) {
    const Tables::Entry* e = t.find(k % 3, Key{ k, -k });
    CHECK(e != nullptr && e->block == blocks[k] && e->view.n == k);
  }
  const Freed freed = release(t);
  CHECK(freed.size() == 200 && t.size() == 0);
  for (int k = 0; k < 200; ++k) CHECK(freed.at({ k % 3, blocks[k] }) == 1);
}
}  // namespace

int main()
{
  miss_then_hit();
  held_entries_survive_a_release();
  give_back_of_an_unknown_block_changes_nothing();
  release_on_an_empty_cache();
  two_hundred_inserts();
  std::printf("device tables: ok\n");
  return 0;
}
