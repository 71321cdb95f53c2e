// Drives the integer code the range-sensor kernels share, alone and on the CPU (tests/test_sense_rays.py builds this with the
// address and undefined-behaviour sanitizers and runs it as a process): the rays of csrc/sense_rays.hpp -- Ray and march(), the
// two statements of one recurrence -- against the closed form, march()'s three ends, clip_of; and the head / chunks / tail split
// of csrc/grid_census.hpp.  Stops at the first wrong answer and names the line.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../ergodic_exploration_amd/csrc/grid_census.hpp"
#include "../ergodic_exploration_amd/csrc/sense_rays.hpp"

using namespace eea;

#define CHECK(cond)                                                                                                     \
  do {                                                                                                                  \
    if (!(cond)) {                                                                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed (case %d %d %d %d)\n", __FILE__, __LINE__, #cond, g_case[0], g_case[1], \
                   g_case[2], g_case[3]);                                                                               \
      std::exit(1);                                                                                                     \
    }                                                                                                                   \
  } while (0)

namespace
{
int g_case[4];
using Cells = std::vector<std::pair<int, int>>;

int sgn(int m) { return m > 0 ? 1 : m < 0 ? -1 : 0; }
int closed_form(int m, int s, int R) { return sgn(m) * ((2 * s * std::abs(m) + R) / (2 * R)); }

// the 8R perimeter cells of [-R, R]^2 in the rays' order: from (R, -R) up the right side, then along the top to the left,
// down the left side, along the bottom to the right
Cells perimeter(int R)
{
  Cells t;
  int x = R, y = -R;
  const int step[4][2] = { { 0, 1 }, { -1, 0 }, { 0, -1 }, { 1, 0 } };
  for (const auto& d : step) {
    for (int k = 0; k < 2 * R; ++k) {
      t.emplace_back(x, y);
      x += d[0];
      y += d[1];
    }
  }
  return t;
}

bool inside(const Clip& w, int dx, int dy) { return dx >= w.xlo && dx <= w.xhi && dy >= w.ylo && dy <= w.yhi; }

// march() with a visit that records the cells and says "blocks" at visit number block_at (0: never)
int recorded_march(int q, int R, const Clip& w, int block_at, Cells& seen)
{
  seen.clear();
  return march(q, R, w, [&](int dx, int dy) {
    seen.emplace_back(dx, dy);
    return static_cast<int>(seen.size()) == block_at;
  });
}

void rays_of(int R, const std::vector<Clip>& clips)
{
  const Cells target = perimeter(R);
  CHECK(static_cast<int>(target.size()) == 8 * R);
  for (int q = 0; q < 8 * R; ++q) {
    g_case[0] = R, g_case[1] = q, g_case[2] = g_case[3] = 0;
    // the closed form, step by step; Ray is held to it on all R steps, in the disc or not
    Cells form;
    Ray ray(q, R);
    CHECK(ray.dx == 0 && ray.dy == 0);
    for (int s = 1; s <= R; ++s) {
      form.emplace_back(closed_form(target[q].first, s, R), closed_form(target[q].second, s, R));
      ray.step(R);
      CHECK(ray.dx == form.back().first && ray.dy == form.back().second);
      CHECK(ray.in_disc(R) == (ray.dx * ray.dx + ray.dy * ray.dy <= R * R));
    }
    CHECK(form.back() == target[q]);  // step R is the perimeter cell itself
    for (size_t n = 0; n < clips.size(); ++n) {
      const Clip& w = clips[n];
      g_case[2] = static_cast<int>(n);
      // what the ray may visit: the steps in front of the first one past the disc or past the clip
      Cells want;
      for (int s = 1; s <= R; ++s) {
        const int dx = form[s - 1].first, dy = form[s - 1].second;
        if (dx * dx + dy * dy > R * R || !inside(w, dx, dy)) break;
        want.emplace_back(dx, dy);
      }
      Cells seen;
      CHECK(recorded_march(q, R, w, 0, seen) == -1);
      CHECK(seen == want);
      // a blocking cell at every place of the ray: the range is its step, nothing behind it is visited
      for (int b = 1; b <= static_cast<int>(want.size()); ++b) {
        g_case[3] = b;
        CHECK(recorded_march(q, R, w, b, seen) == b);
        CHECK(seen == Cells(want.begin(), want.begin() + b));
      }
      g_case[3] = 0;
    }
  }
}

// clip_of against the definition: the offsets of [-R, R]^2 that fall on the grid
Clip checked_clip(const CollisionParams& c, unsigned i0, unsigned j0, int R)
{
  g_case[0] = R, g_case[1] = static_cast<int>(i0), g_case[2] = static_cast<int>(j0), g_case[3] = -1;
  const Clip w = clip_of(c, i0, j0, R);
  for (int d = -R - 1; d <= R + 1; ++d) {
    const long long x = static_cast<long long>(j0) + d, y = static_cast<long long>(i0) + d;
    const bool in_x = d >= -R && d <= R && x >= 0 && x < static_cast<long long>(c.xsize);
    const bool in_y = d >= -R && d <= R && y >= 0 && y < static_cast<long long>(c.ysize);
    CHECK((d >= w.xlo && d <= w.xhi) == in_x);
    CHECK((d >= w.ylo && d <= w.yhi) == in_y);
  }
  CHECK(cell_index(c, i0, j0, w.xlo, w.ylo) == (static_cast<size_t>(i0) + w.ylo) * c.xsize + j0 + w.xlo);
  CHECK(cell_index(c, i0, j0, w.xhi, w.yhi) == (static_cast<size_t>(i0) + w.yhi) * c.xsize + j0 + w.xhi);
  return w;
}

template <unsigned SIZE>
void splits()
{
  alignas(16) static unsigned char buffer[16 + 64 * SIZE];
  for (unsigned off = 0; off < 16u; off += SIZE) {
    const uintptr_t base = reinterpret_cast<uintptr_t>(buffer) + off;
    for (size_t n = 0; n <= 40; ++n) {
      g_case[0] = static_cast<int>(SIZE), g_case[1] = static_cast<int>(off), g_case[2] = static_cast<int>(n), g_case[3] = 0;
      const StreamSplit s = stream_split<SIZE>(base, n);
      constexpr size_t per = 16u / SIZE;
      // head, body and tail in this order cover [0, n) once: head <= tail0 <= n and the body is whole loads
      CHECK(s.head <= n && s.tail0 <= n && s.tail0 == s.head + s.chunks * per);
      CHECK(s.head < per && n - s.tail0 < per);
      CHECK(s.head == n || (base + s.head * SIZE) % 16u == 0u);
      std::vector<int> taken(n, 0);
      for (size_t t = 0; t < s.head; ++t) ++taken[t];
      for (size_t ch = 0; ch < s.chunks; ++ch) {
        for (size_t k = 0; k < per; ++k) ++taken[s.head + per * ch + k];
      }
      for (size_t t = 0; t < n - s.tail0; ++t) ++taken[s.tail0 + t];
      for (size_t t = 0; t < n; ++t) CHECK(taken[t] == 1);
    }
  }
}
}  // namespace

int main()
{
  CollisionParams c{};
  c.xsize = 7, c.ysize = 5;
  for (int R = 1; R <= 24; ++R) {
    std::vector<Clip> clips;
    clips.push_back(Clip{ -R, R, -R, R });         // no clip: the disc alone ends a ray
    clips.push_back(checked_clip(c, 0, 0, R));     // a corner
    clips.push_back(checked_clip(c, 4, 6, R));     // the opposite corner
    clips.push_back(checked_clip(c, 2, 6, R));     // an edge
    clips.push_back(checked_clip(c, 0, 3, R));     // another edge
    clips.push_back(checked_clip(c, 2, 3, R));     // the interior (clipped on every side from R = 4 on)
    rays_of(R, clips);
  }
  // the census' classes of a value
  g_case[0] = g_case[1] = g_case[2] = g_case[3] = 0;
  for (int cutoff = -128; cutoff <= 128; ++cutoff) {
    for (int v = -128; v <= 127; ++v) {
      Census n{ 0u, 0u, 0u };
      count_value(n, v, cutoff);
      g_case[0] = cutoff, g_case[1] = v;
      CHECK(n.unknown + n.below + n.blocking >= 1u && n.unknown + n.below + n.blocking <= 2u);
      CHECK(n.unknown == (v < 0 ? 1u : 0u) && n.blocking == (v >= cutoff ? 1u : 0u));
      CHECK(n.below == ((v >= 0 && v < cutoff) ? 1u : 0u));
    }
  }
  splits<1>();
  splits<4>();
  std::printf("sense rays: ok\n");
  return 0;
}
