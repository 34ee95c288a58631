// surface_ring_host.cpp -- the policy of a stream's surface window (revo_amd/csrc/revo_surface_ring.h) on the host: which
// slot a fused keyframe's copies go into, which view leaves, how many are held.  A model keeps the held views as a plain queue of
// (keyframe number, slot); the ring must hand out a slot no held view has, evict the keyframes in the order they came, and hold
// min(fused, window) views behind every step -- at the windows 1, N and N + 1 slots' worth of steps, with skipped keyframes (which
// are not held) in between, and after the window is set again.  Stand-alone: prints one line per case and "ok".
#include <cstdio>
#include <deque>
#include <utility>
#include <vector>

#include "../../revo_amd/csrc/revo_surface_ring.h"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

// One step of the driver for a stream: the keyframe `kf` was fused (or skipped); -> the keyframe evicted in this step, or -1.
static int step(SurfaceRing& r, std::deque<std::pair<int, int>>& model, std::vector<int>& slot_owner, int kf, bool fused) {
  if (!fused) return -1;  // a skipped keyframe is not held
  CHECK(r.held <= r.window);
  const int next = r.next();
  const int slot = r.push();
  CHECK(slot == next && slot >= 0 && slot < r.slots());
  for (const auto& h : model) CHECK(h.second != slot);  // no held view's copies are overwritten
  model.push_back({kf, slot});
  slot_owner[(size_t)slot] = kf;
  int evicted = -1;
  if (r.over()) {
    CHECK(r.oldest() == model.front().second);
    CHECK(slot_owner[(size_t)r.oldest()] == model.front().first);  // the oldest slot still names the oldest view
    evicted = model.front().first;
    const int freed = r.evict();
    CHECK(freed == model.front().second);
    model.pop_front();
  }
  CHECK(!r.over());
  CHECK(r.held == (int)model.size() && r.held <= r.window);
  return evicted;
}

static void run(int window, int keyframes, int skip_every, const char* name) {
  SurfaceRing r;
  r.set(window);
  CHECK(r.on() && r.slots() == window + 1 && r.held == 0 && r.evictions == 0 && !r.over());
  std::deque<std::pair<int, int>> model;
  std::vector<int> slot_owner((size_t)r.slots(), -1);
  int fused = 0, expect_evicted = 0, last_evicted = -1;
  std::vector<int> order;  // the fused keyframes in order
  for (int kf = 0; kf < keyframes; ++kf) {
    const bool skip = skip_every > 0 && kf % skip_every == skip_every - 1;
    const int ev = step(r, model, slot_owner, kf, !skip);
    if (skip) {
      CHECK(ev == -1 && r.held == (int)model.size());
      continue;
    }
    order.push_back(kf);
    ++fused;
    if (fused > window) {  // from the step that fuses view window + 1 on, every step evicts exactly the oldest
      CHECK(ev == order[(size_t)expect_evicted]);
      ++expect_evicted;
      last_evicted = ev;
    } else {
      CHECK(ev == -1);
    }
    CHECK(r.held == (fused < window ? fused : window));
    CHECK(r.evictions == (uint64_t)expect_evicted);
  }
  // what is held are the last min(fused, window) fused keyframes, oldest first
  const int held = fused < window ? fused : window;
  CHECK((int)model.size() == held);
  for (int i = 0; i < held; ++i) CHECK(model[(size_t)i].first == order[(size_t)(fused - held + i)]);
  std::printf("%s: window %d fused %d held %d evictions %llu last evicted %d\n", name, window, fused, r.held, (unsigned long long)r.evictions, last_evicted);
}

int main() {
  SurfaceRing off;
  CHECK(!off.on() && off.slots() == 0 && !off.over() && off.held == 0);  // the default of every attachment
  CHECK(SurfaceRing::valid(0) && SurfaceRing::valid(1) && SurfaceRing::valid(1024) && !SurfaceRing::valid(-1) && !SurfaceRing::valid(1025));
  run(1, 1, 0, "window 1, one keyframe");            // held 1, nothing leaves
  run(1, 2, 0, "window 1, two keyframes");           // N + 1: the first leaves
  run(1, 9, 0, "window 1, nine keyframes");
  run(4, 3, 0, "window 4, below the window");
  run(4, 4, 0, "window 4, at the window");           // at N: nothing leaves
  run(4, 5, 0, "window 4, one above");               // at N + 1: exactly one leaves, the first
  run(4, 23, 0, "window 4, the ring wraps");
  run(3, 20, 3, "window 3, every third keyframe skipped");
  run(2, 7, 2, "window 2, every second keyframe skipped");
  run(1024, 1030, 0, "the largest window");
  // setting the window again starts an empty one
  SurfaceRing r;
  r.set(2);
  (void)r.push(); (void)r.push(); (void)r.push();
  CHECK(r.over());
  (void)r.evict();
  r.set(3);
  CHECK(r.held == 0 && r.head == 0 && r.evictions == 0 && r.slots() == 4);
  r.set(0);
  CHECK(!r.on() && !r.over());
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
