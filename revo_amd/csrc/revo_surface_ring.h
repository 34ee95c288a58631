// revo_surface_ring.h -- which views a stream's windowed surface holds (revo_vo_multi_surface_window): the policy alone,
// as plain C++.  The driver (revo_vo_multi.hip) keeps what names a view again -- device copies of its depth and colour image, its
// pose -- in the slot this ring hands out; tests/cpp/surface_ring_host.cpp checks the policy on the host.  Internal.
//
// A window of N views has N + 1 slots: a step first fuses and keeps the new keyframe (push) and only then takes the oldest one
// out (evict), so for a moment N + 1 views are held.  Between steps at most N are.  A keyframe that was not fused is not pushed.
#pragma once
#include <cstdint>

#define SURFACE_RING_MAX 1024  // the largest window

struct SurfaceRing {
  int window = 0;          // 0: off
  int head = 0;            // the slot of the oldest held view
  int held = 0;            // the views held
  uint64_t evictions = 0;  // the views that have left since the window was set

  static bool valid(int window) { return window >= 0 && window <= SURFACE_RING_MAX; }
  // A window of `w` views over an empty ring; w = 0 switches it off.
  void set(int w) { window = w; head = 0; held = 0; evictions = 0; }
  bool on() const { return window > 0; }
  int slots() const { return window > 0 ? window + 1 : 0; }
  // A view that was fused is held from now on -> its slot.  A free one exists: held <= window on entry, since every push is
  // followed by the evictions that over() asks for.
  int next() const { return (head + held) % slots(); }  // the slot push() will give
  int push() {
    const int slot = next();
    ++held;
    return slot;
  }
  // More views are held than the window allows: the oldest one leaves.
  bool over() const { return window > 0 && held > window; }
  // The slot of the oldest view, which stays held ...
  int oldest() const { return head; }
  // ... and the oldest view leaves the ring -> the slot it had, free from now on.
  int evict() {
    const int slot = head;
    head = (head + 1) % slots();
    --held;
    ++evictions;
    return slot;
  }
};
