// revo_internal.h -- what the host code of librevo_hip.so's translation units shares.  Internal: not part of the C ABI, and
// not exported (the library exports include/revo_hip.h and nothing else: -fvisibility=hidden plus revo_hip.ver, Makefile).
// Every file that defines or calls one of the hooks below includes this header, so the compiler checks each call and each
// definition against the one declaration.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "../../include/revo_hip.h"

extern "C" {
// revo_host.hip: the thread's error string (what revo_last_error returns)
void revo_set_error_(const char* msg);
// revo_host.hip: the context's lifetime (every handle built on a context holds a reference) and device
void revo_ctx_retain_(revo_ctx* c);
void revo_ctx_release_(revo_ctx* c);
int revo_ctx_device_(const revo_ctx* c);
// revo_host.hip, for revo_vo.hip: split single-pair calls (launch now, read the result later) and the sequencing around them
int revo_ctx_reserve_framesets_(revo_ctx* c, int total);
int revo_track_launch_(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float R[9], const float T[3], int slot,
                       unsigned* seq_out);
int revo_track_wait_(revo_ctx* c, int slot, unsigned seq, float R[9], float T[3], float* err, int* status);
int revo_assess_launch_(revo_ctx* c, const float T_w_curr[16], const revo_pyr* curr, int* nframes_out, unsigned* seq_out);
int revo_assess_wait_(revo_ctx* c, int nframes, unsigned seq, int* status, float* ratio_out);
int revo_pyramid_prepare_keyframe_(revo_pyr* p);
void revo_tracker_reset_past_(revo_ctx* c);
void revo_debug_section_note_(int i, unsigned long long ns);
// revo_host.hip, for revo_pipeline.hip: the next revo_batch_track_only of b records ev0 / ev1 (hipEvent_t) around its grid
void revo_batch_time_next_grid_(revo_batch* b, void* ev0, void* ev1);
}

inline int fail(int code, const std::string& msg) {
  revo_set_error_(msg.c_str());
  return code;
}
#define HIPCHECK(expr)                                                                      \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess)                                                                  \
      return fail(REVO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));        \
  } while (0)

// experiment knobs (environment): clamped integers, defaults are what ships
inline int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = getenv(name);
  if (!e || !*e) return dflt;
  const int v = atoi(e);
  return v < lo ? lo : (v > hi ? hi : v);
}
