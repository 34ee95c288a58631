// revo_internal.h -- what the host code of librevo_hip.so's translation units shares: the hooks that cross units, fail() and
// HIPCHECK, and the one vocabulary of owners (device and pinned memory, streams, events, stream marks, descriptor rows) that
// the handles of the host core (revo_host_impl.h) and of the voxel map (revo_map_impl.h) are written with.  Internal: not part
// of the C ABI, and not exported (the library exports include/revo_hip.h and nothing else: -fvisibility=hidden plus
// revo_hip.ver, Makefile).  Every file that defines or calls one of the hooks below includes this header, so the compiler
// checks each call and each definition against the one declaration.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <memory>
#include <string>

#include "../../include/revo_hip.h"

extern "C" {
// revo_host.hip: the thread's error string (what revo_last_error returns)
void revo_set_error_(const char* msg);
// revo_host.hip: the context's lifetime (every handle built on a context holds a reference) and device
void revo_ctx_retain_(revo_ctx* c);
void revo_ctx_release_(revo_ctx* c);
int revo_ctx_device_(const revo_ctx* c);
// revo_host.hip / revo_single.hip / revo_frame.hip, for revo_vo.hip: split single-pair calls (launch now, read the result
// later) and the sequencing around them
int revo_ctx_reserve_framesets_(revo_ctx* c, int total);
int revo_track_launch_(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float R[9], const float T[3], int slot,
                       unsigned* seq_out);
int revo_track_wait_(revo_ctx* c, int slot, unsigned seq, float R[9], float T[3], float* err, int* status);
int revo_assess_launch_(revo_ctx* c, const float T_w_curr[16], const revo_pyr* curr, int* nframes_out, unsigned* seq_out);
int revo_assess_wait_(revo_ctx* c, int nframes, unsigned seq, int* status, float* ratio_out);
int revo_pyramid_prepare_keyframe_(revo_pyr* p);
void revo_tracker_reset_past_(revo_ctx* c);
void revo_debug_section_note_(int i, unsigned long long ns);
// revo_batch.hip, for revo_pipeline.hip: the next revo_batch_track_only of b records ev0 / ev1 (hipEvent_t) around its grid
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

// ------------------------------------------------------------------------------------------------------------ owners --
#define TRY(expr) do { const int rc__ = (expr); if (rc__) return rc__; } while (0)

struct Owner {  // what the types below are: owners of device resources, released by their destructors, never copied
  Owner() = default;
  Owner(const Owner&) = delete;
  Owner& operator=(const Owner&) = delete;
};

// Device memory of one call: freed when the call returns, whichever way, and a failed call leaves no sticky error behind.
struct DevScratch : Owner {
  char* p = nullptr;
  ~DevScratch() { (void)hipFree(p); (void)hipGetLastError(); }
  int alloc(size_t bytes) { HIPCHECK(hipMalloc((void**)&p, bytes)); return REVO_OK; }
};

// A device buffer of the handle that only grows.  The stream is waited for first: its work may still use the old one.
struct DevBuf : Owner {
  char* p = nullptr; size_t bytes = 0;
  ~DevBuf() { (void)hipFree(p); }
  int reserve(size_t need, hipStream_t s) {
    if (need <= bytes) return REVO_OK;
    HIPCHECK(hipStreamSynchronize(s));
    (void)hipFree(p);
    p = nullptr; bytes = 0;
    HIPCHECK(hipMalloc((void**)&p, need));
    bytes = need;
    return REVO_OK;
  }
};

// Descriptor rows of a launch: written into pinned memory, uploaded, read by the kernels from device memory.  The event
// (recorded behind the upload) is waited for before the pinned rows are rewritten, the stream before device rows that a
// kernel may still read are reallocated (none exist yet when the rows are first reserved: no wait then).  The event is made
// on first use, or ahead of it by create(), where its cost must not fall into the first launch.
template <typename Row>
struct HostRows : Owner {
  Row* h = nullptr; Row* d = nullptr; int cap = 0;
  hipEvent_t ev = nullptr; bool recorded = false;
  ~HostRows() {
    if (recorded) (void)hipEventSynchronize(ev);
    (void)hipHostFree(h); (void)hipFree(d);
    if (ev) (void)hipEventDestroy(ev);
  }
  int create() { if (!ev) HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); return REVO_OK; }
  int reserve(int n, hipStream_t s) {
    if (recorded) HIPCHECK(hipEventSynchronize(ev));  // the previous upload has read the pinned rows
    if (n <= cap) return REVO_OK;
    if (cap) HIPCHECK(hipStreamSynchronize(s));  // the previous call's kernels read the device rows
    (void)hipHostFree(h); (void)hipFree(d);
    h = nullptr; d = nullptr; cap = 0;
    HIPCHECK(hipHostMalloc((void**)&h, sizeof(Row) * n));
    HIPCHECK(hipMalloc((void**)&d, sizeof(Row) * n));
    cap = n;
    return REVO_OK;
  }
  int upload(int n, hipStream_t s, bool mark = true) {  // mark: record the event behind it
    HIPCHECK(hipMemcpyAsync(d, h, sizeof(Row) * n, hipMemcpyHostToDevice, s));
    if (!mark) return REVO_OK;
    TRY(create());
    HIPCHECK(hipEventRecord(ev, s));
    recorded = true;
    return REVO_OK;
  }
};

// The two events around a feature's device work and what *_last_ms makes of them.
struct EventTimer : Owner {
  hipEvent_t e0 = nullptr, e1 = nullptr; bool ready = false;
  ~EventTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  int begin(hipStream_t s) {
    if (!e0) HIPCHECK(hipEventCreate(&e0));
    if (!e1) HIPCHECK(hipEventCreate(&e1));
    HIPCHECK(hipEventRecord(e0, s));
    return REVO_OK;
  }
  int end(hipStream_t s) {
    HIPCHECK(hipEventRecord(e1, s));
    ready = true;
    return REVO_OK;
  }
  int last_ms(float* ms) {
    HIPCHECK(hipEventSynchronize(e1));
    HIPCHECK(hipEventElapsedTime(ms, e0, e1));
    return REVO_OK;
  }
};

// An event of a handle: without timing unless asked, made where the handle makes it today (create() on one that exists is
// nothing), destroyed with the handle.  event_create alone is for the few events that live as long as the process.
inline int event_create(hipEvent_t* e, unsigned flags = hipEventDisableTiming) {
  HIPCHECK(hipEventCreateWithFlags(e, flags));
  return REVO_OK;
}
struct OwnedEvent : Owner {
  hipEvent_t e = nullptr;
  ~OwnedEvent() { if (e) (void)hipEventDestroy(e); }
  int create(unsigned flags = hipEventDisableTiming) { return e ? REVO_OK : event_create(&e, flags); }
  operator hipEvent_t() const { return e; }
};
// A stream mark: an event, the stream it was last recorded on, and whether it ever was.  Who must be ordered behind the
// marked work says which wait it means: wait() always waits (if recorded) -- the enqueued wait is part of the caller's
// stream order even on the recording stream -- and wait_elsewhere() leaves out a consumer on the recording stream, which is
// ordered already.  A mark nobody recorded orders nothing.
struct StreamMark : Owner {
  OwnedEvent ev; hipStream_t stream = nullptr; bool recorded = false;
  int create() { return ev.create(); }
  int record(hipStream_t s) {
    HIPCHECK(hipEventRecord(ev, s));
    recorded = true; stream = s;
    return REVO_OK;
  }
  int wait(hipStream_t s) const { if (recorded) HIPCHECK(hipStreamWaitEvent(s, ev, 0)); return REVO_OK; }
  int wait_elsewhere(hipStream_t s) const { return stream != s ? wait(s) : REVO_OK; }
  int sync() const { if (recorded) HIPCHECK(hipEventSynchronize(ev)); return REVO_OK; }  // the host waits
};
struct OwnedStream : Owner {  // non-blocking, like every stream of the library
  hipStream_t s = nullptr;
  ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
  int create() { HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); return REVO_OK; }
  operator hipStream_t() const { return s; }
};
// n elements of device (pinned host) memory of a handle, allocated once.
template <typename T>
struct DevMem : Owner {
  T* p = nullptr;
  ~DevMem() { (void)hipFree(p); }
  int alloc(size_t n) { HIPCHECK(hipMalloc((void**)&p, sizeof(T) * n)); return REVO_OK; }
  operator T*() const { return p; }
  T* operator->() const { return p; }
};
template <typename T>
struct PinnedMem : Owner {
  T* p = nullptr;
  ~PinnedMem() { (void)hipHostFree(p); }
  int alloc(size_t n) { HIPCHECK(hipHostMalloc((void**)&p, sizeof(T) * n)); return REVO_OK; }
  operator T*() const { return p; }
  T* operator->() const { return p; }
};
// How a handle goes: its destructor releases what it holds (a partly built one holds null handles on purpose, hence the
// cleared error).  Partial<H> is a handle under construction: a create that fails on the way simply returns.
struct HandleDelete {
  template <typename H> void operator()(H* h) const { delete h; (void)hipGetLastError(); }
};
template <typename H> using Partial = std::unique_ptr<H, HandleDelete>;
