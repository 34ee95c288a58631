// revo_multi.h -- the device half of revo_vo_multi (revo_mdev.hip) as seen by its host-side sequencing (revo_vo_multi.hip).
// Internal: not part of the C ABI.  A "set" is one FrameSet of n_streams frames built by one submit; frames are addressed
// as (set, frame index inside the set).
#pragma once
#include "revo_internal.h"

struct revo_mdev;
struct MultiTrack { int stream; void* set; int frame; float R[9], T[3]; int status; };  // R/T in: init, out: result
struct MultiVote { int stream; void* set; int frame; float T_w_curr[16]; int status; };
struct MultiFrame { int stream; void* set; int frame; float T_w[16]; double ts; };     // clouds to add / frames to promote

extern "C" {
int revo_mdev_create_(revo_ctx* c, int n_streams, revo_mdev** out);
void revo_mdev_destroy_(revo_mdev* m);
// device_src: the frames are device pointers, copied device-to-device after the build stream waits for `producer`
int revo_mdev_submit_(revo_mdev* m, int n, const revo_stream_frame* frames, int depth_is_u16, double scale, int device_src,
                      void* producer, void** set_out);
void revo_mdev_release_set_(revo_mdev* m, void* set);  // no frame of the set is queued, current or previous any more
int revo_mdev_track_(revo_mdev* m, int n, MultiTrack* pairs);            // one tracker grid, waits for the poses
int revo_mdev_pair_info_enqueue_(revo_mdev* m, int n);                   // k_pair_info for the n pairs just tracked (asynchronous)
int revo_mdev_pair_info_wait_(revo_mdev* m, int n, revo_pair_info* out); // ... their records
int revo_mdev_vote_(revo_mdev* m, int n, MultiVote* votes);              // one batched vote, waits for the counts
int revo_mdev_add_clouds_(revo_mdev* m, int n, const MultiFrame* f);     // one batched cloud copy (asynchronous)
int revo_mdev_promote_(revo_mdev* m, int n, const MultiFrame* f);        // keyframe slots <- frames, then their EDT
void revo_mdev_clear_past_(revo_mdev* m, int stream, int keep);          // keep the newest `keep` (< 0: N_FRAMES_HIST_VOTING)
revo_pyr* revo_mdev_keyframe_(revo_mdev* m, int stream);
}
