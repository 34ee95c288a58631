// revo_map.h -- what the voxel map (revo_map*.hip) needs from the rest of the library.  Internal: not part of the C ABI.
#pragma once
#include "revo_internal.h"

struct MapSource {  // one keyframe as the map integration reads it: level 0 of its pyramid + its full-resolution colour
  revo_ctx* ctx;
  const float* depth;
  const uint8_t* edges;
  const uint8_t* bgr;
};
struct MapCtxGeom {  // level-0 camera and depth range of a context, the stream the map work goes on
  int device, w, h;
  float fx, fy, cx, cy, dmin, dmax;
  void* stream;      // hipStream_t: the context's tracker stream
};

extern "C" {
// the keyframe's planes, with the context's tracker stream ordered behind everything that writes them
int revo_map_source_(revo_pyr* kf, MapSource* out);
int revo_map_ctx_geom_(const revo_ctx* ctx, MapCtxGeom* out);
// a pyramid's context and whether revo_map_source_ would refuse it as a batch view; enqueues nothing
int revo_map_source_kind_(const revo_pyr* kf, const revo_ctx** ctx, int* batch_view);
// revo_vo_multi: integrate the keyframe slots a step has just promoted (n entries, T_w_kf column-major, 16 floats each)
struct revo_map_stage;
int revo_map_stage_create_(revo_map_stage** out);
void revo_map_stage_destroy_(revo_map_stage* st);
int revo_map_integrate_views_(revo_map_stage* st, int n, revo_map* const* maps, revo_pyr* const* kfs, const float* T16);
// bookkeeping of attachments (a map knows the revo_vo_multi streams that hold it, so that destroying it detaches it)
void revo_map_note_attach_(revo_map* m, revo_vo_multi* mv, int stream, int attach);
const revo_ctx* revo_map_ctx_(const revo_map* m);
void revo_vo_multi_forget_map_(revo_vo_multi* mv, int stream, revo_map* m);
}
