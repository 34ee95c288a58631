"""ctypes loader for revo_amd/librevo_hip.so (the C ABI of include/revo_hip.h).

There is no CPU fallback: a missing library is a hard error, and every entry
point that needs a device fails with REVO_ERR_HIP when no MI355X is visible.
"""
import ctypes as C
import os
import re

from .settings import (ImgPyramidSettings, OptimizerSettings, TrackerSettings, ResidualInfo,
                       PairResult, PairInfo, MapAlignParams, MapAlignInfo, MapAlignOpts, MapNormalsParams, MapPlaneInfo, MapPoseInfo,
                       MapCarveView, MapCarveParams, MapCarveInfo, MapCarveViewInfo, MapRayParams, MapDfBox, MapDfAlignInfo, MapObserveParams, MapGainParams, MapTsdfParams, MapTsdfRayParams, MapTsdfTrackParams, MapTsdfTrackInfo, MapTsdfShiftInfo, MapTsdfRefillInfo, MapTsdfUnfuseInfo, MapTsdfFuseJob, MapTsdfTrackJob, MapTsdfTrackResult, MapTsdfUnfuseJob, MapTsdfRayJob, MultiSurfaceWindowReport, MultiSurface, MultiSurfaceReport, MapView, MAX_LEVELS)

_HERE = os.path.dirname(os.path.abspath(__file__))
# REVO_HIP_SO: an alternative build of the same library (profiling builds under profiles/); never a fallback
SO_PATH = os.environ.get("REVO_HIP_SO") or os.path.join(_HERE, "librevo_hip.so")
HEADER = os.path.join(_HERE, "..", "include", "revo_hip.h")

u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
vp = C.c_void_p
vpp = C.POINTER(C.c_void_p)


class RevoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("revo_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def declared_symbols():
    """Every function the C header declares (used by the CPU-side export test)."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(revo_[a-z0-9_]+)\s*\(", txt)))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImportError(
            "revo_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % SO_PATH)
    # torch (device memory / streams / torch.distributed plumbing) bundles its own ROCm
    # runtime; loading it FIRST makes librevo_hip.so bind to that single copy instead of
    # mixing it with /opt/rocm's (two HIP runtimes in one process corrupt the heap).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(SO_PATH)
    L.revo_last_error.restype = C.c_char_p
    L.revo_version.restype = C.c_char_p
    L.revo_pyr_settings_default.argtypes = [C.POINTER(ImgPyramidSettings)]
    L.revo_opt_settings_default.argtypes = [C.POINTER(OptimizerSettings)]
    L.revo_tracker_settings_default.argtypes = [C.POINTER(TrackerSettings)]
    L.revo_ctx_create.argtypes = [C.c_int, C.POINTER(ImgPyramidSettings), C.POINTER(OptimizerSettings),
                                  C.POINTER(TrackerSettings), vpp]
    L.revo_ctx_destroy.argtypes = [vp]
    L.revo_ctx_destroy.restype = None
    L.revo_ctx_set_tracker.argtypes = [vp, C.POINTER(OptimizerSettings), C.POINTER(TrackerSettings)]
    L.revo_ctx_camera.argtypes = [vp, C.c_int, f32p]
    L.revo_pyramid_create.argtypes = [vp, u8p, C.c_size_t, f32p, C.c_size_t, C.c_double, vpp]
    L.revo_pyramid_create_u16.argtypes = [vp, u8p, C.c_size_t, u16p, C.c_size_t, C.c_double, C.c_double, vpp]
    L.revo_pyramid_destroy.argtypes = [vp]
    L.revo_pyramid_destroy.restype = None
    L.revo_pyramid_make_keyframe.argtypes = [vp]
    L.revo_pyramid_is_keyframe.argtypes = [vp]
    L.revo_pyramid_timestamp.argtypes = [vp]
    L.revo_pyramid_timestamp.restype = C.c_double
    L.revo_pyramid_read.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.revo_pyramid_colored_pcl.argtypes = [vp, C.c_int, C.c_int, f32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.revo_optimizer_track_level.argtypes = [vp, vp, vp, f32p, f32p, C.c_int, C.POINTER(ResidualInfo), f32p]
    L.revo_optimizer_eval.argtypes = [vp, vp, vp, f32p, f32p, C.c_int, C.POINTER(ResidualInfo), f32p, f32p, f32p]
    L.revo_optimizer_solve6.argtypes = [vp, C.c_int, f32p, f32p]
    L.revo_tracker_track_frames.argtypes = [vp, vp, vp, f32p, f32p, f32p, C.POINTER(C.c_int),
                                            C.POINTER(ResidualInfo), i32p]
    L.revo_tracker_assess_quality.argtypes = [vp, f32p, vp, C.POINTER(C.c_int), i32p, i32p]
    L.revo_tracker_add_old_pcl.argtypes = [vp, vp, C.c_int, f32p, C.c_double]
    L.revo_tracker_add_old_pcl_host.argtypes = [vp, f32p, C.c_size_t, f32p, C.c_double]
    L.revo_tracker_clear_past.argtypes = [vp]
    L.revo_tracker_past_size.argtypes = [vp]
    L.revo_batch_create.argtypes = [vp, C.c_int, vpp]
    L.revo_batch_destroy.argtypes = [vp]
    L.revo_batch_destroy.restype = None
    L.revo_batch_track.argtypes = [vp, vp, vp, f32p, vp, vp]
    L.revo_batch_build.argtypes = [vp, vp, vp, vp]
    L.revo_batch_build_borrow.argtypes = [vp, vp, vp, vp]
    L.revo_batch_build_u16.argtypes = [vp, vp, vp, C.c_double, vp]
    L.revo_batch_track_only.argtypes = [vp, f32p, vp, vp]
    L.revo_batch_prepare.argtypes = [vp, vp]
    L.revo_batch_sync.argtypes = [vp, vp]
    L.revo_track_pairs_submit.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double, vpp]
    L.revo_track_pairs_wait.argtypes = [vp, vp]
    L.revo_track_pairs.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double, vp]
    L.revo_batch_frame.argtypes = [vp, C.c_int, vpp]
    L.revo_batch_time_tracker.argtypes = [vp, f32p, vp, vp, C.c_int, f32p]
    L.revo_batch_profile_build.argtypes = [vp, vp, vp, C.c_int, vp]
    L.revo_ctx_histogram_level.argtypes = [vp]
    L.revo_ctx_set_exact_sums.argtypes = [vp, C.c_int]
    L.revo_ctx_exact_sums.argtypes = [vp]
    L.revo_vo_create.argtypes = [vp, vpp]
    L.revo_vo_destroy.argtypes = [vp]
    L.revo_vo_destroy.restype = None
    L.revo_vo_submit.argtypes = [vp, u8p, C.c_size_t, f32p, C.c_size_t, C.c_double]
    L.revo_vo_submit_u16.argtypes = [vp, u8p, C.c_size_t, u16p, C.c_size_t, C.c_double, C.c_double]
    L.revo_vo_track_next.argtypes = [vp, f32p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.revo_vo_queued.argtypes = [vp]
    L.revo_vo_keyframe.argtypes = [vp, vpp, f32p]
    L.revo_vo_set_max_queue.argtypes = [vp, C.c_int]
    L.revo_vo_close.argtypes = [vp]
    L.revo_vo_wait_frame.argtypes = [vp]
    L.revo_vo_num_keyframes.argtypes = [vp]
    L.revo_vo_multi_create.argtypes = [vp, C.c_int, C.c_int, vpp]
    L.revo_vo_multi_destroy.argtypes = [vp]
    L.revo_vo_multi_destroy.restype = None
    L.revo_vo_multi_submit.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double]
    L.revo_vo_multi_step.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.revo_vo_multi_pending.argtypes = [vp, C.c_int]
    L.revo_vo_multi_reset.argtypes = [vp, C.c_int]
    L.revo_vo_multi_num_keyframes.argtypes = [vp, C.c_int]
    L.revo_vo_multi_keyframe.argtypes = [vp, C.c_int, vpp, f32p]
    L.revo_vo_multi_submit_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double, vp]
    L.revo_map_create.argtypes = [vp, C.c_float, C.c_int, C.c_size_t, C.c_size_t, vpp]
    L.revo_map_destroy.argtypes = [vp]
    L.revo_map_destroy.restype = None
    L.revo_map_integrate.argtypes = [vp, vp, f32p]
    L.revo_map_integrate_many.argtypes = [vp, C.c_int, vpp, f32p]
    L.revo_map_clear.argtypes = [vp]
    L.revo_map_info.argtypes = [vp, vp]
    L.revo_map_extract.argtypes = [vp, C.c_size_t, f32p, u8p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]
    L.revo_vo_multi_attach_map.argtypes = [vp, C.c_int, vp]
    L.revo_map_render.argtypes = [vp, C.c_int, vp, vpp, vpp, vp, C.c_int]
    L.revo_map_render_last_ms.argtypes = [vp, f32p]
    L.revo_map_export_raw.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.revo_map_merge_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_size_t, C.c_int32]
    L.revo_map_merge.argtypes = [vp, vp]
    L.revo_map_subtract_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_size_t, C.c_int32]
    L.revo_map_subtract.argtypes = [vp, vp]
    L.revo_map_voxel_size.argtypes = [vp, f32p, C.POINTER(C.c_int)]
    L.revo_map_coarsen.argtypes = [vp, vp, C.c_int]
    L.revo_map_align_eval.argtypes = [vp, vp, C.c_int, f32p, C.POINTER(MapAlignParams), vp, C.c_int]
    L.revo_map_align_system.argtypes = [C.POINTER(MapAlignInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.revo_map_align.argtypes = [vp, vp, f32p, C.POINTER(MapAlignParams), C.POINTER(MapAlignOpts), f32p,
                                 C.POINTER(MapAlignInfo), i32p, i32p]
    L.revo_map_normals.argtypes = [vp, C.POINTER(MapNormalsParams), f32p, f32p, f32p, C.POINTER(C.c_uint32), C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    L.revo_map_align_plane_eval.argtypes = [vp, vp, C.c_int, f32p, C.POINTER(MapAlignParams), C.POINTER(MapNormalsParams), vp, C.c_int]
    L.revo_map_align_plane_system.argtypes = [C.POINTER(MapPlaneInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.revo_map_align_plane.argtypes = [vp, vp, f32p, C.POINTER(MapAlignParams), C.POINTER(MapNormalsParams), C.POINTER(MapAlignOpts),
                                       f32p, C.POINTER(MapPlaneInfo), i32p, i32p]
    L.revo_map_pose_raw.argtypes = [vp, f32p, C.c_float, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int,
                                    C.POINTER(MapPoseInfo)]
    L.revo_map_merge_posed.argtypes = [vp, vp, f32p, C.c_size_t, C.POINTER(MapPoseInfo)]
    L.revo_map_subtract_posed.argtypes = [vp, vp, f32p, C.c_size_t, C.POINTER(MapPoseInfo)]
    for fn in (L.revo_map_carve_eval, L.revo_map_carve):
        fn.argtypes = [vp, C.c_int, C.POINTER(MapCarveView), C.c_int, C.POINTER(MapCarveParams), vp, C.c_size_t, C.POINTER(C.c_size_t),
                       C.c_int, C.POINTER(MapCarveInfo), C.POINTER(MapCarveViewInfo)]
    L.revo_map_raycast.argtypes = [vp, C.c_int, vp, C.POINTER(MapRayParams), vpp, vpp, vpp, vp, C.c_int, vp]
    L.revo_map_cast_rays.argtypes = [vp, C.c_size_t, vp, C.c_int, C.c_uint32, C.POINTER(MapRayParams), vp, C.c_int, vp]
    L.revo_map_raycast_last_ms.argtypes = [vp, f32p]
    L.revo_map_distance_field.argtypes = [vp, C.POINTER(MapDfBox), C.c_uint32, C.c_uint32, vp, C.c_int, vp]
    L.revo_map_bounds.argtypes = [vp, C.c_uint32, i32p, i32p, C.POINTER(C.c_size_t)]
    L.revo_map_df_sample.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_size_t, vp, C.c_int, vp, C.c_int]
    L.revo_map_distance_field_last_ms.argtypes = [vp, f32p]
    L.revo_map_df_align_eval.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_size_t, vp, C.c_int, C.c_int, f32p, C.POINTER(MapAlignParams),
                                         vp, C.c_int]
    L.revo_map_df_align_system.argtypes = [C.POINTER(MapDfAlignInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.revo_map_df_align.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_size_t, vp, C.c_int, f32p, C.POINTER(MapAlignParams),
                                    C.POINTER(MapAlignOpts), f32p, C.POINTER(MapDfAlignInfo), i32p, i32p]
    L.revo_map_plan.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_uint32, C.c_size_t, vp, C.c_uint32, vp, C.c_int, vp]
    L.revo_map_plan_last.argtypes = [vp, f32p, C.POINTER(C.c_uint32)]
    L.revo_map_plan_paths.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_size_t, vp, C.c_uint32, vp, vp, C.c_int]
    L.revo_map_observe.argtypes = [vp, C.POINTER(MapDfBox), C.c_int, C.POINTER(MapCarveView), C.c_int, C.POINTER(MapObserveParams), vp, C.c_int, vp, vp]
    L.revo_map_known_field.argtypes = [vp, C.POINTER(MapDfBox), C.c_uint32, C.c_uint32, vp, C.c_int, C.c_uint32, vp, C.c_int, vp]
    L.revo_map_frontiers.argtypes = [vp, C.POINTER(MapDfBox), C.c_uint32, vp, C.c_int, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
    L.revo_map_view_gain.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.POINTER(MapView), C.c_size_t, vp, C.c_int, C.POINTER(MapGainParams), vp, C.c_int, vp]
    L.revo_map_tsdf_fuse.argtypes = [vp, C.POINTER(MapDfBox), C.c_int, C.POINTER(MapCarveView), C.c_int, C.POINTER(MapTsdfParams), vp, C.c_int, vp, vp]
    L.revo_map_tsdf_mesh.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                     C.POINTER(C.c_size_t), C.c_int, vp]
    L.revo_map_tsdf_fuse_color.argtypes = [vp, C.POINTER(MapDfBox), C.c_int, C.POINTER(MapCarveView), vp, C.c_int, C.POINTER(MapTsdfParams), vp, vp,
                                           C.c_int, vp, vp, vp]
    L.revo_map_tsdf_mesh_attr.argtypes = [vp, C.POINTER(MapDfBox), vp, vp, C.c_int, C.c_uint32, vp, vp, vp, C.c_size_t, vp, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_int, vp]
    L.revo_map_tsdf_raycast.argtypes = [vp, C.POINTER(MapDfBox), vp, vp, C.c_int, C.c_int, vp, C.POINTER(MapTsdfRayParams), vpp, vpp, vpp, vp,
                                        C.c_int, vp]
    L.revo_map_tsdf_track_eval.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_float, C.POINTER(MapCarveView), C.c_int, C.c_int, f32p,
                                           C.POINTER(MapTsdfTrackParams), vp, C.c_int]
    L.revo_map_tsdf_track_system.argtypes = [C.POINTER(MapTsdfTrackInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.revo_map_tsdf_track.argtypes = [vp, C.POINTER(MapDfBox), vp, C.c_int, C.c_float, C.POINTER(MapCarveView), C.c_int, f32p,
                                      C.POINTER(MapTsdfTrackParams), C.POINTER(MapAlignOpts), f32p, C.POINTER(MapTsdfTrackInfo), i32p, i32p]
    L.revo_map_tsdf_shift.argtypes = [vp, C.POINTER(MapDfBox), i32p, vp, vp, vp, vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, vp]
    L.revo_map_tsdf_refill.argtypes = [vp, C.POINTER(MapDfBox), vp, vp, C.c_int, C.c_size_t, vp, C.c_int, C.POINTER(MapTsdfRefillInfo)]
    L.revo_map_tsdf_unfuse.argtypes = [vp, C.POINTER(MapDfBox), C.c_int, C.POINTER(MapCarveView), vp, C.c_int, C.c_float, vp, vp, C.c_int,
                                       C.POINTER(MapTsdfUnfuseInfo), vp]
    L.revo_map_tsdf_fuse_many.argtypes = [vp, C.c_int, C.POINTER(MapTsdfFuseJob)]
    L.revo_map_tsdf_unfuse_many.argtypes = [vp, C.c_int, C.POINTER(MapTsdfUnfuseJob), vp, C.c_int]
    L.revo_map_tsdf_raycast_many.argtypes = [vp, C.c_int, C.POINTER(MapTsdfRayJob)]
    L.revo_map_tsdf_track_eval_many.argtypes = [vp, C.c_int, C.POINTER(MapTsdfTrackJob), vp, C.c_int]
    L.revo_vo_multi_attach_surface.argtypes = [vp, C.c_int, C.POINTER(MultiSurface)]
    L.revo_vo_multi_surface_last.argtypes = [vp, C.c_int, C.POINTER(MultiSurfaceReport)]
    L.revo_vo_multi_surface_window.argtypes = [vp, C.c_int, C.c_int]
    L.revo_vo_multi_surface_window_last.argtypes = [vp, C.c_int, C.POINTER(MultiSurfaceWindowReport)]
    L.revo_map_tsdf_track_many.argtypes = [vp, C.c_int, C.POINTER(MapTsdfTrackJob), C.POINTER(MapAlignOpts), C.POINTER(MapTsdfTrackResult), i32p]
    L.revo_png_probe.argtypes = [C.c_char_p, C.c_size_t, vp]
    L.revo_png_decoder_create.argtypes = [vp, C.c_int, C.c_size_t, C.c_size_t, vpp]
    L.revo_png_decoder_destroy.argtypes = [vp]
    L.revo_png_decoder_destroy.restype = None
    L.revo_png_decode_submit.argtypes = [vp, C.c_int, vp, vp, C.POINTER(C.c_uint64)]
    L.revo_png_decode_wait.argtypes = [vp, C.c_uint64, i32p]
    L.revo_pipeline_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, vpp]
    L.revo_pipeline_destroy.argtypes = [vp]
    L.revo_pipeline_destroy.restype = None
    L.revo_pipeline_submit.argtypes = [vp, vp, vp, C.c_int, C.c_double, f32p, vp, vp, C.POINTER(C.c_uint64), vpp]
    L.revo_pipeline_wait.argtypes = [vp, C.c_uint64, vp]
    L.revo_pipeline_drain.argtypes = [vp]
    L.revo_pipeline_info.argtypes = [vp, vp]
    L.revo_pipeline_batch.argtypes = [vp, C.c_uint64, vpp]
    L.revo_pipeline_time_tracker.argtypes = [vp, C.c_int]
    L.revo_pipeline_tracker_ms.argtypes = [vp, f32p, C.POINTER(C.c_int)]
    L.revo_comm_available.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
    L.revo_comm_unique_id.argtypes = [u8p]
    L.revo_comm_create.argtypes = [vp, u8p, C.c_int, C.c_int, vpp]
    L.revo_comm_destroy.argtypes = [vp]
    L.revo_comm_destroy.restype = None
    L.revo_comm_world.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.revo_comm_allgather_records.argtypes = [vp, vp, vp, C.c_int, vp]
    L.revo_pipeline_set_comm.argtypes = [vp, vp, C.c_int, vp, C.c_int]
    L.revo_pipeline_flush_comm.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.revo_batch_pair_info.argtypes = [vp, vp, f32p, C.c_int, vp, vp]
    L.revo_tracker_pair_info.argtypes = [vp, vp, vp, f32p, f32p, C.c_int, C.POINTER(PairInfo)]
    L.revo_pair_info_covariance.argtypes = [C.POINTER(PairInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.revo_vo_set_pair_info.argtypes = [vp, C.c_int]
    L.revo_vo_last_pair_info.argtypes = [vp, C.POINTER(PairInfo), C.POINTER(C.c_double)]
    L.revo_vo_multi_set_pair_info.argtypes = [vp, C.c_int]
    L.revo_vo_multi_pair_info.argtypes = [vp, C.c_int, C.POINTER(PairInfo), C.POINTER(C.c_double)]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RevoError(rc, (lib().revo_last_error() or b"").decode())
