"""POD mirrors of the reference's settings classes (ctypes layout of include/revo_hip.h).

Reference:
  ImgPyramidSettings  datastructures/camerapyr.h:27-89   (+ config/dataset_tum1.yaml)
  OptimizerSettings   system/optimizer.h:42-112
  TrackerSettings     system/tracker.h:31-55             (+ config/revo_settings.yaml)
  ResidualInfo        system/optimizer.h:118-140
"""
import ctypes as C

MAX_LEVELS = 6

TRACKER_STATE_OK = 0
TRACKER_STATE_LOST = 1
TRACKER_STATE_NEW_KF = 2
TRACKER_STATE_UNKNOWN = 3

PLANE_GRAY, PLANE_DEPTH, PLANE_EDGES, PLANE_EDGES_ORIG = 0, 1, 2, 3
PLANE_DT, PLANE_GRADTABLE, PLANE_EDGES3D, PLANE_HIST = 4, 5, 6, 7
PLANE_EDGES3D_TILED = 8  # the tracker's tile-ordered copy of EDGES3D (what the per-frame build writes)


class ImgPyramidSettings(C.Structure):
    """camerapyr.h:27-89; defaults = config/dataset_tum1.yaml."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("pyr_min_lvl", C.c_int32), ("pyr_max_lvl", C.c_int32),
        ("canny_threshold1", C.c_int32), ("canny_threshold2", C.c_int32),
        ("depth_min", C.c_float), ("depth_max", C.c_float),
        ("use_edge_hist", C.c_int32), ("n_percentage", C.c_float),
        ("hist_patch", C.c_int32 * MAX_LEVELS),
    ]

    def __init__(self, width=640, height=480, fx=517.306408, fy=516.469215,
                 cx=318.643040, cy=255.313989, pyr_min_lvl=2, pyr_max_lvl=0,
                 canny_threshold1=150, canny_threshold2=100, depth_min=0.1,
                 depth_max=5.2, use_edge_hist=1, n_percentage=0.3,
                 hist_patch=(20, 10, 5, 0, 0, 0)):
        super().__init__()
        self.width, self.height = width, height
        self.fx, self.fy, self.cx, self.cy = fx, fy, cx, cy
        self.pyr_min_lvl, self.pyr_max_lvl = pyr_min_lvl, pyr_max_lvl
        self.canny_threshold1, self.canny_threshold2 = canny_threshold1, canny_threshold2
        self.depth_min, self.depth_max = depth_min, depth_max
        self.use_edge_hist, self.n_percentage = use_edge_hist, n_percentage
        for i in range(MAX_LEVELS):
            self.hist_patch[i] = hist_patch[i] if i < len(hist_patch) else 0

    def nLevels(self):  # camerapyr.h:68-71
        return self.pyr_min_lvl - self.pyr_max_lvl + 1

    def level_size(self, lvl):  # Camera(...,scale), camerapyr.h:98-103
        s = 1.0 / (2 ** lvl)
        return int(self.width * s), int(self.height * s)

    @classmethod
    def scaled(cls, width, height, levels, **kw):
        """TUM-1 intrinsics scaled to another resolution (e.g. 1280x960, 160x120)."""
        sx = width / 640.0
        sy = height / 480.0
        return cls(width=width, height=height, fx=517.306408 * sx, fy=516.469215 * sy,
                   cx=318.643040 * sx, cy=255.313989 * sy, pyr_min_lvl=levels - 1, **kw)


class OptimizerSettings(C.Structure):
    """optimizer.h:42-112 (hot-path fields); USE_EDGE_FILTER from tracker.h:46."""
    _fields_ = [
        ("lambda_success_fac", C.c_float), ("lambda_fail_fac", C.c_float),
        ("lambda_initial", C.c_float * MAX_LEVELS),
        ("step_size_min", C.c_float * MAX_LEVELS),
        ("convergence_eps", C.c_float * MAX_LEVELS),
        ("max_its_per_lvl", C.c_int32 * MAX_LEVELS),
        ("edge_distance_lvl", C.c_float * MAX_LEVELS),
        ("huber_edge", C.c_float), ("use_edge_filter", C.c_int32),
    ]

    def __init__(self, use_edge_filter=1):
        super().__init__()
        self.lambda_success_fac = 0.5
        self.lambda_fail_fac = 2.0
        for i, ed in enumerate((30, 20, 10, 5, 5, 5)):
            self.lambda_initial[i] = 0.0
            self.step_size_min[i] = 1e-16
            self.convergence_eps[i] = 0.999
            self.max_its_per_lvl[i] = 100
            self.edge_distance_lvl[i] = ed
        self.huber_edge = 0.3
        self.use_edge_filter = use_edge_filter


class TrackerSettings(C.Structure):
    """tracker.h:31-55; histogramLevel tracker.cpp:229."""
    _fields_ = [
        ("check_tracking_results", C.c_int32), ("check_init_values", C.c_int32),
        ("n_frames_hist_voting", C.c_int32), ("histogram_level", C.c_int32),
    ]

    def __init__(self, check_tracking_results=1, check_init_values=1,
                 n_frames_hist_voting=3, histogram_level=2):
        super().__init__()
        self.check_tracking_results = check_tracking_results
        self.check_init_values = check_init_values
        self.n_frames_hist_voting = n_frames_hist_voting
        self.histogram_level = histogram_level


class ResidualInfo(C.Structure):
    """optimizer.h:118-140."""
    _fields_ = [
        ("good_pts_edges", C.c_int32), ("bad_pts_edges", C.c_int32),
        ("sum_error_unweighted", C.c_float), ("sum_error_weighted", C.c_float),
    ]


class PairResult(C.Structure):
    """revo_pair_result (include/revo_hip.h), 96 bytes."""
    _fields_ = [
        ("R", C.c_float * 9), ("T", C.c_float * 3), ("err", C.c_float),
        ("good", C.c_int32), ("bad", C.c_int32), ("status", C.c_int32),
        ("evals", C.c_int32 * MAX_LEVELS), ("flags", C.c_int32), ("n_pts0", C.c_int32),
    ]


assert C.sizeof(PairResult) == 96


class PairInfo(C.Structure):
    """revo_pair_info (include/revo_hip.h), 192 bytes: the sums of a pair's normal equations at a pose of one level -- H (upper
    triangle, row-major), g, sum w r^2, sum r^2, the good / bad counts -- each the float nearest the exact sum of its terms."""
    _fields_ = [
        ("H", C.c_float * 21), ("g", C.c_float * 6), ("sum_w", C.c_float), ("sum_u", C.c_float),
        ("good", C.c_int32), ("bad", C.c_int32), ("level", C.c_int32), ("flags", C.c_int32),
        ("R", C.c_float * 9), ("T", C.c_float * 3), ("reserved", C.c_int32 * 3),
    ]


assert C.sizeof(PairInfo) == 192
PAIR_INFO_CHUNK = 1024  # points per chunk of k_pair_info (INFO_CHUNK, revo_amd/csrc/revo_dev.h)
PAIR_INFO_MAX_GROUPS = 32


def pair_info_groups(npix):
    """Workgroups per pair of a k_pair_info launch at a level of npix pixels (info_groups, revo_amd/csrc/revo_dev.h)."""
    return max(1, min(PAIR_INFO_MAX_GROUPS, (npix + 8 * PAIR_INFO_CHUNK - 1) // (8 * PAIR_INFO_CHUNK)))


class StreamFrame(C.Structure):
    """revo_stream_frame (include/revo_hip.h): one frame of one stream of revo_vo_multi, host memory."""
    _fields_ = [
        ("stream", C.c_int32), ("bgr", C.c_void_p), ("bgr_stride", C.c_size_t),
        ("depth", C.c_void_p), ("depth_stride", C.c_size_t), ("timestamp", C.c_double),
    ]


class StreamResult(C.Structure):
    """revo_stream_result (include/revo_hip.h): the pose revo_vo_multi_step reports for one stream."""
    _fields_ = [
        ("stream", C.c_int32), ("new_keyframe", C.c_int32), ("timestamp", C.c_double), ("pose", C.c_float * 16),
    ]


class MapInfo(C.Structure):
    """revo_map_info_t (include/revo_hip.h): the state of a voxel map."""
    _fields_ = [
        ("voxels", C.c_size_t), ("points_integrated", C.c_size_t), ("points_dropped", C.c_size_t), ("capacity", C.c_size_t),
        ("keyframes", C.c_int32), ("keyframes_rejected", C.c_int32), ("rehashes", C.c_int32),
    ]


class MapView(C.Structure):
    """revo_map_view (include/revo_hip.h): one view of revo_map_render.  Intrinsics and depth range all zero: the context's
    level-0 camera and DEPTH_MIN / DEPTH_MAX."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("zmin", C.c_float), ("zmax", C.c_float),
        ("T_w_c", C.c_float * 16), ("splat_max", C.c_int32), ("min_count", C.c_uint32),
    ]


assert C.sizeof(MapView) == 104


class MapAlignParams(C.Structure):
    """revo_map_align_params (include/revo_hip.h): the gate, the count thresholds and the rotation centre of a registration."""
    _fields_ = [("max_dist", C.c_float), ("min_count_dst", C.c_uint32), ("min_count_src", C.c_uint32), ("centre", C.c_float * 3)]


class MapAlignInfo(C.Structure):
    """revo_map_align_info (include/revo_hip.h), 160 bytes: the 16 sums of point-to-point ICP between two voxel maps at a
    pose -- each the float nearest the exact sum of its terms -- the exact counts, and the inputs they were taken at."""
    _fields_ = [
        ("S", C.c_float * 16), ("matched", C.c_uint64), ("considered", C.c_uint64), ("skipped", C.c_uint64),
        ("centre", C.c_float * 3), ("max_dist", C.c_float), ("R", C.c_float * 9), ("T", C.c_float * 3),
        ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


class MapAlignOpts(C.Structure):
    """revo_map_align_opts (include/revo_hip.h): where revo_map_align's Gauss-Newton iteration stops."""
    _fields_ = [("max_iters", C.c_int32), ("reserved", C.c_int32), ("eps_t", C.c_double), ("eps_r", C.c_double),
                ("min_matched", C.c_uint64)]


assert C.sizeof(MapAlignParams) == 24 and C.sizeof(MapAlignInfo) == 160 and C.sizeof(MapAlignOpts) == 32
ALIGN_CONVERGED, ALIGN_ITER_LIMIT, ALIGN_LOST = 0, 1, 2


class MapNormalsParams(C.Structure):
    """revo_map_normals_params (include/revo_hip.h): which voxels count, and when a neighbourhood is a plane."""
    _fields_ = [("min_count", C.c_uint32), ("min_neighbours", C.c_uint32), ("planarity", C.c_float), ("min_spread", C.c_float)]


class MapPlaneInfo(C.Structure):
    """revo_map_plane_info (include/revo_hip.h), 208 bytes: the 28 sums of point-to-plane ICP between two voxel maps at a pose
    (the upper triangle of sum J J^T, sum J e, sum e e), the exact counts, the inputs, and the destination's valid normals."""
    _fields_ = [
        ("S", C.c_float * 28), ("matched", C.c_uint64), ("considered", C.c_uint64), ("skipped", C.c_uint64),
        ("centre", C.c_float * 3), ("max_dist", C.c_float), ("R", C.c_float * 9), ("T", C.c_float * 3),
        ("flags", C.c_int32), ("dst_normals", C.c_int32),
    ]


assert C.sizeof(MapNormalsParams) == 16 and C.sizeof(MapPlaneInfo) == 208


class MapPoseInfo(C.Structure):
    """revo_map_pose_info (include/revo_hip.h), 64 bytes: what became of a source map's voxels and points under a pose."""
    _fields_ = [(k, C.c_uint64) for k in ("voxels_in", "voxels_moved", "voxels_dropped", "voxels_skipped", "points_moved",
                                          "points_dropped", "points_skipped", "reserved")]


assert C.sizeof(MapPoseInfo) == 64


class MapCarveView(C.Structure):
    """revo_map_carve_view (include/revo_hip.h), 112 bytes: one view of revo_map_carve -- a pyramid (kf) or a raw depth image."""
    _fields_ = [
        ("kf", C.c_void_p), ("depth", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("zmin", C.c_float), ("zmax", C.c_float),
        ("T_w_c", C.c_float * 16),
    ]


class MapCarveParams(C.Structure):
    """revo_map_carve_params (include/revo_hip.h), 24 bytes."""
    _fields_ = [("radius", C.c_int32), ("min_views", C.c_uint32), ("min_count", C.c_uint32), ("max_count", C.c_uint32),
                ("margin", C.c_float), ("margin_rel", C.c_float)]


class MapCarveInfo(C.Structure):
    """revo_map_carve_info (include/revo_hip.h), 64 bytes: what a carve considered and removed."""
    _fields_ = [(k, C.c_uint64) for k in ("voxels_considered", "voxels_carved", "points_carved", "votes")] + [("reserved", C.c_uint64 * 4)]


class MapCarveViewInfo(C.Structure):
    """revo_map_carve_view_info (include/revo_hip.h), 32 bytes: the candidates of one view by class."""
    _fields_ = [(k, C.c_uint32) for k in ("outside", "unknown", "free_space", "confirmed", "occluded", "edge")] + [("reserved", C.c_uint32 * 2)]


assert (C.sizeof(MapCarveView), C.sizeof(MapCarveParams), C.sizeof(MapCarveInfo), C.sizeof(MapCarveViewInfo)) == (112, 24, 64, 32)


class MapRayParams(C.Structure):
    """revo_map_ray_params (include/revo_hip.h), 16 bytes: the cells a ray examines at most (1 .. 2^20)."""
    _fields_ = [("max_steps", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class MapRay(C.Structure):
    """revo_map_ray (include/revo_hip.h), 32 bytes: the points o + s d for s0 <= s < s1."""
    _fields_ = [("o", C.c_float * 3), ("s0", C.c_float), ("d", C.c_float * 3), ("s1", C.c_float)]


class MapRayHit(C.Structure):
    """revo_map_ray_hit (include/revo_hip.h), 16 bytes: cells holds the cells examined (bits 0-23) and the status (bits 30-31)."""
    _fields_ = [("key", C.c_uint64), ("s", C.c_float), ("cells", C.c_uint32)]


class MapRayInfo(C.Structure):
    """revo_map_ray_info (include/revo_hip.h), 64 bytes: integer sums over the rays of a call."""
    _fields_ = [(k, C.c_uint64) for k in ("rays", "hits", "range", "outside", "exhausted", "cells")] + [("reserved", C.c_uint64 * 2)]


assert (C.sizeof(MapRayParams), C.sizeof(MapRay), C.sizeof(MapRayHit), C.sizeof(MapRayInfo)) == (16, 32, 16, 64)

DF_NONE = 0xFFFFFFFF  # REVO_DF_NONE: the value of every cell of a distance field whose box holds no solid voxel


class MapDfBox(C.Structure):
    """revo_map_df_box (include/revo_hip.h), 24 bytes: the first voxel index and the cells (1 .. 1024) per axis x, y, z."""
    _fields_ = [("lo", C.c_int32 * 3), ("n", C.c_int32 * 3)]


class MapDfInfo(C.Structure):
    """revo_map_df_info (include/revo_hip.h), 64 bytes: integer sums and maxima of a distance-field call."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "solid", "outside", "below", "max_d2")] + [("reserved", C.c_uint64 * 3)]


class MapDfSample(C.Structure):
    """revo_map_df_sample_t (include/revo_hip.h), 16 bytes: a point's distance in metres (-1: outside the box, +inf: no solid
    voxel) and the dimensionless gradient of the distance."""
    _fields_ = [("dist", C.c_float), ("grad", C.c_float * 3)]


assert (C.sizeof(MapDfBox), C.sizeof(MapDfInfo), C.sizeof(MapDfSample)) == (24, 64, 16)


class MapDfAlignInfo(C.Structure):
    """revo_map_df_align_info (include/revo_hip.h), 208 bytes: the 28 sums of registering a point set against a distance field
    at a pose (the upper triangle of sum J J^T, sum J e, sum e e with J = (g, u x g), g the field's gradient), the exact counts
    and the inputs.  The gated points are considered - matched - skipped."""
    _fields_ = [
        ("S", C.c_float * 28), ("matched", C.c_uint64), ("considered", C.c_uint64), ("skipped", C.c_uint64),
        ("centre", C.c_float * 3), ("max_dist", C.c_float), ("R", C.c_float * 9), ("T", C.c_float * 3),
        ("flags", C.c_int32), ("reserved", C.c_int32),
    ]


assert C.sizeof(MapDfAlignInfo) == 208


PLAN_NONE = 0xFFFFFFFF  # REVO_PLAN_NONE: the cost of a cell that is not free or that no seed reaches
PLAN_REACHED, PLAN_UNREACHABLE, PLAN_OUTSIDE, PLAN_TRUNCATED = 0, 1, 2, 3  # REVO_PLAN_*: how a path ended


class MapPlanSeed(C.Structure):
    """revo_map_plan_seed (include/revo_hip.h), 16 bytes: a goal's voxel index and the cost there (<= 2^24)."""
    _fields_ = [("cell", C.c_int32 * 3), ("cost0", C.c_uint32)]


class MapPlanInfo(C.Structure):
    """revo_map_plan_info (include/revo_hip.h), 64 bytes: integer sums and maxima of a planning call."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "free", "reachable", "max_cost", "seeds_used", "seeds_outside", "seeds_blocked", "reserved")]


class MapPlanPath(C.Structure):
    """revo_map_plan_path (include/revo_hip.h), 16 bytes: the cells written for a start, how its path ended, the start's cost."""
    _fields_ = [("length", C.c_uint32), ("status", C.c_uint32), ("cost", C.c_uint32), ("reserved", C.c_uint32)]


assert (C.sizeof(MapPlanSeed), C.sizeof(MapPlanInfo), C.sizeof(MapPlanPath)) == (16, 64, 16)


class MapObserveParams(C.Structure):
    """revo_map_observe_params (include/revo_hip.h), 16 bytes: the pixel window, whether the call accumulates, the margins."""
    _fields_ = [("radius", C.c_int32), ("accumulate", C.c_uint32), ("margin", C.c_float), ("margin_rel", C.c_float)]


class MapObserveInfo(C.Structure):
    """revo_map_observe_info (include/revo_hip.h), 64 bytes: integer sums of an observe call."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "cells_free", "cells_surface", "votes", "newly_known")] + [("reserved", C.c_uint64 * 3)]


class MapKnownInfo(C.Structure):
    """revo_map_known_info (include/revo_hip.h), 64 bytes: revo_map_df_info's five words, then unknown and known_free."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "solid", "outside", "below", "max_d2", "unknown", "known_free", "reserved")]


assert (C.sizeof(MapObserveParams), C.sizeof(MapObserveInfo), C.sizeof(MapKnownInfo)) == (16, 64, 64)


class MapGainParams(C.Structure):
    """revo_map_gain_params (include/revo_hip.h), 32 bytes: the pixel window, the votes that make a cell known, the margins, the
    depth a miss pixel is read as (0: a hole) and the cells a ray examines at most."""
    _fields_ = [("radius", C.c_int32), ("min_views", C.c_uint32), ("margin", C.c_float), ("margin_rel", C.c_float),
                ("miss_depth", C.c_float), ("max_steps", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class MapGain(C.Structure):
    """revo_map_gain (include/revo_hip.h), 32 bytes per pose: the unknown cells of the box by their class in the predicted view,
    and the view's hit pixels."""
    _fields_ = [(k, C.c_uint32) for k in ("unknown_free", "unknown_surface", "unknown_inside", "hits")] + [("reserved", C.c_uint32 * 4)]


class MapGainInfo(C.Structure):
    """revo_map_gain_info (include/revo_hip.h), 64 bytes: integer sums of a view_gain call."""
    _fields_ = [(k, C.c_uint64) for k in ("poses", "cells", "unknown", "unknown_free", "unknown_surface", "unknown_inside", "rays", "ray_hits")]


assert (C.sizeof(MapGainParams), C.sizeof(MapGain), C.sizeof(MapGainInfo)) == (32, 32, 64)


class MapTsdfCell(C.Structure):
    """revo_map_tsdf_cell (include/revo_hip.h), 8 bytes: the integer sum of a cell's truncated distances and its updates."""
    _fields_ = [("sum", C.c_int32), ("weight", C.c_uint32)]


class MapTsdfParams(C.Structure):
    """revo_map_tsdf_params (include/revo_hip.h), 16 bytes: the truncation distance in metres and whether the call accumulates."""
    _fields_ = [("trunc", C.c_float), ("accumulate", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class MapTsdfInfo(C.Structure):
    """revo_map_tsdf_info (include/revo_hip.h), 64 bytes: integer sums of a fuse call."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "updates", "cells_weighted", "cells_inside", "saturated")] + [("reserved", C.c_uint64 * 3)]


class MapMeshInfo(C.Structure):
    """revo_map_mesh_info (include/revo_hip.h), 64 bytes: the counts of a mesh call."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "valid", "inside", "cubes", "cubes_active", "vertices", "triangles", "reserved")]


assert (C.sizeof(MapTsdfCell), C.sizeof(MapTsdfParams), C.sizeof(MapTsdfInfo), C.sizeof(MapMeshInfo)) == (8, 16, 64, 64)


class MapTsdfColor(C.Structure):
    """revo_map_tsdf_color (include/revo_hip.h), 16 bytes: the sums of a cell's colour updates per channel and their number."""
    _fields_ = [("sum_b", C.c_uint32), ("sum_g", C.c_uint32), ("sum_r", C.c_uint32), ("weight", C.c_uint32)]


class MapTsdfColorInfo(C.Structure):
    """revo_map_tsdf_color_info (include/revo_hip.h), 32 bytes: the colour counters of a fuse call."""
    _fields_ = [("color_updates", C.c_uint64), ("cells_colored", C.c_uint64), ("reserved", C.c_uint64 * 2)]


assert (C.sizeof(MapTsdfColor), C.sizeof(MapTsdfColorInfo)) == (16, 32)


class MapTsdfRayParams(C.Structure):
    """revo_map_tsdf_ray_params (include/revo_hip.h), 16 bytes: the step in metres of camera depth (0: the voxel edge), the views a
    cell needs (0 counts as 1) and the samples of a ray at most (0: 4096)."""
    _fields_ = [("step", C.c_float), ("min_weight", C.c_uint32), ("max_steps", C.c_uint32), ("reserved", C.c_uint32)]


class MapTsdfRayInfo(C.Structure):
    """revo_map_tsdf_ray_info (include/revo_hip.h), 64 bytes: integer sums over the rays of a surface ray cast."""
    _fields_ = [(k, C.c_uint64) for k in ("rays", "hits", "range", "backface", "exhausted", "samples", "uncolored", "reserved")]


assert (C.sizeof(MapTsdfRayParams), C.sizeof(MapTsdfRayInfo)) == (16, 64)


class MapTsdfTrackParams(C.Structure):
    """revo_map_tsdf_track_params (include/revo_hip.h), 32 bytes: the gate in metres (0: trunc / 2), the pixel stride (0: 1, at most
    8), the views a cell needs (0 counts as 1) and the rotation centre."""
    _fields_ = [("max_dist", C.c_float), ("stride", C.c_uint32), ("min_weight", C.c_uint32), ("centre", C.c_float * 3), ("reserved", C.c_uint32 * 2)]


class MapTsdfTrackInfo(C.Structure):
    """revo_map_tsdf_track_info (include/revo_hip.h), 208 bytes, MapDfAlignInfo's layout: the 28 sums of tracking a depth frame against
    the TSDF surface at a pose (the upper triangle of sum J J^T, sum J e, sum e e with J = (g, u x g), g the interpolant's gradient), the
    exact counts and the inputs.  The gated pixels are considered - matched - skipped."""
    _fields_ = list(MapDfAlignInfo._fields_)


assert (C.sizeof(MapTsdfTrackParams), C.sizeof(MapTsdfTrackInfo)) == (32, 208)


class MapTsdfRecord(C.Structure):
    """revo_map_tsdf_record (include/revo_hip.h), 32 bytes: a cell that has left the surface volume's box -- its voxel index as the
    map's packed key and the bytes of its TSDF and colour cells (mapfile.TSDF_RECORD_DTYPE)."""
    _fields_ = [("key", C.c_uint64), ("sum", C.c_int32), ("weight", C.c_uint32), ("sum_b", C.c_uint32), ("sum_g", C.c_uint32),
                ("sum_r", C.c_uint32), ("color_weight", C.c_uint32)]


class MapTsdfShiftInfo(C.Structure):
    """revo_map_tsdf_shift_info (include/revo_hip.h), 64 bytes: the cells of a shift by what became of them."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "staying", "leaving", "records", "dropped")] + [("reserved", C.c_uint64 * 3)]


class MapTsdfRefillInfo(C.Structure):
    """revo_map_tsdf_refill_info (include/revo_hip.h), 32 bytes: the records of a refill by what became of them."""
    _fields_ = [(k, C.c_uint64) for k in ("records", "applied", "outside", "reserved")]


assert (C.sizeof(MapTsdfRecord), C.sizeof(MapTsdfShiftInfo), C.sizeof(MapTsdfRefillInfo)) == (32, 64, 32)


class MapTsdfUnfuseInfo(C.Structure):
    """revo_map_tsdf_unfuse_info (include/revo_hip.h), 64 bytes: what an unfuse took out and what is left; misfits > 0: it was
    refused and changed nothing."""
    _fields_ = [(k, C.c_uint64) for k in ("cells", "updates", "cells_weighted", "cells_inside", "misfits", "color_updates", "cells_colored", "reserved")]


assert C.sizeof(MapTsdfUnfuseInfo) == 64


class MapTsdfFuseJob(C.Structure):
    """revo_map_tsdf_fuse_job (include/revo_hip.h), 200 bytes: one (volume, view) of revo_map_tsdf_fuse_many -- the map that gives the
    voxel edge (NULL: the call's), the box, trunc (0: 4 voxel edges), the device volumes (color may be NULL), the view, a raw view's
    device colour image and the job's optional device records."""
    _fields_ = [("map", C.c_void_p), ("box", MapDfBox), ("trunc", C.c_float), ("reserved", C.c_uint32), ("tsdf", C.c_void_p), ("color", C.c_void_p),
                ("view", MapCarveView), ("bgr", C.c_void_p), ("info", C.c_void_p), ("color_info", C.c_void_p), ("view_info", C.c_void_p)]


class MapTsdfTrackJob(C.Structure):
    """revo_map_tsdf_track_job (include/revo_hip.h), 200 bytes: one (volume, frame) of revo_map_tsdf_track_eval_many and
    revo_map_tsdf_track_many -- the map that gives the voxel edge, the box, the volume's trunc, the poses of the evaluation, the device
    volume, the frame, the parameters and the host poses (the evaluation's n_poses 4x4, or the loop's T_init)."""
    _fields_ = [("map", C.c_void_p), ("box", MapDfBox), ("trunc", C.c_float), ("n_poses", C.c_int32), ("tsdf", C.c_void_p), ("frame", MapCarveView),
                ("prm", MapTsdfTrackParams), ("poses", C.c_void_p)]


class MapTsdfTrackResult(C.Structure):
    """revo_map_tsdf_track_result (include/revo_hip.h), 288 bytes: what revo_map_tsdf_track gives for one job of revo_map_tsdf_track_many,
    and the records its loop took."""
    _fields_ = [("T", C.c_float * 16), ("info", MapTsdfTrackInfo), ("iterations", C.c_int32), ("status", C.c_int32), ("evaluations", C.c_int32),
                ("reserved", C.c_int32)]


assert (C.sizeof(MapTsdfFuseJob), C.sizeof(MapTsdfTrackJob), C.sizeof(MapTsdfTrackResult)) == (200, 200, 288)


class MapTsdfUnfuseJob(C.Structure):
    """revo_map_tsdf_unfuse_job (include/revo_hip.h), 192 bytes: one (volume, view) of revo_map_tsdf_unfuse_many -- MapTsdfFuseJob's
    members with the unfuse's meaning: trunc is what the view was fused with, info a revo_map_tsdf_unfuse_info on the device."""
    _fields_ = [("map", C.c_void_p), ("box", MapDfBox), ("trunc", C.c_float), ("reserved", C.c_uint32), ("tsdf", C.c_void_p), ("color", C.c_void_p),
                ("view", MapCarveView), ("bgr", C.c_void_p), ("info", C.c_void_p), ("view_info", C.c_void_p)]


class MapTsdfUnfuseResult(C.Structure):
    """revo_map_tsdf_unfuse_result (include/revo_hip.h), 80 bytes: a job's info and its status -- 0, or -1 (REVO_ERR_INVALID_ARG) for a
    job that had a misfit and changed nothing."""
    _fields_ = [("info", MapTsdfUnfuseInfo), ("status", C.c_int32), ("reserved", C.c_int32 * 3)]


assert (C.sizeof(MapTsdfUnfuseJob), C.sizeof(MapTsdfUnfuseResult)) == (192, 80)


class MapTsdfRayJob(C.Structure):
    """revo_map_tsdf_ray_job (include/revo_hip.h), 120 bytes: one (volume, views) of revo_map_tsdf_raycast_many -- the map that gives the
    voxel edge (NULL: the call's), the box, the parameters by value (all zero: the defaults), the device volumes (color may be NULL),
    1 .. 64 views in a host array, host arrays of the views' device images (normal and bgr may be NULL), and the job's optional
    device hit words and info record.  Jobs may share a volume."""
    _fields_ = [("map", C.c_void_p), ("box", MapDfBox), ("prm", MapTsdfRayParams), ("tsdf", C.c_void_p), ("color", C.c_void_p), ("n_views", C.c_int32),
                ("reserved", C.c_uint32), ("views", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("bgr", C.c_void_p), ("hits", C.c_void_p),
                ("info", C.c_void_p)]


assert C.sizeof(MapTsdfRayJob) == 120


class MultiSurface(C.Structure):
    """revo_vo_multi_surface (include/revo_hip.h), 120 bytes: the surface of one stream of revo_vo_multi -- the map that gives the voxel
    edge, the box, trunc (0: 4 voxel edges), whether each keyframe is tracked before it is fused, the caller-owned device volumes
    (color may be NULL), and the tracking parameters and options."""
    _fields_ = [("map", C.c_void_p), ("box", MapDfBox), ("trunc", C.c_float), ("track", C.c_int32), ("tsdf", C.c_void_p), ("color", C.c_void_p),
                ("track_prm", MapTsdfTrackParams), ("track_opts", MapAlignOpts)]


class MultiSurfaceReport(C.Structure):
    """revo_vo_multi_surface_report (include/revo_hip.h), 408 bytes: a stream's last keyframe as its surface saw it."""
    _fields_ = [("timestamp", C.c_double), ("T_w_kf", C.c_float * 16), ("T_fused", C.c_float * 16), ("track", MapTsdfTrackInfo), ("iterations", C.c_int32),
                ("status", C.c_int32), ("tracked", C.c_int32), ("fused", C.c_int32), ("view_info", MapCarveViewInfo), ("keyframes_fused", C.c_uint64),
                ("keyframes_skipped", C.c_uint64)]


assert (C.sizeof(MultiSurface), C.sizeof(MultiSurfaceReport)) == (120, 408)


class MultiSurfaceWindowReport(C.Structure):
    """revo_vo_multi_surface_window_report (include/revo_hip.h), 104 bytes: a stream's surface window as it stands -- its size, the views
    held, the evictions so far, and the last eviction's keyframe time stamp and result (status -1: refused, the view stayed in the
    volumes and was forgotten)."""
    _fields_ = [("window", C.c_int32), ("held", C.c_int32), ("evictions", C.c_uint64), ("evicted_timestamp", C.c_double), ("evicted", MapTsdfUnfuseResult)]


assert C.sizeof(MultiSurfaceWindowReport) == 104


class PairIn(C.Structure):
    """revo_pair_in (include/revo_hip.h): one frame-pair in host memory."""
    _fields_ = [
        ("ref_bgr", C.c_void_p), ("ref_bgr_stride", C.c_size_t),
        ("ref_depth", C.c_void_p), ("ref_depth_stride", C.c_size_t),
        ("cur_bgr", C.c_void_p), ("cur_bgr_stride", C.c_size_t),
        ("cur_depth", C.c_void_p), ("cur_depth_stride", C.c_size_t),
        ("R_init", C.c_float * 9), ("T_init", C.c_float * 3), ("use_init", C.c_int32),
    ]
