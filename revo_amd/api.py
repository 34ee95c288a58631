"""Host-side mirror of the reference's hot-path classes over the C ABI.

Same names, argument meaning and error behaviour as the reference so the parity
tests read like tests of the reference itself:

  CameraPyr        datastructures/camerapyr.h:113-193   (owns the device context)
  ImgPyramidRGBD   datastructures/imgpyramidrgbd.h:27-250
  Optimizer        system/optimizer.h:114-186
  TrackerNew       system/tracker.h:56-105
  BatchTracker     new: B independent frame-pairs resident in HBM

numpy matrices are ordinary row-major views (R[i, j]); the column-major
conversion the C ABI wants (Eigen storage) happens here.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import RevoError, check, f32p, i32p, u8p, u16p, vp
from .settings import (ImgPyramidSettings, OptimizerSettings, TrackerSettings, ResidualInfo, PairResult, PairInfo, PairIn, MapInfo, MapView, MapAlignParams, MapAlignInfo, MapAlignOpts, MapNormalsParams, MapPlaneInfo, MapPoseInfo, MapCarveView, MapCarveParams, MapCarveInfo, MapCarveViewInfo, MapRayParams, MapRayInfo, MapDfBox, MapDfInfo, MapDfAlignInfo, MapPlanSeed, MapPlanInfo, MapPlanPath, MapObserveParams, MapObserveInfo, MapKnownInfo, MapGainParams, MapGain, MapGainInfo, MapTsdfParams, MapTsdfInfo, MapTsdfColorInfo, MapMeshInfo, MapTsdfRayParams, MapTsdfTrackInfo, MapTsdfShiftInfo, MapTsdfRefillInfo, MapTsdfUnfuseInfo, MapTsdfTrackParams, MapTsdfRayInfo, MapTsdfFuseJob, MapTsdfUnfuseJob, MapTsdfRayJob, MapTsdfUnfuseResult, MapTsdfTrackJob, MapTsdfTrackResult,
                       MAX_LEVELS, PLANE_GRAY, PLANE_DEPTH, PLANE_EDGES, PLANE_EDGES_ORIG, PLANE_DT,
                       PLANE_GRADTABLE, PLANE_EDGES3D, PLANE_HIST, PLANE_EDGES3D_TILED, TRACKER_STATE_OK, TRACKER_STATE_NEW_KF)


def _p(a, t):
    return a.ctypes.data_as(t)


def _cm3(R):
    return np.ascontiguousarray(np.asarray(R, np.float32).T).reshape(9)


def _cm4(M):
    return np.ascontiguousarray(np.asarray(M, np.float32).T).reshape(16)


class Camera:
    """camerapyr.h:90-111"""

    def __init__(self, fx, fy, cx, cy, width, height):
        self.fx, self.fy, self.cx, self.cy = fx, fy, cx, cy
        self.width, self.height = int(width), int(height)
        self.area = self.width * self.height

    def returnSize(self):
        return (self.width, self.height)


class CameraPyr:
    """camerapyr.h:113-193.  Also owns the HIP context (device, stream, HBM pools)."""

    def __init__(self, settingsPyr, device=0, optimizerSettings=None, trackerSettings=None, exact_sums=False):
        self.settings = settingsPyr
        self.device = int(device)
        self._h = vp()
        opt = optimizerSettings or OptimizerSettings()
        trk = trackerSettings or TrackerSettings()
        check(_lib.lib().revo_ctx_create(device, C.byref(settingsPyr), C.byref(opt), C.byref(trk), C.byref(self._h)))
        if exact_sums:
            self.setExactSums(True)
        self.camPyr = []
        for lvl in range(settingsPyr.nLevels()):
            out = np.empty(6, np.float32)
            check(_lib.lib().revo_ctx_camera(self._h, lvl, _p(out, f32p)))
            self.camPyr.append(Camera(*[float(x) for x in out[:4]], out[4], out[5]))

    def setExactSums(self, on):
        """Exact-sums mode of the tracker (revo_ctx_set_exact_sums): applies from the next tracker
        launch of this context."""
        check(_lib.lib().revo_ctx_set_exact_sums(self._h, 1 if on else 0))

    @property
    def exact_sums(self):
        return bool(_lib.lib().revo_ctx_exact_sums(self._h))

    def size(self):
        return len(self.camPyr)

    def at(self, lvl):
        return self.camPyr[lvl]

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().revo_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DT = {PLANE_GRAY: (np.uint8, 1), PLANE_DEPTH: (np.float32, 1), PLANE_EDGES: (np.uint8, 1),
       PLANE_EDGES_ORIG: (np.uint8, 1), PLANE_DT: (np.float32, 1), PLANE_GRADTABLE: (np.float32, 4),
       PLANE_EDGES3D: (np.float32, 4), PLANE_HIST: (np.uint8, 1), PLANE_EDGES3D_TILED: (np.float32, 4)}


class ImgPyramidRGBD:
    """imgpyramidrgbd.h:27-250.  fullResRgb is BGR8 [H,W,3], fullResDepth float32 metres [H,W]
    (or uint16 raw + depth_scale_factor, fusing iowrapperRGBD.cpp:326-327)."""

    def __init__(self, settings, cameraPyr, fullResRgb=None, fullResDepth=None, timestamp=0.0,
                 depth_scale_factor=None, _handle=None, _owned=True):
        self.mSettings = settings
        self.cameraPyr = cameraPyr
        self.frameId = 0
        self._owned = _owned
        self._T_w_f = np.eye(4, dtype=np.float32)
        if _handle is not None:
            self._h = _handle
            return
        bgr = np.ascontiguousarray(fullResRgb, np.uint8)
        h, w = bgr.shape[:2]
        if bgr.shape != (h, w, 3) or np.shape(fullResDepth) != (h, w) or (w, h) != (settings.width, settings.height):
            raise ValueError("image size does not match the settings")
        self._h = vp()
        L = _lib.lib()
        if depth_scale_factor is not None:
            d = np.ascontiguousarray(fullResDepth, np.uint16)
            check(L.revo_pyramid_create_u16(cameraPyr._h, _p(bgr, u8p), w * 3, _p(d, u16p), w * 2,
                                            float(depth_scale_factor), float(timestamp), C.byref(self._h)))
        else:
            d = np.ascontiguousarray(fullResDepth, np.float32)
            check(L.revo_pyramid_create(cameraPyr._h, _p(bgr, u8p), w * 3, _p(d, f32p), w * 4, float(timestamp),
                                        C.byref(self._h)))

    def __del__(self):
        try:
            if self._owned and getattr(self, "_h", None):
                _lib.lib().revo_pyramid_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- keyframe promotion (imgpyramidrgbd.cpp:231-252)
    def makeKeyframe(self):
        check(_lib.lib().revo_pyramid_make_keyframe(self._h))

    def _read(self, what, lvl):
        dt, k = _DT[what]
        n = C.c_size_t()
        check(_lib.lib().revo_pyramid_read(self._h, what, lvl, None, 0, C.byref(n)))
        buf = np.empty((n.value, k) if k > 1 else (n.value,), dt)
        if n.value:
            check(_lib.lib().revo_pyramid_read(self._h, what, lvl, buf.ctypes.data_as(vp), buf.nbytes, C.byref(n)))
        w, h = self.mSettings.level_size(lvl)
        if what in (PLANE_EDGES3D, PLANE_EDGES3D_TILED) or n.value == 0:
            return buf
        if what == PLANE_HIST:
            p = self.mSettings.hist_patch[lvl]
            return buf.reshape(h // p, w // p)
        return buf.reshape((h, w, 4) if k > 1 else (h, w))

    # -- accessors (imgpyramidrgbd.h:45-117)
    def returnK(self, lvl):
        cam = self.cameraPyr.at(lvl)
        K = np.eye(3, dtype=np.float32)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = cam.fx, cam.fy, cam.cx, cam.cy
        return K

    def returnDistTransform(self, lvl):
        return self._read(PLANE_DT, lvl)

    def returnEdges(self, lvl):
        return self._read(PLANE_EDGES, lvl)

    def returnOrigEdges(self, lvl):
        return self._read(PLANE_EDGES_ORIG, lvl)

    def return3DEdges(self, lvl):
        """N x 4 float32 rows (X,Y,Z,1) == the columns of the reference's 4xN Eigen::MatrixXf."""
        return self._read(PLANE_EDGES3D, lvl)

    def edges3DTiled(self, lvl):
        """The same N points as return3DEdges in the order the tracker reads them: 32x32-pixel tiles in raster order,
        row-major inside a tile (what the per-frame build writes; not a reference accessor)."""
        return self._read(PLANE_EDGES3D_TILED, lvl)

    def generateColoredPcl(self, lvl, densePcl=False):
        """imgpyramidrgbd.cpp:279-327: N x 8 float32 rows (X,Y,Z,1,r,g,b,1), colours in [0,1] ==
        the columns of the reference's 8xN clrPcl; densePcl: every usable-depth pixel, else edges."""
        w, h = self.mSettings.level_size(lvl)
        buf = np.empty((w * h, 8), np.float32)
        n = C.c_size_t()
        check(_lib.lib().revo_pyramid_colored_pcl(self._h, lvl, int(bool(densePcl)), buf.ctypes.data_as(_lib.f32p),
                                                  w * h, C.byref(n)))
        return buf[:n.value].copy()

    def returnDepth(self, lvl):
        return self._read(PLANE_DEPTH, lvl)

    def returnGray(self, lvl):
        return self._read(PLANE_GRAY, lvl)

    def returnOptimizationStructure(self, lvl):
        return self._read(PLANE_GRADTABLE, lvl)

    def returnHist(self, lvl):
        return self._read(PLANE_HIST, lvl)

    def returnTimestamp(self):
        return _lib.lib().revo_pyramid_timestamp(self._h)

    def returnMaxLvl(self):
        return self.mSettings.pyr_max_lvl

    def returnMinLvl(self):
        return self.mSettings.pyr_min_lvl

    def isKeyframe(self):
        return bool(_lib.lib().revo_pyramid_is_keyframe(self._h))

    # -- pose bookkeeping (imgpyramidrgbd.h:126-151): plain host state
    def setTwf(self, T):
        self._T_w_f = np.array(T, np.float32).reshape(4, 4)

    def getTransKFtoWorld(self):
        return self._T_w_f

    def prepareKfForStorage(self):  # imgpyramidrgbd.h:156-169: effectively a no-op in the reference
        return None


class VoxelMap:
    """World-frame voxel map fused on the device (revo_map_* in include/revo_hip.h): what MapDrawer shows, one coloured point
    per voxel of edge `voxel` metres.  integrate(pyr, T_w) adds the level-0 points of pyr.generateColoredPcl(0, dense) at the
    keyframe pose T_w (4x4, keyframe -> world); the map depends on those points and poses only, not on the order, batching or
    driver of the integrations.  The table grows on the device; max_voxels is a hard bound (REVO_ERR_CAPACITY: the keyframe
    is not integrated, the map is unchanged)."""

    def __init__(self, cameraPyr, voxel, dense=False, max_voxels=1 << 24, initial_voxels=1 << 16):
        self.cameraPyr = cameraPyr  # the map lives on this context
        self._h = vp()
        check(_lib.lib().revo_map_create(cameraPyr._h, C.c_float(voxel), 1 if dense else 0, int(initial_voxels),
                                         int(max_voxels), C.byref(self._h)))
        v, d = C.c_float(), C.c_int()
        check(_lib.lib().revo_map_voxel_size(self._h, C.byref(v), C.byref(d)))
        self._voxel, self._dense = float(v.value), bool(d.value)

    @property
    def voxel(self):
        """The voxel edge in metres as the map holds it (float32)."""
        return self._voxel

    @property
    def dense(self):
        return self._dense

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().revo_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def integrate(self, pyr, T_w):
        """Asynchronous on the device; the pyramid may go right after the call."""
        check(_lib.lib().revo_map_integrate(self._h, pyr._h, _p(_cm4(T_w), f32p)))

    def integrate_many(self, pyrs, T_ws):
        """Several keyframes in one launch: the same map as integrating them one by one, in any order."""
        pyrs = list(pyrs)
        hs = (vp * max(1, len(pyrs)))(*[p._h.value for p in pyrs])
        T = np.ascontiguousarray(np.concatenate([_cm4(M) for M in T_ws]) if pyrs else np.zeros(16, np.float32))
        check(_lib.lib().revo_map_integrate_many(self._h, len(pyrs), hs, _p(T, f32p)))

    def clear(self):
        check(_lib.lib().revo_map_clear(self._h))

    def info(self):
        i = MapInfo()
        check(_lib.lib().revo_map_info(self._h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in MapInfo._fields_}

    def points(self, min_count=1):
        """(N x 3 float32 xyz, N x 3 uint8 RGB, N uint32 count) in ascending packed-key order."""
        L = _lib.lib()
        n = C.c_size_t()
        check(L.revo_map_extract(self._h, int(min_count), None, None, None, 0, C.byref(n)))
        xyz = np.empty((n.value, 3), np.float32)
        rgb = np.empty((n.value, 3), np.uint8)
        cnt = np.empty(n.value, np.uint32)
        m = C.c_size_t()
        check(L.revo_map_extract(self._h, int(min_count), _p(xyz, f32p), _p(rgb, u8p), cnt.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 n.value, C.byref(m)))
        return xyz[:m.value], rgb[:m.value], cnt[:m.value]

    def save_ply(self, path, min_count=1, normals=False):
        """Binary little-endian PLY, one vertex per voxel in key order: xyz float32, RGB uchar, `count` uint32; with
        normals=True also nx ny nz float32 (normals(min_count) at its defaults; (0, 0, 0) where there is no valid normal)."""
        from . import ply
        if normals:
            return ply.write_voxel_ply_normals(path, *self.points(min_count), self.normals(min_count)[1])
        return ply.write_voxel_ply(path, *self.points(min_count))

    # -- the map as data (revo_map_export_raw / revo_map_merge*; records and files: revo_amd/mapfile.py)
    def export_raw(self):
        """Every voxel's integer sums as a structured array of mapfile.RAW_DTYPE in ascending key order: the canonical form,
        equal maps give equal bytes."""
        from . import mapfile
        L = _lib.lib()
        n = C.c_size_t()
        check(L.revo_map_export_raw(self._h, None, 0, C.byref(n), 0))
        rec = np.zeros(n.value, mapfile.RAW_DTYPE)
        m = C.c_size_t()
        check(L.revo_map_export_raw(self._h, rec.ctypes.data_as(vp) if n.value else None, n.value, C.byref(m), 0))
        return rec[:m.value]

    @staticmethod
    def _raw_tensor(t):
        if not (t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.uint8"):
            raise ValueError("voxel records on the device are a contiguous uint8 device tensor, 64 bytes per record")
        return t.numel() // 64

    def export_raw_into(self, d_tensor):
        """export_raw() into a torch uint8 device tensor (64 bytes per record, 16-byte aligned, on the map's device), in
        unspecified order; returns the number of records written.  Waits for the map."""
        import torch
        cap = self._raw_tensor(d_tensor)
        torch.cuda.current_stream(d_tensor.device).synchronize()  # the tensor's earlier use is over before the tracker stream writes
        n = C.c_size_t()
        check(_lib.lib().revo_map_export_raw(self._h, vp(d_tensor.data_ptr()), cap, C.byref(n), 1))
        return n.value

    def merge_raw(self, records, points_dropped=0, keyframes=0, n=None):
        """Adds voxel records to the map: a mapfile.RAW_DTYPE array (or its bytes) from host memory, or a torch uint8 device
        tensor (its first n records; all of them by default).  Keys may repeat: several exports go in one call, concatenated.
        All or nothing (REVO_ERR_CAPACITY past max_voxels, REVO_ERR_INVALID_ARG for a record with count 0 or key bit 63)."""
        L = _lib.lib()
        if hasattr(records, "data_ptr"):
            import torch
            have = self._raw_tensor(records)
            n = have if n is None else int(n)
            if n < 0 or n > have:
                raise ValueError("the tensor holds %d records" % have)
            torch.cuda.current_stream(records.device).synchronize()  # the tensor is written before the tracker stream reads it
            check(L.revo_map_merge_raw(self._h, vp(records.data_ptr()), n, 1, int(points_dropped), int(keyframes)))
            self.sync()  # the tensor may go
            return
        from . import mapfile
        rec = mapfile.as_records(records)
        if n is not None:
            rec = rec[:int(n)]
        check(L.revo_map_merge_raw(self._h, rec.ctypes.data_as(vp) if len(rec) else None, len(rec), 0, int(points_dropped),
                                   int(keyframes)))

    def merge(self, other):
        """Adds every voxel of `other` (same voxel edge, same device) with its points_dropped and keyframes, straight from its
        table on the device; `other` is unchanged.  The result is the map one handle would have built from both maps' keyframes."""
        check(_lib.lib().revo_map_merge(self._h, other._h))

    # -- taking voxels out again (revo_map_subtract*)
    def subtract_raw(self, records, points_dropped=0, keyframes=0, n=None):
        """The exact inverse of merge_raw: the records' sums leave their voxels, and a voxel whose count reaches 0 is gone.
        Takes what merge_raw takes.  All or nothing (REVO_ERR_INVALID_ARG, the map unchanged bit for bit): a record with count 0
        or key bit 63, a key the map does not hold, more than a voxel has, a voxel left at count 0 with another sum, or more
        points_dropped or keyframes than the map counts.  Records that fit but never were part of the map cannot be told
        apart: that is the caller's responsibility.  Waits for the device."""
        L = _lib.lib()
        if hasattr(records, "data_ptr"):
            import torch
            have = self._raw_tensor(records)
            n = have if n is None else int(n)
            if n < 0 or n > have:
                raise ValueError("the tensor holds %d records" % have)
            torch.cuda.current_stream(records.device).synchronize()  # the tensor is written before the tracker stream reads it
            check(L.revo_map_subtract_raw(self._h, vp(records.data_ptr()), n, 1, int(points_dropped), int(keyframes)))
            return
        from . import mapfile
        rec = mapfile.as_records(records)
        if n is not None:
            rec = rec[:int(n)]
        check(L.revo_map_subtract_raw(self._h, rec.ctypes.data_as(vp) if len(rec) else None, len(rec), 0, int(points_dropped),
                                      int(keyframes)))

    def subtract(self, other):
        """The inverse of merge(other): every voxel of `other` (same voxel edge, same device) leaves the map with its
        points_dropped and keyframes, straight from its table on the device; `other` is unchanged.  All or nothing."""
        check(_lib.lib().revo_map_subtract(self._h, other._h))

    def save(self, path):
        """The map as a .rvm file (mapfile): header and canonical records.  Equal maps give equal files."""
        from . import mapfile
        rec = self.export_raw()
        info = self.info()
        return mapfile.write(path, mapfile.make_header(self.voxel, self.dense, rec, info["points_dropped"], info["keyframes"]), rec)

    @classmethod
    def load(cls, cameraPyr, path, max_voxels=1 << 24, initial_voxels=1 << 16):
        """A map on cameraPyr's context holding what the .rvm file holds: voxels, counters, voxel edge and cloud mode.
        Integrations and merges continue it exactly as if it had never left the device."""
        from . import mapfile
        header, rec = mapfile.read(path)
        m = cls(cameraPyr, header["voxel"], dense=bool(header["dense"]), max_voxels=max_voxels,
                initial_voxels=max(int(initial_voxels), len(rec)))
        m.merge_raw(rec, header["points_dropped"], header["keyframes"])
        return m

    # -- registration (revo_map_coarsen / revo_map_align*)
    def coarsen(self, shift, max_voxels=1 << 24):
        """A new map on the same context with a voxel edge 2^shift times as long, holding this map's sums: byte for byte the
        map built at that edge from the same keyframes (while no point was dropped for key range).  This map is unchanged."""
        out = VoxelMap(self.cameraPyr, float(np.ldexp(np.float32(self.voxel), int(shift))), dense=self.dense, max_voxels=max_voxels,
                       initial_voxels=max(1, self.info()["voxels"]))
        check(_lib.lib().revo_map_coarsen(out._h, self._h, int(shift)))
        return out

    def _align_params(self, max_dist, min_count_dst, min_count_src, centre):
        p = MapAlignParams()
        p.max_dist = self.voxel if max_dist is None else float(max_dist)
        p.min_count_dst, p.min_count_src = int(min_count_dst), int(min_count_src)
        p.centre[:] = [float(x) for x in np.asarray(centre, np.float32).reshape(3)]
        return p

    def align_eval(self, src, poses, max_dist=None, min_count_dst=1, min_count_src=1, centre=(0.0, 0.0, 0.0), d_out=None):
        """The registration sums of `src` against this map (the destination) at each pose (4x4, source -> destination frame; one
        pose or a list / (n, 4, 4) array): MapAlignInfo records, all from one launch.  max_dist defaults to this map's voxel
        edge.  d_out: a torch uint8 device tensor of n x 160 bytes takes the records instead (returns None).  Waits."""
        T = np.asarray(poses, np.float32)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        n = len(T)
        flat = np.ascontiguousarray(np.concatenate([_cm4(M) for M in T]))
        p = self._align_params(max_dist, min_count_dst, min_count_src, centre)
        if d_out is not None:
            if not (d_out.is_cuda and d_out.is_contiguous() and d_out.numel() * d_out.element_size() >= n * C.sizeof(MapAlignInfo)):
                raise ValueError("d_out must be a contiguous device tensor of n x %d bytes" % C.sizeof(MapAlignInfo))
            import torch
            torch.cuda.current_stream(d_out.device).synchronize()
            check(_lib.lib().revo_map_align_eval(self._h, src._h, n, _p(flat, f32p), C.byref(p), vp(d_out.data_ptr()), 1))
            return None
        out = (MapAlignInfo * n)()
        check(_lib.lib().revo_map_align_eval(self._h, src._h, n, _p(flat, f32p), C.byref(p), C.cast(out, vp), 0))
        return out[0] if single else list(out)

    def align(self, src, T_init=None, max_dist=None, min_count_dst=1, min_count_src=1, centre=(0.0, 0.0, 0.0), max_iters=30,
              eps_t=1e-6, eps_r=1e-6, min_matched=12):
        """Point-to-point ICP of `src` onto this map from T_init (4x4, source -> destination; identity by default): Gauss-Newton
        on the host over align_eval's records.  -> dict: T (4x4 float32), info (the MapAlignInfo at T), iterations, status
        (settings.ALIGN_CONVERGED / ALIGN_ITER_LIMIT / ALIGN_LOST), cov (6x6, sigma2 H^-1 with sigma2 = S[15] / (3 matched - 6);
        None when H cannot be inverted) and sigma2."""
        p = self._align_params(max_dist, min_count_dst, min_count_src, centre)
        o = MapAlignOpts(int(max_iters), 0, float(eps_t), float(eps_r), int(min_matched))
        T0 = _cm4(np.eye(4) if T_init is None else T_init)
        T1 = np.zeros(16, np.float32)
        info, it, st = MapAlignInfo(), C.c_int32(), C.c_int32()
        check(_lib.lib().revo_map_align(self._h, src._h, _p(T0, f32p), C.byref(p), C.byref(o), _p(T1, f32p), C.byref(info),
                                        C.byref(it), C.byref(st)))
        cov, s2 = align_covariance(info)
        return {"T": T1.reshape(4, 4).T.copy(), "info": info, "iterations": it.value, "status": st.value, "cov": cov, "sigma2": s2}

    # -- point-to-plane registration (revo_map_normals / revo_map_align_plane*)
    @staticmethod
    def _normals_params(min_count, min_neighbours, planarity, min_spread):
        return MapNormalsParams(max(1, int(min_count)), int(min_neighbours), float(planarity), float(min_spread))

    def normals(self, min_count=1, min_neighbours=5, planarity=0.1, min_spread=0.1):
        """Per voxel of points(min_count), in its order: (xyz N x 3 float32, normal N x 3 float32 -- (0, 0, 0) where the
        neighbourhood is no plane --, lambda N x 3 float32 ascending, neighbours N uint32).  A pure function of the map."""
        L = _lib.lib()
        p = MapNormalsParams(int(min_count), int(min_neighbours), float(planarity), float(min_spread))
        n = C.c_size_t()
        check(L.revo_map_normals(self._h, C.byref(p), None, None, None, None, 0, C.byref(n)))
        xyz, nrm, lam = (np.empty((n.value, 3), np.float32) for _ in range(3))
        nb = np.empty(n.value, np.uint32)
        m = C.c_size_t()
        check(L.revo_map_normals(self._h, C.byref(p), _p(xyz, f32p), _p(nrm, f32p), _p(lam, f32p), nb.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 n.value, C.byref(m)))
        return xyz[:m.value], nrm[:m.value], lam[:m.value], nb[:m.value]

    def align_plane_eval(self, src, poses, max_dist=None, min_count_dst=1, min_count_src=1, centre=(0.0, 0.0, 0.0), min_neighbours=5,
                         planarity=0.1, min_spread=0.1, d_out=None):
        """align_eval for the point-to-plane metric: MapPlaneInfo records (208 bytes), all from one launch; only destination
        voxels with a valid normal (min_neighbours, planarity, min_spread: see normals) are matched."""
        T = np.asarray(poses, np.float32)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        n = len(T)
        flat = np.ascontiguousarray(np.concatenate([_cm4(M) for M in T]))
        p = self._align_params(max_dist, min_count_dst, min_count_src, centre)
        q = self._normals_params(min_count_dst, min_neighbours, planarity, min_spread)
        if d_out is not None:
            if not (d_out.is_cuda and d_out.is_contiguous() and d_out.numel() * d_out.element_size() >= n * C.sizeof(MapPlaneInfo)):
                raise ValueError("d_out must be a contiguous device tensor of n x %d bytes" % C.sizeof(MapPlaneInfo))
            import torch
            torch.cuda.current_stream(d_out.device).synchronize()
            check(_lib.lib().revo_map_align_plane_eval(self._h, src._h, n, _p(flat, f32p), C.byref(p), C.byref(q), vp(d_out.data_ptr()), 1))
            return None
        out = (MapPlaneInfo * n)()
        check(_lib.lib().revo_map_align_plane_eval(self._h, src._h, n, _p(flat, f32p), C.byref(p), C.byref(q), C.cast(out, vp), 0))
        return out[0] if single else list(out)

    def align_plane(self, src, T_init=None, max_dist=None, min_count_dst=1, min_count_src=1, centre=(0.0, 0.0, 0.0), max_iters=30,
                    eps_t=1e-6, eps_r=1e-6, min_matched=12, min_neighbours=5, planarity=0.1, min_spread=0.1):
        """align() with the point-to-plane metric over align_plane_eval's records: the same loop, options and statuses.
        -> dict as align's, info a MapPlaneInfo, cov = sigma2 H^-1 with sigma2 = S[27] / (matched - 6)."""
        p = self._align_params(max_dist, min_count_dst, min_count_src, centre)
        q = self._normals_params(min_count_dst, min_neighbours, planarity, min_spread)
        o = MapAlignOpts(int(max_iters), 0, float(eps_t), float(eps_r), int(min_matched))
        T0 = _cm4(np.eye(4) if T_init is None else T_init)
        T1 = np.zeros(16, np.float32)
        info, it, st = MapPlaneInfo(), C.c_int32(), C.c_int32()
        check(_lib.lib().revo_map_align_plane(self._h, src._h, _p(T0, f32p), C.byref(p), C.byref(q), C.byref(o), _p(T1, f32p),
                                              C.byref(info), C.byref(it), C.byref(st)))
        cov, s2 = align_plane_covariance(info)
        return {"T": T1.reshape(4, 4).T.copy(), "info": info, "iterations": it.value, "status": st.value, "cov": cov, "sigma2": s2}

    # -- maps under a pose (revo_map_pose_raw / revo_map_merge_posed / revo_map_subtract_posed)
    @staticmethod
    def _pose_info(i):
        return {k: int(getattr(i, k)) for k, _ in MapPoseInfo._fields_ if k != "reserved"}

    def pose_raw(self, T, voxel=None, min_count=1, device=False):
        """This map seen under the pose T (4x4, this map's frame -> the destination's) at the destination edge `voxel` (this
        map's by default): per voxel with count >= min_count its count and colour sums at the moved mean point.
        -> (records, info).  device=False: a mapfile.RAW_DTYPE array in the canonical form (ascending keys, equal keys summed):
        what an empty map of that edge exports after merge_posed.  device=True: a torch uint8 device tensor, one 64-byte record
        per moved voxel in unspecified order, keys may repeat -- what merge_raw / subtract_raw take.  info: a dict of
        voxels_in, voxels_moved, voxels_dropped, voxels_skipped, points_moved, points_dropped, points_skipped."""
        from . import mapfile
        L = _lib.lib()
        v = C.c_float(self.voxel if voxel is None else float(voxel))
        Tc = _cm4(T)
        n, i = C.c_size_t(), MapPoseInfo()
        if device:
            import torch
            cap = self.info()["voxels"]
            buf = torch.empty(64 * max(cap, 1), dtype=torch.uint8, device="cuda:%d" % self.cameraPyr.device)
            check(L.revo_map_pose_raw(self._h, _p(Tc, f32p), v, int(min_count), vp(buf.data_ptr()), cap, C.byref(n), 1, C.byref(i)))
            self.sync()  # the records are written
            return buf[:64 * n.value], self._pose_info(i)
        cap = self.info()["voxels"]  # the canonical form has at most one record per source voxel
        rec = np.zeros(cap, mapfile.RAW_DTYPE)
        check(L.revo_map_pose_raw(self._h, _p(Tc, f32p), v, int(min_count), rec.ctypes.data_as(vp) if cap else None, cap,
                                  C.byref(n), 0, C.byref(i)))
        return rec[:n.value], self._pose_info(i)

    def merge_posed(self, src, T, min_count=1):
        """Adds `src` (same device; the voxel edges and cloud modes may differ) as it lies under T (4x4, source -> this map's
        frame): merge_raw of src.pose_raw(T, self.voxel, min_count) with src's points_dropped plus the move's and src's
        keyframes, made on the device.  All or nothing on max_voxels (REVO_ERR_CAPACITY).  `src` is unchanged.  -> the info dict."""
        i = MapPoseInfo()
        check(_lib.lib().revo_map_merge_posed(self._h, src._h, _p(_cm4(T), f32p), int(min_count), C.byref(i)))
        return self._pose_info(i)

    def subtract_posed(self, src, T, min_count=1):
        """The exact inverse of merge_posed(src, T, min_count): afterwards this map is byte for byte what it was before it,
        counters included.  Refused (REVO_ERR_INVALID_ARG, nothing changed) as subtract_raw refuses.  -> the info dict."""
        i = MapPoseInfo()
        check(_lib.lib().revo_map_subtract_posed(self._h, src._h, _p(_cm4(T), f32p), int(min_count), C.byref(i)))
        return self._pose_info(i)

    def repose(self, src, T_old, T_new, min_count=1):
        """A submap follows its corrected pose: subtract_posed(src, T_old) then merge_posed(src, T_new).  If the merge is
        refused, src is merged back at T_old -- which restores this map exactly -- and the error is raised.
        -> (info of the subtraction, info of the merge)."""
        out = self.subtract_posed(src, T_old, min_count)
        try:
            return out, self.merge_posed(src, T_new, min_count)
        except RevoError:
            self.merge_posed(src, T_old, min_count)
            raise

    # -- free-space carving (revo_map_carve_eval / revo_map_carve)
    @staticmethod
    def _carve_views(views):
        """-> (the revo_map_carve_view array of a carve or observe call, device_in, what keeps the images alive)."""
        views = list(views)
        n = len(views)
        if not 1 <= n <= 64:
            raise ValueError("a carve takes 1 .. 64 views")
        cv = (MapCarveView * n)()
        keep, on_device = [], []
        for v, view in zip(cv, views):
            src, T = view[0], view[1]
            k = view[2] if len(view) > 2 and view[2] is not None else (0.0,) * 6
            if isinstance(src, ImgPyramidRGBD):
                v.kf = src._h
            elif hasattr(src, "data_ptr"):
                if not (src.is_cuda and src.is_contiguous() and str(src.dtype) == "torch.float32" and src.dim() == 2):
                    raise ValueError("a depth image on the device is a contiguous [h, w] float32 device tensor")
                import torch
                torch.cuda.current_stream(src.device).synchronize()  # the tensor is written before the tracker stream reads it
                v.depth, v.height, v.width = src.data_ptr(), int(src.shape[0]), int(src.shape[1])
                on_device.append(True)
                keep.append(src)
            else:
                a = np.ascontiguousarray(np.asarray(src, np.float32))
                if a.ndim != 2:
                    raise ValueError("a depth image is an [h, w] float32 array")
                v.depth, v.height, v.width = a.ctypes.data, int(a.shape[0]), int(a.shape[1])
                on_device.append(False)
                keep.append(a)
            if len(k) != 6:
                raise ValueError("the intrinsics of a view are (fx, fy, cx, cy, zmin, zmax)")
            v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax = [float(x) for x in k]
            v.T_w_c[:] = _cm4(T).tolist()
        if len(set(on_device)) > 1:
            raise ValueError("the raw depth images of one carve are all host arrays or all device tensors")
        return cv, 1 if on_device and on_device[0] else 0, keep

    def _carve(self, fn, views, radius, min_views, min_count, max_count, margin, margin_rel, device, records=True):
        from . import mapfile
        cv, device_in, keep = self._carve_views(views)
        n = len(cv)
        prm = MapCarveParams(int(radius), int(min_views), int(min_count), int(max_count),
                             float(self.voxel if margin is None else margin), float(margin_rel))
        L = _lib.lib()
        n_rec, info, vinfo = C.c_size_t(), MapCarveInfo(), (MapCarveViewInfo * n)()
        if not records:  # the driver's path: one call, nothing comes back but the counters
            check(fn(self._h, n, cv, device_in, C.byref(prm), None, 0, C.byref(n_rec), 0, C.byref(info), vinfo))
            rec = None
        elif device:
            import torch
            check(L.revo_map_carve_eval(self._h, n, cv, device_in, C.byref(prm), None, 0, C.byref(n_rec), 1, None, None))
            out = torch.empty(64 * max(n_rec.value, 1), dtype=torch.uint8, device="cuda:%d" % self.cameraPyr.device)
            torch.cuda.current_stream(out.device).synchronize()
            check(fn(self._h, n, cv, device_in, C.byref(prm), vp(out.data_ptr()), n_rec.value, C.byref(n_rec), 1, C.byref(info), vinfo))
            self.sync()  # the records are written
            rec = out[:64 * n_rec.value]
        else:
            check(L.revo_map_carve_eval(self._h, n, cv, device_in, C.byref(prm), None, 0, C.byref(n_rec), 0, None, None))
            rec = np.zeros(n_rec.value, mapfile.RAW_DTYPE)
            check(fn(self._h, n, cv, device_in, C.byref(prm), rec.ctypes.data_as(vp) if n_rec.value else None, n_rec.value, C.byref(n_rec),
                     0, C.byref(info), vinfo))
            rec = rec[:n_rec.value]
        del keep
        return rec, {k: int(getattr(info, k)) for k in mapfile.CARVE_INFO_KEYS}, self._view_counts(vinfo)

    @staticmethod
    def _view_counts(vinfo):
        names = (("outside", "outside"), ("unknown", "unknown"), ("free", "free_space"), ("confirmed", "confirmed"),
                 ("occluded", "occluded"), ("edge", "edge"))
        return [{name: int(getattr(vi, field)) for name, field in names} for vi in vinfo]

    def carve_eval(self, views, radius=1, min_views=1, min_count=1, max_count=0, margin=None, margin_rel=0.0, device=False, records=True):
        """What carve() would remove; the map is untouched.  views: 1 .. 64 of (pyr, T_w_c) -- a pyramid of this map's context:
        its level-0 depth plane with the context's camera -- or (depth, T_w_c[, (fx, fy, cx, cy, zmin, zmax)]) with an [h, w]
        float32 numpy array or torch device tensor of metres (no intrinsics: the context's).  T_w_c: 4x4, camera -> world.
        Per voxel with min_count <= count (<= max_count unless 0) and per view one of six classes: outside the
        image or depth range; unknown (a hole in the (2 radius + 1)^2 pixel window); free (nearer than every depth of the window
        by more than margin + margin_rel * depth; margin None: the voxel edge); confirmed; occluded; edge.  A voxel free in
        at least min_views views is carved.  -> (records, info, per-view class counts): records as a mapfile.RAW_DTYPE array
        in ascending key order, or with device=True a torch uint8 device tensor in unspecified order; info: voxels_considered,
        voxels_carved, points_carved, votes.  records=False: one library call that brings no records back (None in their
        place): the counters only."""
        return self._carve(_lib.lib().revo_map_carve_eval, views, radius, min_views, min_count, max_count, margin, margin_rel, device, records)

    def carve(self, views, radius=1, min_views=1, min_count=1, max_count=0, margin=None, margin_rel=0.0, device=False, records=True):
        """Free-space carving: the voxels carve_eval names leave the map with their whole records (exact subtraction:
        points_integrated falls by their counts, keyframes and points_dropped stay).  merge_raw(records) afterwards restores
        the map byte for byte.  Takes and returns what carve_eval does (records=False: the voxels go, only the counters come
        back)."""
        return self._carve(_lib.lib().revo_map_carve, views, radius, min_views, min_count, max_count, margin, margin_rel, device, records)

    def _views(self, T_w_c, camera, zrange, splat_max, min_count):
        """-> (MapView array, single): camera None = the context's level-0 camera and depth range (zrange must be None too),
        else an api.Camera or (fx, fy, cx, cy, width, height) and zrange (zmin, zmax) or None = the context's range."""
        T = np.asarray(T_w_c, np.float32)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        s = self.cameraPyr.settings
        if camera is None:
            if zrange is not None:
                c0 = self.cameraPyr.at(0)
                camera = (c0.fx, c0.fy, c0.cx, c0.cy, c0.width, c0.height)
            else:
                w, h, k = s.width, s.height, (0.0,) * 6
        if camera is not None:
            if isinstance(camera, Camera):
                camera = (camera.fx, camera.fy, camera.cx, camera.cy, camera.width, camera.height)
            fx, fy, cx, cy, w, h = camera
            zmin, zmax = zrange if zrange is not None else (s.depth_min, s.depth_max)
            k = (fx, fy, cx, cy, zmin, zmax)
        views = (MapView * max(1, len(T)))()
        for v, M in zip(views, T):
            v.width, v.height = int(w), int(h)
            v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax = [float(x) for x in k]
            v.T_w_c[:] = _cm4(M).tolist()
            v.splat_max, v.min_count = int(splat_max), int(min_count)
        return views, len(T), single

    def render(self, T_w_c, camera=None, zrange=None, splat_max=4, min_count=1):
        """The map seen from the camera pose T_w_c (4x4, camera -> world) as (depth [h, w] float32 metres, 0 = nothing there;
        bgr [h, w, 3] uint8; covered = written pixels): a z-buffered splat on the device (revo_map_render), the same
        bytes whatever the order of the integrations.  A list or (n, 4, 4) array of poses renders n views in ONE library call
        and returns three lists.  camera, zrange: see _views; splat_max 0 .. 8 bounds a voxel's footprint in pixels."""
        views, n, single = self._views(T_w_c, camera, zrange, splat_max, min_count)
        if n == 0:
            return [], [], []
        depth = [np.empty((v.height, v.width), np.float32) for v in views]
        bgr = [np.empty((v.height, v.width, 3), np.uint8) for v in views]
        cov = np.zeros(n, np.uint32)
        dp = (vp * n)(*[a.ctypes.data for a in depth])
        bp = (vp * n)(*[a.ctypes.data for a in bgr])
        check(_lib.lib().revo_map_render(self._h, n, views, dp, bp, cov.ctypes.data_as(vp), 0))
        if single:
            return depth[0], bgr[0], int(cov[0])
        return depth, bgr, [int(c) for c in cov]

    def render_into(self, d_depth, d_bgr, T_w_c, camera=None, zrange=None, splat_max=4, min_count=1, d_covered=None, wait=True):
        """render() into torch device tensors: d_depth [n, h, w] float32 (or [h, w] for one pose), d_bgr [n, h, w, 3] uint8,
        d_covered None or an int32 / uint32 tensor of n entries; contiguous, on the map's device.  The work is enqueued on the
        context's tracker stream, not on a torch stream: wait=True returns when it is done, wait=False at once (sync() or any
        waiting call of the map orders later reads)."""
        views, n, single = self._views(T_w_c, camera, zrange, splat_max, min_count)
        h, w = views[0].height, views[0].width
        if tuple(d_depth.shape) != ((h, w) if single else (n, h, w)) or tuple(d_bgr.shape) != tuple(d_depth.shape) + (3,):
            raise ValueError("output tensors do not match the views")
        if str(d_depth.dtype) != "torch.float32" or str(d_bgr.dtype) != "torch.uint8":
            raise ValueError("d_depth must be float32 and d_bgr uint8")
        if not (d_depth.is_contiguous() and d_bgr.is_contiguous() and d_depth.is_cuda and d_bgr.is_cuda):
            raise ValueError("output tensors must be contiguous device tensors")
        if d_covered is not None and (d_covered.numel() != n or d_covered.element_size() != 4 or not d_covered.is_contiguous()):
            raise ValueError("d_covered needs n 32-bit entries")
        dp = (vp * n)(*[d_depth.data_ptr() + 4 * h * w * i for i in range(n)])
        bp = (vp * n)(*[d_bgr.data_ptr() + 3 * h * w * i for i in range(n)])
        import torch
        torch.cuda.current_stream(d_depth.device).synchronize()  # the tensors' earlier use is over before the tracker stream writes
        check(_lib.lib().revo_map_render(self._h, n, views, dp, bp, vp(d_covered.data_ptr()) if d_covered is not None else None, 1))
        if wait:
            self.sync()

    # -- rays through the map (revo_map_raycast / revo_map_cast_rays)
    @staticmethod
    def _ray_info(i):
        from . import mapfile
        return {k: int(getattr(i, k)) for k in mapfile.RAY_INFO_KEYS}

    def raycast(self, T_w_c, camera=None, zrange=None, min_count=1, max_steps=4096, keys=False):
        """The map seen from the camera pose T_w_c by marching one ray per pixel through the voxel grid (revo_map_raycast,
        DESIGN 20): (depth [h, w] float32 metres, 0 = no voxel on the ray; bgr [h, w, 3] uint8; hits = pixels with a depth) and,
        with keys=True, a fourth value: the hit voxel's key per pixel ([h, w] uint64, all ones = miss).  No footprint
        parameter and no holes: a pixel shows the nearest voxel whose cell its ray crosses, at that voxel's mean.  A list or
        (n, 4, 4) array of poses is ONE library call and returns lists.  camera, zrange: see _views.  `ray_info` holds the
        call's counters afterwards (mapfile.RAY_INFO_KEYS)."""
        views, n, single = self._views(T_w_c, camera, zrange, 0, min_count)
        if n == 0:
            return ([], [], [], []) if keys else ([], [], [])
        depth = [np.empty((v.height, v.width), np.float32) for v in views]
        bgr = [np.empty((v.height, v.width, 3), np.uint8) for v in views]
        key = [np.empty((v.height, v.width), np.uint64) for v in views] if keys else None
        hits = np.zeros(n, np.uint32)
        info = MapRayInfo()
        dp = (vp * n)(*[a.ctypes.data for a in depth])
        bp = (vp * n)(*[a.ctypes.data for a in bgr])
        kp = (vp * n)(*[a.ctypes.data for a in key]) if keys else None
        prm = MapRayParams(int(max_steps))
        check(_lib.lib().revo_map_raycast(self._h, n, views, C.byref(prm), dp, bp, kp, hits.ctypes.data_as(vp), 0, C.byref(info)))
        self.ray_info = self._ray_info(info)
        out = (depth[0], bgr[0], int(hits[0])) if single else (depth, bgr, [int(c) for c in hits])
        return out + ((key[0] if single else key,) if keys else ())

    def raycast_into(self, d_depth, d_bgr, T_w_c, camera=None, zrange=None, min_count=1, max_steps=4096, d_keys=None, d_hits=None,
                     d_info=None, wait=True):
        """raycast() into torch device tensors: d_depth [n, h, w] float32 (or [h, w] for one pose), d_bgr [n, h, w, 3] uint8 or
        None, d_keys None or an int64 / uint64 tensor shaped like d_depth, d_hits None or n 32-bit entries, d_info None or a
        64-byte tensor (revo_map_ray_info); contiguous, on the map's device, every view's part 16-byte aligned.  Enqueued on
        the context's tracker stream: wait=True returns when it is done, wait=False at once (sync() orders later reads)."""
        views, n, single = self._views(T_w_c, camera, zrange, 0, min_count)
        h, w = views[0].height, views[0].width
        shape = (h, w) if single else (n, h, w)
        if tuple(d_depth.shape) != shape or (d_bgr is not None and tuple(d_bgr.shape) != shape + (3,)) or \
                (d_keys is not None and tuple(d_keys.shape) != shape):
            raise ValueError("output tensors do not match the views")
        if str(d_depth.dtype) != "torch.float32" or (d_bgr is not None and str(d_bgr.dtype) != "torch.uint8") or \
                (d_keys is not None and d_keys.element_size() != 8):
            raise ValueError("d_depth must be float32, d_bgr uint8 and d_keys a 64-bit integer tensor")
        for t_ in (d_depth, d_bgr, d_keys, d_hits, d_info):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("output tensors must be contiguous device tensors")
        if d_hits is not None and (d_hits.numel() != n or d_hits.element_size() != 4):
            raise ValueError("d_hits needs n 32-bit entries")
        if d_info is not None and d_info.numel() * d_info.element_size() != 64:
            raise ValueError("d_info needs 64 bytes")
        dp = (vp * n)(*[d_depth.data_ptr() + 4 * h * w * i for i in range(n)])
        bp = (vp * n)(*[d_bgr.data_ptr() + 3 * h * w * i for i in range(n)]) if d_bgr is not None else None
        kp = (vp * n)(*[d_keys.data_ptr() + 8 * h * w * i for i in range(n)]) if d_keys is not None else None
        import torch
        torch.cuda.current_stream(d_depth.device).synchronize()  # the tensors' earlier use is over before the tracker stream writes
        prm = MapRayParams(int(max_steps))
        check(_lib.lib().revo_map_raycast(self._h, n, views, C.byref(prm), dp, bp, kp, vp(d_hits.data_ptr()) if d_hits is not None else None,
                                          1, vp(d_info.data_ptr()) if d_info is not None else None))
        if wait:
            self.sync()

    def cast_rays(self, origins, dirs, s0, s1, min_count=1, max_steps=4096, device=False):
        """Range queries (revo_map_cast_rays): ray i is the points origins[i] + s dirs[i] for s0[i] <= s < s1[i]
        (dirs need not be normalised; s0, s1 scalars or [N]), marched through the voxel grid until it meets a voxel with count
        >= min_count.  -> (keys uint64 [N], all ones unless a hit; s float32 [N], the entry parameter of the last cell examined
        -- of the hit voxel's cell for a hit; cells uint32 [N]; status uint8 [N], the index into mapfile.RAY_STATUS: hit, range,
        outside, exhausted; info dict of mapfile.RAY_INFO_KEYS).  A ray that is not finite or has s0 >= s1 comes back
        `outside` with 0 cells.  device=True: the rays go through a torch device tensor and the results come back through one
        (the library's device path); the return values are the same."""
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        n = len(o)
        rays = np.empty((n, 8), np.float32)
        rays[:, 0:3], rays[:, 4:7] = o, np.asarray(dirs, np.float32).reshape(-1, 3)
        rays[:, 3], rays[:, 7] = np.asarray(s0, np.float32), np.asarray(s1, np.float32)
        prm = MapRayParams(int(max_steps))
        from . import mapfile
        L = _lib.lib()
        if device:
            import torch
            dev = "cuda:%d" % self.cameraPyr.device
            d_rays = torch.from_numpy(rays).to(dev)
            d_out = torch.empty(16 * n, dtype=torch.uint8, device=dev)
            d_info = torch.empty(64, dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(d_out.device).synchronize()
            check(L.revo_map_cast_rays(self._h, n, vp(d_rays.data_ptr()), 1, int(min_count), C.byref(prm), vp(d_out.data_ptr()), 1,
                                       vp(d_info.data_ptr())))
            self.sync()
            out, info = d_out.cpu().numpy(), d_info.cpu().numpy().view(np.uint64)
        else:
            out, info = np.zeros(16 * n, np.uint8), np.zeros(8, np.uint64)
            check(L.revo_map_cast_rays(self._h, n, rays.ctypes.data_as(vp), 0, int(min_count), C.byref(prm), out.ctypes.data_as(vp), 0,
                                       info.ctypes.data_as(vp)))
        r = out.view(np.dtype([("key", "<u8"), ("s", "<f4"), ("cells", "<u4")]))
        return (r["key"].copy(), r["s"].copy(), r["cells"] & np.uint32(0xFFFFFF), (r["cells"] >> np.uint32(30)).astype(np.uint8),
                dict(zip(mapfile.RAY_INFO_KEYS, (int(x) for x in info[:6]))))

    # -- the distance field (revo_map_distance_field / revo_map_bounds / revo_map_df_sample)
    def bounds(self, min_count=1):
        """(lo [3], hi [3] int32, n): the smallest and largest voxel index per axis over the voxels with count >= min_count, and
        how many there are (zeros when there are none).  Waits for the map."""
        lo, hi, n = np.zeros(3, np.int32), np.zeros(3, np.int32), C.c_size_t()
        check(_lib.lib().revo_map_bounds(self._h, int(min_count), _p(lo, i32p), _p(hi, i32p), C.byref(n)))
        return lo, hi, int(n.value)

    def _df_box(self, lo, n, pad, min_count):
        from . import mapfile
        if (lo is None) != (n is None):
            raise ValueError("give both lo and n, or neither (the map's bounds grown by pad)")
        if lo is None:
            b = self.bounds(min_count)
            lo, n = mapfile.padded_box(b[0], b[1], pad)
        else:
            lo, n = mapfile.check_box(lo, n)
        return MapDfBox((C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in n]))

    @staticmethod
    def _df_info(i):
        from . import mapfile
        return {k: int(getattr(i, k)) for k in mapfile.DF_INFO_KEYS}

    def distance_field(self, lo=None, n=None, pad=8, min_count=1, clamp=0, seen=None, min_views=1):
        """The exact squared Euclidean distance, in cells, from every cell of a box of voxel indices to the nearest voxel with
        count >= min_count inside the box (revo_map_distance_field) -> DistanceField.  lo, n: the box's first voxel
        index and its cells (1 .. 1024) per axis, at most 2^27 cells; by default the map's bounds grown by `pad` cells.  Voxels
        outside the box are not seen, so pad by the distance that matters.  clamp > 0: values are min(value, clamp).
        seen: a SeenVolume -- the known field (revo_map_known_field) over its box: every cell that is neither solid
        nor known (>= min_views free votes, or the surface bit) is an obstacle too; lo, n and pad are then not given."""
        if seen is not None:
            return self._known_field(seen, min_views, lo, n, min_count, clamp)
        box = self._df_box(lo, n, pad, min_count)
        d2 = np.empty(tuple(box.n), np.uint32)
        info = MapDfInfo()
        check(_lib.lib().revo_map_distance_field(self._h, C.byref(box), int(min_count), int(clamp), d2.ctypes.data_as(vp), 0, C.byref(info)))
        return DistanceField(d2, np.array(list(box.lo), np.int32), self.voxel, self._df_info(info), self, clamp=int(clamp))

    def _seen_box(self, seen, lo=None, n=None):
        if lo is not None or n is not None:
            raise ValueError("a seen volume brings its own box: lo and n are not given with it")
        if np.float32(seen.voxel).tobytes() != np.float32(self.voxel).tobytes():
            raise ValueError("the seen volume was observed at voxels of %g m, the map has %g m" % (seen.voxel, self.voxel))
        vol = np.ascontiguousarray(seen.seen, np.uint8)
        return self._df_box(seen.lo, vol.shape, 0, 1), vol

    def _known_field(self, seen, min_views, lo, n, min_count, clamp):
        from . import mapfile
        box, vol = self._seen_box(seen, lo, n)
        d2 = np.empty(tuple(box.n), np.uint32)
        info = MapKnownInfo()
        check(_lib.lib().revo_map_known_field(self._h, C.byref(box), int(min_count), int(clamp), vol.ctypes.data_as(vp), 0, int(min_views),
                                              d2.ctypes.data_as(vp), 0, C.byref(info)))
        f = DistanceField(d2, np.array(list(box.lo), np.int32), self.voxel, {k: int(getattr(info, k)) for k in mapfile.KNOWN_INFO_KEYS}, self,
                          clamp=int(clamp))
        f.known, f.min_views = True, max(1, int(min_views))
        return f

    def known_field_into(self, d_d2, d_seen, lo, n, min_count=1, clamp=0, min_views=1, d_info=None, wait=True):
        """The known field between torch device tensors: d_seen the seen volume (uint8 of the box's shape n), d_d2 and d_info
        as distance_field_into takes them (d_info: 64 bytes, revo_map_known_info)."""
        box = self._df_box(lo, n, 0, 1)
        if tuple(d_d2.shape) != tuple(box.n) or d_d2.element_size() != 4 or d_d2.is_floating_point():
            raise ValueError("d_d2 must be a 32-bit integer tensor of the box's shape")
        if tuple(d_seen.shape) != tuple(box.n) or str(d_seen.dtype) != "torch.uint8":
            raise ValueError("d_seen must be a uint8 tensor of the box's shape")
        for t_ in (d_d2, d_seen, d_info):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("tensors must be contiguous device tensors")
        if d_info is not None and d_info.numel() * d_info.element_size() != 64:
            raise ValueError("d_info needs 64 bytes")
        import torch
        torch.cuda.current_stream(d_d2.device).synchronize()  # the volume is written, the outputs' earlier use is over
        check(_lib.lib().revo_map_known_field(self._h, C.byref(box), int(min_count), int(clamp), vp(d_seen.data_ptr()), 1, int(min_views),
                                              vp(d_d2.data_ptr()), 1, vp(d_info.data_ptr()) if d_info is not None else None))
        if wait:
            self.sync()

    # -- known space (revo_map_observe / revo_map_frontiers)
    def observe(self, views, lo=None, n=None, pad=0, radius=1, margin=None, margin_rel=0.0, into=None):
        """What the views have looked at -> SeenVolume: one byte per cell of a box of voxel indices -- the views that look
        through the cell's centre (free votes, at most 127) and, in bit 7, whether one measured a surface there
        (revo_map_observe).  views, radius, margin, margin_rel: as carve_eval takes them; the class of a cell's
        centre in a view is carve_eval's class of that point.  lo, n: the box (by default the map's bounds grown by `pad`
        cells).  into: a SeenVolume to accumulate into (votes add and saturate, the surface bit stays); its box is the
        call's, so lo and n are not given.  The map's voxels play no part."""
        from . import mapfile
        cv, device_in, keep = self._carve_views(views)
        if into is not None:
            box, vol = self._seen_box(into, lo, n)
            vol = vol.copy()
        else:
            box = self._df_box(lo, n, pad, 1)
            vol = np.empty(tuple(box.n), np.uint8)
        prm = MapObserveParams(int(radius), 0 if into is None else 1, float(self.voxel if margin is None else margin), float(margin_rel))
        info, vinfo = MapObserveInfo(), (MapCarveViewInfo * len(cv))()
        check(_lib.lib().revo_map_observe(self._h, C.byref(box), len(cv), cv, device_in, C.byref(prm), vol.ctypes.data_as(vp), 0, C.byref(info),
                                          C.cast(vinfo, vp)))
        del keep
        return SeenVolume(vol, np.array(list(box.lo), np.int32), self.voxel, {k: int(getattr(info, k)) for k in mapfile.SEEN_INFO_KEYS},
                          self._view_counts(vinfo))

    def observe_into(self, d_seen, views, lo, radius=1, margin=None, margin_rel=0.0, accumulate=False, d_info=None, d_view_info=None, wait=True):
        """observe() into a torch device tensor: d_seen uint8 of the box's shape (its cells are the box's n), d_info None or 64
        bytes (revo_map_observe_info), d_view_info None or 32 bytes per view (revo_map_carve_view_info); contiguous, 16-byte
        aligned, on the map's device.  accumulate: d_seen is read and updated.  With device or pyramid views the call is only
        enqueued on the context's tracker stream: wait=False returns at once (sync() orders later reads)."""
        cv, device_in, keep = self._carve_views(views)
        if d_seen.dim() != 3 or str(d_seen.dtype) != "torch.uint8":
            raise ValueError("d_seen must be a 3-D uint8 tensor")
        box = self._df_box(lo, tuple(d_seen.shape), 0, 1)
        for t_, size in ((d_seen, None), (d_info, 64), (d_view_info, 32 * len(cv))):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("output tensors must be contiguous device tensors")
            if t_ is not None and size is not None and t_.numel() * t_.element_size() != size:
                raise ValueError("d_info needs 64 bytes and d_view_info 32 bytes per view")
        prm = MapObserveParams(int(radius), 1 if accumulate else 0, float(self.voxel if margin is None else margin), float(margin_rel))
        import torch
        torch.cuda.current_stream(d_seen.device).synchronize()  # the tensors' earlier use is over before the tracker stream writes
        check(_lib.lib().revo_map_observe(self._h, C.byref(box), len(cv), cv, device_in, C.byref(prm), vp(d_seen.data_ptr()), 1,
                                          vp(d_info.data_ptr()) if d_info is not None else None,
                                          vp(d_view_info.data_ptr()) if d_view_info is not None else None))
        if wait:
            self.sync()
        del keep

    # -- a surface (revo_map_tsdf_fuse / revo_map_tsdf_mesh)
    def _tsdf_box(self, vol, lo=None, n=None):
        if lo is not None or n is not None:
            raise ValueError("a TSDF volume brings its own box: lo and n are not given with it")
        if np.float32(vol.voxel).tobytes() != np.float32(self.voxel).tobytes():
            raise ValueError("the TSDF volume was fused at voxels of %g m, the map has %g m" % (vol.voxel, self.voxel))
        cells = np.ascontiguousarray(vol.cells)
        return self._df_box(vol.lo, cells.shape, 0, 1), cells

    def _color_views(self, views):
        """The views of a colour fuse -> (_carve_views' three results, the bgr pointer array of revo_map_tsdf_fuse_color, what
        keeps the colour images alive).  A raw view is (depth, T, intrinsics-or-None, bgr), a pyramid view brings its own."""
        views = list(views)
        for v in views:
            if not isinstance(v[0], ImgPyramidRGBD) and (len(v) < 4 or v[3] is None):
                raise ValueError("with color=True a raw view is (depth, T, intrinsics or None, bgr)")
        cv, device_in, keep = self._carve_views([v[:3] for v in views])
        ptrs, keep_c = (C.c_void_p * len(views))(), []
        for i, v in enumerate(views):
            if isinstance(v[0], ImgPyramidRGBD):
                continue
            im, shape = v[3], (int(cv[i].height), int(cv[i].width), 3)
            if device_in:
                if not (hasattr(im, "data_ptr") and im.is_cuda and im.is_contiguous() and str(im.dtype) == "torch.uint8" and tuple(im.shape) == shape):
                    raise ValueError("the colour image of a device depth image is a contiguous [h, w, 3] uint8 device tensor")
                import torch
                torch.cuda.current_stream(im.device).synchronize()
                ptrs[i] = im.data_ptr()
            else:
                if hasattr(im, "data_ptr"):
                    raise ValueError("the colour image of a host depth image is a host array")
                im = np.asarray(im)
                if im.dtype != np.uint8 or im.shape != shape:
                    raise ValueError("a colour image is an [h, w, 3] uint8 array of the depth image's size")
                im = np.ascontiguousarray(im)
                ptrs[i] = im.ctypes.data
            keep_c.append(im)
        return cv, device_in, keep, ptrs, keep_c

    def fuse(self, views, lo=None, n=None, pad=8, trunc=None, into=None, color=False):
        """The views fused into a truncated signed distance volume -> TsdfVolume: per cell of a box of voxel indices the integer
        sum of the views' signed distances to the surface they measured, in units of trunc / 1024, and the number of views that
        gave one (revo_map_tsdf_fuse).  views: as carve_eval and observe take them; the class of a cell's centre in a
        view is carve_eval's at radius 0 with margin = trunc.  lo, n: the box (by default the map's bounds grown by `pad` cells).
        trunc: metres (default 4 voxel edges).  into: a TsdfVolume to accumulate into (it is not changed); its box and trunc are
        the call's, so lo, n and trunc are not given.  The map's voxels play no part.
        color: the colour volume is fused in the same pass (revo_map_tsdf_fuse_color): a raw view is (depth, T,
        intrinsics or None, bgr) with bgr an [h, w, 3] uint8 array (a device tensor beside a device depth image), a pyramid view
        brings its level-0 colour plane.  The result has .color and .color_info; `into` must then carry a colour volume, and
        must not without color."""
        from . import mapfile
        if into is not None and (into.color is not None) != bool(color):
            raise ValueError("a volume with colour is accumulated into with color=True, one without it with color=False")
        if color:
            cv, device_in, keep, bgr, keep_c = self._color_views(views)
        else:
            cv, device_in, keep = self._carve_views(views)
        if into is not None:
            if trunc is not None and np.float32(trunc).tobytes() != np.float32(into.trunc).tobytes():
                raise ValueError("a TSDF volume brings its own trunc")
            box, vol = self._tsdf_box(into, lo, n)
            vol, trunc = vol.copy(), into.trunc
            col = np.ascontiguousarray(into.color).copy() if color else None
        else:
            box = self._df_box(lo, n, pad, 1)
            vol = np.empty(tuple(box.n), mapfile.TSDF_CELL_DTYPE)
            col = np.empty(tuple(box.n), mapfile.TSDF_COLOR_DTYPE) if color else None
        trunc = float(mapfile.tsdf_trunc(self.voxel, trunc))
        prm = MapTsdfParams(trunc, 0 if into is None else 1)
        info, vinfo, cinfo = MapTsdfInfo(), (MapCarveViewInfo * len(cv))(), MapTsdfColorInfo()
        if color:
            check(_lib.lib().revo_map_tsdf_fuse_color(self._h, C.byref(box), len(cv), cv, C.cast(bgr, vp), device_in, C.byref(prm),
                                                      vol.ctypes.data_as(vp), col.ctypes.data_as(vp), 0, C.byref(info), C.byref(cinfo), C.cast(vinfo, vp)))
            del keep_c
        else:
            check(_lib.lib().revo_map_tsdf_fuse(self._h, C.byref(box), len(cv), cv, device_in, C.byref(prm), vol.ctypes.data_as(vp), 0, C.byref(info),
                                                C.cast(vinfo, vp)))
        del keep
        return TsdfVolume(vol, np.array(list(box.lo), np.int32), self.voxel, trunc, {k: int(getattr(info, k)) for k in mapfile.TSDF_INFO_KEYS},
                          self._view_counts(vinfo), self, color=col,
                          color_info={k: int(getattr(cinfo, k)) for k in mapfile.TSDF_COLOR_INFO_KEYS} if color else None)

    def fuse_into(self, d_tsdf, views, lo, trunc=None, accumulate=False, d_info=None, d_view_info=None, wait=True, d_color=None, d_color_info=None):
        """fuse() into a torch device tensor: d_tsdf int32 [n0, n1, n2, 2] (sum, weight; the box's cells are its first three
        sizes), d_info None or 64 bytes (revo_map_tsdf_info), d_view_info None or 32 bytes per view; contiguous, 16-byte aligned,
        on the map's device.  accumulate: d_tsdf is read and updated.  With device or pyramid views the call is only enqueued on
        the context's tracker stream: wait=False returns at once (sync() orders later reads).
        d_color: int32 [n0, n1, n2, 4] (sum_b, sum_g, sum_r, weight) -- the colour volume is fused in the same pass, the views are
        those of fuse(color=True); d_color_info: None or 32 bytes (revo_map_tsdf_color_info)."""
        from . import mapfile
        if d_color is not None:
            cv, device_in, keep, bgr, keep_c = self._color_views(views)
        else:
            if d_color_info is not None:
                raise ValueError("d_color_info goes with d_color")
            cv, device_in, keep = self._carve_views(views)
        if d_tsdf.dim() != 4 or d_tsdf.shape[3] != 2 or str(d_tsdf.dtype) != "torch.int32":
            raise ValueError("d_tsdf must be an int32 tensor [n0, n1, n2, 2]")
        if d_color is not None and (tuple(d_color.shape) != tuple(d_tsdf.shape[:3]) + (4,) or str(d_color.dtype) != "torch.int32"):
            raise ValueError("d_color must be an int32 tensor [n0, n1, n2, 4] over d_tsdf's box")
        box = self._df_box(lo, tuple(d_tsdf.shape[:3]), 0, 1)
        for t_, size in ((d_tsdf, None), (d_info, 64), (d_view_info, 32 * len(cv)), (d_color, None), (d_color_info, 32)):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("output tensors must be contiguous device tensors")
            if t_ is not None and size is not None and t_.numel() * t_.element_size() != size:
                raise ValueError("d_info needs 64 bytes, d_view_info 32 bytes per view and d_color_info 32 bytes")
        prm = MapTsdfParams(float(mapfile.tsdf_trunc(self.voxel, trunc)), 1 if accumulate else 0)
        import torch
        torch.cuda.current_stream(d_tsdf.device).synchronize()  # the tensors' earlier use is over before the tracker stream writes
        ptr = lambda t_: vp(t_.data_ptr()) if t_ is not None else None  # noqa: E731
        if d_color is not None:
            check(_lib.lib().revo_map_tsdf_fuse_color(self._h, C.byref(box), len(cv), cv, C.cast(bgr, vp), device_in, C.byref(prm), ptr(d_tsdf),
                                                      ptr(d_color), 1, ptr(d_info), ptr(d_color_info), ptr(d_view_info)))
        else:
            check(_lib.lib().revo_map_tsdf_fuse(self._h, C.byref(box), len(cv), cv, device_in, C.byref(prm), ptr(d_tsdf), 1, ptr(d_info), ptr(d_view_info)))
        if wait:
            self.sync()
        del keep

    # -- views taken out of a surface again (revo_map_tsdf_unfuse)
    @staticmethod
    def _check_unfuse(rc, info):
        """check(rc); a refusal's RevoError carries misfits and info (the dict of mapfile.TSDF_UNFUSE_INFO_KEYS; None when the call
        was given no info record)."""
        from . import mapfile
        as_dict = lambda: None if info is None else {k: int(getattr(info, k)) for k in mapfile.TSDF_UNFUSE_INFO_KEYS}  # noqa: E731
        try:
            check(rc)
        except RevoError as e:
            e.info = as_dict()
            e.misfits = None if info is None else e.info["misfits"]
            raise
        return as_dict()

    def unfuse(self, volume, views):
        """Views taken out of a TsdfVolume again -> a new TsdfVolume (revo_map_tsdf_unfuse): the exact inverse of
        fuse(into=), with the volume's box and trunc.  views: as fuse takes them, with the colour images of fuse(color=True) when
        the volume has colour.  All or nothing: RevoError (REVO_ERR_INVALID_ARG) carrying .misfits when a cell would not fit -- a
        view that is not in the volume, a full weight, sums no fuse can reach; the volume is not changed either way.  The
        result's info is the dict of mapfile.TSDF_UNFUSE_INFO_KEYS."""
        from . import mapfile
        color = volume.color is not None
        if color:
            cv, device_in, keep, bgr, keep_c = self._color_views(views)
        else:
            cv, device_in, keep = self._carve_views(views)
            bgr, keep_c = None, None
        box, vol = self._tsdf_box(volume)
        vol = vol.copy()
        col = np.ascontiguousarray(volume.color).copy() if color else None
        info, vinfo = MapTsdfUnfuseInfo(), (MapCarveViewInfo * len(cv))()
        out = self._check_unfuse(_lib.lib().revo_map_tsdf_unfuse(self._h, C.byref(box), len(cv), cv, C.cast(bgr, vp) if color else None, device_in,
                                                                 float(volume.trunc), vol.ctypes.data_as(vp), col.ctypes.data_as(vp) if color else None, 0,
                                                                 C.byref(info), C.cast(vinfo, vp)), info)
        del keep, keep_c
        return TsdfVolume(vol, np.array(list(box.lo), np.int32), self.voxel, volume.trunc, out, self._view_counts(vinfo), self, color=col)

    def unfuse_into(self, d_tsdf, views, lo, trunc=None, d_color=None, d_view_info=None, wait=True):
        """unfuse() between torch device tensors: d_tsdf int32 [n0, n1, n2, 2] and d_color int32 [n0, n1, n2, 4] or None (then the
        views carry no colour images and no colour volume is touched), as fuse_into takes them; trunc: what the views were fused
        with (default 4 voxel edges); d_view_info: None or 32 bytes per view.  The call waits for its check pass; all or nothing:
        RevoError carrying .misfits and .info, with no byte of the volumes changed.  wait=True -> the info dict of
        mapfile.TSDF_UNFUSE_INFO_KEYS; wait=False -> None, the apply pass only enqueued on the map's stream (sync() orders later
        reads; the images must stay alive until then)."""
        from . import mapfile
        import torch
        if d_color is not None:
            cv, device_in, keep, bgr, keep_c = self._color_views(views)
        else:
            cv, device_in, keep = self._carve_views(views)
            bgr, keep_c = None, None
        self._surface_tensors(d_tsdf, d_color, "d_tsdf")
        if d_view_info is not None and not (d_view_info.is_cuda and d_view_info.is_contiguous() and
                                            d_view_info.numel() * d_view_info.element_size() == 32 * len(cv)):
            raise ValueError("d_view_info needs 32 bytes per view on the device")
        box = self._df_box(lo, tuple(d_tsdf.shape[:3]), 0, 1)
        tr = float(mapfile.tsdf_trunc(self.voxel, None if trunc is None or trunc == 0 else trunc))
        torch.cuda.current_stream(d_tsdf.device).synchronize()  # the tensors' earlier use is over before the tracker stream touches them
        info = MapTsdfUnfuseInfo()
        out = self._check_unfuse(_lib.lib().revo_map_tsdf_unfuse(self._h, C.byref(box), len(cv), cv, C.cast(bgr, vp) if d_color is not None else None,
                                                                 device_in, tr, vp(d_tsdf.data_ptr()), vp(d_color.data_ptr()) if d_color is not None else None,
                                                                 1, C.byref(info) if wait else None,
                                                                 vp(d_view_info.data_ptr()) if d_view_info is not None else None), info if wait else None)
        del keep, keep_c
        return out

    def mesh(self, tsdf, min_weight=1, normals=False, colors=False):
        """The mesh of a TsdfVolume's zero level set -> mapfile.Mesh: vertices, triangles and the call's counts, in the contract's
        canonical order (revo_map_tsdf_mesh).  A cell counts when its weight >= max(min_weight, 1).
        normals, colors: the mesh carries per-vertex unit normals and B, G, R, k bytes (revo_map_tsdf_mesh_attr);
        colours need a volume fused with color=True."""
        from . import mapfile
        box, cells = self._tsdf_box(tsdf)
        L, nv, nt, info = _lib.lib(), C.c_size_t(), C.c_size_t(), MapMeshInfo()
        if not (normals or colors):
            args = (self._h, C.byref(box), cells.ctypes.data_as(vp), 0, int(min_weight))
            check(L.revo_map_tsdf_mesh(*args, None, 0, None, 0, C.byref(nv), C.byref(nt), 0, C.byref(info)))
            v, t = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.uint32)
            if nv.value or nt.value:
                check(L.revo_map_tsdf_mesh(*args, v.ctypes.data_as(vp), nv.value, t.ctypes.data_as(vp), nt.value, C.byref(nv), C.byref(nt), 0, C.byref(info)))
            return mapfile.Mesh(v, t, {k: int(getattr(info, k)) for k in mapfile.MESH_INFO_KEYS})
        if colors and tsdf.color is None:
            raise ValueError("the volume has no colour: fuse it with color=True")
        col = np.ascontiguousarray(tsdf.color) if colors else None
        args = (self._h, C.byref(box), cells.ctypes.data_as(vp), col.ctypes.data_as(vp) if colors else None, 0, int(min_weight))
        check(L.revo_map_tsdf_mesh_attr(*args, None, None, None, 0, None, 0, C.byref(nv), C.byref(nt), 0, C.byref(info)))
        v, t = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.uint32)
        nrm = np.zeros((nv.value, 3), np.float32) if normals else None
        rgb = np.zeros((nv.value, 4), np.uint8) if colors else None
        if nv.value or nt.value:
            check(L.revo_map_tsdf_mesh_attr(*args, v.ctypes.data_as(vp), nrm.ctypes.data_as(vp) if normals else None,
                                            rgb.ctypes.data_as(vp) if colors else None, nv.value, t.ctypes.data_as(vp), nt.value,
                                            C.byref(nv), C.byref(nt), 0, C.byref(info)))
        return mapfile.Mesh(v, t, {k: int(getattr(info, k)) for k in mapfile.MESH_INFO_KEYS}, nrm, rgb)

    def mesh_into(self, d_vertices, d_triangles, d_tsdf, lo, min_weight=1, d_normals=None, d_colors=None, d_color=None):
        """mesh() between torch device tensors: d_tsdf int32 [n0, n1, n2, 2] as fuse_into leaves it, d_vertices float32 [cap, 3],
        d_triangles int32 [cap, 3]; contiguous, 16-byte aligned, on the map's device.  -> (vertices, triangles, info dict): the
        counts; RevoError (REVO_ERR_CAPACITY), with nothing written, when a tensor holds fewer.  Both None: count only.  The call
        waits for the map's stream first, so a fuse_into(wait=False) before it needs no sync().
        d_normals float32 [cap, 3], d_colors uint8 [cap, 4] (both of d_vertices' capacity) and d_color, the colour volume int32
        [n0, n1, n2, 4]: the vertices' attributes (revo_map_tsdf_mesh_attr); d_colors needs d_color."""
        from . import mapfile
        if d_tsdf.dim() != 4 or d_tsdf.shape[3] != 2 or str(d_tsdf.dtype) != "torch.int32":
            raise ValueError("d_tsdf must be an int32 tensor [n0, n1, n2, 2]")
        box = self._df_box(lo, tuple(d_tsdf.shape[:3]), 0, 1)
        for t_, dt in ((d_vertices, "torch.float32"), (d_triangles, "torch.int32"), (d_normals, "torch.float32")):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda and t_.dim() == 2 and t_.shape[1] == 3 and str(t_.dtype) == dt):
                raise ValueError("d_vertices and d_normals are float32 and d_triangles an int32 contiguous device tensor [cap, 3]")
        if d_colors is not None and not (d_colors.is_contiguous() and d_colors.is_cuda and d_colors.dim() == 2 and d_colors.shape[1] == 4
                                         and str(d_colors.dtype) == "torch.uint8"):
            raise ValueError("d_colors is a uint8 contiguous device tensor [cap, 4]")
        if d_colors is not None and d_color is None:
            raise ValueError("d_colors needs the colour volume d_color")
        if d_color is not None and not (tuple(d_color.shape) == tuple(d_tsdf.shape[:3]) + (4,) and str(d_color.dtype) == "torch.int32"
                                        and d_color.is_contiguous() and d_color.is_cuda):
            raise ValueError("d_color must be a contiguous int32 device tensor [n0, n1, n2, 4] over d_tsdf's box")
        if not (d_tsdf.is_contiguous() and d_tsdf.is_cuda):
            raise ValueError("d_tsdf must be a contiguous device tensor")
        caps = {len(t_) for t_ in (d_vertices, d_normals, d_colors) if t_ is not None}
        if len(caps) > 1:
            raise ValueError("d_vertices, d_normals and d_colors hold the same number of vertices")
        import torch
        torch.cuda.current_stream(d_tsdf.device).synchronize()
        nv, nt, info = C.c_size_t(), C.c_size_t(), MapMeshInfo()
        ptr = lambda t_: vp(t_.data_ptr()) if t_ is not None else None  # noqa: E731
        if d_normals is None and d_colors is None:
            check(_lib.lib().revo_map_tsdf_mesh(self._h, C.byref(box), vp(d_tsdf.data_ptr()), 1, int(min_weight),
                                                ptr(d_vertices), len(d_vertices) if d_vertices is not None else 0,
                                                ptr(d_triangles), len(d_triangles) if d_triangles is not None else 0,
                                                C.byref(nv), C.byref(nt), 1, C.byref(info)))
        else:
            check(_lib.lib().revo_map_tsdf_mesh_attr(self._h, C.byref(box), vp(d_tsdf.data_ptr()), ptr(d_color), 1, int(min_weight),
                                                     ptr(d_vertices), ptr(d_normals), ptr(d_colors), caps.pop(),
                                                     ptr(d_triangles), len(d_triangles) if d_triangles is not None else 0,
                                                     C.byref(nv), C.byref(nt), 1, C.byref(info)))
        return nv.value, nt.value, {k: int(getattr(info, k)) for k in mapfile.MESH_INFO_KEYS}

    @staticmethod
    def _surface_tensors(d_tsdf, d_color, what):
        if d_tsdf.dim() != 4 or d_tsdf.shape[3] != 2 or str(d_tsdf.dtype) != "torch.int32" or not (d_tsdf.is_contiguous() and d_tsdf.is_cuda):
            raise ValueError("%s must be a contiguous int32 device tensor [n0, n1, n2, 2]" % what)
        if d_color is not None and not (tuple(d_color.shape) == tuple(d_tsdf.shape[:3]) + (4,) and str(d_color.dtype) == "torch.int32"
                                        and d_color.is_contiguous() and d_color.is_cuda):
            raise ValueError("%s's colour volume must be a contiguous int32 device tensor [n0, n1, n2, 4] over its box" % what)

    def shift_into(self, d_dst, d_src, lo, delta, d_dst_color=None, d_src_color=None, d_records=None, count_only=False, d_info=None):
        """The surface volumes of the box at lo moved into the volumes of the box at lo + delta, between torch device tensors
        (revo_map_tsdf_shift): d_src, d_dst int32 [n0, n1, n2, 2], the colour volumes int32 [n0, n1, n2, 4] (both or
        neither); the move is out of place.  A cell that lies in both boxes keeps its bytes, an entering cell is zero, and
        d_records: a contiguous device tensor of 32 bytes per record -- the leaving cells that are not EMPTY are written to it as
              mapfile.TSDF_RECORD_DTYPE in ascending key order -> (records, info dict of mapfile.TSDF_SHIFT_INFO_KEYS); RevoError
              (REVO_ERR_CAPACITY), with d_dst untouched, when it holds fewer.  The call waits for the count.
        count_only: -> (records, info) without writing d_dst.
        neither: the leaving cells are dropped and the call is only enqueued (sync() orders later reads); d_info: None or 64 bytes
              on the device, revo_map_tsdf_shift_info with `dropped`.  -> None.
        The move (and the emit pass) run on the map's stream behind the call: every tensor given must stay alive, and unwritten by
        other streams, until the map's sync() -- torch's allocator does not know that stream."""
        from . import mapfile
        import torch
        self._surface_tensors(d_src, d_src_color, "d_src")
        self._surface_tensors(d_dst, d_dst_color, "d_dst")
        if tuple(d_src.shape) != tuple(d_dst.shape):
            raise ValueError("d_src and d_dst are volumes of boxes of one size")
        if count_only and d_records is not None:
            raise ValueError("count_only writes no records")
        box = self._df_box(lo, tuple(d_src.shape[:3]), 0, 1)
        dl = (C.c_int32 * 3)(*[int(x) for x in np.asarray(delta, np.int64).reshape(3)])
        cap = 0
        if d_records is not None:
            if not (d_records.is_cuda and d_records.is_contiguous()):
                raise ValueError("d_records must be a contiguous device tensor")
            cap = d_records.numel() * d_records.element_size() // 32
        drop = d_records is None and not count_only
        if d_info is not None and not (drop and d_info.is_cuda and d_info.is_contiguous() and d_info.numel() * d_info.element_size() == 64):
            raise ValueError("d_info is 64 bytes on the device and goes with a move that drops the leaving cells")
        torch.cuda.current_stream(d_src.device).synchronize()  # the tensors' earlier use is over before the tracker stream touches them
        ptr = lambda t_: vp(t_.data_ptr()) if t_ is not None else None  # noqa: E731
        n, info = C.c_size_t(), MapTsdfShiftInfo()
        check(_lib.lib().revo_map_tsdf_shift(self._h, C.byref(box), dl, ptr(d_src), ptr(d_src_color), ptr(d_dst), ptr(d_dst_color), 1,
                                             ptr(d_records), cap, None if drop else C.byref(n), 1,
                                             ptr(d_info) if drop else C.cast(C.byref(info), vp)))
        if drop:
            return None
        return n.value, {k: int(getattr(info, k)) for k in mapfile.TSDF_SHIFT_INFO_KEYS}

    def refill_into(self, d_tsdf, lo, d_records, n=None, d_color=None):
        """Records added back into the cells of the box at lo, between torch device tensors (revo_map_tsdf_refill):
        d_records a contiguous device tensor of 32 bytes per record (mapfile.TSDF_RECORD_DTYPE, strictly ascending keys), n how
        many of them (default: all it holds).  Records outside the box are ignored.  All or nothing: RevoError
        (REVO_ERR_INVALID_ARG), with both volumes unchanged, when the keys are out of order, a record carries colour without
        d_color, or a cell would pass the sums a fuse can reach.  The call waits for its check and enqueues the update on the map's
        stream: d_records (and the volumes) must stay alive until the map's sync() -- torch's allocator does not know that stream,
        and a tensor dropped earlier may be handed out again while the update still reads it.
        -> info dict of mapfile.TSDF_REFILL_INFO_KEYS."""
        from . import mapfile
        import torch
        self._surface_tensors(d_tsdf, d_color, "d_tsdf")
        box = self._df_box(lo, tuple(d_tsdf.shape[:3]), 0, 1)
        if d_records is None:
            n = 0
        else:
            if not (d_records.is_cuda and d_records.is_contiguous()):
                raise ValueError("d_records must be a contiguous device tensor")
            cap = d_records.numel() * d_records.element_size() // 32
            n = cap if n is None else int(n)
            if n < 0 or n > cap:
                raise ValueError("d_records holds %d records, not %d" % (cap, n))
        torch.cuda.current_stream(d_tsdf.device).synchronize()
        info = MapTsdfRefillInfo()
        check(_lib.lib().revo_map_tsdf_refill(self._h, C.byref(box), vp(d_tsdf.data_ptr()), vp(d_color.data_ptr()) if d_color is not None else None, 1,
                                              n, vp(d_records.data_ptr()) if n else None, 1, C.byref(info)))
        return {k: int(getattr(info, k)) for k in mapfile.TSDF_REFILL_INFO_KEYS}

    def surface_shift(self, cells, lo, delta, color=None, records=True):
        """revo_map_tsdf_shift on host volumes (numpy, mapfile's dtypes): -> (cells2, color2, records, info) as
        mapfile.tsdf_shift_records gives them; records=False drops the leaving cells (records is None, info counts `dropped`)."""
        from . import mapfile
        cells = np.ascontiguousarray(mapfile._tsdf_volume(cells))
        color = None if color is None else np.ascontiguousarray(mapfile._tsdf_color_volume(color, cells.shape))
        box = self._df_box(lo, cells.shape, 0, 1)
        dl = (C.c_int32 * 3)(*[int(x) for x in np.asarray(delta, np.int64).reshape(3)])
        out = np.zeros(cells.shape, mapfile.TSDF_CELL_DTYPE)
        cout = None if color is None else np.zeros(cells.shape, mapfile.TSDF_COLOR_DTYPE)
        hp = lambda a: a.ctypes.data_as(vp) if a is not None else None  # noqa: E731
        L, n, info = _lib.lib(), C.c_size_t(), MapTsdfShiftInfo()
        args = (self._h, C.byref(box), dl, hp(cells), hp(color), hp(out), hp(cout), 0)
        rec = None
        if records:
            check(L.revo_map_tsdf_shift(*args, None, 0, C.byref(n), 0, C.cast(C.byref(info), vp)))
            rec = np.zeros(n.value, mapfile.TSDF_RECORD_DTYPE)
            if n.value:
                check(L.revo_map_tsdf_shift(*args, rec.ctypes.data_as(vp), n.value, C.byref(n), 0, C.cast(C.byref(info), vp)))
            else:  # nothing to emit: the move alone
                check(L.revo_map_tsdf_shift(*args, None, 0, None, 0, C.cast(C.byref(info), vp)))
        else:
            check(L.revo_map_tsdf_shift(*args, None, 0, None, 0, C.cast(C.byref(info), vp)))
        return out, cout, rec, {k: int(getattr(info, k)) for k in mapfile.TSDF_SHIFT_INFO_KEYS}

    def surface_refill(self, cells, lo, records, color=None):
        """revo_map_tsdf_refill on host volumes and records (numpy): -> (cells2, color2, info) as mapfile.tsdf_refill_records gives
        them; the inputs are not changed.  RevoError (REVO_ERR_INVALID_ARG) where that one raises ValueError."""
        from . import mapfile
        out = np.array(mapfile._tsdf_volume(cells), copy=True, order="C")
        cout = None if color is None else np.array(mapfile._tsdf_color_volume(color, out.shape), copy=True, order="C")
        rec = np.ascontiguousarray(mapfile.tsdf_record_array(records))
        box = self._df_box(lo, out.shape, 0, 1)
        info = MapTsdfRefillInfo()
        check(_lib.lib().revo_map_tsdf_refill(self._h, C.byref(box), out.ctypes.data_as(vp), cout.ctypes.data_as(vp) if cout is not None else None, 0,
                                              len(rec), rec.ctypes.data_as(vp) if len(rec) else None, 0, C.byref(info)))
        return out, cout, {k: int(getattr(info, k)) for k in mapfile.TSDF_REFILL_INFO_KEYS}

    # -- views of the surface (revo_map_tsdf_raycast)
    def _surface_views(self, poses, camera, size, zrange):
        """-> (MapView array, n, single) for the poses (one 4x4 camera -> world pose, or a list / (n, 4, 4) array of 1 .. 64);
        camera, size, zrange: see _gain_camera."""
        T = np.asarray(poses, np.float32)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        if not 1 <= len(T) <= 64:
            raise ValueError("a surface ray cast takes 1 .. 64 poses")
        cam = self._gain_camera(camera, size, zrange, 1)
        views = (MapView * len(T))()
        for v, M in zip(views, T):
            C.memmove(C.byref(v), C.byref(cam), C.sizeof(MapView))
            v.T_w_c[:] = _cm4(M).tolist()
        return views, len(T), single

    @staticmethod
    def _tsdf_ray_params(step, min_weight, max_steps):
        if int(min_weight) < 0 or int(max_steps) < 0:
            raise ValueError("min_weight and max_steps are >= 0")
        return MapTsdfRayParams(0.0 if step is None else float(step), int(min_weight), int(max_steps), 0)

    def surface_raycast(self, tsdf, poses, camera=None, size=None, zrange=None, step=None, min_weight=1, max_steps=4096, normals=True, colors=True):
        """A TsdfVolume's surface seen from camera poses (revo_map_tsdf_raycast): one ray per pixel marched through the
        fused field in steps of `step` metres of camera depth (default: the voxel edge), the surface found between two samples
        from the trilinear interpolant.  -> dict: depth [h, w] float32 metres (0 = no surface on the ray), normals [h, w, 3]
        float32 unit vectors in the world frame pointing out of the surface (None with normals=False), bgr [h, w, 3] uint8 (None
        with colors=False), hits = the pixels with a depth, info = the call's counters (mapfile.TSDF_RAY_INFO_KEYS).  A list or
        (n, 4, 4) array of 1 .. 64 poses is ONE library call and gives lists under depth, normals, bgr and hits.  camera, size,
        zrange: see _gain_camera.  colors needs a volume fused with color=True.  The map's voxels play no part."""
        from . import mapfile
        if colors and tsdf.color is None:
            raise ValueError("the volume has no colour: fuse it with color=True, or pass colors=False")
        box, cells = self._tsdf_box(tsdf)
        col = np.ascontiguousarray(tsdf.color) if colors else None
        views, n, single = self._surface_views(poses, camera, size, zrange)
        depth = [np.empty((v.height, v.width), np.float32) for v in views]
        nrm = [np.empty((v.height, v.width, 3), np.float32) for v in views] if normals else None
        bgr = [np.empty((v.height, v.width, 3), np.uint8) for v in views] if colors else None
        hits, info = np.zeros(n, np.uint32), MapTsdfRayInfo()
        ptrs = lambda arrays: (vp * n)(*[a.ctypes.data for a in arrays]) if arrays is not None else None  # noqa: E731
        prm = self._tsdf_ray_params(step, min_weight, max_steps)
        check(_lib.lib().revo_map_tsdf_raycast(self._h, C.byref(box), cells.ctypes.data_as(vp), col.ctypes.data_as(vp) if colors else None, 0, n,
                                               views, C.byref(prm), ptrs(depth), ptrs(nrm), ptrs(bgr), hits.ctypes.data_as(vp), 0, C.byref(info)))
        pick = (lambda a: None if a is None else a[0]) if single else (lambda a: a)
        return {"depth": pick(depth), "normals": pick(nrm), "bgr": pick(bgr), "hits": int(hits[0]) if single else [int(x) for x in hits],
                "info": {k: int(getattr(info, k)) for k in mapfile.TSDF_RAY_INFO_KEYS}}

    def surface_raycast_into(self, d_depth, d_tsdf, lo, poses, camera=None, size=None, zrange=None, step=None, min_weight=1, max_steps=4096,
                             d_normals=None, d_bgr=None, d_color=None, d_hits=None, d_info=None, wait=True):
        """surface_raycast() between torch device tensors: d_tsdf int32 [n0, n1, n2, 2] as fuse_into leaves it and d_color int32
        [n0, n1, n2, 4] (needed for d_bgr), d_depth float32 [n, h, w] (or [h, w] for one pose), d_normals float32 shaped like
        d_depth + (3,) or None, d_bgr uint8 likewise or None, d_hits None or n 32-bit entries, d_info None or 64 bytes
        (revo_map_tsdf_ray_info); contiguous, on the map's device, every view's part 16-byte aligned.  Only enqueued on the
        context's tracker stream: wait=True returns when it is done, wait=False at once (sync() orders later reads)."""
        if d_tsdf.dim() != 4 or d_tsdf.shape[3] != 2 or str(d_tsdf.dtype) != "torch.int32":
            raise ValueError("d_tsdf must be an int32 tensor [n0, n1, n2, 2]")
        if d_color is not None and (tuple(d_color.shape) != tuple(d_tsdf.shape[:3]) + (4,) or str(d_color.dtype) != "torch.int32"):
            raise ValueError("d_color must be an int32 tensor [n0, n1, n2, 4] over d_tsdf's box")
        if d_bgr is not None and d_color is None:
            raise ValueError("d_bgr needs the colour volume d_color")
        box = self._df_box(lo, tuple(d_tsdf.shape[:3]), 0, 1)
        views, n, single = self._surface_views(poses, camera, size, zrange)
        h, w = views[0].height, views[0].width
        shape = (h, w) if single else (n, h, w)
        if tuple(d_depth.shape) != shape or any(t_ is not None and tuple(t_.shape) != shape + (3,) for t_ in (d_normals, d_bgr)):
            raise ValueError("output tensors do not match the views")
        if str(d_depth.dtype) != "torch.float32" or (d_normals is not None and str(d_normals.dtype) != "torch.float32") or \
                (d_bgr is not None and str(d_bgr.dtype) != "torch.uint8"):
            raise ValueError("d_depth and d_normals must be float32 and d_bgr uint8")
        for t_ in (d_tsdf, d_color, d_depth, d_normals, d_bgr, d_hits, d_info):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("the tensors must be contiguous device tensors")
        if d_hits is not None and (d_hits.numel() != n or d_hits.element_size() != 4):
            raise ValueError("d_hits needs n 32-bit entries")
        if d_info is not None and d_info.numel() * d_info.element_size() != 64:
            raise ValueError("d_info needs 64 bytes")
        ptrs = lambda t_, per: (vp * n)(*[t_.data_ptr() + per * h * w * i for i in range(n)]) if t_ is not None else None  # noqa: E731
        ptr = lambda t_: vp(t_.data_ptr()) if t_ is not None else None  # noqa: E731
        import torch
        torch.cuda.current_stream(d_depth.device).synchronize()  # the tensors' earlier use is over before the tracker stream touches them
        prm = self._tsdf_ray_params(step, min_weight, max_steps)
        check(_lib.lib().revo_map_tsdf_raycast(self._h, C.byref(box), ptr(d_tsdf), ptr(d_color), 1, n, views, C.byref(prm), ptrs(d_depth, 4),
                                               ptrs(d_normals, 12), ptrs(d_bgr, 3), ptr(d_hits), 1, ptr(d_info)))
        if wait:
            self.sync()

    def surface_raycast_many_into(self, jobs, wait=True):
        """The ray casts of many (volume, views) jobs in one call (revo_map_tsdf_raycast_many): every job's tensors hold
        afterwards what surface_raycast_into leaves for that job alone.  A job is a dict: d_tsdf (int32 device tensor [n0, n1, n2, 2]),
        lo, poses (one 4x4 or 1 .. 64 of them), d_depth (float32 [n, h, w], or [h, w] for one pose), and optionally camera, size,
        zrange, step, min_weight, max_steps, d_color (int32 [n0, n1, n2, 4], needed for d_bgr), d_normals, d_bgr, d_hits (n 32-bit
        entries), d_info (64 bytes), map (the VoxelMap that gives the job's voxel edge; default: this one).  The volumes are only
        read, so jobs may share one: several jobs on a volume are more than 64 views of it in one call, and its block mask is built
        once.  1 .. 1024 jobs with at most 4096 views between them, everything on the device; the call is only enqueued on the
        context's tracker stream: wait=False returns at once."""
        import torch
        jobs = list(jobs)
        arr = (MapTsdfRayJob * max(len(jobs), 1))()
        keep = []
        for j, job in zip(arr, jobs):
            m = self._job_map(job)
            d_tsdf, d_color, d_depth = job["d_tsdf"], job.get("d_color"), job["d_depth"]
            d_normals, d_bgr, d_hits, d_info = job.get("d_normals"), job.get("d_bgr"), job.get("d_hits"), job.get("d_info")
            self._surface_tensors(d_tsdf, d_color, "d_tsdf")
            if d_bgr is not None and d_color is None:
                raise ValueError("d_bgr needs the colour volume d_color")
            views, n, single = m._surface_views(job["poses"], job.get("camera"), job.get("size"), job.get("zrange"))
            h, w = views[0].height, views[0].width
            shape = (h, w) if single else (n, h, w)
            if tuple(d_depth.shape) != shape or any(t_ is not None and tuple(t_.shape) != shape + (3,) for t_ in (d_normals, d_bgr)):
                raise ValueError("output tensors do not match the views")
            if str(d_depth.dtype) != "torch.float32" or (d_normals is not None and str(d_normals.dtype) != "torch.float32") or \
                    (d_bgr is not None and str(d_bgr.dtype) != "torch.uint8"):
                raise ValueError("d_depth and d_normals must be float32 and d_bgr uint8")
            for t_ in (d_depth, d_normals, d_bgr, d_hits, d_info):
                if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                    raise ValueError("the tensors must be contiguous device tensors")
            if d_hits is not None and (d_hits.numel() != n or d_hits.element_size() != 4):
                raise ValueError("d_hits needs n 32-bit entries")
            if d_info is not None and d_info.numel() * d_info.element_size() != 64:
                raise ValueError("d_info needs 64 bytes")
            ptrs = lambda t_, per: (vp * n)(*[t_.data_ptr() + per * h * w * i for i in range(n)]) if t_ is not None else None  # noqa: E731
            rows = (ptrs(d_depth, 4), ptrs(d_normals, 12), ptrs(d_bgr, 3))
            j.map = m._h
            j.box = m._df_box(job["lo"], tuple(d_tsdf.shape[:3]), 0, 1)
            j.prm = self._tsdf_ray_params(job.get("step"), job.get("min_weight", 1), job.get("max_steps", 4096))
            j.tsdf = d_tsdf.data_ptr()
            j.color = d_color.data_ptr() if d_color is not None else None
            j.n_views = n
            j.views = C.addressof(views)
            j.depth, j.normal, j.bgr = (C.addressof(r) if r is not None else None for r in rows)
            j.hits = d_hits.data_ptr() if d_hits is not None else None
            j.info = d_info.data_ptr() if d_info is not None else None
            keep.append((views, rows, job))
        if jobs:
            torch.cuda.current_stream(jobs[0]["d_tsdf"].device).synchronize()  # the tensors' earlier use is over before the tracker stream touches them
        check(_lib.lib().revo_map_tsdf_raycast_many(self._h, len(jobs), arr))
        if wait:
            self.sync()
        del keep

    # -- tracking a depth frame against the surface (revo_map_tsdf_track_eval / revo_map_tsdf_track)
    def _surface_track_args(self, tsdf, lo, trunc, frame, max_dist, stride, min_weight, centre):
        """(box, volume pointer, its side, the frame's MapCarveView array, its side, trunc, params, what keeps the memory alive) of a
        tracking call.  tsdf: a numpy array of mapfile.TSDF_CELL_DTYPE cells [n0, n1, n2] or a torch int32 device tensor [n0, n1, n2, 2]
        as fuse_into leaves it; frame: a pyramid (its level-0 depth plane, the context's camera and range) or (depth, camera[,
        zrange]) with depth an [h, w] float32 array or device tensor, camera (fx, fy, cx, cy), an api.Camera or None (the
        context's), zrange (zmin, zmax) or None (the context's).  centre None: the middle of the box."""
        from . import mapfile
        keep = []
        if hasattr(tsdf, "data_ptr"):
            if tsdf.dim() != 4 or tsdf.shape[3] != 2 or str(tsdf.dtype) != "torch.int32" or not (tsdf.is_contiguous() and tsdf.is_cuda):
                raise ValueError("a device volume must be a contiguous int32 tensor [n0, n1, n2, 2]")
            shape, tp, tdev = tuple(int(x) for x in tsdf.shape[:3]), vp(tsdf.data_ptr()), 1
            import torch
            torch.cuda.current_stream(tsdf.device).synchronize()  # the volume is written before the tracker stream reads it
        else:
            tsdf = np.ascontiguousarray(tsdf)
            if tsdf.dtype != mapfile.TSDF_CELL_DTYPE or tsdf.ndim != 3:
                raise ValueError("a TSDF volume is a 3-D array of (sum int32, weight uint32) cells")
            shape, tp, tdev = tsdf.shape, tsdf.ctypes.data_as(vp), 0
        keep.append(tsdf)
        if isinstance(frame, ImgPyramidRGBD):
            view = (frame, np.eye(4, dtype=np.float32))
        else:
            frame = tuple(frame)
            if not 2 <= len(frame) <= 3:
                raise ValueError("a frame is a pyramid or (depth, camera[, zrange])")
            cam, zr = frame[1], frame[2] if len(frame) > 2 else None
            if cam is None:
                if zr is not None:
                    raise ValueError("a zrange goes with a camera: without one the context's camera and range are used")
                k = None
            else:
                if isinstance(cam, Camera):
                    cam = (cam.fx, cam.fy, cam.cx, cam.cy)
                st = self.cameraPyr.settings
                k = tuple(cam) + (tuple(zr) if zr is not None else (st.depth_min, st.depth_max))
            view = (frame[0], np.eye(4, dtype=np.float32), k)
        cv, device_in, kv = self._carve_views([view])
        keep.append(kv)
        if int(stride) < 0 or int(min_weight) < 0:
            raise ValueError("stride and min_weight are >= 0")
        if centre is None:
            centre = mapfile.tsdf_track_centre(lo, shape, self.voxel)
        p = MapTsdfTrackParams()
        p.max_dist, p.stride, p.min_weight = 0.0 if max_dist is None else float(max_dist), int(stride), int(min_weight)
        p.centre[:] = [float(x) for x in np.asarray(centre, np.float32).reshape(3)]
        return self._df_box(lo, shape, 0, 1), tp, tdev, cv, device_in, float(trunc), p, keep

    def surface_track_eval(self, tsdf, lo, trunc, frame, poses, max_dist=None, stride=1, min_weight=1, centre=None, d_out=None):
        """The tracking sums of a depth frame against the TSDF volume `tsdf` of the box at lo (fused at this map's voxel edge with the
        truncation distance trunc) at each camera pose T_w_c (one 4x4 or [n, 4, 4], 1 .. 4096): MapTsdfTrackInfo records, all from
        one launch (revo_map_tsdf_track_eval).  tsdf, frame, centre: see _surface_track_args.  max_dist defaults to trunc / 2.
        d_out: a torch uint8 device tensor of n x 208 bytes takes the records instead (returns None; with a device volume and a
        device or pyramid frame the call only enqueues: sync() orders later reads)."""
        T = np.asarray(poses, np.float32)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        n = len(T)
        flat = np.ascontiguousarray(np.concatenate([_cm4(M) for M in T]))
        box, tp, tdev, cv, din, tr, p, keep = self._surface_track_args(tsdf, lo, trunc, frame, max_dist, stride, min_weight, centre)
        if d_out is not None:
            if not (d_out.is_cuda and d_out.is_contiguous() and d_out.numel() * d_out.element_size() >= n * C.sizeof(MapTsdfTrackInfo)):
                raise ValueError("d_out must be a contiguous device tensor of n x %d bytes" % C.sizeof(MapTsdfTrackInfo))
            import torch
            torch.cuda.current_stream(d_out.device).synchronize()
            check(_lib.lib().revo_map_tsdf_track_eval(self._h, C.byref(box), tp, tdev, tr, cv, din, n, _p(flat, f32p), C.byref(p), vp(d_out.data_ptr()), 1))
            return None
        out = (MapTsdfTrackInfo * n)()
        check(_lib.lib().revo_map_tsdf_track_eval(self._h, C.byref(box), tp, tdev, tr, cv, din, n, _p(flat, f32p), C.byref(p), C.cast(out, vp), 0))
        return out[0] if single else list(out)

    def surface_track(self, tsdf, lo, trunc, frame, T_init, max_dist=None, stride=1, min_weight=1, centre=None, max_iters=30, eps_t=1e-6,
                      eps_r=1e-6, min_matched=12):
        """Gauss-Newton of the frame's camera pose onto the surface from T_init over surface_track_eval's records
        (revo_map_tsdf_track): align()'s loop, options and statuses.  -> dict: T (the refined T_w_c), info (the MapTsdfTrackInfo at T),
        iterations, status, cov = sigma2 H^-1 with sigma2 = S[27] / (matched - 6), sigma2, centre."""
        T0 = np.asarray(T_init, np.float32).reshape(4, 4)
        box, tp, tdev, cv, din, tr, p, keep = self._surface_track_args(tsdf, lo, trunc, frame, max_dist, stride, min_weight, centre)
        o = MapAlignOpts(int(max_iters), 0, float(eps_t), float(eps_r), int(min_matched))
        T1 = np.zeros(16, np.float32)
        info, it, st = MapTsdfTrackInfo(), C.c_int32(), C.c_int32()
        check(_lib.lib().revo_map_tsdf_track(self._h, C.byref(box), tp, tdev, tr, cv, din, _p(_cm4(T0), f32p), C.byref(p), C.byref(o), _p(T1, f32p),
                                             C.byref(info), C.byref(it), C.byref(st)))
        cov, s2 = tsdf_track_covariance(info)
        return {"T": T1.reshape(4, 4).T.copy(), "info": info, "iterations": it.value, "status": st.value, "cov": cov, "sigma2": s2,
                "centre": np.array(list(p.centre), np.float32)}

    # -- surfaces for many sequences at once (revo_map_tsdf_fuse_many / _track_eval_many / _track_many)
    def _job_map(self, job):
        m = job.get("map")
        m = self if m is None else (m.map if isinstance(m, MapWindow) else m)
        if not isinstance(m, VoxelMap):
            raise ValueError("a job's map is a VoxelMap (or a MapWindow) of this map's context")
        return m

    def _fuse_jobs(self, jobs):
        """-> (the revo_map_tsdf_fuse_job array of fuse_many_into's jobs, how many, what keeps the memory alive)."""
        import torch
        from . import mapfile
        jobs = list(jobs)
        arr = (MapTsdfFuseJob * max(len(jobs), 1))()
        keep = []
        for j, job in zip(arr, jobs):
            m = self._job_map(job)
            d_tsdf, d_color = job["d_tsdf"], job.get("d_color")
            self._surface_tensors(d_tsdf, d_color, "d_tsdf")
            view = tuple(job["view"])
            if d_color is not None:
                cv, device_in, kv, bgr, kc_ = m._color_views([view])
                j.bgr = bgr[0]
                keep.append(kc_)
            else:
                cv, device_in, kv = m._carve_views([view])
            if not isinstance(view[0], ImgPyramidRGBD) and not device_in:
                raise ValueError("the images of a batched fuse are device tensors")
            keep.append(kv)
            j.map = m._h
            j.box = m._df_box(job["lo"], tuple(d_tsdf.shape[:3]), 0, 1)
            j.trunc = float(mapfile.tsdf_trunc(m.voxel, job.get("trunc")))
            j.tsdf = d_tsdf.data_ptr()
            j.color = d_color.data_ptr() if d_color is not None else None
            C.memmove(C.byref(j.view), C.byref(cv[0]), C.sizeof(MapCarveView))
            for key, field, size in (("d_info", "info", 64), ("d_color_info", "color_info", 32), ("d_view_info", "view_info", 32)):
                t_ = job.get(key)
                if t_ is None:
                    continue
                if not (t_.is_contiguous() and t_.is_cuda and t_.numel() * t_.element_size() == size):
                    raise ValueError("d_info needs 64 bytes, d_view_info and d_color_info 32 bytes each, contiguous on the device")
                setattr(j, field, t_.data_ptr())
            keep.append(job)
        if jobs:
            torch.cuda.current_stream(jobs[0]["d_tsdf"].device).synchronize()  # the tensors' earlier use is over before the tracker stream writes
        return arr, len(jobs), keep

    def fuse_many_into(self, jobs, wait=True):
        """Many (volume, view) fuses in one launch (revo_map_tsdf_fuse_many): every job's volumes hold afterwards what
        fuse_into(..., accumulate=True) leaves for that job alone.  A job is a dict: d_tsdf (int32 device tensor [n0, n1, n2, 2]), lo,
        view (as fuse_into takes one: a pyramid view, or a raw view with device images -- (depth, T, intrinsics or None[, bgr])), and
        optionally trunc, d_color (int32 [n0, n1, n2, 4]), map (the VoxelMap that gives the job's voxel edge; default: this one),
        d_info (64 bytes), d_color_info (32 bytes), d_view_info (32 bytes).  1 .. 1024 jobs, everything on the device; the call is
        only enqueued on the context's tracker stream: wait=False returns at once."""
        arr, n, keep = self._fuse_jobs(jobs)
        check(_lib.lib().revo_map_tsdf_fuse_many(self._h, n, arr))
        if wait:
            self.sync()
        del keep

    def unfuse_many_into(self, jobs, wait=True, d_results=None):
        """Many (volume, view) unfuses in a check and an apply launch (revo_map_tsdf_unfuse_many): per job what
        unfuse_into(d_tsdf, [view], ...) does for that job alone, except that a refusal is the job's result and not an error --
        a job with a misfit changes nothing, every other job is applied.  A job is a dict as fuse_many_into takes it, without
        d_color_info; trunc is what the view was fused with; d_info is 64 bytes of revo_map_tsdf_unfuse_info.  The verdict stays
        on the device: nothing waits between the passes.
        wait=True -> a list of (info dict of mapfile.TSDF_UNFUSE_INFO_KEYS, status) per job, status 0 or -1 (REVO_ERR_INVALID_ARG,
        refused), from host results: the call's one wait.  wait=False -> None, the call only enqueued; d_results (a contiguous
        device tensor of 80 bytes per job, revo_map_tsdf_unfuse_result) then takes the records, status included."""
        import torch
        from . import mapfile
        jobs = list(jobs)
        fj, n, keep = self._fuse_jobs(jobs)
        arr = (MapTsdfUnfuseJob * max(n, 1))()
        for j, f, job in zip(arr, fj, jobs):
            if job.get("d_color_info") is not None:
                raise ValueError("an unfuse job has no d_color_info: its info holds the colour counters")
            for name, _t in MapTsdfUnfuseJob._fields_:
                setattr(j, name, getattr(f, name))
        if d_results is not None:
            if wait:
                raise ValueError("d_results goes with wait=False: wait=True returns the host results")
            if not (d_results.is_cuda and d_results.is_contiguous() and d_results.numel() * d_results.element_size() == 80 * n):
                raise ValueError("d_results needs 80 bytes per job, contiguous on the device")
            torch.cuda.current_stream(d_results.device).synchronize()
        res = (MapTsdfUnfuseResult * max(n, 1))() if wait else None
        check(_lib.lib().revo_map_tsdf_unfuse_many(self._h, n, arr, C.cast(res, vp) if wait else (vp(d_results.data_ptr()) if d_results is not None else None),
                                                   0 if wait else 1))
        del keep
        if not wait:
            return None
        return [({k: int(getattr(r.info, k)) for k in mapfile.TSDF_UNFUSE_INFO_KEYS}, int(r.status)) for r in res[:n]]

    def _track_jobs(self, jobs, with_poses):
        """-> (the revo_map_tsdf_track_job array of a batched tracking call, the poses per job, what keeps the memory alive).  A job is a
        dict: tsdf (int32 device tensor), lo, trunc, frame (a pyramid or (device depth, camera[, zrange])), poses (with_poses: one 4x4 or
        [n, 4, 4]) or T_init, and optionally max_dist, stride, min_weight, centre, map and (the loop) max_iters, the job's own limit."""
        jobs = list(jobs)
        arr = (MapTsdfTrackJob * max(len(jobs), 1))()
        keep, counts = [], []
        for j, job in zip(arr, jobs):
            m = self._job_map(job)
            box, tp, tdev, cv, din, tr, p, kp = m._surface_track_args(job["tsdf"], job["lo"], job["trunc"], job["frame"], job.get("max_dist"),
                                                                      job.get("stride", 1), job.get("min_weight", 1), job.get("centre"))
            if not tdev or (not isinstance(job["frame"], ImgPyramidRGBD) and not din):
                raise ValueError("the volumes and images of a batched tracking call are device tensors")
            T = np.asarray(job["poses"] if with_poses else job["T_init"], np.float32).reshape(-1, 4, 4)
            if not with_poses and len(T) != 1:
                raise ValueError("T_init is one 4x4 pose")
            flat = np.ascontiguousarray(np.concatenate([_cm4(M) for M in T]) if len(T) else np.zeros(0, np.float32))
            keep += [kp, flat]
            counts.append(len(T))
            j.map, j.box, j.trunc, j.n_poses, j.tsdf = m._h, box, tr, len(T) if with_poses else int(job.get("max_iters") or 0), tp
            C.memmove(C.byref(j.frame), C.byref(cv[0]), C.sizeof(MapCarveView))
            j.prm = p
            j.poses = flat.ctypes.data
        return arr, len(jobs), counts, keep

    def surface_track_eval_many(self, jobs, d_out=None):
        """The tracking sums of many (volume, frame) jobs, all poses of all jobs in one launch (revo_map_tsdf_track_eval_many; at most 4096
        poses in total): per job the MapTsdfTrackInfo records surface_track_eval gives for it alone -> a list of lists.  jobs: see
        _track_jobs.  d_out: a torch uint8 device tensor of (all poses) x 208 bytes takes the records, job after job, instead
        (returns None; the call only enqueues)."""
        arr, n, counts, keep = self._track_jobs(jobs, True)
        total = sum(counts)
        if d_out is not None:
            if not (d_out.is_cuda and d_out.is_contiguous() and d_out.numel() * d_out.element_size() >= total * C.sizeof(MapTsdfTrackInfo)):
                raise ValueError("d_out must be a contiguous device tensor of (all poses) x %d bytes" % C.sizeof(MapTsdfTrackInfo))
            import torch
            torch.cuda.current_stream(d_out.device).synchronize()
            check(_lib.lib().revo_map_tsdf_track_eval_many(self._h, n, arr, vp(d_out.data_ptr()), 1))
            return None
        out = (MapTsdfTrackInfo * max(total, 1))()
        check(_lib.lib().revo_map_tsdf_track_eval_many(self._h, n, arr, C.cast(out, vp), 0))
        del keep
        recs, at = [], 0
        for c in counts:
            recs.append([out[at + i] for i in range(c)])
            at += c
        return recs

    def surface_track_many(self, jobs, max_iters=30, eps_t=1e-6, eps_r=1e-6, min_matched=12):
        """surface_track's Gauss-Newton loop for many (volume, frame, T_init) jobs in lockstep (revo_map_tsdf_track_many): one launch, one
        copy and one wait per round for all jobs.  -> (a list of dicts as surface_track gives them, plus `evaluations`; rounds)."""
        arr, n, _, keep = self._track_jobs(jobs, False)
        o = MapAlignOpts(int(max_iters), 0, float(eps_t), float(eps_r), int(min_matched))
        res, rounds = (MapTsdfTrackResult * max(n, 1))(), C.c_int32()
        check(_lib.lib().revo_map_tsdf_track_many(self._h, n, arr, C.byref(o), res, C.byref(rounds)))
        del keep
        out = []
        for j, r in zip(arr, res):
            info = MapTsdfTrackInfo.from_buffer_copy(bytes(r.info))
            cov, s2 = tsdf_track_covariance(info)
            out.append({"T": np.array(list(r.T), np.float32).reshape(4, 4).T.copy(), "info": info, "iterations": int(r.iterations), "status": int(r.status),
                        "cov": cov, "sigma2": s2, "centre": np.array(list(j.prm.centre), np.float32), "evaluations": int(r.evaluations)})
        return out, int(rounds.value)

    def frontiers(self, seen, min_views=1, min_count=1):
        """Where known space ends -> [k, 3] int32 voxel indices in ascending order of the cell's place in the box: the cells
        of a SeenVolume that are not solid, have >= min_views free votes and have a face neighbour inside the box that is
        neither solid nor known (revo_map_frontiers).  DistanceField.plan takes them as goals."""
        box, vol = self._seen_box(seen)
        L, k = _lib.lib(), C.c_size_t()
        args = (self._h, C.byref(box), int(min_count), vol.ctypes.data_as(vp), 0, int(min_views))
        check(L.revo_map_frontiers(*args, None, 0, C.byref(k), 0))
        rec = np.zeros(k.value, np.dtype([("cell", "<i4", (3,)), ("cost0", "<u4")]))
        if k.value:
            check(L.revo_map_frontiers(*args, rec.ctypes.data_as(vp), k.value, C.byref(k), 0))
        return rec["cell"][:k.value].copy()

    def frontiers_into(self, d_cells, d_seen, lo, min_views=1, min_count=1):
        """frontiers() between torch device tensors: d_seen the seen volume (3-D uint8), d_cells room for 16-byte records
        (revo_map_plan_seed: the cell, cost0 = 0) or None to count only -> the number of frontier cells; the records come in
        unspecified order.  RevoError (REVO_ERR_CAPACITY), nothing written, when d_cells holds fewer."""
        if d_seen.dim() != 3 or str(d_seen.dtype) != "torch.uint8" or not (d_seen.is_contiguous() and d_seen.is_cuda):
            raise ValueError("d_seen must be a contiguous 3-D uint8 device tensor")
        if d_cells is not None and not (d_cells.is_contiguous() and d_cells.is_cuda):
            raise ValueError("d_cells must be a contiguous device tensor")
        box = self._df_box(lo, tuple(d_seen.shape), 0, 1)
        import torch
        torch.cuda.current_stream(d_seen.device).synchronize()
        k = C.c_size_t()
        cap = 0 if d_cells is None else d_cells.numel() * d_cells.element_size() // 16
        check(_lib.lib().revo_map_frontiers(self._h, C.byref(box), int(min_count), vp(d_seen.data_ptr()), 1, int(min_views),
                                            vp(d_cells.data_ptr()) if d_cells is not None else None, cap, C.byref(k), 1))
        return int(k.value)

    # -- what a view would add (revo_map_view_gain)
    def _gain_camera(self, camera, size, zrange, min_count):
        """-> MapView without a pose.  camera None: the context's level-0 camera, size and depth range (size and zrange are then
        not given); else an api.Camera or (fx, fy, cx, cy) with size (width, height) -- the Camera's own by default -- and
        zrange (zmin, zmax) or None = the context's range."""
        s = self.cameraPyr.settings
        v = MapView()
        if camera is None:
            if size is not None or zrange is not None:
                raise ValueError("size and zrange go with a camera: without one the context's camera, size and range are used")
            v.width, v.height = int(s.width), int(s.height)
        else:
            if isinstance(camera, Camera):
                size = (camera.width, camera.height) if size is None else size
                camera = (camera.fx, camera.fy, camera.cx, camera.cy)
            if len(camera) != 4 or size is None:
                raise ValueError("a camera is (fx, fy, cx, cy) with a size (width, height)")
            zmin, zmax = zrange if zrange is not None else (s.depth_min, s.depth_max)
            v.width, v.height = int(size[0]), int(size[1])
            v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax = [float(x) for x in tuple(camera) + (zmin, zmax)]
        v.T_w_c[:] = _cm4(np.eye(4, dtype=np.float32)).tolist()
        v.min_count = int(min_count)
        return v

    def _gain_params(self, min_views, radius, margin, margin_rel, miss_depth, max_steps):
        return MapGainParams(int(radius), int(min_views), float(self.voxel if margin is None else margin), float(margin_rel), float(miss_depth),
                             int(max_steps))

    def view_gain(self, seen, poses, camera=None, size=None, min_views=1, radius=1, margin=None, margin_rel=0.0, miss_depth=0.0, min_count=1,
                  max_steps=4096, zrange=None):
        """What a depth view from each of `poses` (one 4x4 camera -> world pose, or 1 .. 4096 of them) would add to `seen` (a
        SeenVolume; its box is the call's) -> mapfile.GainRecords: per pose unknown_free, unknown_surface, unknown_inside -- the
        cells that are unknown now (not solid, fewer than min_views free votes, no surface bit) and would be seen free, on a
        surface, or lie inside the view at all -- and hits, the pixels of the predicted depth image that show a voxel; `.info`
        holds the call's sums (mapfile.GAIN_INFO_KEYS).  The predicted image is raycast()'s from that pose, the class of a cell
        observe()'s; nothing is observed or written (revo_map_view_gain).  camera, size, zrange: see _gain_camera.
        miss_depth 0: a ray that hits nothing leaves a depth hole, as a sensor would; else the depth such a pixel is read as
        (free space seen up to there)."""
        from . import mapfile
        box, vol = self._seen_box(seen)
        T = mapfile.gain_poses(poses)
        cm = np.ascontiguousarray(T.transpose(0, 2, 1))
        cam = self._gain_camera(camera, size, zrange, min_count)
        prm = self._gain_params(min_views, radius, margin, margin_rel, miss_depth, max_steps)
        out = np.zeros(len(T), mapfile.GAIN_DTYPE)
        info = MapGainInfo()
        check(_lib.lib().revo_map_view_gain(self._h, C.byref(box), vol.ctypes.data_as(vp), 0, C.byref(cam), len(T), cm.ctypes.data_as(vp), 0,
                                            C.byref(prm), out.ctypes.data_as(vp), 0, C.byref(info)))
        return mapfile.gain_result(out, {k: int(getattr(info, k)) for k in mapfile.GAIN_INFO_KEYS})

    def view_gain_into(self, d_out, d_seen, lo, d_poses, camera=None, size=None, min_views=1, radius=1, margin=None, margin_rel=0.0, miss_depth=0.0,
                       min_count=1, max_steps=4096, zrange=None, d_info=None, wait=True):
        """view_gain() between torch device tensors: d_seen the seen volume (3-D uint8; its shape is the box's n), d_poses
        [k, 16] or [k, 4, 4] float32 with every pose COLUMN-major (a row-major pose transposed), d_out 32 bytes per pose
        (revo_map_gain), d_info None or 64 bytes (revo_map_gain_info); contiguous, 16-byte aligned, on the map's device.  Poses
        in device memory are not checked: one that is not finite or not orthogonal gets an all-zero record.  The call is only
        enqueued on the context's tracker stream: wait=False returns at once (sync() orders later reads)."""
        if d_seen.dim() != 3 or str(d_seen.dtype) != "torch.uint8":
            raise ValueError("d_seen must be a 3-D uint8 tensor")
        if str(d_poses.dtype) != "torch.float32" or d_poses.numel() % 16 or d_poses.numel() == 0:
            raise ValueError("d_poses must hold 16 float32 numbers per pose")
        k = d_poses.numel() // 16
        for t_, size_ in ((d_seen, None), (d_poses, None), (d_out, 32 * k), (d_info, 64)):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("tensors must be contiguous device tensors")
            if t_ is not None and size_ is not None and t_.numel() * t_.element_size() != size_:
                raise ValueError("d_out needs 32 bytes per pose and d_info 64 bytes")
        box = self._df_box(lo, tuple(d_seen.shape), 0, 1)
        cam = self._gain_camera(camera, size, zrange, min_count)
        prm = self._gain_params(min_views, radius, margin, margin_rel, miss_depth, max_steps)
        import torch
        torch.cuda.current_stream(d_out.device).synchronize()  # the inputs are written, the outputs' earlier use is over
        check(_lib.lib().revo_map_view_gain(self._h, C.byref(box), vp(d_seen.data_ptr()), 1, C.byref(cam), k, vp(d_poses.data_ptr()), 1, C.byref(prm),
                                            vp(d_out.data_ptr()), 1, vp(d_info.data_ptr()) if d_info is not None else None))
        if wait:
            self.sync()

    def distance_field_into(self, d_d2, lo, n, min_count=1, clamp=0, d_info=None, wait=True):
        """distance_field() into a torch device tensor: d_d2 of shape n with 32-bit integers, d_info None or a 64-byte tensor
        (revo_map_df_info); contiguous, 16-byte aligned, on the map's device.  Enqueued on the context's tracker stream: wait=True
        returns when it is done, wait=False at once (sync() orders later reads)."""
        box = self._df_box(lo, n, 0, min_count)
        if tuple(d_d2.shape) != tuple(box.n) or d_d2.element_size() != 4 or d_d2.is_floating_point():
            raise ValueError("d_d2 must be a 32-bit integer tensor of the box's shape")
        for t_ in (d_d2, d_info):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("output tensors must be contiguous device tensors")
        if d_info is not None and d_info.numel() * d_info.element_size() != 64:
            raise ValueError("d_info needs 64 bytes")
        import torch
        torch.cuda.current_stream(d_d2.device).synchronize()  # the tensors' earlier use is over before the tracker stream writes
        check(_lib.lib().revo_map_distance_field(self._h, C.byref(box), int(min_count), int(clamp), vp(d_d2.data_ptr()), 1,
                                                 vp(d_info.data_ptr()) if d_info is not None else None))
        if wait:
            self.sync()

    def df_sample(self, field, points):
        """Distance and gradient at points ([N, 3] float32 metres, the map's frame) from a DistanceField of a map with this
        map's voxel edge (revo_map_df_sample) -> a mapfile.DF_SAMPLE_DTYPE array: dist in metres (-1: outside the box, +inf:
        the box holds no voxel), grad dimensionless."""
        from . import mapfile
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        out = np.zeros(len(p), mapfile.DF_SAMPLE_DTYPE)
        if len(p) == 0:
            return out
        d2 = np.ascontiguousarray(field.d2, np.uint32)
        box = self._df_box(field.lo, d2.shape, 0, 1)
        check(_lib.lib().revo_map_df_sample(self._h, C.byref(box), d2.ctypes.data_as(vp), 0, len(p), p.ctypes.data_as(vp), 0,
                                            out.ctypes.data_as(vp), 0))
        return out

    def sample_into(self, d_out, d_d2, lo, d_points, wait=True):
        """df_sample() between torch device tensors: d_d2 the field (32-bit integers, its shape is the box's n), d_points
        [N, 3] float32, d_out [N, 4] float32 (dist, grad x y z); contiguous, 16-byte aligned, on the map's device."""
        if d_d2.dim() != 3 or d_d2.element_size() != 4 or d_d2.is_floating_point():
            raise ValueError("d_d2 must be a 3-D tensor of 32-bit integers")
        n = int(d_points.shape[0])
        if tuple(d_points.shape) != (n, 3) or tuple(d_out.shape) != (n, 4) or str(d_points.dtype) != "torch.float32" or str(d_out.dtype) != "torch.float32":
            raise ValueError("d_points must be [N, 3] and d_out [N, 4] float32")
        for t_ in (d_out, d_d2, d_points):
            if not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("tensors must be contiguous device tensors")
        box = self._df_box(lo, tuple(d_d2.shape), 0, 1)
        import torch
        torch.cuda.current_stream(d_out.device).synchronize()  # the inputs are written, the output's earlier use is over
        check(_lib.lib().revo_map_df_sample(self._h, C.byref(box), vp(d_d2.data_ptr()), 1, n, vp(d_points.data_ptr()), 1, vp(d_out.data_ptr()), 1))
        if wait:
            self.sync()

    # -- registration against a distance field (revo_map_df_align_eval / revo_map_df_align)
    def _df_align_args(self, d2, lo, points, max_dist, centre, T_first):
        """(box, field pointer, its side, points pointer, their side, n, params, what keeps the memory alive) of a call: d2 and
        points are numpy arrays or, as sample_into takes them, contiguous torch device tensors (then the current stream is
        waited for).  centre None: the mean of the points under T_first in float64, rounded to float32."""
        keep = []
        on_device = False
        if hasattr(d2, "data_ptr"):
            if d2.dim() != 3 or d2.element_size() != 4 or d2.is_floating_point() or not (d2.is_contiguous() and d2.is_cuda):
                raise ValueError("a device field must be a contiguous 3-D tensor of 32-bit integers")
            shape, fp, fdev, on_device = tuple(d2.shape), vp(d2.data_ptr()), 1, True
        else:
            d2 = np.ascontiguousarray(d2, np.uint32)
            if d2.ndim != 3:
                raise ValueError("the field is a 3-D array")
            shape, fp, fdev = d2.shape, d2.ctypes.data_as(vp), 0
        keep.append(d2)
        if hasattr(points, "data_ptr"):
            if points.dim() != 2 or points.shape[1] != 3 or str(points.dtype) != "torch.float32" or not (points.is_contiguous() and points.is_cuda):
                raise ValueError("device points must be a contiguous [N, 3] float32 tensor")
            n, pp, pdev, on_device = int(points.shape[0]), vp(points.data_ptr()), 1, True
            mean = points.double().mean(0).cpu().numpy() if n else np.zeros(3)
        else:
            points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
            n, pp, pdev = len(points), points.ctypes.data_as(vp), 0
            mean = points.astype(np.float64).mean(0) if n else np.zeros(3)
        keep.append(points)
        if n < 1:
            raise ValueError("no points to register")
        if centre is None:
            T = np.asarray(T_first, np.float32).astype(np.float64)
            centre = (T[:3, :3] @ mean + T[:3, 3]).astype(np.float32)
        p = MapAlignParams()
        p.max_dist, p.min_count_dst, p.min_count_src = float(max_dist), 0, 0
        p.centre[:] = [float(x) for x in np.asarray(centre, np.float32).reshape(3)]
        if on_device:
            import torch
            torch.cuda.current_stream("cuda:%d" % self.cameraPyr.device).synchronize()  # the inputs are written
        return self._df_box(lo, shape, 0, 1), fp, fdev, pp, pdev, n, p, keep

    def df_align_eval(self, d2, lo, points, poses, max_dist, centre=None, d_out=None):
        """The registration sums of `points` ([N, 3] float32, source frame) against the distance field d2 of the box at lo
        (a field of a map with this map's voxel edge) at each pose (4x4 source -> field frame; one pose or [n, 4, 4]):
        MapDfAlignInfo records, all from one launch (revo_map_df_align_eval).  centre defaults to the mean of the points under
        the first pose.  d_out: a torch uint8 device tensor of n x 208 bytes takes the records instead (returns None; with
        a device field and device points the call only enqueues: sync() orders later reads)."""
        T = np.asarray(poses, np.float32)
        single = T.ndim == 2
        T = T.reshape(-1, 4, 4)
        n = len(T)
        flat = np.ascontiguousarray(np.concatenate([_cm4(M) for M in T]))
        box, fp, fdev, pp, pdev, npts, p, keep = self._df_align_args(d2, lo, points, max_dist, centre, T[0])
        if d_out is not None:
            if not (d_out.is_cuda and d_out.is_contiguous() and d_out.numel() * d_out.element_size() >= n * C.sizeof(MapDfAlignInfo)):
                raise ValueError("d_out must be a contiguous device tensor of n x %d bytes" % C.sizeof(MapDfAlignInfo))
            import torch
            torch.cuda.current_stream(d_out.device).synchronize()
            check(_lib.lib().revo_map_df_align_eval(self._h, C.byref(box), fp, fdev, npts, pp, pdev, n, _p(flat, f32p), C.byref(p),
                                                    vp(d_out.data_ptr()), 1))
            return None
        out = (MapDfAlignInfo * n)()
        check(_lib.lib().revo_map_df_align_eval(self._h, C.byref(box), fp, fdev, npts, pp, pdev, n, _p(flat, f32p), C.byref(p),
                                                C.cast(out, vp), 0))
        return out[0] if single else list(out)

    def df_align(self, d2, lo, points, T_init=None, max_dist=None, centre=None, max_iters=30, eps_t=1e-6, eps_r=1e-6, min_matched=12):
        """Gauss-Newton of `points` onto the distance field from T_init (identity by default) over df_align_eval's records
        (revo_map_df_align): align()'s loop, options and statuses.  max_dist defaults to 8 voxels.  -> dict: T, info (the
        MapDfAlignInfo at T), iterations, status, cov = sigma2 H^-1 with sigma2 = S[27] / (matched - 6), sigma2, centre."""
        T0 = np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32).reshape(4, 4)
        max_dist = 8.0 * self.voxel if max_dist is None else max_dist
        box, fp, fdev, pp, pdev, npts, p, keep = self._df_align_args(d2, lo, points, max_dist, centre, T0)
        o = MapAlignOpts(int(max_iters), 0, float(eps_t), float(eps_r), int(min_matched))
        T1 = np.zeros(16, np.float32)
        info, it, st = MapDfAlignInfo(), C.c_int32(), C.c_int32()
        check(_lib.lib().revo_map_df_align(self._h, C.byref(box), fp, fdev, npts, pp, pdev, _p(_cm4(T0), f32p), C.byref(p), C.byref(o),
                                           _p(T1, f32p), C.byref(info), C.byref(it), C.byref(st)))
        cov, s2 = df_align_covariance(info)
        return {"T": T1.reshape(4, 4).T.copy(), "info": info, "iterations": it.value, "status": st.value, "cov": cov, "sigma2": s2,
                "centre": np.array(list(p.centre), np.float32)}

    # -- planning through the map (revo_map_plan / revo_map_plan_paths)
    @staticmethod
    def _plan_seeds(seeds):
        from . import mapfile
        s = mapfile.plan_seeds(seeds)
        rec = np.zeros(len(s), np.dtype([("cell", "<i4", (3,)), ("cost0", "<u4")]))
        rec["cell"], rec["cost0"] = s[:, :3], s[:, 3]
        assert rec.itemsize == C.sizeof(MapPlanSeed)
        return rec

    @staticmethod
    def _plan_info(i):
        from . import mapfile
        return {k: int(getattr(i, k)) for k in mapfile.PLAN_INFO_KEYS}

    def plan(self, field, seeds, r2, max_rounds=0):
        """The clearance-aware cost-to-go over a DistanceField of a map with this map's voxel edge (revo_map_plan)
        -> (cost uint32 [n0, n1, n2], info dict of mapfile.PLAN_INFO_KEYS).  A cell is free iff d2 >= r2; seeds: what
        mapfile.plan_seeds takes as integers ([k, 3] cells or [k, 4] with cost0).  RevoError (REVO_ERR_CAPACITY) when the
        relaxation has not settled within max_rounds (0: 65 536)."""
        d2 = np.ascontiguousarray(field.d2, np.uint32)
        box = self._df_box(field.lo, d2.shape, 0, 1)
        rec = self._plan_seeds(seeds)
        cost = np.empty(d2.shape, np.uint32)
        info = MapPlanInfo()
        check(_lib.lib().revo_map_plan(self._h, C.byref(box), d2.ctypes.data_as(vp), 0, int(r2), len(rec), rec.ctypes.data_as(vp), int(max_rounds),
                                       cost.ctypes.data_as(vp), 0, C.byref(info)))
        return cost, self._plan_info(info)

    def plan_into(self, d_cost, d_d2, lo, n, seeds, r2, max_rounds=0, d_info=None):
        """plan() between torch device tensors: d_d2 the field and d_cost the cost (32-bit integers of the box's shape n),
        d_info None or a 64-byte tensor (revo_map_plan_info); contiguous, 16-byte aligned, on the map's device.  The call
        waits: the host decides when the relaxation has settled."""
        box = self._df_box(lo, n, 0, 1)
        for t_ in (d_cost, d_d2):
            if tuple(t_.shape) != tuple(box.n) or t_.element_size() != 4 or t_.is_floating_point():
                raise ValueError("d_cost and d_d2 must be 32-bit integer tensors of the box's shape")
        for t_ in (d_cost, d_d2, d_info):
            if t_ is not None and not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("tensors must be contiguous device tensors")
        if d_info is not None and d_info.numel() * d_info.element_size() != 64:
            raise ValueError("d_info needs 64 bytes")
        rec = self._plan_seeds(seeds)
        import torch
        torch.cuda.current_stream(d_cost.device).synchronize()  # the field is written, the outputs' earlier use is over
        check(_lib.lib().revo_map_plan(self._h, C.byref(box), vp(d_d2.data_ptr()), 1, int(r2), len(rec), rec.ctypes.data_as(vp), int(max_rounds),
                                       vp(d_cost.data_ptr()), 1, vp(d_info.data_ptr()) if d_info is not None else None))

    def plan_paths(self, cost, lo, starts, max_len=4096):
        """Paths down a cost field (revo_map_plan_paths) -> a list of (cells int32 [length, 3], status, cost) per start, what
        mapfile.plan_paths gives.  cost: a uint32 [n0, n1, n2] array; starts: [k, 3] voxel indices."""
        cost = np.ascontiguousarray(cost, np.uint32)
        if cost.ndim != 3:
            raise ValueError("the cost field is a 3-D array")
        box = self._df_box(lo, cost.shape, 0, 1)
        st = np.ascontiguousarray(np.asarray(starts, np.int64).reshape(-1, 3).astype(np.int32))
        max_len = int(max_len)
        if len(st) < 1 or max_len < 1 or len(st) * max_len > 1 << 26:
            raise ValueError("at least one start and one cell, and at most 2^26 path cells per call")
        cells = np.zeros((len(st), max_len, 3), np.int32)
        rec = (MapPlanPath * len(st))()
        check(_lib.lib().revo_map_plan_paths(self._h, C.byref(box), cost.ctypes.data_as(vp), 0, len(st), st.ctypes.data_as(vp), max_len,
                                             cells.ctypes.data_as(vp), C.cast(rec, vp), 0))
        return [(cells[i, :r.length].copy(), int(r.status), int(r.cost)) for i, r in enumerate(rec)]

    def plan_paths_into(self, d_cells, d_paths, d_cost, lo, starts, max_len, wait=True):
        """plan_paths() between torch device tensors: d_cost the cost field (32-bit integers, its shape is the box's n),
        d_cells [k, max_len, 3] int32, d_paths k x 16 bytes (revo_map_plan_path: length, status, cost, 0); contiguous,
        16-byte aligned, on the map's device.  starts: [k, 3] voxel indices in host memory.  Entries of d_cells past a
        path's length are not written.  Enqueued on the context's tracker stream: wait=False returns at once."""
        if d_cost.dim() != 3 or d_cost.element_size() != 4 or d_cost.is_floating_point():
            raise ValueError("d_cost must be a 3-D tensor of 32-bit integers")
        st = np.ascontiguousarray(np.asarray(starts, np.int64).reshape(-1, 3).astype(np.int32))
        k, max_len = len(st), int(max_len)
        if tuple(d_cells.shape) != (k, max_len, 3) or str(d_cells.dtype) != "torch.int32" or d_paths.numel() * d_paths.element_size() != 16 * k:
            raise ValueError("d_cells must be [k, max_len, 3] int32 and d_paths k x 16 bytes")
        for t_ in (d_cells, d_paths, d_cost):
            if not (t_.is_contiguous() and t_.is_cuda):
                raise ValueError("tensors must be contiguous device tensors")
        box = self._df_box(lo, tuple(d_cost.shape), 0, 1)
        import torch
        torch.cuda.current_stream(d_cost.device).synchronize()  # the cost field is written, the outputs' earlier use is over
        check(_lib.lib().revo_map_plan_paths(self._h, C.byref(box), vp(d_cost.data_ptr()), 1, k, st.ctypes.data_as(vp), max_len,
                                             vp(d_cells.data_ptr()), vp(d_paths.data_ptr()), 1))
        if wait:
            self.sync()

    def last_plan(self):
        """(ms, rounds) of the last plan / plan_into call: its device time (HIP events, the host's looks between the groups of
        rounds included) and the last relaxation round in which a tile did work."""
        ms, rounds = C.c_float(), C.c_uint32()
        check(_lib.lib().revo_map_plan_last(self._h, C.byref(ms), C.byref(rounds)))
        return ms.value, int(rounds.value)

    def last_distance_field_ms(self):
        """Device time of the last distance_field / distance_field_into call (HIP events), in milliseconds; waits for it."""
        ms = C.c_float()
        check(_lib.lib().revo_map_distance_field_last_ms(self._h, C.byref(ms)))
        return ms.value

    def sync(self):
        """Waits for the map's enqueued work (integrations and render_into calls)."""
        self.info()

    def last_raycast_ms(self):
        """Device time of the last raycast / raycast_into / cast_rays call (block table + march, HIP events), in milliseconds."""
        ms = C.c_float()
        check(_lib.lib().revo_map_raycast_last_ms(self._h, C.byref(ms)))
        return ms.value

    def last_render_ms(self):
        """Device time of the last render / render_into call (splat + resolve, HIP events), in milliseconds; waits for it."""
        ms = C.c_float()
        check(_lib.lib().revo_map_render_last_ms(self._h, C.byref(ms)))
        return ms.value


class DistanceField:
    """A voxel map's distance field over a box of voxel indices (VoxelMap.distance_field, `mapfile esdf`): lo the
    box's first voxel index, n its cells per axis, voxel the map's edge in metres, d2 [n0, n1, n2] uint32 the squared distance
    in cells to the nearest voxel inside the box (settings.DF_NONE everywhere when there is none), info the call's counters
    (mapfile.DF_INFO_KEYS; None for a loaded field), clamp the clamp it was built with (0: none, or not known)."""

    def __init__(self, d2, lo, voxel, info=None, map=None, clamp=0):
        self.clamp = int(clamp)
        self.d2 = d2
        self.lo = np.asarray(lo, np.int32).reshape(3)
        self.n = np.asarray(d2.shape, np.int32)
        self.voxel = float(np.float32(voxel))
        self.info = info
        self._map = map
        self.known, self.min_views = False, None  # a known field (VoxelMap.distance_field(seen=...)) says so, and with which votes

    def metres(self):
        """[n0, n1, n2] float32: sqrt(d2) * voxel, +inf where there is no voxel."""
        from . import mapfile
        with np.errstate(all="ignore"):
            return np.where(self.d2 == mapfile.DF_NONE, np.float32(np.inf), np.sqrt(self.d2.astype(np.float32)) * np.float32(self.voxel))

    def sample(self, points):
        """Distance (metres) and gradient at points ([N, 3] metres): on the device of the map the field came from, and through
        mapfile.df_sample -- the same bytes -- for a loaded field or a closed map."""
        from . import mapfile
        if self._map is not None and getattr(self._map, "_h", None):
            return self._map.df_sample(self, points)
        return mapfile.df_sample(self.d2, self.lo, self.voxel, points)

    def _live(self):
        return self._map is not None and bool(getattr(self._map, "_h", None))

    def align_eval(self, points, poses, max_dist, centre=None):
        """The registration sums of `points` ([N, 3] float32 or a torch device tensor, source frame) against this field at
        each pose (4x4 source -> field frame, or [n, 4, 4]) -> MapDfAlignInfo records: on the device of the map the
        field came from, and through mapfile.df_align_records -- the same bytes -- for a loaded field or a closed map."""
        if self._live():
            return self._map.df_align_eval(self.d2, self.lo, points, poses, max_dist, centre)
        from . import mapfile
        T = np.asarray(poses, np.float32)
        if centre is None:
            centre = mapfile.df_align_centre(points, T.reshape(-1, 4, 4)[0])
        rec = mapfile.df_align_records(self.d2, self.lo, self.n, self.voxel, points, T, max_dist, centre)
        out = [MapDfAlignInfo.from_buffer_copy(r.tobytes()) for r in rec]
        return out[0] if T.ndim == 2 else out

    def align(self, points, T_init=None, max_dist=None, centre=None, **opts):
        """Registers `points` against this field from T_init (VoxelMap.df_align; opts: max_iters, eps_t, eps_r, min_matched)
        -> dict: T, info, iterations, status, cov, sigma2, centre.  Without a live map: mapfile.df_align, the same loop."""
        if self._live():
            return self._map.df_align(self.d2, self.lo, points, T_init, max_dist, centre, **opts)
        from . import mapfile
        T0 = np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32).reshape(4, 4)
        if centre is None:
            centre = mapfile.df_align_centre(points, T0)
        max_dist = 8.0 * self.voxel if max_dist is None else max_dist
        T, rec, it, st = mapfile.df_align(self.d2, self.lo, self.n, self.voxel, points, T0, max_dist, centre, **opts)
        info = MapDfAlignInfo.from_buffer_copy(rec.tobytes())
        cov, s2 = df_align_covariance(info)
        return {"T": T, "info": info, "iterations": it, "status": st, "cov": cov, "sigma2": s2, "centre": np.asarray(centre, np.float32)}

    def plan(self, goals, clearance=None, r2=None, max_rounds=0):
        """The cost-to-go from `goals` to every cell that keeps a clearance from every surface -> CostField.
        goals: [k, 3] integer voxel indices, [k, 4] with a cost0 (<= 2^24) per goal, or [k, 3] floating-point metres (the
        cell floor(p / voxel)).  clearance: metres, r2 = max(1, ceil((clearance / voxel)^2)); or r2 itself, the squared
        clearance in cells: a cell is free iff d2 >= r2.  A field built with a clamp below r2 is refused: it would have no
        free cell.  On the device of the map the field came from, and through mapfile.plan_records -- the same bytes -- for
        a loaded field or a closed map."""
        from . import mapfile
        if (clearance is None) == (r2 is None):
            raise ValueError("give the clearance in metres or r2 in cells squared, not both")
        r2 = mapfile.plan_r2(clearance, self.voxel) if r2 is None else int(r2)
        if r2 < 1:
            raise ValueError("r2 must be >= 1")
        if 0 < self.clamp < r2:
            raise ValueError("the field was built with clamp %d < r2 %d: no cell of it can be free; build it without a clamp" % (self.clamp, r2))
        seeds = mapfile.plan_seeds(goals, self.voxel)
        if self._live():
            cost, info = self._map.plan(self, seeds, r2, max_rounds)
        else:
            cost, info = mapfile.plan_records(self.d2, self.lo, self.n, seeds, r2)
        return CostField(cost, self.lo, self.voxel, r2, info, self._map)

    def save(self, path):
        """The .npz `python -m revo_amd.mapfile esdf` writes: d2, lo, n, voxel."""
        from . import mapfile
        return mapfile.write_field(path, self.d2, self.lo, self.voxel)

    @classmethod
    def load(cls, path):
        from . import mapfile
        return cls(*mapfile.read_field(path))


class SeenVolume:
    """What has been looked at, over a box of voxel indices (VoxelMap.observe, `mapfile observe`): seen [n0, n1, n2]
    uint8 -- the low seven bits the views that looked through the cell's centre (free votes, at most 127), bit 7 whether a view
    measured a surface there --, lo the box's first voxel index, n its cells per axis, voxel the map's edge in metres, info the
    last call's counters (mapfile.SEEN_INFO_KEYS) and view_info its per-view class counts (None for a loaded volume)."""

    def __init__(self, seen, lo, voxel, info=None, view_info=None):
        seen = np.asarray(seen)
        if seen.dtype != np.uint8 or seen.ndim != 3:
            raise ValueError("a seen volume is a 3-D uint8 array")
        self.seen = seen
        self.lo = np.asarray(lo, np.int32).reshape(3)
        self.n = np.asarray(seen.shape, np.int32)
        self.voxel = float(np.float32(voxel))
        self.info = info
        self.view_info = view_info

    def free(self, min_views=1):
        """[n0, n1, n2] bool: the cells with at least min_views free votes."""
        from . import mapfile
        return mapfile.seen_free(self.seen, min_views)

    def known(self, solid=None, min_views=1):
        """[n0, n1, n2] bool: the cells that are free or carry the surface bit -- or are solid, where `solid` (a bool volume
        of the box, mapfile.solid_cells) says so."""
        from . import mapfile
        return mapfile.seen_known(self.seen, min_views, solid)

    def save(self, path):
        """The .npz `python -m revo_amd.mapfile observe` writes: seen, lo, n, voxel."""
        from . import mapfile
        return mapfile.write_seen(path, self.seen, self.lo, self.voxel)

    @classmethod
    def load(cls, path):
        from . import mapfile
        return cls(*mapfile.read_seen(path))


class TsdfVolume:
    """Depth views fused into a truncated signed distance volume over a box of voxel indices (VoxelMap.fuse, `mapfile tsdf`;
    DESIGN 26): cells [n0, n1, n2] of (sum int32, weight uint32) -- the integer sum of the views' signed distances in units of
    trunc / 1024 and the views that gave one --, lo the box's first voxel index, n its cells per axis, voxel the map's edge and
    trunc the truncation distance in metres, info the last call's counters (mapfile.TSDF_INFO_KEYS) and view_info its per-view
    class counts (None for a loaded volume)."""

    def __init__(self, cells, lo, voxel, trunc, info=None, view_info=None, map=None, color=None, color_info=None):
        from . import mapfile
        cells = np.asarray(cells)
        if cells.dtype != mapfile.TSDF_CELL_DTYPE or cells.ndim != 3:
            raise ValueError("a TSDF volume is a 3-D array of (sum int32, weight uint32) cells")
        if color is not None:
            color = np.asarray(color)
            if color.dtype != mapfile.TSDF_COLOR_DTYPE or color.shape != cells.shape:
                raise ValueError("a colour volume is an array of (sum_b, sum_g, sum_r, weight uint32) cells of the TSDF volume's shape")
        self.color = color            # mapfile.TSDF_COLOR_DTYPE [n0, n1, n2], or None: fused without colour
        self.color_info = color_info  # the last call's colour counters (mapfile.TSDF_COLOR_INFO_KEYS)
        self.cells = cells
        self.lo = np.asarray(lo, np.int32).reshape(3)
        self.n = np.asarray(cells.shape, np.int32)
        self.voxel = float(np.float32(voxel))
        self.trunc = float(mapfile.tsdf_trunc(voxel, trunc))
        self.info = info
        self.view_info = view_info
        self._map = map

    def sdf(self):
        """[n0, n1, n2] float64 metres: sum / weight * trunc / 1024 (positive in front of the surface), NaN where no view gave
        a distance."""
        from . import mapfile
        return mapfile.tsdf_sdf(self.cells, self.trunc)

    def mesh(self, min_weight=1, normals=False, colors=False, map=None):
        """The mesh of the zero level set -> mapfile.Mesh, on the device of the map the volume was fused with (or `map`); a
        loaded volume without one is meshed by mapfile.mesh_records, which gives the same bytes.  normals, colors: with the
        vertices' attributes (VoxelMap.mesh; mapfile.mesh_attr_records without a map)."""
        from . import mapfile
        m = map if map is not None else self._map
        if colors and self.color is None:
            raise ValueError("the volume has no colour: fuse it with color=True")
        if m is None:
            if not (normals or colors):
                return mapfile.mesh_records(self.cells, self.lo, self.voxel, min_weight)
            out = mapfile.mesh_attr_records(self.cells, self.color if colors else None, self.lo, self.voxel, min_weight)
            if not normals:
                out.normals = None
            return out
        return m.mesh(self, min_weight, normals, colors)

    def raycast(self, poses, camera=None, size=None, step=None, min_weight=1, max_steps=4096, normals=True, colors=True, zrange=None, map=None):
        """The surface seen from camera poses -> dict of depth, normals, bgr, hits and info (VoxelMap.surface_raycast),
        on the device of the map the volume was fused with (or `map`).  colors=True needs a colour volume; a volume without one
        gives bgr None.  A loaded volume without a map is ray-cast by mapfile.tsdf_raycast_records, which gives the same bytes;
        it needs a camera (fx, fy, cx, cy), a size and a zrange."""
        from . import mapfile
        m = map if map is not None else self._map
        colors = bool(colors) and self.color is not None
        if m is not None:
            return m.surface_raycast(self, poses, camera, size, zrange, step, min_weight, max_steps, normals, colors)
        if camera is None or size is None or zrange is None:
            raise ValueError("without a map the camera (fx, fy, cx, cy), the size and the zrange must be given")
        if isinstance(camera, Camera):
            camera = (camera.fx, camera.fy, camera.cx, camera.cy)
        T = np.asarray(poses, np.float32)
        single = T.ndim == 2
        views = [(M, tuple(camera) + tuple(zrange), size) for M in T.reshape(-1, 4, 4)]
        r = mapfile.tsdf_raycast_records(self.cells, self.color if colors else None, self.lo, self.voxel, views, step, min_weight, max_steps)
        pick = (lambda a: a[0]) if single else (lambda a: a)
        return {"depth": pick(r["depth"]), "normals": pick(r["normals"]) if normals else None, "bgr": pick(r["bgr"]) if colors else None,
                "hits": pick(r["hits"]), "info": r["info"]}

    def track_eval(self, frame, poses, max_dist=None, stride=1, min_weight=1, centre=None, map=None):
        """The tracking sums of a depth frame against this surface at camera poses -> MapTsdfTrackInfo records
        (VoxelMap.surface_track_eval), on the device of the map the volume was fused with (or `map`).  frame: a pyramid
        or (depth, camera[, zrange])."""
        m = map if map is not None else self._map
        if m is None:
            raise ValueError("tracking runs on a map's device: pass map= (mapfile.tsdf_track_records is the contract on the CPU)")
        m._tsdf_box(self)
        return m.surface_track_eval(self.cells, self.lo, self.trunc, frame, poses, max_dist, stride, min_weight, centre)

    def track(self, frame, T_init, max_dist=None, stride=1, min_weight=1, centre=None, map=None, **opts):
        """The frame's camera pose refined against this surface from T_init (VoxelMap.surface_track) -> dict of T, info,
        iterations, status, cov, sigma2 and centre, as align gives them.  opts: max_iters, eps_t, eps_r, min_matched."""
        m = map if map is not None else self._map
        if m is None:
            raise ValueError("tracking runs on a map's device: pass map= (mapfile.tsdf_track is the contract on the CPU)")
        m._tsdf_box(self)
        return m.surface_track(self.cells, self.lo, self.trunc, frame, T_init, max_dist, stride, min_weight, centre, **opts)

    def unfuse(self, views, map=None):
        """Views taken out of the volume again -> a new TsdfVolume (VoxelMap.unfuse), on the device of the map the
        volume was fused with (or `map`); a loaded volume without one goes through mapfile.tsdf_unfuse_records, which gives the
        same bytes and raises mapfile.TsdfUnfuseRefused where the map raises RevoError.  A volume with colour takes raw views as
        (depth, T, intrinsics, bgr)."""
        from . import mapfile
        m = map if map is not None else self._map
        if m is not None:
            return m.unfuse(self, views)
        views = list(views)
        bgr = [v[3] for v in views] if self.color is not None else None
        cells, col, info, counts = mapfile.tsdf_unfuse_records(self.cells, self.color, self.lo, self.voxel, [tuple(v[:3]) for v in views], self.trunc, bgr=bgr)
        return TsdfVolume(cells, self.lo, self.voxel, self.trunc, info, counts, color=col)

    def save(self, path):
        """The .npz `python -m revo_amd.mapfile tsdf` writes: sum, weight, lo, n, voxel, trunc, and with a colour volume
        color_sum and color_weight."""
        from . import mapfile
        return mapfile.write_tsdf(path, self.cells, self.lo, self.voxel, self.trunc, self.color)

    @classmethod
    def load(cls, path):
        from . import mapfile
        cells, lo, voxel, trunc, color = mapfile.read_tsdf(path, color=True)
        return cls(cells, lo, voxel, trunc, color=color)


class SurfaceVolume:
    """The surface of a running sequence: the two device volumes of a box that is decided before the run, cleared on
    creation.  integrate(view) is one accumulating fuse call, enqueued only; volume() downloads a TsdfVolume;
    mesh() meshes on the device.  vo.REVO(surface=) feeds it every keyframe.  lo, n: the box in voxel indices of the map's world
    frame; trunc: metres (default 4 voxel edges); color=False keeps the TSDF volume alone.  The box moves only when shift() is
    called; FollowingSurface calls it as the camera goes."""

    def __init__(self, map, lo, n, trunc=None, color=True):
        import torch
        from . import mapfile
        self.map = map
        box = map._df_box(lo, n, 0, 1)
        self.lo = np.array(list(box.lo), np.int32)
        self.n = np.array(list(box.n), np.int32)
        self.trunc = float(mapfile.tsdf_trunc(map.voxel, trunc))
        dev = torch.device("cuda", map.cameraPyr.device)
        shape = tuple(int(x) for x in self.n)
        self.d_tsdf = torch.zeros(shape + (2,), dtype=torch.int32, device=dev)
        self.d_color = torch.zeros(shape + (4,), dtype=torch.int32, device=dev) if color else None
        self.views = 0
        self._vinfo = []  # one [8] int32 device tensor per integrated view: revo_map_carve_view_info
        self._pending = []  # the device images of raw views whose fuse is enqueued and not yet waited for

    def integrate(self, view):
        """One view -- (pyramid, T_w_c), or a raw view as VoxelMap.fuse takes it with device images -- fused into the volumes:
        one accumulating call on the map's stream, which returns at once.  The call is only enqueued and torch's allocator does not
        know the map's stream, so a raw view's device images are kept referenced here until that stream has been waited for
        (volume(), view_counts(), or after 64 such views a wait of its own): the caller may drop them at once."""
        import torch
        vi = torch.zeros(8, dtype=torch.int32, device=self.d_tsdf.device)
        self.map.fuse_into(self.d_tsdf, [view], self.lo, self.trunc, accumulate=True, d_view_info=vi, wait=False, d_color=self.d_color)
        self._vinfo.append(vi)
        self.views += 1
        images = [x for x in view if hasattr(x, "data_ptr")]
        if images:
            if len(self._pending) >= 64:
                self.map.sync()
                self._pending.clear()
            self._pending.append(images)

    def view_counts(self):
        """Per integrated view the cells of the box by class (mapfile.CARVE_CLASSES); waits for the map's stream."""
        import torch
        from . import mapfile
        self.map.sync()
        self._pending.clear()
        if not self._vinfo:
            return []
        rows = torch.stack(self._vinfo).cpu().numpy().view(np.uint32)
        return [{name: int(r[i]) for i, name in enumerate(mapfile.CARVE_CLASSES)} for r in rows]

    def volume(self):
        """The volumes as they stand -> TsdfVolume (with .color unless created with color=False); waits for the map's stream."""
        from . import mapfile
        self.map.sync()
        self._pending.clear()
        cells = np.ascontiguousarray(self.d_tsdf.cpu().numpy()).view(mapfile.TSDF_CELL_DTYPE)[..., 0]
        col = None if self.d_color is None else np.ascontiguousarray(self.d_color.cpu().numpy()).view(mapfile.TSDF_COLOR_DTYPE)[..., 0]
        return TsdfVolume(cells, self.lo, self.map.voxel, self.trunc, map=self.map, color=col)

    def mesh(self, min_weight=1, normals=True, colors=True):
        """The mesh of the volumes as they stand, on the device -> mapfile.Mesh.  colors needs color=True at creation."""
        import torch
        from . import mapfile
        if colors and self.d_color is None:
            raise ValueError("the surface was created without colour")
        nv, nt, _ = self.map.mesh_into(None, None, self.d_tsdf, self.lo, min_weight)
        dev = self.d_tsdf.device
        d_v = torch.zeros((max(nv, 1), 3), dtype=torch.float32, device=dev)
        d_t = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device=dev)
        d_n = torch.zeros((max(nv, 1), 3), dtype=torch.float32, device=dev) if normals else None
        d_c = torch.zeros((max(nv, 1), 4), dtype=torch.uint8, device=dev) if colors else None
        nv, nt, info = self.map.mesh_into(d_v, d_t, self.d_tsdf, self.lo, min_weight, d_normals=d_n, d_colors=d_c,
                                          d_color=self.d_color if colors else None)
        self.map.sync()
        return mapfile.Mesh(d_v[:nv].cpu().numpy(), d_t[:nt].cpu().numpy().view(np.uint32), info,
                            d_n[:nv].cpu().numpy() if normals else None, d_c[:nv].cpu().numpy() if colors else None)

    def raycast(self, poses, camera=None, size=None, step=None, min_weight=1, max_steps=4096, normals=True, colors=True, zrange=None, device=False):
        """The surface as it stands seen from camera poses (VoxelMap.surface_raycast_into on the device volumes): no
        host copy of the volumes, the call is only enqueued behind the integrations.  -> dict of depth, normals, bgr, hits and
        info as TsdfVolume.raycast gives them; device=True: the torch device tensors themselves (depth [n, h, w] or [h, w],
        normals, bgr, hits int32 [n], info int64 [8] in mapfile.TSDF_RAY_INFO_KEYS' order), valid behind the map's sync()."""
        import torch
        from . import mapfile
        colors = bool(colors) and self.d_color is not None
        views, n, single = self.map._surface_views(poses, camera, size, zrange)
        h, w = views[0].height, views[0].width
        dev = self.d_tsdf.device
        shape = (h, w) if single else (n, h, w)
        if not single and (h * w) % 16:  # every view's part of a stacked tensor is 16-byte aligned
            raise ValueError("several device views at once need a pixel count that is a multiple of 16")
        d_depth = torch.empty(shape, dtype=torch.float32, device=dev)
        d_nrm = torch.empty(shape + (3,), dtype=torch.float32, device=dev) if normals else None
        d_bgr = torch.empty(shape + (3,), dtype=torch.uint8, device=dev) if colors else None
        d_hits = torch.zeros(max(n, 4), dtype=torch.int32, device=dev)[:n]
        d_info = torch.zeros(8, dtype=torch.int64, device=dev)
        self.map.surface_raycast_into(d_depth, self.d_tsdf, self.lo, poses, camera, size, zrange, step, min_weight, max_steps, d_normals=d_nrm,
                                      d_bgr=d_bgr, d_color=self.d_color if colors else None, d_hits=d_hits, d_info=d_info, wait=False)
        if device:
            return {"depth": d_depth, "normals": d_nrm, "bgr": d_bgr, "hits": d_hits, "info": d_info}
        self.map.sync()
        host = lambda t_: None if t_ is None else t_.cpu().numpy()  # noqa: E731
        split = (lambda a: a) if single else (lambda a: None if a is None else list(a))
        hits, info = d_hits.cpu().numpy(), d_info.cpu().numpy()
        return {"depth": split(host(d_depth)), "normals": split(host(d_nrm)), "bgr": split(host(d_bgr)),
                "hits": int(hits[0]) if single else [int(x) for x in hits],
                "info": {k: int(info[i]) for i, k in enumerate(mapfile.TSDF_RAY_INFO_KEYS)}}

    def track_eval(self, frame, poses, max_dist=None, stride=1, min_weight=1, centre=None, d_out=None):
        """The tracking sums of a depth frame against the surface as it stands (VoxelMap.surface_track_eval on the device volume,
        DESIGN 29): no host copy of the volume; with a pyramid or device frame and d_out the call is only enqueued behind the
        integrations."""
        return self.map.surface_track_eval(self.d_tsdf, self.lo, self.trunc, frame, poses, max_dist, stride, min_weight, centre, d_out)

    def track(self, frame, T_init, max_dist=None, stride=1, min_weight=1, centre=None, **opts):
        """The frame's camera pose refined against the surface as it stands, from T_init (VoxelMap.surface_track on the device
        volume) -> dict of T, info, iterations, status, cov, sigma2 and centre."""
        return self.map.surface_track(self.d_tsdf, self.lo, self.trunc, frame, T_init, max_dist, stride, min_weight, centre, **opts)

    def shift(self, delta, spill=True):
        """The box moved by delta cells (VoxelMap.shift_into): the volumes are moved out of place into a second pair of
        device volumes, allocated at the first shift, and the pairs are swapped; lo += delta.  spill=True -> the cells that left and
        were not EMPTY, as mapfile.TSDF_RECORD_DTYPE in ascending key order (the call waits for them); spill=False drops them, is
        only enqueued and returns None.  shift_info: the last shift's counters (None after a dropping one).
        The records go through a device buffer that is kept and only grows: a shift emits straight into it (one counting pass); only
        when it holds fewer records than leave (REVO_ERR_CAPACITY, nothing moved) is the shift counted, the buffer grown to that
        count and the shift made again."""
        import torch
        from . import mapfile
        d = np.asarray(delta, np.int64).reshape(3)
        mapfile.check_box(self.lo.astype(np.int64) + d, self.n)
        if getattr(self, "_alt", None) is None:
            self._alt = (torch.empty_like(self.d_tsdf), None if self.d_color is None else torch.empty_like(self.d_color))
        a_t, a_c = self._alt
        rec, info = None, None
        if spill:
            args = (a_t, self.d_tsdf, self.lo, d, a_c, self.d_color)
            done = False
            if getattr(self, "_spill", None) is not None:
                try:
                    n, info = self.map.shift_into(*args, d_records=self._spill)
                    done = True
                except RevoError as e:
                    if e.code != -5:  # REVO_ERR_CAPACITY: nothing was moved
                        raise
            if not done:
                n, info = self.map.shift_into(*args, count_only=True)
                self._spill = torch.empty(32 * max(n, 1), dtype=torch.uint8, device=self.d_tsdf.device)
                n, info = self.map.shift_into(*args, d_records=self._spill)
            self.map.sync()
            rec = self._spill[:32 * n].cpu().numpy().view(mapfile.TSDF_RECORD_DTYPE).copy()
        else:
            self.map.shift_into(a_t, self.d_tsdf, self.lo, d, a_c, self.d_color)
        self._alt = (self.d_tsdf, self.d_color)
        self.d_tsdf, self.d_color = a_t, a_c
        self.lo = (self.lo.astype(np.int64) + d).astype(np.int32)
        self.shift_info = info
        return rec

    def refill(self, records):
        """Records (mapfile.TSDF_RECORD_DTYPE, strictly ascending keys) added back into the cells of the box as it stands
        (VoxelMap.refill_into): all or nothing -> the dict of mapfile.TSDF_REFILL_INFO_KEYS.  Waits for the map's stream: the
        update reads a device copy of the records that this call owns and lets go of."""
        import torch
        from . import mapfile
        rec = np.ascontiguousarray(mapfile.tsdf_record_array(records))
        if len(rec) == 0:
            return {"records": 0, "applied": 0, "outside": 0}
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(self.d_tsdf.device)
        try:
            return self.map.refill_into(self.d_tsdf, self.lo, d_rec, len(rec), self.d_color)
        finally:
            self.map.sync()  # d_rec goes back to torch's allocator only behind the update that reads it

    def remove(self, view, index=None):
        """One view that was integrated taken out of the volumes again (VoxelMap.unfuse_into): one unfuse call, which
        waits for its check pass.  view: as integrate takes it, at the pose it was integrated with.  All or nothing: RevoError
        carrying .misfits, with the volumes unchanged, when the view is not in them (or a weight is full).  `views` and the
        per-view counts are kept current: index says which integrated view it was (its place in view_counts()); by default the
        first one whose class counts are this view's (rows with equal counts are interchangeable).  A view that fits the volumes
        and was not integrated through this object has no such row: RuntimeError behind the unfuse, with `views` and the counts
        unchanged.  -> the info dict of mapfile.TSDF_UNFUSE_INFO_KEYS."""
        import torch
        vi = torch.zeros(8, dtype=torch.int32, device=self.d_tsdf.device)
        info = self.map.unfuse_into(self.d_tsdf, [view], self.lo, self.trunc, d_color=self.d_color, d_view_info=vi)
        if index is None:
            same = (torch.stack(self._vinfo) == vi).all(dim=1).nonzero() if self._vinfo else []
            index = int(same[0]) if len(same) else None
        if index is None or not 0 <= index < len(self._vinfo):
            raise RuntimeError("the view has been taken out of the volumes, but no integrated view of this surface has its class counts "
                               "(or its index): views and view_counts() are left as they were")
        del self._vinfo[index]
        self.views -= 1
        return info

    def repose(self, view, T_old, T_new, index=None):
        """A view that was integrated at the pose T_old moved to T_new: one unfuse at T_old, then one fuse at T_new.
        view: as integrate takes it; its own pose entry is not looked at.  -> the unfuse's info dict; when the unfuse is refused
        nothing is fused, the volumes are unchanged and the dict is the refusal's (misfits > 0)."""
        view = tuple(view)
        at = lambda T: (view[0], np.asarray(T, np.float32).reshape(4, 4)) + view[2:]  # noqa: E731
        try:
            info = self.remove(at(T_old), index)
        except RevoError as e:
            if getattr(e, "misfits", None):
                return e.info
            raise
        self.integrate(at(T_new))
        return info


class SurfaceWindow(SurfaceVolume):
    """A surface that holds exactly the last `window` integrated views: the bounded surface of a long run, beside MapWindow's
    bounded map.  Its volumes are byte for byte those of a fresh SurfaceVolume fused from those views alone.
    integrate(view) fuses the view and then takes the oldest one out again (SurfaceVolume.remove: one unfuse call, which waits for
    its check pass).  vo.REVO(voxelMap=MapWindow(...), surface=SurfaceWindow(...)) feeds it every keyframe.

    What it keeps to name a view again: a pyramid it may keep (one the caller owns) is kept as it is, as MapWindow keeps its
    keyframes; the driver's keyframe pyramid is only borrowed until the next frame, so of it -- and of a raw device view -- device
    copies of the depth and the colour image are kept: window x (4 + 3) bytes per pixel.  A borrowed pyramid's colour plane cannot
    be read back, so integrate takes the frame's colour image beside it (bgr=, the image the pyramid was built from; the driver
    passes it)."""

    def __init__(self, map, lo, n, window=1, trunc=None, color=True):
        import collections
        if int(window) < 1:
            raise ValueError("window must be >= 1 view")
        self._held = collections.deque()  # the views as they can be named again, oldest first
        super().__init__(map, lo, n, trunc, color)
        self.window = int(window)

    def _keepable(self, view, bgr):
        """The view in a form that stays valid while the window holds it."""
        import torch
        src = view[0]
        dev = self.d_tsdf.device
        if isinstance(src, ImgPyramidRGBD):
            if src._owned:
                return (src, np.array(view[1], np.float32).reshape(4, 4)) + tuple(view[2:])
            if self.d_color is not None and bgr is None:
                raise ValueError("a borrowed pyramid's colour plane cannot be read back: pass the frame's colour image as bgr=")
            depth = torch.from_numpy(src.returnDepth(0)).to(dev)
            T = np.array(view[1], np.float32).reshape(4, 4)
            if self.d_color is None:
                return (depth, T, None)
            im = np.ascontiguousarray(bgr, np.uint8)
            if im.shape != tuple(depth.shape) + (3,):
                raise ValueError("bgr is the [h, w, 3] uint8 image the pyramid was built from")
            return (depth, T, None, torch.from_numpy(im).to(dev))
        if not hasattr(src, "data_ptr"):
            raise ValueError("a raw view of a surface has device images")
        held = (src.clone(), np.array(view[1], np.float32).reshape(4, 4), view[2] if len(view) > 2 else None)
        return held + (view[3].clone(),) if self.d_color is not None and len(view) > 3 and view[3] is not None else held

    def held_views(self):
        """The views the window holds (`views` is their number, as SurfaceVolume's), oldest first, as they can be named again:
        (pyramid or device depth, T_w_c, intrinsics or None[, device bgr])."""
        return list(self._held)

    def _place(self, view):
        i = int(view) if isinstance(view, (int, np.integer)) else next((j for j, h in enumerate(self._held) if h is view), None)
        if i is None or not 0 <= i < len(self._held):
            raise ValueError("the window names a view it holds by the entry of held_views() or by its place in it")
        return i

    def integrate(self, view, bgr=None):
        """The view fused, and once more than `window` views are held the oldest one taken out again.  bgr: the colour image of a
        borrowed pyramid (see the class).  When that unfuse is refused (a cell of the oldest view has reached the full weight
        2^20, so its history cannot be inverted) the RevoError goes to the caller with the new view fused and held: the window then
        holds window + 1 views, every one of them in the volumes and in held_views(), and the next integrate tries the eviction again."""
        held = self._keepable(view, bgr)
        super().integrate(held)
        self._held.append(held)
        while len(self._held) > self.window:
            self.remove(0)

    def remove(self, view, index=None):
        """A view the window holds (an entry of held_views(), or its place in it) taken out of the volumes and of the window."""
        i = self._place(view)
        info = super().remove(self._held[i], i)
        del self._held[i]
        return info

    def repose(self, view, T_old, T_new, index=None):
        """SurfaceVolume.repose of a view the window holds (an entry of held_views(), or its place in it): it keeps its place in the
        window, at the new pose."""
        i = self._place(view)
        old = self._held[i]
        new = (old[0], np.asarray(T_new, np.float32).reshape(4, 4)) + tuple(old[2:])
        try:
            info = SurfaceVolume.remove(self, (old[0], np.asarray(T_old, np.float32).reshape(4, 4)) + tuple(old[2:]), i)
        except RevoError as e:
            if getattr(e, "misfits", None):
                return e.info
            raise
        SurfaceVolume.integrate(self, new)
        self._vinfo.insert(i, self._vinfo.pop())  # the per-view counts keep the window's order
        self._held[i] = new
        return info

    def clear(self):
        """An empty window over zero volumes."""
        self.map.sync()
        self.d_tsdf.zero_()
        if self.d_color is not None:
            self.d_color.zero_()
        import torch
        torch.cuda.current_stream(self.d_tsdf.device).synchronize()
        self._held.clear()
        self._vinfo.clear()
        self._pending.clear()
        self.views = 0


class FollowingSurface(SurfaceVolume):
    """A SurfaceVolume whose box follows the camera: n cells per axis, placed by mapfile.follow_lo -- centred `ahead`
    metres (default n[2] * voxel / 2) along the camera's z axis and snapped to multiples of `step` cells.  follow(T_w_c) moves the
    box when the policy's answer differs from lo: the cells that leave go to `store` (a mapfile.SurfaceStore, by default a fresh
    one), the store's records inside the new box come back into it.  integrate(view) follows the view's pose and then fuses, so
    vo.REVO(surface=FollowingSurface(...)) works as with a SurfaceVolume.  shifts: how often the box has moved.  Until the first
    follow the box sits where the identity pose puts it; the first follow places it without a move, since nothing is fused yet.
    assemble() is the whole surface, mesh() its mesh.  MultiREVO, an in-place shift and a pyramid of volumes are not part of it."""

    def __init__(self, map, n, trunc=None, color=True, step=16, ahead=None, store=None):
        from . import mapfile
        n = np.asarray(n, np.int64).reshape(3)
        self.step = int(step)
        self.ahead = float(n[2]) * float(map.voxel) / 2.0 if ahead is None else float(ahead)
        super().__init__(map, mapfile.follow_lo(np.eye(4, dtype=np.float32), n, map.voxel, self.ahead, self.step), n, trunc, color)
        self.store = store if store is not None else mapfile.SurfaceStore(voxel=map.voxel, trunc=self.trunc)
        self.store.check(map.voxel, self.trunc)  # a given store must be of this voxel edge and truncation
        if self.store.voxel is None:
            self.store.voxel = float(np.float32(map.voxel))
        if self.store.trunc is None:
            self.store.trunc = self.trunc
        self.shifts = 0
        self._placed = False

    def _take_back(self):
        """The store's records inside the box, into the box.  All or nothing: a refill that is refused (a store of the caller's whose
        records do not FIT on top of the box, or hold colour the surface has no volume for) leaves them in the store."""
        back = self.store.take(self.lo, self.n)
        if len(back) == 0:
            return
        try:
            if self.d_color is None and any(np.any(back[k] != 0) for k in ("sum_b", "sum_g", "sum_r", "color_weight")):
                raise ValueError("the store holds colour and the surface was created without colour")
            super().refill(back)
        except Exception:
            self.store.add(back)
            raise

    def follow(self, T_w_c):
        """The box goes where mapfile.follow_lo puts it for the pose -> True when it moved."""
        from . import mapfile
        lo = mapfile.follow_lo(T_w_c, self.n, self.map.voxel, self.ahead, self.step)
        if not self._placed:
            self._placed = True
            self.lo = lo.astype(np.int32)
            self._take_back()
            return False
        d = lo - self.lo.astype(np.int64)
        if not d.any():
            return False
        self.store.add(self.shift(d, spill=True))
        self._take_back()
        self.shifts += 1
        return True

    def refill(self, records):
        self._placed = True
        return super().refill(records)

    def integrate(self, view):
        """follow(the view's pose), then SurfaceVolume.integrate."""
        self.follow(view[1])
        super().integrate(view)

    def remove(self, view, index=None):
        """Not supported: cells the view updated may have left the box for the store, where no view can be taken out of them."""
        raise NotImplementedError("a FollowingSurface cannot unfuse: cells of the view may lie in its store")

    def repose(self, view, T_old, T_new, index=None):
        raise NotImplementedError("a FollowingSurface cannot unfuse: cells of the view may lie in its store")

    def assemble(self, lo=None, n=None):
        """The store plus the box as it stands -> TsdfVolume over the box (lo, n), by default the bounds of both; ValueError with a
        message when that is more than one volume holds (an axis above 1024 cells or more than 2^27 cells).  Nothing is changed."""
        from . import mapfile
        cur = self.volume()
        b = self.store.bounds()
        b_lo = self.lo.astype(np.int64) if b is None else np.minimum(b[0], self.lo)
        b_hi = self.lo.astype(np.int64) + self.n if b is None else np.maximum(b[0] + b[1], self.lo.astype(np.int64) + self.n)
        lo, n = mapfile.surface_assemble_box((b_lo, b_hi - b_lo), lo, n)
        cells, color = self.store.volume(lo, n)
        a = np.maximum(lo, self.lo)                      # the part of the current box inside (lo, n)
        e = np.minimum(lo + n, self.lo.astype(np.int64) + self.n)
        if np.all(e > a):
            dst = tuple(slice(int(a[k] - lo[k]), int(e[k] - lo[k])) for k in range(3))
            src = tuple(slice(int(a[k] - self.lo[k]), int(e[k] - self.lo[k])) for k in range(3))
            for k in ("sum", "weight"):
                cells[k][dst] += cur.cells[k][src]
            if cur.color is not None:
                for k in ("sum_b", "sum_g", "sum_r", "weight"):
                    color[k][dst] += cur.color[k][src]
        return TsdfVolume(cells, lo.astype(np.int32), self.map.voxel, self.trunc, map=self.map, color=color if self.d_color is not None else None)

    def mesh(self, min_weight=1, normals=True, colors=True):
        """The mesh of assemble() -> mapfile.Mesh; ValueError as assemble() when the surface does not fit one volume."""
        if colors and self.d_color is None:
            raise ValueError("the surface was created without colour")
        return self.assemble().mesh(min_weight, normals, colors)


def fuse_surfaces(pairs, wait=False):
    """[(SurfaceVolume, view), ...] -- one view into each surface of as many running sequences, all in one launch
    (VoxelMap.fuse_many_into): each volume afterwards holds what its own integrate(view) leaves, and its `views` and
    per-view counts go on as there.  The surfaces' maps share one context; the volumes are distinct.
    A SurfaceWindow entry ((window, view) or (window, view, bgr), as its integrate takes them) is honoured as its integrate honours
    it: the view is made keepable and held, and behind the one fuse every window that now holds more than `window`
    views has its oldest one taken out, all in one batched unfuse with host results (unfuse_surfaces).  A refused eviction keeps
    integrate's rule: that window holds window + 1 views, and a RevoError (.refused: [(window, info), ...]) is raised after every
    job of the call has been handled."""
    import torch
    pairs = [tuple(p) for p in pairs]
    if not pairs:
        return
    jobs, windows = [], []
    for surf, view, *rest in pairs:
        if isinstance(surf, SurfaceWindow):  # the view as the window can name it again, held from here on
            view = surf._keepable(view, rest[0] if rest else None)
            windows.append((surf, view))
        vi = torch.zeros(8, dtype=torch.int32, device=surf.d_tsdf.device)
        jobs.append(dict(map=surf.map, d_tsdf=surf.d_tsdf, d_color=surf.d_color, lo=surf.lo, trunc=surf.trunc, view=view, d_view_info=vi))
    pairs[0][0].map.fuse_many_into(jobs, wait=wait)
    for (surf, *_), job in zip(pairs, jobs):
        surf._vinfo.append(job["d_view_info"])
        surf.views += 1
    for surf, held in windows:
        surf._held.append(held)
    # the evictions: one batched unfuse with host results per round over every window that holds more than `window` views
    over, refused = [w for w, _ in windows], []
    while True:
        over = [w for w in over if len(w._held) > w.window]
        if not over:
            break
        res = unfuse_surfaces([(w, 0) for w in over])
        for w, (info, status) in zip(list(over), res):
            if status:
                refused.append((w, info))
                over.remove(w)
    if refused:
        e = RevoError(-1, "%d evictions were refused (a cell of the oldest view has reached the full weight): those windows hold window + 1 views"
                      % len(refused))
        e.refused, e.info, e.misfits = refused, refused[0][1], refused[0][1]["misfits"]
        raise e


def raycast_surfaces(entries, step=None, min_weight=1, max_steps=4096, normals=True, colors=True, device=False):
    """[(surface, poses[, camera, size, zrange]), ...] -- views of the surfaces of as many running sequences, all in batched calls
    (VoxelMap.surface_raycast_many_into) -> per entry what SurfaceVolume.raycast(poses, camera, size, ...) returns for
    that surface alone, byte for byte (device=True: the torch device tensors, valid behind the map's sync()).  A surface is a
    SurfaceVolume or a SurfaceWindow; the surfaces' maps share one context.  An entry with more than 64 poses is split into jobs
    that share its volume, and its info is the sum over them; a list of more than 4096 views, or 1024 jobs, goes in several calls.
    The calls are only enqueued behind the surfaces' integrations: no wait is needed between a fuse and the views."""
    import torch
    from . import mapfile
    entries = [tuple(e) for e in entries]
    if not entries:
        return []
    plans, jobs = [], []
    for surf, poses, *rest in entries:
        if isinstance(surf, FollowingSurface):
            raise NotImplementedError("a FollowingSurface is not ray-cast in a batch: its box moves and part of its surface lies in its store")
        camera, size, zrange = (list(rest) + [None, None, None])[:3]
        T = np.asarray(poses, np.float32)
        single = T.ndim == 2
        T = np.ascontiguousarray(T.reshape(-1, 4, 4))
        if len(T) < 1:
            raise ValueError("an entry needs at least one pose")
        col = bool(colors) and surf.d_color is not None
        cam = surf.map._gain_camera(camera, size, zrange, 1)
        h, w = int(cam.height), int(cam.width)
        n, dev = len(T), surf.d_tsdf.device
        if n > 1 and (h * w) % 16:  # every view's part of a stacked tensor is 16-byte aligned
            raise ValueError("several device views at once need a pixel count that is a multiple of 16")
        d_depth = torch.empty((n, h, w), dtype=torch.float32, device=dev)
        d_nrm = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev) if normals else None
        d_bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev) if col else None
        parts = [(a, min(a + 64, n)) for a in range(0, n, 64)]
        d_hits = torch.zeros(64 * len(parts), dtype=torch.int32, device=dev)  # a job's hit words start 16-byte aligned
        d_info = torch.zeros((len(parts), 8), dtype=torch.int64, device=dev)
        for k, (a, b) in enumerate(parts):
            jobs.append(dict(map=surf.map, d_tsdf=surf.d_tsdf, d_color=surf.d_color if col else None, lo=surf.lo, poses=T[a:b], camera=camera, size=size,
                             zrange=zrange, step=step, min_weight=min_weight, max_steps=max_steps, d_depth=d_depth[a:b],
                             d_normals=None if d_nrm is None else d_nrm[a:b], d_bgr=None if d_bgr is None else d_bgr[a:b],
                             d_hits=d_hits[64 * k:64 * k + (b - a)], d_info=d_info[k]))
        plans.append((single, parts, d_depth, d_nrm, d_bgr, d_hits, d_info))
    call, views = [], 0
    m = entries[0][0].map
    for job in jobs + [None]:  # calls of at most 1024 jobs and 4096 views
        if call and (job is None or len(call) == 1024 or views + len(job["poses"]) > 4096):
            m.surface_raycast_many_into(call, wait=False)
            call, views = [], 0
        if job is not None:
            call.append(job)
            views += len(job["poses"])
    if not device or any(len(p[1]) > 1 for p in plans):
        m.sync()  # the views are done before their counters are joined or anything is read
    out = []
    for single, parts, d_depth, d_nrm, d_bgr, d_hits, d_info in plans:
        d_hits = d_hits[:parts[0][1]] if len(parts) == 1 else torch.cat([d_hits[64 * k:64 * k + (b - a)] for k, (a, b) in enumerate(parts)])
        d_info = d_info[0] if len(parts) == 1 else d_info.sum(dim=0)
        pick = (lambda t_: None if t_ is None else t_[0]) if single else (lambda t_: t_)
        if device:
            out.append({"depth": pick(d_depth), "normals": pick(d_nrm), "bgr": pick(d_bgr), "hits": d_hits, "info": d_info})
            continue
        host = lambda t_: None if t_ is None else (t_.cpu().numpy()[0] if single else list(t_.cpu().numpy()))  # noqa: E731
        hits, info = d_hits.cpu().numpy(), d_info.cpu().numpy()
        out.append({"depth": host(d_depth), "normals": host(d_nrm), "bgr": host(d_bgr), "hits": int(hits[0]) if single else [int(x) for x in hits],
                    "info": {k: int(info[i]) for i, k in enumerate(mapfile.TSDF_RAY_INFO_KEYS)}})
    return out


def _unfuse_jobs(entries):
    """-> (the jobs of one unfuse_many_into, the place of each view in its window or None) for [(surface, view), ...]."""
    import torch
    jobs, places = [], []
    for surf, view in entries:
        if isinstance(surf, FollowingSurface):
            raise NotImplementedError("a FollowingSurface cannot unfuse: cells of the view may lie in its store")
        place = surf._place(view) if isinstance(surf, SurfaceWindow) else None
        if place is not None:
            view = surf._held[place]
        vi = torch.zeros(8, dtype=torch.int32, device=surf.d_tsdf.device)
        jobs.append(dict(map=surf.map, d_tsdf=surf.d_tsdf, d_color=surf.d_color, lo=surf.lo, trunc=surf.trunc, view=view, d_view_info=vi))
        places.append(place)
    return jobs, places


def _unfuse_rows(surf, place, vi):
    """The applied unfuse of one view in the surface's books, as SurfaceVolume.remove keeps them -> False when no integrated view
    of the surface has the view's class counts."""
    import torch
    index = place
    if index is None:
        same = (torch.stack(surf._vinfo) == vi).all(dim=1).nonzero() if surf._vinfo else []
        index = int(same[0]) if len(same) else None
    if index is None or not 0 <= index < len(surf._vinfo):
        return False
    del surf._vinfo[index]
    surf.views -= 1
    if place is not None:
        del surf._held[place]
    return True


def unfuse_surfaces(pairs):
    """[(SurfaceVolume, view), ...] -- one view out of each surface again, all in one batched call (VoxelMap.unfuse_many_into,
    DESIGN 33): per surface what its own remove(view) does, except that a refusal is that job's result and raises nothing.  A
    SurfaceWindow names its view as its remove does (an entry of held_views() or its place).  `views` and the per-view counts are
    kept current for the applied jobs only.  -> [(info dict of mapfile.TSDF_UNFUSE_INFO_KEYS, status), ...], status 0 or -1 (refused:
    the surface is unchanged).  RuntimeError as SurfaceVolume.remove's, behind the call, for an applied view no row of its
    surface matches."""
    pairs = [tuple(p) for p in pairs]
    if not pairs:
        return []
    jobs, places = _unfuse_jobs(pairs)
    res = pairs[0][0].map.unfuse_many_into(jobs, wait=True)
    lost = 0
    for (surf, _), place, job, (_info, status) in zip(pairs, places, jobs, res):
        if status == 0 and not _unfuse_rows(surf, place, job["d_view_info"]):
            lost += 1
    if lost:
        raise RuntimeError("%d views have been taken out of their volumes, but no integrated view of their surfaces has their class counts: "
                           "views and view_counts() are left as they were" % lost)
    return res


def repose_surfaces(quads):
    """[(SurfaceVolume, view, T_old, T_new), ...] -- the keyframes of many streams corrected after a loop closure: one batched
    unfuse at the old poses, then one batched fuse at the new ones over the jobs that fitted.  Per surface what its own
    repose does: a refused job is not fused and its surface is unchanged; a window's view keeps its place.
    -> [(the unfuse's info dict, status), ...]."""
    quads = [tuple(q) for q in quads]
    if not quads:
        return []
    pose = lambda T: np.asarray(T, np.float32).reshape(4, 4)  # noqa: E731
    olds = []
    for surf, view, T_old, _ in quads:
        if isinstance(surf, SurfaceWindow):
            olds.append((surf, surf._place(view)))
        else:
            view = tuple(view)
            olds.append((surf, (view[0], pose(T_old)) + view[2:]))
    jobs, places = _unfuse_jobs(olds)
    for job, place, (surf, _, T_old, _) in zip(jobs, places, quads):
        if place is not None:
            job["view"] = (job["view"][0], pose(T_old)) + tuple(job["view"][2:])
    res = quads[0][0].map.unfuse_many_into(jobs, wait=True)
    again, lost = [], 0
    for (surf, _, _, T_new), place, job, (_info, status) in zip(quads, places, jobs, res):
        if status:
            continue
        new = (job["view"][0], pose(T_new)) + tuple(job["view"][2:])
        held = list(surf._held) if place is not None else None
        if not _unfuse_rows(surf, place, job["d_view_info"]):
            lost += 1
            continue
        again.append((surf, place, new, held))
    if again:
        import torch
        fj = []
        for surf, place, new, _ in again:
            vi = torch.zeros(8, dtype=torch.int32, device=surf.d_tsdf.device)
            fj.append(dict(map=surf.map, d_tsdf=surf.d_tsdf, d_color=surf.d_color, lo=surf.lo, trunc=surf.trunc, view=new, d_view_info=vi))
        again[0][0].map.fuse_many_into(fj, wait=True)
        for (surf, place, new, held), job in zip(again, fj):
            surf.views += 1
            if place is None:
                surf._vinfo.append(job["d_view_info"])
            else:  # the per-view counts and the held views keep the window's order
                surf._vinfo.insert(place, job["d_view_info"])
                held[place] = new
                surf._held.clear()
                surf._held.extend(held)
    if lost:
        raise RuntimeError("%d views have been taken out of their volumes, but no integrated view of their surfaces has their class counts" % lost)
    return res


def track_surfaces(triples, max_dist=None, stride=1, min_weight=1, centre=None, **opts):
    """[(SurfaceVolume, frame, T_init), ...] -- each frame's camera pose refined against its own surface as it stands, all loops in
    lockstep (VoxelMap.surface_track_many) -> (a list of dicts as SurfaceVolume.track gives them, rounds)."""
    triples = list(triples)
    if not triples:
        return [], 0
    jobs = [dict(map=s.map, tsdf=s.d_tsdf, lo=s.lo, trunc=s.trunc, frame=f, T_init=T, max_dist=max_dist, stride=stride, min_weight=min_weight, centre=centre)
            for s, f, T in triples]
    return triples[0][0].map.surface_track_many(jobs, **opts)


def explore(m, seen, start, clearance, min_views=1, min_count=1, max_len=4096):
    """The whole route from mapping to exploration on the map's device: the known field of `seen` (a SeenVolume), its
    frontiers, the cost-to-go with the frontiers as goals at the clearance (metres), and the path from `start` (a voxel index,
    or metres) down to the nearest frontier -> dict: field (DistanceField), frontiers [k, 3], cost (CostField), path
    (cells, status, cost).  ValueError when the volume has no frontier cell, or when the clearance is above one voxel edge: a
    frontier cell touches unseen space, which the known field counts as an obstacle, so none keeps a larger clearance."""
    field = m.distance_field(seen=seen, min_views=min_views, min_count=min_count)
    fr = m.frontiers(seen, min_views, min_count)
    if len(fr) == 0:
        raise ValueError("the seen volume has no frontier cell")
    cost = field.plan(fr, clearance=clearance)
    if cost.info["seeds_used"] == 0:  # a frontier cell touches unseen space: d2 = 1 in the known field
        raise ValueError("no frontier cell keeps the clearance: unseen space counts against it, so explore needs r2 = 1 (at most one voxel edge)")
    return {"field": field, "frontiers": fr, "cost": cost, "path": cost.path(np.asarray(start).reshape(1, 3), max_len)[0]}


def next_view(m, seen, start, clearance, camera=None, size=None, headings=8, up=(0, -1, 0), stride=4, max_candidates=1024, weight=1.0,
              min_count=1, max_len=4096, **gain_params):
    """Where to look next, on the map's device: the known field of `seen` (a SeenVolume), the cost-to-go from
    `start` (a voxel index, or metres) at the clearance (metres), the reachable cells on the lattice of absolute indices that
    are multiples of `stride` (ascending cell order, at most max_candidates // headings), `headings` yaws about `up` at each
    (mapfile.next_view_poses), their view gain (gain_params: VoxelMap.view_gain's min_views, radius, margin, margin_rel,
    miss_depth, max_steps, zrange) and the score unknown_free / (1 + weight * metres of the way), ties to the lowest index
    -> dict: pose (4x4), cell, heading, record, index, scores, poses, cells, gain, field, cost (CostField), path ((cells,
    status, cost) from the position back to `start`).  ValueError when no candidate position is reachable."""
    from . import mapfile
    field = m.distance_field(seen=seen, min_views=gain_params.get("min_views", 1), min_count=min_count)
    st = np.asarray(start)
    cost = field.plan(st.reshape(1, 3) if st.dtype.kind == "f" else st.astype(np.int64).reshape(1, 3), clearance=clearance)
    cells = mapfile.next_view_candidates(cost.cost, cost.lo, stride, headings, max_candidates)
    if len(cells) == 0:
        raise ValueError("no candidate position is reachable from the start (%d seeds used, %d cells reachable)"
                         % (cost.info["seeds_used"], cost.info["reachable"]))
    poses = mapfile.next_view_poses(cells, m.voxel, headings, up)
    gain = m.view_gain(seen, poses, camera, size, min_count=min_count, **gain_params)
    at = tuple((cells - cost.lo.astype(np.int64)).T)
    scores, best = mapfile.next_view_choice(gain, cost.cost[at], m.voxel, headings, weight)
    cell = cells[best // int(headings)]
    return {"pose": poses[best], "cell": cell.astype(np.int32), "heading": best % int(headings), "record": gain[best], "index": best, "scores": scores,
            "poses": poses, "cells": cells.astype(np.int32), "gain": gain, "field": field, "cost": cost, "path": cost.path(cell.reshape(1, 3), max_len)[0]}


class CostField:
    """A cost-to-go field over a box of voxel indices (DistanceField.plan, `mapfile plan --cost`): cost [n0, n1, n2]
    uint32, the cheapest way to a goal over free cells in units of a third of a voxel edge per straight step (3, 4, 5 for a
    step along 1, 2, 3 axes), settings.PLAN_NONE where a cell is not free or not reachable; lo, n the box, voxel the map's edge
    in metres, r2 the squared clearance in cells, info the call's counters (mapfile.PLAN_INFO_KEYS; None for a loaded field)."""

    def __init__(self, cost, lo, voxel, r2, info=None, map=None):
        self.cost = cost
        self.lo = np.asarray(lo, np.int32).reshape(3)
        self.n = np.asarray(cost.shape, np.int32)
        self.voxel = float(np.float32(voxel))
        self.r2 = int(r2)
        self.info = info
        self._map = map

    def reachable(self):
        """[n0, n1, n2] bool: the cells a goal can be reached from."""
        from . import mapfile
        return self.cost != mapfile.PLAN_NONE

    def metres(self):
        """[n0, n1, n2] float32: cost * voxel / 3, +inf where there is none.  This is the length of the way in the 3-4-5
        chamfer metric (a diagonal step counts 4/3 or 5/3 of an edge), up to 8 % above or 5 % below the Euclidean length of
        the same way -- not the Euclidean length."""
        with np.errstate(all="ignore"):
            return np.where(self.reachable(), self.cost.astype(np.float32) * np.float32(self.voxel) / np.float32(3), np.float32(np.inf))

    def path(self, starts, max_len=4096):
        """The paths from `starts` ([k, 3] integer voxel indices, or floating-point metres) down the cost field -> a list of
        (cells int32 [length, 3] absolute voxel indices from the start to a goal, status settings.PLAN_*, the start's cost):
        on the device of the map the field came from, and through mapfile.plan_paths -- the same -- otherwise."""
        from . import mapfile
        st = np.asarray(starts)
        if st.dtype.kind == "f":
            st = np.floor(st.astype(np.float32).reshape(-1, 3) / np.float32(self.voxel))
        st = st.astype(np.int64).reshape(-1, 3)
        if self._map is not None and getattr(self._map, "_h", None):
            return self._map.plan_paths(self.cost, self.lo, st, max_len)
        return mapfile.plan_paths(self.cost, self.lo, self.n, st, max_len)

    def path_points(self, starts, max_len=4096):
        """path() with the cells as float32 metres at their centres."""
        from . import mapfile
        return [(mapfile.plan_path_points(c, self.voxel), st, cost) for c, st, cost in self.path(starts, max_len)]

    def save(self, path):
        """The .npz `python -m revo_amd.mapfile plan --cost` writes: cost, lo, n, voxel, r2."""
        from . import mapfile
        return mapfile.write_cost(path, self.cost, self.lo, self.voxel, self.r2)

    @classmethod
    def load(cls, path):
        from . import mapfile
        return cls(*mapfile.read_cost(path))


def align_system(info):
    """(H [6, 6], g [6]) float64 of a MapAlignInfo: the Gauss-Newton system of revo_map_align_system (unknowns v, w)."""
    H, g = np.zeros(36, np.float64), np.zeros(6, np.float64)
    check(_lib.lib().revo_map_align_system(C.byref(info), _p(H, C.POINTER(C.c_double)), _p(g, C.POINTER(C.c_double))))
    return H.reshape(6, 6), g


def align_covariance(info):
    """(cov [6, 6] = sigma2 H^-1, sigma2 = S[15] / (3 matched - 6)) of a record; (None, None) without an evaluation, with too
    few matches or with a singular H."""
    if (info.flags & 1) or 3 * info.matched <= 6:
        return None, None
    H, _ = align_system(info)
    s2 = float(info.S[15]) / float(3 * info.matched - 6)
    try:
        X = np.linalg.inv(H)
    except np.linalg.LinAlgError:
        return None, None
    return s2 * 0.5 * (X + X.T), s2


def align_plane_system(info):
    """(H [6, 6], g [6]) float64 of a MapPlaneInfo: the Gauss-Newton system of revo_map_align_plane_system (unknowns v, w)."""
    H, g = np.zeros(36, np.float64), np.zeros(6, np.float64)
    check(_lib.lib().revo_map_align_plane_system(C.byref(info), _p(H, C.POINTER(C.c_double)), _p(g, C.POINTER(C.c_double))))
    return H.reshape(6, 6), g


def align_plane_covariance(info):
    """(cov [6, 6] = sigma2 H^-1, sigma2 = S[27] / (matched - 6)) of a point-to-plane record (one residual per match);
    (None, None) without an evaluation, with too few matches or with a singular H."""
    if (info.flags & 1) or info.matched <= 6:
        return None, None
    H, _ = align_plane_system(info)
    s2 = float(info.S[27]) / float(info.matched - 6)
    try:
        X = np.linalg.inv(H)
    except np.linalg.LinAlgError:
        return None, None
    return s2 * 0.5 * (X + X.T), s2


def df_align_system(info):
    """(H [6, 6], g [6]) float64 of a MapDfAlignInfo: the Gauss-Newton system of revo_map_df_align_system (unknowns v, w)."""
    H, g = np.zeros(36, np.float64), np.zeros(6, np.float64)
    check(_lib.lib().revo_map_df_align_system(C.byref(info), _p(H, C.POINTER(C.c_double)), _p(g, C.POINTER(C.c_double))))
    return H.reshape(6, 6), g


def df_align_covariance(info):
    """(cov [6, 6] = sigma2 H^-1, sigma2 = S[27] / (matched - 6)) of a distance-field record (one residual per point);
    (None, None) without an evaluation, with too few points or with a singular H."""
    if (info.flags & 1) or info.matched <= 6:
        return None, None
    H, _ = df_align_system(info)
    s2 = float(info.S[27]) / float(info.matched - 6)
    try:
        X = np.linalg.inv(H)
    except np.linalg.LinAlgError:
        return None, None
    return s2 * 0.5 * (X + X.T), s2


def tsdf_track_system(info):
    """(H [6, 6], g [6]) float64 of a MapTsdfTrackInfo: the Gauss-Newton system of revo_map_tsdf_track_system (unknowns v, w)."""
    H, g = np.zeros(36, np.float64), np.zeros(6, np.float64)
    check(_lib.lib().revo_map_tsdf_track_system(C.byref(info), _p(H, C.POINTER(C.c_double)), _p(g, C.POINTER(C.c_double))))
    return H.reshape(6, 6), g


def tsdf_track_covariance(info):
    """(cov [6, 6] = sigma2 H^-1, sigma2 = S[27] / (matched - 6)) of a surface tracking record (one residual per pixel);
    (None, None) without an evaluation, with too few pixels or with a singular H."""
    if (info.flags & 1) or info.matched <= 6:
        return None, None
    H, _ = tsdf_track_system(info)
    s2 = float(info.S[27]) / float(info.matched - 6)
    try:
        X = np.linalg.inv(H)
    except np.linalg.LinAlgError:
        return None, None
    return s2 * 0.5 * (X + X.T), s2


def align_maps(dst, src, T_init=None, shifts=(2, 1, 0), centre=None, min_count_dst=1, min_count_src=1, metric="point", **align_kw):
    """Coarse-to-fine registration of `src` onto `dst` (two VoxelMaps of the same voxel edge): per level of `shifts` both maps
    are coarsened by that shift (0: the maps themselves), aligned with max_dist = that level's edge, and the pose is handed
    down.  centre defaults to the mean of the source's points under T_init, rounded to float32, and stays fixed for the
    whole ladder.  metric: "point" (align) or "plane" (align_plane, whose normal parameters go through align_kw).
    -> the finest level's align() result, with "levels": every level's result."""
    if metric not in ("point", "plane"):
        raise ValueError("metric must be 'point' or 'plane'")
    T = np.eye(4, dtype=np.float32) if T_init is None else np.asarray(T_init, np.float32)
    if centre is None:
        xyz = src.points(min_count_src)[0].astype(np.float64)
        centre = (T[:3, :3].astype(np.float64) @ xyz.mean(0) + T[:3, 3]).astype(np.float32) if len(xyz) else np.zeros(3, np.float32)
    levels = []
    for sh in shifts:
        d, s_ = (dst, src) if sh == 0 else (dst.coarsen(sh), src.coarsen(sh))
        r = (d.align_plane if metric == "plane" else d.align)(s_, T, max_dist=d.voxel, min_count_dst=min_count_dst,
                                                               min_count_src=min_count_src, centre=centre, **align_kw)
        if sh != 0:
            d.close()
            s_.close()
        levels.append(r)
        T = r["T"]
    return dict(levels[-1], levels=levels, centre=np.asarray(centre, np.float32))


def align_merge(dst, src, T_init=None, metric="plane", accept_limit=False, min_count=1, **ladder_kw):
    """Registers `src` onto `dst` with align_maps(dst, src, T_init, metric=metric, **ladder_kw) and, if the ladder converged
    (or stopped at its iteration limit and accept_limit is set), merges it at the pose found: dst.merge_posed(src, T,
    min_count).  -> align_maps' result with "pose_info": merge_posed's info.  RuntimeError, dst unchanged: the ladder was lost,
    or hit its iteration limit without accept_limit."""
    from .settings import ALIGN_CONVERGED, ALIGN_ITER_LIMIT
    r = align_maps(dst, src, T_init, metric=metric, **ladder_kw)
    if not (r["status"] == ALIGN_CONVERGED or (accept_limit and r["status"] == ALIGN_ITER_LIMIT)):
        raise RuntimeError("align_merge: the registration %s (nothing merged)"
                           % ("stopped at its iteration limit" if r["status"] == ALIGN_ITER_LIMIT else "was lost"))
    return dict(r, pose_info=dst.merge_posed(src, r["T"], min_count))


def localize(dst, source, T_init=None, max_dist=None, pad=None, refine="plane", min_count=1, **opts):
    """Registers `source` onto the map `dst` from a start that may lie many voxels off: the distance field of
    dst is built on the device over dst.bounds() grown by `pad` cells (default ceil(max_dist / voxel) + 2), the source's points
    are registered against it (VoxelMap.df_align; opts are its options), and, when source is a map and refine is "plane" or
    "point", the pose found is handed to dst.align_plane / dst.align with max_dist = the voxel edge.
    source: an [N, 3] array of points, a VoxelMap (its points()) or a keyframe pyramid (the xyz of its level-0
    generateColoredPcl, dense as dst is).  max_dist (metres) defaults to 8 voxels.
    -> the last stage's result, with "stages": [("field", result), ("plane" | "point", result)] and "box": (lo, n)."""
    import math
    import torch
    from . import mapfile
    if refine not in ("plane", "point", None):
        raise ValueError("refine must be 'plane', 'point' or None")
    m = dst.map if isinstance(dst, MapWindow) else dst
    src_map = source.map if isinstance(source, MapWindow) else (source if isinstance(source, VoxelMap) else None)
    if src_map is not None:
        pts = src_map.points(min_count)[0]
    elif isinstance(source, ImgPyramidRGBD):
        pts = np.ascontiguousarray(source.generateColoredPcl(0, m.dense)[:, :3])
    else:
        pts = np.ascontiguousarray(np.asarray(source, np.float32).reshape(-1, 3))
    max_dist = 8.0 * m.voxel if max_dist is None else float(max_dist)
    pad = int(math.ceil(float(np.float32(max_dist) / np.float32(m.voxel)))) + 2 if pad is None else int(pad)  # the ratio in float32: 0.24 / 0.02 is 12
    lo, hi, n_solid = m.bounds(min_count)
    if n_solid == 0:
        raise ValueError("localize: the destination map holds no voxel")
    lo, n = mapfile.padded_box(lo, hi, pad)
    dev = "cuda:%d" % m.cameraPyr.device
    d_d2 = torch.empty(tuple(int(x) for x in n), dtype=torch.int32, device=dev)
    m.distance_field_into(d_d2, lo, n, min_count=min_count, wait=False)
    d_pts = torch.from_numpy(pts).to(dev)
    stages = [("field", m.df_align(d_d2, lo, d_pts, T_init, max_dist, **opts))]
    if src_map is not None and refine is not None:
        r = stages[0][1]
        fine = (m.align_plane if refine == "plane" else m.align)(src_map, r["T"], max_dist=m.voxel, min_count_dst=min_count,
                                                                   min_count_src=min_count, centre=r["centre"])
        stages.append((refine, dict(fine, centre=r["centre"])))
    return dict(stages[-1][1], stages=stages, box=(np.asarray(lo, np.int32), np.asarray(n, np.int32)))


class MapWindow:
    """A voxel map that holds exactly the last `window` integrated keyframes: the bounded local map of a long run.  It is
    byte for byte the VoxelMap a fresh handle would build from those keyframes alone.  integrate(kf, T_w_kf) is
    VoxelMap's, so vo.REVO(voxelMap=MapWindow(...)) works unchanged; every other attribute (info, points, render, save, ...)
    is the inner VoxelMap's (`.map`).  keyframes: the poses currently in the map, oldest first; timestamps: their time stamps.

    Per keyframe: it is integrated into a private scratch map on the same context, the scratch map's records are kept in a
    device buffer and merged into the map, and once more than `window` keyframes are held the oldest one's records are
    subtracted again.  Device memory held: 64 bytes x voxels per kept keyframe (at most 64 B x width x height each), beside
    the map and the scratch map of one keyframe.  map_kw: VoxelMap's max_voxels / initial_voxels for the map itself."""

    def __init__(self, cameraPyr, voxel, dense=False, window=1, **map_kw):
        import collections
        if int(window) < 1:
            raise ValueError("window must be >= 1 keyframe")
        self.window = int(window)
        self.map = VoxelMap(cameraPyr, voxel, dense=dense, **map_kw)
        npix = cameraPyr.settings.width * cameraPyr.settings.height  # a keyframe has at most one voxel per pixel
        self._scratch = VoxelMap(cameraPyr, voxel, dense=dense, max_voxels=npix, initial_voxels=npix)
        self._held = collections.deque()  # (T_w_kf, device records or None, voxels, points_dropped, time stamp)

    def __getattr__(self, name):
        if name in ("map", "_scratch", "_held", "window"):
            raise AttributeError(name)
        return getattr(self.map, name)

    @property
    def keyframes(self):
        return [h[0].copy() for h in self._held]

    @property
    def timestamps(self):
        return [h[4] for h in self._held]

    def integrate(self, pyr, T_w):
        import torch
        T_w = np.array(T_w, np.float32).reshape(4, 4)
        sc = self._scratch
        sc.clear()
        sc.integrate(pyr, T_w)
        i = sc.info()
        buf = None
        if i["voxels"]:
            buf = torch.empty(64 * i["voxels"], dtype=torch.uint8, device="cuda:%d" % self.map.cameraPyr.device)
            if sc.export_raw_into(buf) != i["voxels"]:
                raise RuntimeError("the scratch map's export does not match its voxel count")
        self.map.merge(sc)  # REVO_ERR_CAPACITY past max_voxels: the keyframe is not in the map and not in the window
        self._held.append((T_w, buf, i["voxels"], i["points_dropped"], float(pyr.returnTimestamp())))
        while len(self._held) > self.window:
            self._evict()

    def integrate_many(self, pyrs, T_ws):
        for p, T in zip(pyrs, T_ws):
            self.integrate(p, T)

    def raycast(self, *args, **kw):
        """The inner map's raycast (the window only decides which keyframes the map holds)."""
        return self.map.raycast(*args, **kw)

    def raycast_into(self, *args, **kw):
        return self.map.raycast_into(*args, **kw)

    def cast_rays(self, *args, **kw):
        return self.map.cast_rays(*args, **kw)

    def observe(self, *args, **kw):
        """The inner map's observe: what views have looked at, over the voxels the window holds now."""
        return self.map.observe(*args, **kw)

    def distance_field(self, *args, **kw):
        """The inner map's distance field (seen=: the known field)."""
        return self.map.distance_field(*args, **kw)

    def frontiers(self, *args, **kw):
        return self.map.frontiers(*args, **kw)

    def view_gain(self, *args, **kw):
        """The inner map's view_gain: what candidate views would add, over the voxels the window holds now."""
        return self.map.view_gain(*args, **kw)

    def view_gain_into(self, *args, **kw):
        return self.map.view_gain_into(*args, **kw)

    def fuse(self, *args, **kw):
        """The inner map's fuse: depth views into a TSDF volume, by default over the voxels the window holds now."""
        return self.map.fuse(*args, **kw)

    def fuse_into(self, *args, **kw):
        return self.map.fuse_into(*args, **kw)

    def unfuse(self, *args, **kw):
        """The inner map's unfuse: views taken out of a TsdfVolume again (the window's voxels play no part)."""
        return self.map.unfuse(*args, **kw)

    def unfuse_into(self, *args, **kw):
        return self.map.unfuse_into(*args, **kw)

    def mesh(self, *args, **kw):
        return self.map.mesh(*args, **kw)

    def mesh_into(self, *args, **kw):
        return self.map.mesh_into(*args, **kw)

    def surface_raycast(self, *args, **kw):
        """The inner map's surface_raycast: views of a TsdfVolume's surface (the window's voxels play no part)."""
        return self.map.surface_raycast(*args, **kw)

    def surface_raycast_into(self, *args, **kw):
        return self.map.surface_raycast_into(*args, **kw)

    def surface_raycast_many_into(self, *args, **kw):
        """The inner map's surface_raycast_many_into: the window's voxels play no part."""
        return self.map.surface_raycast_many_into(*args, **kw)

    def surface_track_eval(self, *args, **kw):
        """The inner map's surface_track_eval: a depth frame against a TSDF volume (the window's voxels play no part)."""
        return self.map.surface_track_eval(*args, **kw)

    def surface_track(self, *args, **kw):
        return self.map.surface_track(*args, **kw)

    def fuse_many_into(self, *args, **kw):
        """The inner map's batched surface calls: the window's voxels play no part."""
        return self.map.fuse_many_into(*args, **kw)

    def unfuse_many_into(self, *args, **kw):
        """The inner map's unfuse_many_into (the window's voxels play no part)."""
        return self.map.unfuse_many_into(*args, **kw)

    def surface_track_eval_many(self, *args, **kw):
        return self.map.surface_track_eval_many(*args, **kw)

    def surface_track_many(self, *args, **kw):
        return self.map.surface_track_many(*args, **kw)

    def shift_into(self, *args, **kw):
        """The inner map's shift_into: surface volumes moved with their box (the window's voxels play no part)."""
        return self.map.shift_into(*args, **kw)

    def refill_into(self, *args, **kw):
        return self.map.refill_into(*args, **kw)

    def surface_shift(self, *args, **kw):
        return self.map.surface_shift(*args, **kw)

    def surface_refill(self, *args, **kw):
        return self.map.surface_refill(*args, **kw)

    def carve(self, *args, **kw):
        """Not supported: the window evicts a keyframe by subtracting the records it kept of it, and a carved voxel has lost
        sums those records still hold -- the subtraction would be refused.  Carve a plain VoxelMap (carve_eval, which changes
        nothing, is the inner map's)."""
        raise NotImplementedError("MapWindow cannot be carved: its per-keyframe records must stay subtractable")

    def _evict(self):
        _, buf, n, dropped, _ = self._held[0]
        if n:
            self.map.subtract_raw(buf, points_dropped=dropped, keyframes=1, n=n)
        else:  # a keyframe without a voxel still counted: an empty subtraction is a no-op, so its counters ride on one record
            from . import mapfile
            one = np.zeros(1, mapfile.RAW_DTYPE)
            one["count"] = 1
            self.map.merge_raw(one)
            self.map.subtract_raw(one, points_dropped=dropped, keyframes=1)
        self._held.popleft()

    def clear(self):
        self.map.clear()
        self._held.clear()

    def close(self):
        self._held.clear()
        self._scratch.close()
        self.map.close()


class Optimizer:
    """system/optimizer.h:114-186 (the LM loop of one level runs on the device)."""

    ResidualInfo = ResidualInfo

    def __init__(self, settings, cameraPyr):
        self.mSettings = settings
        self._cam = cameraPyr

    def trackFrames(self, refFrame, currFrame, R, T, lvl, resInfo=None):
        """-> (last_residual, R, T): optimizer.cpp:235-311."""
        Rc, Tc = _cm3(R), np.array(T, np.float32).reshape(3)
        info = resInfo if resInfo is not None else ResidualInfo()
        err = C.c_float()
        check(_lib.lib().revo_optimizer_track_level(self._cam._h, refFrame._h, currFrame._h, _p(Rc, f32p),
                                                    _p(Tc, f32p), lvl, C.byref(info), C.byref(err)))
        return err.value, Rc.reshape(3, 3).T.copy(), Tc

    def evalAt(self, refFrame, currFrame, R, T, lvl):
        """calcErrorAndBuffers + calculateWarpUpdate at a fixed pose -> (err, info, A[6,6], b[6])."""
        Rc, Tc = _cm3(R), np.ascontiguousarray(T, np.float32).reshape(3)
        info = ResidualInfo()
        err = C.c_float()
        A = np.empty(36, np.float32)
        b = np.empty(6, np.float32)
        check(_lib.lib().revo_optimizer_eval(self._cam._h, refFrame._h, currFrame._h, _p(Rc, f32p), _p(Tc, f32p), lvl,
                                             C.byref(info), C.byref(err), _p(A, f32p), _p(b, f32p)))
        return err.value, info, A.reshape(6, 6), b


def solve6(cameraPyr, A, b, lam):
    """A.ldlt().solve(b) with A(i,i) *= 1 + lam (optimizer.cpp:258-262) on the device.
    A [n,6,6] symmetric, b [n,6], lam [n] -> x [n,6]."""
    A = np.asarray(A, np.float32).reshape(-1, 36)
    n = A.shape[0]
    buf = np.concatenate([A, np.asarray(b, np.float32).reshape(n, 6), np.asarray(lam, np.float32).reshape(n, 1)], axis=1)
    buf = np.ascontiguousarray(buf, np.float32)
    x = np.empty((n, 6), np.float32)
    check(_lib.lib().revo_optimizer_solve6(cameraPyr._h, n, _p(buf, f32p), _p(x, f32p)))
    return x


class TrackerNew:
    """system/tracker.h:56-105."""

    TRACKER_STATE_OK, TRACKER_STATE_LOST, TRACKER_STATE_NEW_KF, TRACKER_STATE_UNKNOWN = 0, 1, 2, 3

    def __init__(self, config, pyrConfig, cameraPyr):
        self.mSettings = config
        self.mPyrConfig = pyrConfig
        self._cam = cameraPyr
        self.optimizerSettings = getattr(config, "optimizerSettings", None) or OptimizerSettings()
        check(_lib.lib().revo_ctx_set_tracker(cameraPyr._h, C.byref(self.optimizerSettings), C.byref(config)))
        self.histogramLevel = config.histogram_level
        self.mOptimizer = Optimizer(self.optimizerSettings, cameraPyr)
        self.last_evals = np.zeros(MAX_LEVELS, np.int32)
        self.last_info = ResidualInfo()

    def trackFrames(self, R, T, refFrame, currFrame):
        """-> (status, R, T, error): tracker.cpp:294-353."""
        Rc, Tc = _cm3(R), np.array(T, np.float32).reshape(3)
        err, status = C.c_float(), C.c_int()
        evals = np.zeros(MAX_LEVELS, np.int32)
        info = ResidualInfo()
        check(_lib.lib().revo_tracker_track_frames(self._cam._h, refFrame._h, currFrame._h, _p(Rc, f32p), _p(Tc, f32p),
                                                   C.byref(err), C.byref(status), C.byref(info), _p(evals, i32p)))
        self.last_evals, self.last_info = evals, info
        return status.value, Rc.reshape(3, 3).T.copy(), Tc, err.value

    def pairInfo(self, refFrame, currFrame, R, T, lvl):
        """-> PairInfo: the sums of the pair's normal equations at pose (R, T) of level lvl (revo_tracker_pair_info)."""
        Rc, Tc = _cm3(R), np.ascontiguousarray(T, np.float32).reshape(3)
        out = PairInfo()
        check(_lib.lib().revo_tracker_pair_info(self._cam._h, refFrame._h, currFrame._h, _p(Rc, f32p), _p(Tc, f32p), lvl,
                                                C.byref(out)))
        return out

    def assessTrackingQuality(self, estimatedPose, currFrame, return_hist=False):
        Mc = _cm4(estimatedPose)
        st = C.c_int()
        h4 = np.zeros(4, np.int32)
        o4 = np.zeros(4, np.int32)
        check(_lib.lib().revo_tracker_assess_quality(self._cam._h, _p(Mc, f32p), currFrame._h, C.byref(st), _p(h4, i32p),
                                                     _p(o4, i32p)))
        return (st.value, h4, o4) if return_hist else st.value

    def addOldPclAndPose(self, srcFrame, lvl, worldPose, timeStamp=0.0):
        """tracker.cpp:209-223; the cloud is srcFrame.return3DEdges(lvl) and stays in HBM."""
        Mc = _cm4(worldPose)
        check(_lib.lib().revo_tracker_add_old_pcl(self._cam._h, srcFrame._h, lvl, _p(Mc, f32p), float(timeStamp)))

    def addOldPcl(self, pcl, worldPose, timeStamp=0.0):
        """The reference's own signature, addOldPclAndPose(const Eigen::MatrixXf& pcl, worldPose, timeStamp)
        (tracker.cpp:209-223): pcl = N x 4 rows (X,Y,Z,1) in host memory (what return3DEdges gives)."""
        a = np.ascontiguousarray(pcl, np.float32).reshape(-1, 4)
        Mc = _cm4(worldPose)
        check(_lib.lib().revo_tracker_add_old_pcl_host(self._cam._h, _p(a, f32p), a.shape[0], _p(Mc, f32p), float(timeStamp)))

    def clearUpPastLists(self):
        check(_lib.lib().revo_tracker_clear_past(self._cam._h))

    def pastSize(self):
        return _lib.lib().revo_tracker_past_size(self._cam._h)


class BatchTracker:
    """B independent frame-pairs resident in HBM: pyramids of all 2B frames, keyframe
    promotion of the B references and TrackerNew::trackFrames of every pair, enqueued on
    one stream without host round trips.  Inputs/outputs are raw device pointers (e.g.
    torch tensors' data_ptr())."""

    def __init__(self, cameraPyr, n_pairs):
        self._cam = cameraPyr
        self.n_pairs = n_pairs
        self._h = vp()
        check(_lib.lib().revo_batch_create(cameraPyr._h, n_pairs, C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().revo_batch_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @staticmethod
    def _init(init_RT):
        if init_RT is None:
            return None, None
        a = np.ascontiguousarray(init_RT, np.float32)
        return a, _p(a, f32p)

    def track(self, d_bgr, d_depth, d_results, init_RT=None, stream=None):
        keep, ptr = self._init(init_RT)
        check(_lib.lib().revo_batch_track(self._h, d_bgr, d_depth, ptr, d_results, stream))

    def build(self, d_bgr, d_depth, stream=None, borrow_depth=False):
        """borrow_depth: level 0 of the depth pyramid is d_depth itself (no copy); the caller keeps the buffer alive
        and unchanged until the next build of this batch."""
        fn = _lib.lib().revo_batch_build_borrow if borrow_depth else _lib.lib().revo_batch_build
        check(fn(self._h, d_bgr, d_depth, stream))

    def build_u16(self, d_bgr, d_depth_raw, depth_scale_factor, stream=None):
        """build() for raw uint16 depth (device pointer); the metres conversion is fused into the build."""
        check(_lib.lib().revo_batch_build_u16(self._h, d_bgr, d_depth_raw, float(depth_scale_factor), stream))

    def prepare(self, stream=None):
        """Runs on `stream` the part of the last build that was left to its first consumer (the keyframes' distance
        transforms); track_only() does this itself -- call it first only to keep that work out of a timed launch."""
        check(_lib.lib().revo_batch_prepare(self._h, stream))

    def track_only(self, d_results, init_RT=None, stream=None):
        keep, ptr = self._init(init_RT)
        check(_lib.lib().revo_batch_track_only(self._h, ptr, d_results, stream))

    def pair_info(self, d_results=None, RT=None, lvl=0, d_info=None, stream=None):
        """revo_batch_pair_info: the level-lvl PairInfo of every pair in one launch, at the poses of d_results (raw device
        pointer to n_pairs PairResult records, e.g. the ones track_only just wrote) or of RT (host, [n_pairs, 12]: R
        column-major, T) -- exactly one of the two.  d_info: raw device pointer to n_pairs * 192 bytes, 16-byte aligned; the call
        only enqueues.  d_info=None: a buffer of the call's own, and the records come back as a list of PairInfo (waits)."""
        keep, ptr = self._init(RT)
        own = None
        if d_info is None:
            import torch
            own = torch.empty(self.n_pairs * C.sizeof(PairInfo), dtype=torch.uint8, device="cuda")
            d_info = own.data_ptr()
        check(_lib.lib().revo_batch_pair_info(self._h, d_results, ptr, lvl, d_info, stream))
        if own is None:
            return None
        check(_lib.lib().revo_batch_sync(self._h, stream))
        return pair_infos_from_buffer(own.cpu().numpy().tobytes(), self.n_pairs)

    def sync(self, stream=None):
        """Waits for the stream and for the batch's last tracker grid (on whichever stream it ran) and checks its records'
        flags.  The d_results buffer of that launch must still be alive: it is read here (revo_hip.h, revo_batch_sync)."""
        check(_lib.lib().revo_batch_sync(self._h, stream))

    def frame(self, f, settings):
        h = vp()
        check(_lib.lib().revo_batch_frame(self._h, f, C.byref(h)))
        return ImgPyramidRGBD(settings, self._cam, _handle=h, _owned=False)

    def profile_build(self, d_bgr, d_depth, reps=3):
        """-> [(kernel name, mean us alone)]: every kernel of build(borrow_depth=True) + prepare(), HIP events between the
        launches on the batch's own stream (revo_batch_profile_build)."""
        st = StageTimes()
        check(_lib.lib().revo_batch_profile_build(self._h, d_bgr, d_depth, reps, C.byref(st)))
        return [(st.name[i].value.decode(), float(st.us[i])) for i in range(st.n)]

    def time_tracker(self, d_results, reps=5, init_RT=None, stream=None):
        keep, ptr = self._init(init_RT)
        ms = C.c_float()
        check(_lib.lib().revo_batch_time_tracker(self._h, ptr, d_results, stream, reps, C.byref(ms)))
        return ms.value


class StageTimes(C.Structure):
    """revo_stage_times"""
    _fields_ = [("n", C.c_int32), ("us", C.c_float * 24), ("name", (C.c_char * 32) * 24)]


class PipelineInfo(C.Structure):
    """revo_pipeline_info_t"""
    _fields_ = [("batches", C.c_int32), ("pairs_per_step", C.c_int32), ("tracker_streams", C.c_int32),
                ("distinct_hw_queues", C.c_int32), ("streams_replaced", C.c_int32), ("probes_run", C.c_int32),
                ("streams", C.c_void_p * 4), ("steps_submitted", C.c_uint64)]


class Pipeline:
    """revo_pipeline_*: the pipelined batch mode behind one handle -- `depth` resident batches rotate over four streams
    the library owns (build | edge lists + keyframe EDT | two tracker streams), the counterpart of the reference's IO
    thread + REVO::start loop (system.cpp:96,128-284).  submit() returns (ticket, stream): work enqueued on that stream
    before the next-but-one submit runs behind the step's tracker grid (the slot for the result collective)."""

    DEPTH_F32_BORROWED, DEPTH_F32_COPIED, DEPTH_U16 = 0, 1, 2

    def __init__(self, cameraPyr, n_pairs, depth=0, host_results=False):
        self._cam = cameraPyr
        self.n_pairs = n_pairs
        self.host_results = bool(host_results)
        self._h = vp()
        check(_lib.lib().revo_pipeline_create(cameraPyr._h, n_pairs, depth, int(bool(host_results)), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().revo_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, d_bgr, d_depth, d_results=None, init_RT=None, depth_kind=0, depth_scale_factor=1.0, input_ready_event=None):
        """-> (ticket, stream handle the step's tracker grid runs on).  d_*: raw device pointers."""
        keep, ptr = BatchTracker._init(init_RT)
        ticket, stream = C.c_uint64(), vp()
        check(_lib.lib().revo_pipeline_submit(self._h, d_bgr, d_depth, depth_kind, float(depth_scale_factor), ptr, d_results,
                                              input_ready_event, C.byref(ticket), C.byref(stream)))
        return ticket.value, stream.value

    def wait(self, ticket):
        """Blocks until the step (and what the caller put behind its grid) is complete; with host_results -> its records."""
        if not self.host_results:
            check(_lib.lib().revo_pipeline_wait(self._h, ticket, None))
            return None
        out = (PairResult * self.n_pairs)()
        check(_lib.lib().revo_pipeline_wait(self._h, ticket, C.cast(out, vp)))
        return results_from_buffer(bytes(out), self.n_pairs)

    def drain(self):
        check(_lib.lib().revo_pipeline_drain(self._h))

    def info(self):
        i = PipelineInfo()
        check(_lib.lib().revo_pipeline_info(self._h, C.byref(i)))
        return dict(batches=i.batches, pairs_per_step=i.pairs_per_step, tracker_streams=i.tracker_streams,
                    distinct_hw_queues=i.distinct_hw_queues, streams_replaced=i.streams_replaced, probes_run=i.probes_run,
                    streams=[int(x or 0) for x in i.streams], steps_submitted=int(i.steps_submitted))

    def batch_frame(self, ticket, f, settings):
        """Pyramid view of frame f of the batch that holds step `ticket` (valid until its slot is submitted again)."""
        b, h = vp(), vp()
        check(_lib.lib().revo_pipeline_batch(self._h, ticket, C.byref(b)))
        check(_lib.lib().revo_batch_frame(b, f, C.byref(h)))
        return ImgPyramidRGBD(settings, self._cam, _handle=h, _owned=False)

    def pair_info(self, ticket, stream, d_info, d_results=None, RT=None, lvl=0):
        """The PairInfo records of step `ticket`, enqueued on `stream` -- pass the stream submit() returned: the launch then rides
        in the step's after-grid slot (revo_batch_pair_info on revo_pipeline_batch).  d_results: the step's device records."""
        keep, ptr = BatchTracker._init(RT)
        b = vp()
        check(_lib.lib().revo_pipeline_batch(self._h, ticket, C.byref(b)))
        check(_lib.lib().revo_batch_pair_info(b, d_results, ptr, lvl, d_info, stream))

    def time_tracker(self, every_n):
        check(_lib.lib().revo_pipeline_time_tracker(self._h, every_n))

    def set_comm(self, comm, every, d_gathered, ring):
        """revo_pipeline_set_comm: the handle enqueues the all-gather of every window of `every` steps itself, in the
        after-grid slot of the window's last step; d_gathered: raw device pointer, ring * world * every * n_pairs records."""
        check(_lib.lib().revo_pipeline_set_comm(self._h, comm._h if comm is not None else None, every, d_gathered, ring))
        self._comm = comm  # keep it alive as long as it is attached

    def flush_comm(self):
        """-> (steps of the incomplete last window that were gathered, its slot in d_gathered); (0, slot) if nothing was pending."""
        n, slot = C.c_int(), C.c_int()
        check(_lib.lib().revo_pipeline_flush_comm(self._h, C.byref(n), C.byref(slot)))
        return n.value, slot.value

    def tracker_ms(self):
        ms, n = C.c_float(), C.c_int()
        check(_lib.lib().revo_pipeline_tracker_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def rccl_available():
    """(path, version) of the RCCL library librevo_hip.so binds at run time, or raises RevoError."""
    buf, ver = C.create_string_buffer(256), C.c_int()
    check(_lib.lib().revo_comm_available(buf, 256, C.byref(ver)))
    return buf.value.decode(), ver.value


def comm_unique_id():
    """revo_comm_unique_id (rank 0): 128 bytes to ship to the other ranks."""
    buf = (C.c_uint8 * 128)()
    check(_lib.lib().revo_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """revo_comm_*: an RCCL communicator behind the C ABI (one process per GPU).  `uid`: the 128 bytes rank 0 got
    from comm_unique_id(), shipped to every rank by the caller.  Creation is a collective (ncclCommInitRank)."""

    def __init__(self, cameraPyr, uid, world_size, rank):
        self._cam = cameraPyr
        self._h = vp()
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        check(_lib.lib().revo_comm_create(cameraPyr._h, buf, int(world_size), int(rank), C.byref(self._h)))
        self.world_size, self.rank = int(world_size), int(rank)

    def allgather_records(self, d_send, d_recv, n_records, stream=None):
        check(_lib.lib().revo_comm_allgather_records(self._h, d_send, d_recv, int(n_records), stream))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().revo_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBatchTracker:
    """n independent frame-pairs from HOST buffers (revo_track_pairs_*): what a producer like
    IOWrapperRGBD::readNextFrame (iowrapperRGBD.cpp:301-333) holds after decoding -- BGR8 [H,W,3] and depth
    [H,W] (float32 metres, or raw uint16 + depth_scale_factor) per frame.  submit() returns when the inputs
    have been read (H2D done) while the kernels of this and earlier jobs continue; wait() returns the
    records.  Page-locked arrays (e.g. torch pin_memory) are read by DMA at PCIe speed."""

    def __init__(self, cameraPyr, depth_scale_factor=None):
        self._cam = cameraPyr
        self.depth_scale_factor = depth_scale_factor

    def _pack(self, pairs, init_RT):
        n = len(pairs)
        arr = (PairIn * n)()
        keep = []
        want = np.uint16 if self.depth_scale_factor is not None else np.float32
        # revo_track_pairs_submit takes H and W from the context and copies H rows of W pixels out of every buffer:
        # a smaller or differently shaped frame would be read past its end
        H, W = int(self._cam.settings.height), int(self._cam.settings.width)
        if init_RT is not None and len(init_RT) != n:
            raise ValueError("init_RT has %d entries for %d pairs" % (len(init_RT), n))
        for i, (ref, cur) in enumerate(pairs):
            for name, (bgr, dep) in (("ref", ref), ("cur", cur)):
                if bgr.shape != (H, W, 3) or dep.shape != (H, W):
                    raise ValueError("pair %d %s: frames must be BGR [%d,%d,3] and depth [%d,%d] (the context's size), got %s and %s"
                                     % (i, name, H, W, H, W, tuple(bgr.shape), tuple(dep.shape)))
                if bgr.dtype != np.uint8 or dep.dtype != want or bgr.strides[-1] != 1 or bgr.strides[-2] != 3 or dep.strides[-1] != dep.itemsize:
                    raise ValueError("frames must be uint8 BGR [H,W,3] and %s depth [H,W] with contiguous rows" % np.dtype(want).name)
                keep += [bgr, dep]
                setattr(arr[i], name + "_bgr", bgr.ctypes.data)
                setattr(arr[i], name + "_bgr_stride", bgr.strides[0])
                setattr(arr[i], name + "_depth", dep.ctypes.data)
                setattr(arr[i], name + "_depth_stride", dep.strides[0])
            if init_RT is not None:
                R, T = init_RT[i]
                arr[i].R_init[:] = _cm3(R).tolist()
                arr[i].T_init[:] = np.asarray(T, np.float32).tolist()
                arr[i].use_init = 1
        return arr, keep

    def submit(self, pairs, init_RT=None):
        """pairs: list of ((ref_bgr, ref_depth), (cur_bgr, cur_depth)) -> job handle."""
        arr, keep = self._pack(pairs, init_RT)
        job = vp()
        u16 = self.depth_scale_factor is not None
        check(_lib.lib().revo_track_pairs_submit(self._cam._h, len(pairs), C.cast(arr, vp), int(u16),
                                                 float(1.0 if self.depth_scale_factor is None else self.depth_scale_factor), C.byref(job)))
        return (job, len(pairs))

    def wait(self, job):
        h, n = job
        out = (PairResult * n)()
        check(_lib.lib().revo_track_pairs_wait(h, C.cast(out, vp)))
        return results_from_buffer(bytes(out), n)

    def track(self, pairs, init_RT=None):
        return self.wait(self.submit(pairs, init_RT))


def pack_init_RT(Rs, Ts):
    """list of (R 3x3 row-major numpy, T) -> n x 12 float32 (R column-major, T) for BatchTracker."""
    out = np.empty((len(Rs), 12), np.float32)
    for i, (R, T) in enumerate(zip(Rs, Ts)):
        out[i, :9] = _cm3(R)
        out[i, 9:] = np.asarray(T, np.float32)
    return out


def results_from_buffer(buf, n):
    """bytes / uint8 numpy of n revo_pair_result records -> list of dicts."""
    arr = (PairResult * n).from_buffer_copy(bytes(buf))
    out = []
    for r in arr:
        out.append(dict(R=np.array(r.R, np.float32).reshape(3, 3).T.copy(), T=np.array(r.T, np.float32),
                        err=r.err, good=r.good, bad=r.bad, status=r.status,
                        evals=np.array(r.evals, np.int32), flags=r.flags, n_pts0=r.n_pts0))
    return out


def pair_infos_from_buffer(buf, n):
    """n PairInfo records out of a bytes-like object (e.g. a device buffer copied to the host)."""
    arr = (PairInfo * n).from_buffer_copy(bytes(buf)[:n * C.sizeof(PairInfo)])
    return [arr[i] for i in range(n)]


def pair_covariance(info):
    """-> (cov [6, 6] float64, sigma2): revo_pair_info_covariance -- sigma2 = sum_w / (good - 6), cov = sigma2 * H^-1 (translation
    0-2, rotation 3-5, the left-multiplied increment's tangent parameters).  RevoError(REVO_ERR_INVALID_ARG) when the record
    carries no evaluation, has good <= 6 or a rank-deficient H."""
    cov = np.empty(36, np.float64)
    s2 = C.c_double()
    check(_lib.lib().revo_pair_info_covariance(C.byref(info), cov.ctypes.data_as(C.POINTER(C.c_double)), C.byref(s2)))
    return cov.reshape(6, 6), s2.value
