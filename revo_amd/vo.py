"""Sequential visual-odometry driver: REVO::start (system/system.cpp:84-305) through the C ABI
(revo_vo_* in include/revo_hip.h).

The reference runs a producer thread that builds pyramids into a queue and a consumer loop that
tracks the oldest one.  `submit` is the producer side (asynchronous on the device: the pyramid of
frame N+1 is built while frame N is tracked), `track_next` one body of the consumer loop.  `push`
is submit + track_next (no look-ahead); `run` drives both sides like the reference: a producer
(IO) thread feeding a bounded queue and the consumer loop on the calling thread.

Single stream = one GPU (frame N's initial pose and keyframe depend on frame N-1); MultiREVO runs many
independent sequences at once (one tracker grid per step for all of them), api.BatchTracker is the frame-pair
throughput mode.
"""
import ctypes as C
import threading

import numpy as np

from . import _lib, api
from ._lib import check, f32p, u16p, u8p, vp
from .settings import MapTsdfTrackInfo, MultiSurface, MultiSurfaceReport, MultiSurfaceWindowReport, PairInfo, StreamFrame, StreamResult, TrackerSettings


class REVO:
    def __init__(self, settingsPyr, settingsTracker=None, device=0, cameraPyr=None, depth_scale_factor=None,
                 mapDrawer=None, generate_dense_pcl=False, voxelMap=None, pair_info=False, carve=None, surface=None, surface_track=None):
        self.settingsPyr = settingsPyr
        self.settingsTracker = settingsTracker or TrackerSettings()
        self.camPyr = cameraPyr or api.CameraPyr(settingsPyr, device=device)
        self.mTracker = api.TrackerNew(self.settingsTracker, settingsPyr, self.camPyr)
        self._h = vp()
        check(_lib.lib().revo_vo_create(self.camPyr._h, C.byref(self._h)))
        self.poses = []  # (timestamp, 4x4 curr->world)
        self.depth_scale_factor = depth_scale_factor  # set: depth arrives as raw uint16
        # ply.ModelExporter (MapDrawer's model half): gets one coloured cloud + pose per keyframe like
        # system.cpp:162-168,232-238; generate_dense_pcl is DO_GENERATE_DENSE_PCL
        self.mpMapDrawer = mapDrawer
        self.generate_dense_pcl = bool(generate_dense_pcl)
        # api.VoxelMap: every keyframe the driver reports (the first frame included) is fused into it at its T_w_kf, the moment
        # the drawer gets its cloud; on the device, no cloud goes through the host
        self.voxelMap = voxelMap
        # carve: True or a dict of api.VoxelMap.carve's parameters (radius, min_views, min_count, max_count, margin, margin_rel):
        # free-space carving with every new keyframe's own pyramid at its T_w_kf, BEFORE that keyframe is
        # integrated -- what the keyframe looks through leaves the map, then what it sees joins it.  carves[i]: (keyframe time
        # stamp, T_w_kf, info dict) per keyframe, info None where the pose's rotation fails the library's is_orthogonal rule
        # (that keyframe carves nothing, is counted in carve_skipped and warned about once; it is integrated all the same).  Off by default: nothing new is enqueued.
        self.carve = None if carve is None or carve is False else ({} if carve is True else dict(carve))
        self.carves = []
        self.carve_skipped = 0  # keyframes that carved nothing for their pose (warned about once)
        if self.carve is not None:
            if voxelMap is None:
                raise ValueError("carve needs a voxelMap")
            if isinstance(voxelMap, api.MapWindow):
                raise ValueError("carve is not supported with a MapWindow: its per-keyframe records must stay subtractable")
        # surface: an api.SurfaceVolume of voxelMap: every keyframe's pyramid is fused into its volumes at T_w_kf where
        # the keyframe is reported to the map, after the carve and beside the integration -- one accumulating call, enqueued only.
        # A keyframe whose pose's rotation fails the library's is_orthogonal rule is not fused and counted in surface_skipped.
        # Off by default: nothing new is enqueued.
        self.surface = surface
        self.surface_skipped = 0
        if surface is not None:
            if voxelMap is None:
                raise ValueError("surface needs a voxelMap")
            if isinstance(voxelMap, api.MapWindow) and not isinstance(surface, api.SurfaceWindow):
                raise ValueError("surface is not supported with a MapWindow: the volumes keep what the window evicts")
            if surface.map is not voxelMap:
                raise ValueError("the surface belongs to another map than voxelMap")
        # surface_track: True or a dict of api.SurfaceVolume.track's parameters (max_dist, stride, min_weight, centre, max_iters, eps_t,
        # eps_r, min_matched): frame-to-model tracking.  Every keyframe is tracked against the surface as it stands, from
        # its T_w_kf, before it is fused; where that converges the keyframe is fused at the refined pose, otherwise at T_w_kf (the
        # first keyframes meet an empty volume: LOST, nothing changes).  surface_tracks[i]: (keyframe time stamp, T_w_kf, the pose it
        # was fused at, the MapTsdfTrackInfo at the loop's last pose or None, status); a keyframe whose rotation fails the is_orthogonal
        # rule is not tracked (info None, LOST).  The reported trajectory, the voxel map's integration and the carve keep T_w_kf.  Off
        # by default: nothing new is enqueued.  With an api.FollowingSurface the box follows the keyframe's pose before it is
        # tracked (and, as always, before it is fused); any other surface is not asked to move.
        # an api.SurfaceWindow names a keyframe again when it leaves the window, and the driver's keyframe pyramid is only
        # borrowed: the window keeps device copies of its images, and the colour image is the submitted frame's, kept here by time
        # stamp from submit until the frame after it has been tracked.  Nothing is kept for any other surface.
        # run(io_thread=True) submits on a producer thread while track_next reads and prunes here: both sides hold _window_lock.
        self._window_bgr = {} if isinstance(surface, api.SurfaceWindow) and surface.d_color is not None else None
        self._window_lock = threading.Lock()
        self.surface_track = None if surface_track is None or surface_track is False else ({} if surface_track is True else dict(surface_track))
        self.surface_tracks = []
        if self.surface_track is not None and surface is None:
            raise ValueError("surface_track needs a surface")
        # pair_info: every reported pose comes with its level-0 settings.PairInfo (the information matrix of the relative pose
        # curr -> keyframe at the final pose) and that keyframe's time stamp: pair_infos[i] belongs to poses[i]
        self.pair_info = bool(pair_info)
        self.pair_infos = []  # (PairInfo, keyframe timestamp)
        if self.pair_info:
            check(_lib.lib().revo_vo_set_pair_info(self._h, 1))

    def last_pair_info(self):
        """(PairInfo, keyframe timestamp) of the frame track_next reported last (pair_info=True)."""
        info, kts = PairInfo(), C.c_double()
        check(_lib.lib().revo_vo_last_pair_info(self._h, C.byref(info), C.byref(kts)))
        return info, kts.value

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().revo_vo_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def nKeyFrames(self):
        return _lib.lib().revo_vo_num_keyframes(self._h)

    def submit(self, bgr, depth, timestamp):
        """IOWrapperRGBD::generateImgPyramidFromFiles: build the pyramid, push it to the queue."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if self._window_bgr is not None:
            held = bgr.copy()
            with self._window_lock:
                self._window_bgr[float(timestamp)] = held
        if self.depth_scale_factor is not None and np.asarray(depth).dtype == np.uint16:
            # iowrapperRGBD.cpp:326-327 (depth.convertTo(CV_32FC1, 1/scale)) runs inside the device build
            raw = np.ascontiguousarray(depth, np.uint16)
            h, w = raw.shape
            if bgr.shape != (h, w, 3) or (w, h) != (self.settingsPyr.width, self.settingsPyr.height):
                raise ValueError("image size does not match the settings")
            check(_lib.lib().revo_vo_submit_u16(self._h, bgr.ctypes.data_as(u8p), w * 3, raw.ctypes.data_as(u16p), w * 2,
                                                float(self.depth_scale_factor), float(timestamp)))
            return
        depth = np.ascontiguousarray(depth, np.float32)
        h, w = depth.shape
        if bgr.shape != (h, w, 3) or (w, h) != (self.settingsPyr.width, self.settingsPyr.height):
            raise ValueError("image size does not match the settings")
        check(_lib.lib().revo_vo_submit(self._h, bgr.ctypes.data_as(u8p), w * 3, depth.ctypes.data_as(f32p), w * 4,
                                        float(timestamp)))

    def track_next(self):
        """One loop body of REVO::start on the oldest queued frame -> (4x4 pose, new_keyframe)."""
        pose = np.empty(16, np.float32)
        kf, ts = C.c_int(), C.c_double()
        check(_lib.lib().revo_vo_track_next(self._h, pose.ctypes.data_as(f32p), C.byref(kf), C.byref(ts)))
        M = pose.reshape(4, 4).T.copy()
        self.poses.append((ts.value, M))
        if self.pair_info:
            self.pair_infos.append(self.last_pair_info())
        if kf.value and (self.mpMapDrawer is not None or self.voxelMap is not None):
            kfPyr, T_w_kf = self.keyframe()
            if self.mpMapDrawer is not None:
                self.mpMapDrawer.addPclAndKfPoseToQueue(kfPyr.generateColoredPcl(0, self.generate_dense_pcl), T_w_kf)
            if self.voxelMap is not None:
                if self.carve is not None:
                    self._carve_with(kfPyr, T_w_kf)
                self.voxelMap.integrate(kfPyr, T_w_kf)
                if self.surface is not None:
                    self._surface_with(kfPyr, T_w_kf if self.surface_track is None else self._surface_track_with(kfPyr, T_w_kf))
        if self._window_bgr is not None and len(self.poses) > 1:  # a keyframe is the frame just tracked or the one before it
            with self._window_lock:
                for t in [t for t in self._window_bgr if t < self.poses[-2][0]]:
                    del self._window_bgr[t]
        return M, bool(kf.value)

    def _surface_track_with(self, kfPyr, T_w_kf):
        """The keyframe tracked against the surface as it stands -> the pose to fuse it at."""
        from . import mapfile
        T0 = np.asarray(T_w_kf, np.float32)
        info, status, T = None, mapfile.ALIGN_LOST, T0
        if mapfile.pose_is_orthogonal(T0[:3, :3]):
            follow = getattr(self.surface, "follow", None)
            if follow is not None:  # an api.FollowingSurface: the box goes where the keyframe looks before it is tracked
                follow(T0)
            r = self.surface.track(kfPyr, T0, **self.surface_track)
            info, status = r["info"], r["status"]
            if status == mapfile.ALIGN_CONVERGED:
                T = r["T"]
        self.surface_tracks.append((kfPyr.returnTimestamp(), T0, T, info, status))
        return T

    def _surface_with(self, kfPyr, T_w_kf):
        from . import mapfile
        if mapfile.pose_is_orthogonal(np.asarray(T_w_kf, np.float32)[:3, :3]):
            if self._window_bgr is not None:
                with self._window_lock:
                    bgr = self._window_bgr[float(kfPyr.returnTimestamp())]
                self.surface.integrate((kfPyr, T_w_kf), bgr=bgr)
            else:
                self.surface.integrate((kfPyr, T_w_kf))
            return
        self.surface_skipped += 1
        if self.surface_skipped == 1:
            import warnings
            warnings.warn("REVO surface: the rotation of a keyframe pose is no longer orthogonal to 1e-5 (float32 drift); that "
                          "keyframe is not fused -- see REVO.surface_skipped for how many", RuntimeWarning, stacklevel=3)

    def _carve_with(self, kfPyr, T_w_kf):
        from . import mapfile
        info = None
        if mapfile.pose_is_orthogonal(np.asarray(T_w_kf, np.float32)[:3, :3]):
            _, info, _ = self.voxelMap.carve([(kfPyr, T_w_kf)], records=False, **self.carve)
        else:
            self.carve_skipped += 1
            if self.carve_skipped == 1:
                import warnings
                warnings.warn("REVO carve: the rotation of a keyframe pose is no longer orthogonal to 1e-5 (float32 drift); that "
                              "keyframe carves nothing -- see REVO.carve_skipped for how many", RuntimeWarning, stacklevel=3)
        self.carves.append((kfPyr.returnTimestamp(), np.array(T_w_kf, np.float32), info))

    def keyframe(self):
        """(kfPyr, kfPyr->getTransKFtoWorld()); the pyramid is borrowed -- valid until the next track_next."""
        h = vp()
        T = np.empty(16, np.float32)
        check(_lib.lib().revo_vo_keyframe(self._h, C.byref(h), T.ctypes.data_as(f32p)))
        pyr = api.ImgPyramidRGBD(self.settingsPyr, self.camPyr, _handle=h, _owned=False)
        pyr._vo = self  # keep the driver (owner of the handle) alive
        return pyr, T.reshape(4, 4).T.copy()

    def push(self, bgr, depth, timestamp):
        self.submit(bgr, depth, timestamp)
        return self.track_next()

    def run(self, frames, io_thread=True, max_queue=4):
        """frames: iterable of (bgr, depth, timestamp).

        io_thread=True is the reference's threading (system.cpp:96, iowrapperRGBD.cpp:279-288): a
        producer thread builds pyramids into the queue (host copy into pinned staging + asynchronous
        device build) while this thread runs the consumer loop.  io_thread=False keeps one frame of
        look-ahead on a single thread.  Both give the same bits as `push` per frame."""
        if not io_thread:
            out = []
            it = iter(frames)
            try:
                f = next(it)
            except StopIteration:
                return out
            self.submit(*f[:3])
            for f in it:
                self.submit(*f[:3])
                out.append(self.track_next())
            out.append(self.track_next())
            return out
        L = _lib.lib()
        check(L.revo_vo_set_max_queue(self._h, int(max_queue)))  # bounded queue inside the library, stream open
        state = {"err": None}

        def producer():
            try:
                for f in frames:
                    if state["err"] is not None:
                        break
                    self.submit(*f[:3])  # blocks while max_queue pyramids wait
            except BaseException as e:  # surfaced on the consumer thread
                state["err"] = e
            finally:
                L.revo_vo_close(self._h)  # end of stream: the consumer's wait returns 0 once the queue drained

        th = threading.Thread(target=producer, name="revo-io", daemon=True)
        th.start()
        out = []
        try:
            while L.revo_vo_wait_frame(self._h) == 1:
                out.append(self.track_next())
        except BaseException as e:
            state["err"] = state["err"] or e
            raise
        finally:
            L.revo_vo_set_max_queue(self._h, 0)  # never leave the producer blocked on a full queue
            th.join()
        if state["err"] is not None:
            raise state["err"]
        return out

    def tum_lines(self):
        """REVO::writePose, system.cpp:76-80 (see tum_lines below)."""
        return tum_lines(self.poses)


def tum_lines(poses):
    """REVO::writePose, system.cpp:76-80: 'ts tx ty tz qx qy qz qw', std::fixed, for [(timestamp, 4x4 pose)].  The stream's
    precision is set to 9 AFTER the time stamp has been written and stays set (std::setprecision is sticky): the first line
    carries the time stamp with the default 6 decimals, every later line with 9 -- reproduced as the reference's file has it."""
    out = []
    for i, (ts, M) in enumerate(poses):
        q = _quat_xyzw(M[:3, :3])
        out.append(("%.6f" if i == 0 else "%.9f") % ts + " %.9f %.9f %.9f %.9f %.9f %.9f %.9f" % (tuple(M[:3, 3]) + tuple(q)))
    return out


class SequenceResult(list):
    """One sequence of MultiREVO.run: [(4x4 pose, new_keyframe)] in frame order, `poses` [(timestamp, 4x4)], tum_lines(),
    `map`: its api.VoxelMap (MultiREVO(map_voxel=...)) or None, and `surface`, `surface_tracks`, `surface_skipped`: its
    api.SurfaceVolume (MultiREVO(surface=...)) with what REVO.surface_tracks and REVO.surface_skipped hold for the sequence.  With
    MultiREVO(surface=dict(..., window=N)) surface.views is the number of views the window holds, and surface_evictions and
    surface_evictions_refused count the views that left it and those of them the device refused to take out."""

    def __init__(self):
        super().__init__()
        self.poses = []
        self.pair_infos = []  # MultiREVO(pair_info=True): (PairInfo, keyframe timestamp) per pose
        self.map = None
        # MultiREVO(surface=...): the sequence's api.SurfaceVolume, REVO.surface_tracks' tuples (surface_track) and the keyframes not fused
        self.surface = None
        self.surface_tracks = []
        self.surface_skipped = 0
        # MultiREVO(surface=dict(..., window=N)): the views that left the window, and those of them the device refused to take out
        # (such a view was forgotten and stayed in the volumes)
        self.surface_evictions = 0
        self.surface_evictions_refused = 0

    def tum_lines(self):
        return tum_lines(self.poses)


class MultiREVO:
    """Many independent sequences at once (revo_vo_multi_* in include/revo_hip.h): n_streams REVO::start loops advanced in
    lockstep, one tracker grid and one quality vote per step for all of them.  Per stream the poses, keyframe decisions and
    time stamps are those of a REVO on that sequence alone.

    The tracker settings are a snapshot taken when the handle is created, and so is the exact-sums mode (exact_sums: it
    applies to the context the handle creates; a cameraPyr handed in keeps its own, see api.CameraPyr.setExactSums).

    submit([(stream, bgr, depth, timestamp), ...]) queues at most one frame per stream (one batched build), step() runs one
    loop body for every stream with work and returns [(stream, 4x4 pose, new_keyframe, timestamp)].  A keyframe change is
    reported one step late: the step whose vote asks for it reports nothing for that stream, the next one reports the frame
    (re-tracked against the new keyframe) with new_keyframe = True."""

    map_voxel, map_dense, map_max_voxels = None, False, 1 << 24  # run()'s per-sequence maps: off unless __init__ sets them
    pair_info = False  # run() collects each pose's PairInfo: off unless __init__ sets it
    surface, surface_track = None, None  # run()'s per-sequence surfaces: off unless __init__ sets them

    def __init__(self, settingsPyr, n_streams, settingsTracker=None, device=0, cameraPyr=None, depth_scale_factor=None,
                 max_queue=2, exact_sums=False, map_voxel=None, map_dense=False, map_max_voxels=1 << 24, pair_info=False, surface=None,
                 surface_track=None):
        self.settingsPyr = settingsPyr
        self.settingsTracker = settingsTracker or TrackerSettings()
        if cameraPyr is None:
            self.camPyr = api.CameraPyr(settingsPyr, device=device, exact_sums=exact_sums)
            self.mTracker = api.TrackerNew(self.settingsTracker, settingsPyr, self.camPyr)  # the context's tracker settings
        else:
            # A context handed in may be shared with a running REVO: setting its tracker would clear that driver's past clouds
            # and change its settings.  The handle takes the context's tracker settings as they are.
            if settingsTracker is not None:
                raise ValueError("MultiREVO on a given cameraPyr uses that context's tracker settings: pass settingsTracker=None")
            if exact_sums:
                raise ValueError("MultiREVO on a given cameraPyr uses that context's exact-sums mode: set it on the cameraPyr")
            self.camPyr = cameraPyr
        self.device = int(device)
        self.n_streams = int(n_streams)
        self.max_queue = int(max_queue)
        self.depth_scale_factor = depth_scale_factor  # set: depth arrives as raw uint16
        self._h = vp()
        check(_lib.lib().revo_vo_multi_create(self.camPyr._h, self.n_streams, self.max_queue, C.byref(self._h)))
        self._out = (StreamResult * self.n_streams)()
        # run(): one api.VoxelMap per sequence (voxel edge map_voxel, cloud mode map_dense = DO_GENERATE_DENSE_PCL), fed by the
        # step's batched integration of the keyframes its stream promotes
        self.map_voxel = map_voxel
        self.map_dense = bool(map_dense)
        self.map_max_voxels = int(map_max_voxels)
        self._maps = [None] * self.n_streams
        # run(): one api.SurfaceVolume per sequence on its map (surface: dict(lo=, n=[, trunc=, color=, window=])), fed by the step's batched
        # track and fuse of the keyframes its stream promotes; surface_track: None | True | dict, as REVO takes it.
        # window=N: each surface holds its stream's last N fused keyframes (attach_surface's window)
        if surface is not None and map_voxel is None:
            raise ValueError("surface= needs map_voxel: a sequence's surface lives on its map")
        if surface_track is not None and surface_track is not False and surface is None:
            raise ValueError("surface_track needs a surface")
        self.surface = dict(surface) if surface is not None else None
        self.surface_track = surface_track
        self._surfaces = [None] * self.n_streams  # per stream: (SurfaceVolume, the log its reports go to, keyframes seen, tracking)
        # pair_info: one information launch per step for all streams; last_pair_info(stream) belongs to the stream's last reported pose
        self.pair_info = bool(pair_info)
        if self.pair_info:
            check(_lib.lib().revo_vo_multi_set_pair_info(self._h, 1))

    def last_pair_info(self, stream):
        """(PairInfo, keyframe timestamp) of the frame the stream reported last (pair_info=True)."""
        info, kts = PairInfo(), C.c_double()
        check(_lib.lib().revo_vo_multi_pair_info(self._h, int(stream), C.byref(info), C.byref(kts)))
        return info, kts.value

    def attach_map(self, stream, voxelMap):
        """Every keyframe `stream` promotes from now on is integrated into voxelMap (None detaches); reset() detaches."""
        check(_lib.lib().revo_vo_multi_attach_map(self._h, int(stream), voxelMap._h if voxelMap is not None else None))
        self._maps[int(stream)] = voxelMap

    def attach_surface(self, stream, surface, track=None, log=None, window=None):
        """Every keyframe `stream` promotes from now on is fused into `surface` (an api.SurfaceVolume on a map of this handle's
        context; None detaches; reset() detaches), in the step's one batched launch, as REVO(surface=) does it for one sequence.
        track: None | True | dict of SurfaceVolume.track's options (REVO's surface_track) -- the keyframe is tracked against the
        surface as it stands first, all streams' loops in lockstep, and fused at the refined pose where the loop converged.
        log: the object whose surface_tracks (REVO.surface_tracks' tuples) and surface_skipped are kept current (default: the
        surface itself gets both attributes).  The surface's `views` and per-view counts are kept current too.
        window: None | N >= 1 -- the surface holds the stream's last N fused keyframes (revo_vo_multi_surface_window): the
        step keeps device copies of each fused keyframe's depth and colour image and takes the oldest view out again, all streams'
        evictions in one batched unfuse, without a wait.  `views` is then the number of views held; log.surface_evictions and
        log.surface_evictions_refused count the views that left and those the device refused (forgotten, still in the volumes).
        The ring lives in the driver: an api.SurfaceWindow is refused (two rings would disagree) -- pass a SurfaceVolume and window=."""
        from . import mapfile
        s = int(stream)
        if isinstance(surface, api.SurfaceWindow):
            raise ValueError("MultiREVO keeps the window itself: attach an api.SurfaceVolume with window=N, not an api.SurfaceWindow")
        if window is not None and not 1 <= int(window) <= 1024:
            raise ValueError("window= is None or 1 .. 1024 views")
        if surface is None:
            check(_lib.lib().revo_vo_multi_attach_surface(self._h, s, None))
            self._surfaces[s] = None
            return
        if track is False:
            track = None
        opts = {} if track is None or track is True else dict(track)
        rec = MultiSurface()
        rec.map = surface.map._h
        rec.box = surface.map._df_box(surface.lo, tuple(int(x) for x in surface.n), 0, 1)
        rec.trunc = float(surface.trunc)
        rec.track = 0 if track is None else 1
        rec.tsdf = surface.d_tsdf.data_ptr()
        rec.color = surface.d_color.data_ptr() if surface.d_color is not None else None
        if track is not None:
            known = ("max_dist", "stride", "min_weight", "centre", "max_iters", "eps_t", "eps_r", "min_matched")
            if set(opts) - set(known):
                raise ValueError("surface_track takes %s" % ", ".join(known))
            centre = opts.get("centre")
            if centre is None:
                centre = mapfile.tsdf_track_centre(surface.lo, tuple(int(x) for x in surface.n), surface.map.voxel)
            p = rec.track_prm
            p.max_dist = 0.0 if opts.get("max_dist") is None else float(opts["max_dist"])
            p.stride, p.min_weight = int(opts.get("stride", 1)), int(opts.get("min_weight", 1))
            p.centre[:] = [float(x) for x in np.asarray(centre, np.float32).reshape(3)]
            o = rec.track_opts
            o.max_iters, o.eps_t, o.eps_r = int(opts.get("max_iters", 30)), float(opts.get("eps_t", 1e-6)), float(opts.get("eps_r", 1e-6))
            o.min_matched = int(opts.get("min_matched", 12))
        import torch
        torch.cuda.current_stream(surface.d_tsdf.device).synchronize()  # the volumes' earlier use is over before the tracker stream writes
        check(_lib.lib().revo_vo_multi_attach_surface(self._h, s, C.byref(rec)))
        if window is not None:
            check(_lib.lib().revo_vo_multi_surface_window(self._h, s, int(window)))
        log = surface if log is None else log
        log.surface_tracks, log.surface_skipped = [], 0
        log.surface_evictions, log.surface_evictions_refused = 0, 0
        self._surfaces[s] = [surface, log, self.nKeyFrames(s), track is not None, window is not None]

    def surface_last(self, stream):
        """The MultiSurfaceReport of the stream's last keyframe since its surface was attached; waits for that step's fuse."""
        rep = MultiSurfaceReport()
        check(_lib.lib().revo_vo_multi_surface_last(self._h, int(stream), C.byref(rep)))
        return rep

    def surface_window_last(self, stream):
        """The MultiSurfaceWindowReport of the stream's surface window: the views held, the evictions so far and the last one's
        keyframe time stamp and result; waits for that step's work."""
        rep = MultiSurfaceWindowReport()
        check(_lib.lib().revo_vo_multi_surface_window_last(self._h, int(stream), C.byref(rep)))
        return rep

    def surface_views(self, poses_by_stream, **kw):
        """Views of the streams' attached surfaces as they stand (api.raycast_surfaces): all streams' views in batched
        calls, enqueued on the tracker stream behind the last step's fuse, so views of running sequences need no wait in between.
        poses_by_stream: {stream: poses} or a list with one entry per stream (None: no views of that stream); an entry is the poses
        (one 4x4, or any number of them) or a tuple (poses[, camera, size, zrange]).  kw: raycast_surfaces' step, min_weight,
        max_steps, normals, colors, device.  -> {stream: what SurfaceVolume.raycast returns for that stream's surface}."""
        items = poses_by_stream.items() if isinstance(poses_by_stream, dict) else enumerate(poses_by_stream)
        streams, entries = [], []
        for s, entry in items:
            if entry is None:
                continue
            s = int(s)
            if not 0 <= s < self.n_streams or self._surfaces[s] is None:
                raise ValueError("stream %d has no surface attached" % s)
            streams.append(s)
            entries.append((self._surfaces[s][0],) + (tuple(entry) if isinstance(entry, tuple) else (entry,)))
        return dict(zip(streams, api.raycast_surfaces(entries, **kw)))

    def _poll_surfaces(self):
        """Behind a step: the report of every stream that promoted a keyframe in it goes to the stream's log and surface."""
        for s, att in enumerate(self._surfaces):
            if att is None:
                continue
            n = self.nKeyFrames(s)
            if n == att[2]:
                continue
            att[2] = n
            surface, log, _, tracking, windowed = att
            rep = self.surface_last(s)
            as44 = lambda a: np.array(list(a), np.float32).reshape(4, 4).T.copy()  # noqa: E731
            if tracking:
                info = MapTsdfTrackInfo.from_buffer_copy(bytes(rep.track)) if rep.tracked else None
                log.surface_tracks.append((float(rep.timestamp), as44(rep.T_w_kf), as44(rep.T_fused), info, int(rep.status)))
            log.surface_skipped = int(rep.keyframes_skipped)
            if rep.fused:
                import torch
                vi = rep.view_info
                row = [vi.outside, vi.unknown, vi.free_space, vi.confirmed, vi.occluded, vi.edge, 0, 0]
                surface._vinfo.append(torch.tensor(np.array(row, np.uint32).view(np.int32), dtype=torch.int32, device=surface.d_tsdf.device))
                surface.views += 1
            if windowed:  # a step evicts at most one view per stream: the oldest row leaves with it, refused or not
                win = self.surface_window_last(s)
                if int(win.evictions) > log.surface_evictions:
                    log.surface_evictions = int(win.evictions)
                    log.surface_evictions_refused += 1 if win.evicted.status else 0
                    del surface._vinfo[0]
                surface.views = int(win.held)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().revo_vo_multi_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def submit(self, frames):
        """frames: [(stream, bgr, depth, timestamp)], at most one per stream; all f32 metres or (depth_scale_factor set) all
        raw uint16."""
        frames = list(frames)
        if not frames:
            return
        w, h = self.settingsPyr.width, self.settingsPyr.height
        u16 = self.depth_scale_factor is not None and np.asarray(frames[0][2]).dtype == np.uint16
        arr = (StreamFrame * len(frames))()
        keep = []
        for i, (s, bgr, depth, ts) in enumerate(frames):
            bgr = np.ascontiguousarray(bgr, np.uint8)
            depth = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32)
            if bgr.shape != (h, w, 3) or depth.shape != (h, w):
                raise ValueError("image size does not match the settings")
            keep += [bgr, depth]
            arr[i].stream = int(s)
            arr[i].bgr, arr[i].bgr_stride = bgr.ctypes.data, w * 3
            arr[i].depth, arr[i].depth_stride = depth.ctypes.data, w * depth.itemsize
            arr[i].timestamp = float(ts)
        check(_lib.lib().revo_vo_multi_submit(self._h, len(frames), arr, 1 if u16 else 0,
                                              float(self.depth_scale_factor) if u16 else 0.0))

    def submit_device(self, frames, producer_stream=None):
        """submit() with torch device tensors: [(stream, bgr [H,W,3] uint8, depth [H,W] float32 metres or (depth_scale_factor
        set) uint16, timestamp)], rows packed.  The frames are copied on the device after `producer_stream` (default: the
        current torch stream) reaches this point; returns once they are copied, so the tensors may be reused.  Per stream the
        results are bit-identical to submit() on the same pixels."""
        import torch
        frames = list(frames)
        if not frames:
            return
        w, h = self.settingsPyr.width, self.settingsPyr.height
        u16 = frames[0][2].dtype == torch.uint16
        if u16 and self.depth_scale_factor is None:
            raise ValueError("uint16 depth needs depth_scale_factor")
        arr = (StreamFrame * len(frames))()
        for i, (s, bgr, depth, ts) in enumerate(frames):
            if bgr.dtype != torch.uint8 or tuple(bgr.shape) != (h, w, 3) or tuple(depth.shape) != (h, w):
                raise ValueError("image size or type does not match the settings")
            if depth.dtype != (torch.uint16 if u16 else torch.float32):
                raise ValueError("all depth maps of one submit are uint16 or all float32")
            if bgr.stride() != (w * 3, 3, 1) or depth.stride(1) != 1:
                raise ValueError("rows must be packed")
            arr[i].stream = int(s)
            arr[i].bgr, arr[i].bgr_stride = bgr.data_ptr(), w * 3
            arr[i].depth, arr[i].depth_stride = depth.data_ptr(), depth.stride(0) * depth.element_size()
            arr[i].timestamp = float(ts)
        ps = producer_stream if producer_stream is not None else torch.cuda.current_stream(frames[0][1].device)
        check(_lib.lib().revo_vo_multi_submit_device(self._h, len(frames), arr, 1 if u16 else 0,
                                                     float(self.depth_scale_factor) if u16 else 0.0, C.c_void_p(ps.cuda_stream)))

    def step(self):
        n = C.c_int()
        check(_lib.lib().revo_vo_multi_step(self._h, self._out, C.byref(n)))
        if any(a is not None for a in self._surfaces):
            self._poll_surfaces()
        res = []
        for r in self._out[:n.value]:
            M = np.ctypeslib.as_array(r.pose).reshape(4, 4).T.copy()
            res.append((int(r.stream), M, bool(r.new_keyframe), float(r.timestamp)))
        return res

    def pending(self, stream):
        return _lib.lib().revo_vo_multi_pending(self._h, int(stream))

    def reset(self, stream):
        check(_lib.lib().revo_vo_multi_reset(self._h, int(stream)))
        self._maps[int(stream)] = None
        self._surfaces[int(stream)] = None

    def nKeyFrames(self, stream):
        return _lib.lib().revo_vo_multi_num_keyframes(self._h, int(stream))

    def keyframe(self, stream):
        """(kfPyr, getTransKFtoWorld()) of one stream; the pyramid is borrowed -- valid until the next step."""
        hp = vp()
        T = np.empty(16, np.float32)
        check(_lib.lib().revo_vo_multi_keyframe(self._h, int(stream), C.byref(hp), T.ctypes.data_as(f32p)))
        pyr = api.ImgPyramidRGBD(self.settingsPyr, self.camPyr, _handle=hp, _owned=False)
        pyr._vo = self
        return pyr, T.reshape(4, 4).T.copy()

    def run(self, sequences):
        """sequences: any number of iterables of (bgr, depth, timestamp), host arrays or device tensors (submit_device,
        complete when yielded, e.g. tum.GpuFrameSource).  Runs them n_streams at a time (a stream that
        finishes its sequence is reset and takes the next one, lowest stream first) and returns one SequenceResult per
        sequence, in the order given.  The frames of step t+1 are submitted before step t runs, so their build overlaps it."""
        seqs = list(sequences)
        out = [SequenceResult() for _ in seqs]
        seq_of = [None] * self.n_streams      # stream -> sequence index
        it_of = [None] * self.n_streams
        done_of = [True] * self.n_streams     # the stream's sequence has no more frames
        nxt = 0

        def refill():
            nonlocal nxt
            for s in range(self.n_streams):
                if seq_of[s] is not None and done_of[s] and self.pending(s) == 0:
                    seq_of[s] = None
                    self.reset(s)
                if seq_of[s] is None and nxt < len(seqs):
                    seq_of[s], it_of[s], done_of[s] = nxt, iter(seqs[nxt]), False
                    if self.map_voxel is not None:
                        out[nxt].map = api.VoxelMap(self.camPyr, self.map_voxel, dense=self.map_dense,
                                                    max_voxels=self.map_max_voxels)
                        self.attach_map(s, out[nxt].map)
                        if self.surface is not None:
                            box = {k: v for k, v in self.surface.items() if k != "window"}
                            out[nxt].surface = api.SurfaceVolume(out[nxt].map, **box)
                            self.attach_surface(s, out[nxt].surface, self.surface_track, log=out[nxt], window=self.surface.get("window"))
                    nxt += 1

        def feed():  # one submit: the next frame of every stream with room in its queue
            frames = []
            for s in range(self.n_streams):
                if seq_of[s] is None or done_of[s] or self.pending(s) >= self.max_queue:
                    continue
                try:
                    f = next(it_of[s])
                except StopIteration:
                    done_of[s] = True
                    continue
                frames.append((s, f[0], f[1], f[2]))
            dev = [fr for fr in frames if hasattr(fr[1], "data_ptr")]
            host = [fr for fr in frames if not hasattr(fr[1], "data_ptr")]
            if host:
                self.submit(host)
            if dev:
                self.submit_device(dev)
            return len(frames)

        while True:
            refill()
            for _ in range(self.max_queue):
                if not feed():
                    break
            if not any(self.pending(s) > 0 for s in range(self.n_streams)):
                if nxt >= len(seqs) and all(q is None or done_of[s] for s, q in enumerate(seq_of)):
                    refill()
                    if all(q is None for q in seq_of):
                        break
                continue
            for s, M, kf, ts in self.step():
                r = out[seq_of[s]]
                r.append((M, kf))
                r.poses.append((ts, M))
                if self.pair_info:
                    r.pair_infos.append(self.last_pair_info(s))
        return out


def _quat_xyzw(R):
    """Eigen::Quaternionf(R) (system.cpp:78), returned as (x, y, z, w)."""
    R = np.asarray(R, np.float32)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, np.float32)  # w x y z
    if t > 0:
        t = np.sqrt(np.float32(t + 1.0))
        q[0] = 0.5 * t
        t = np.float32(0.5) / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(np.float32(R[i, i] - R[j, j] - R[k, k] + 1.0))
        q[1 + i] = 0.5 * t
        t = np.float32(0.5) / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q[1], q[2], q[3], q[0]
