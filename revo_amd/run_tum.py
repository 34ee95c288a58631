"""`python -m revo_amd.run_tum <settings.yaml> <dataset.yaml>` -- the reference's command line
(main.cpp:22-47: REVO <settings.yaml> <dataset.yaml>) for TUM-layout datasets: runs the sequential
VO on one GPU and writes poses_<dataset>.txt in TUM format (system.cpp:48-49,76-80).

--streams N runs the YAML's Datasets list N at a time through one vo.MultiREVO handle (a finished dataset's stream takes the
next one) and writes the same poses_<dataset>.txt files; the PNG decoders are split among the datasets that run at once.
--gpu-decode (with --streams) decodes the PNGs on the GPU instead (tum.GpuFrameSource): same pose files.
--exact-sums runs the tracker in its exact-sums mode (api.CameraPyr.setExactSums): sequential or with --streams.
--map VOXEL fuses every keyframe into a world-frame voxel map of that edge (metres) on the GPU (api.VoxelMap; the settings'
DO_GENERATE_DENSE_PCL picks dense or edge clouds) and writes map_<dataset>.ply next to the pose file: sequential or with
--streams, the same file either way.
--map-save FILE (with --map) also writes the finished map's integer sums as a .rvm file (revo_amd/mapfile.py) that
api.VoxelMap.load continues and `python -m revo_amd.mapfile` merges; FILE with _<dataset> in front of its extension with
--streams or more than one dataset.
--map-views DIR (with --map) renders the finished map from the estimated pose of every keyframe, or with --map-views-every K
of every K-th tracked frame, on the GPU (api.VoxelMap.render) and writes a TUM-layout data set into DIR (tum.write_map_views:
rgb/, depth/, associate.txt, poses.txt); DIR/<dataset>/ with --streams or more than one dataset.
--map-views-raycast (with --map-views) writes those views with the ray march (api.VoxelMap.raycast) in place of the
splat: no footprint parameter, no holes.  The pose file does not depend on it.
--map-esdf FILE (with --map) writes the finished map's distance field (api.VoxelMap.distance_field) over the map's
bounds grown by --map-esdf-pad N cells (default 8) as a .npz (d2, lo, n, voxel): the file `python -m revo_amd.mapfile esdf`
writes from --map-save's .rvm; FILE with _<dataset> in front of its extension with --streams or more than one dataset.
--map-window N (with --map, sequential driver only) keeps only the last N keyframes in the map (api.MapWindow: each older
keyframe's voxel sums are subtracted again, exactly): map_<dataset>.ply, --map-save and --map-views then describe that windowed
map, and map_window_<dataset>.txt lists the keyframes it holds, oldest first: time stamp and the 16 entries of T_w_kf (row-major,
%.9g: float32 exactly).  The pose file does not depend on it.
--map-carve (with --map, sequential driver only) carves free space with every new keyframe before it is integrated (vo.REVO's
carve): voxels the keyframe's depth image looks through -- moved objects, people, mixed-depth points -- leave the
map.  --map-carve-margin M sets the margin in metres (default: the voxel edge), --map-carve-views K the views a voxel must be
free in (default 1; a keyframe is one view, so K > 1 carves nothing).  An error with --map-window and with --streams.  The pose
file does not depend on it.
--surface FILE.ply (with --map, sequential driver only) fuses every keyframe's depth and colour into a TSDF and a colour volume
while the sequence runs (vo.REVO's surface, api.SurfaceVolume) and writes the mesh with per-vertex normals and colours
at the end.  --surface-box I0 J0 K0 N0 N1 N2 is the box in voxel indices of the world frame (the first camera's frame), decided
before the run (default -128 -128 -32 256 256 256); surfaces outside it are not there, and the keyframes that confirm no cell of
it are counted on stderr.  --surface-trunc M: the truncation distance in metres (default 4 voxel edges); --surface-min-weight K:
the views a cell needs.  An error with --map-window (unless --surface-window bounds the surface too) and with --streams.  The pose
file does not depend on it.
--surface-window N (with --surface) keeps only the last N keyframes in the surface (api.SurfaceWindow): each older keyframe
is taken out of the volumes again, exactly, when it leaves the window, so the mesh written at the end is that of the last N keyframes.
With it --surface is allowed together with --map-window.  An error with --surface-follow and with --streams.
--surface-track (with --surface) tracks every keyframe against the surface as it stands before it is fused (vo.REVO's surface_track,
api.SurfaceVolume.track): a keyframe whose tracking converges is fused at the refined pose; surface_poses_<dataset>.txt
gets the poses the keyframes were fused at.  The trajectory in poses_<dataset>.txt is the tracker's, unchanged.
--surface-follow (with --surface) lets the box follow the camera (api.FollowingSurface): a box of --surface-follow-size
N0 N1 N2 cells (default 256 256 256) centred ahead of the camera and snapped to multiples of --surface-follow-step K cells (default
16); the cells that leave it are kept in a sparse store and come back when the camera returns.  The mesh written at the end is that
of the whole surface, store and box together; where that spans more than one volume holds (1024 cells on an axis, 2^27 cells) a
message says so and the store is written instead (--surface-store FILE.npz, default FILE.npz beside the mesh; `python -m
revo_amd.mapfile surface-assemble` cuts boxes out of it).  --surface-store FILE.npz writes the store in any case.  An error with
--surface-box and with --surface-views.  MultiREVO, an in-place shift and a pyramid of volumes are not part of it.
--streams-surface FILE.ply (with --streams and --map) gives every dataset of a multi-stream run its own surface on its map
(vo.MultiREVO's surface): the keyframes a step promotes are fused, all streams in one launch, into volumes of
--surface-box (the sequential default), with --surface-trunc and --surface-min-weight as --surface takes them; FILE_<dataset>.ply is
written per dataset, the sequential run's bytes.  --streams-surface-track tracks every keyframe against its stream's surface first,
all loops in lockstep, and writes surface_poses_<dataset>.txt as --surface-track does.  An error without --streams or --map.
--streams-surface-window N (with --streams-surface) keeps only the last N keyframes (1 .. 1024) in every dataset's surface
(vo.MultiREVO's surface window): the step keeps device copies of each fused keyframe's images and takes the oldest
keyframe out again, all streams in one batched unfuse and without a wait; the mesh written is that of the last N keyframes.
--streams-surface-views DIR (with --streams-surface) ray-casts every dataset's finished surface from the estimated pose of each of
its keyframes, or with --streams-surface-views-every K of every K-th tracked frame, all datasets in batched calls
(api.raycast_surfaces), and writes DIR/<dataset>/ in --surface-views' layout: the files the sequential
--surface --surface-views run of that dataset writes.
--surface-views DIR (with --surface) ray-casts the finished surface from the estimated pose of every keyframe, or with
--surface-views-every K of every K-th tracked frame, on the GPU (api.SurfaceVolume.raycast, DESIGN 28: depth and colour from the
sign change of the fused field, sub-voxel accurate and without holes) and writes the TUM-layout data set that --map-views writes
(tum.write_surface_views: rgb/, depth/, associate.txt, poses.txt) into DIR; DIR/<dataset>/ with more than one dataset.
--covariances writes cov_<dataset>.txt next to the pose file, one line per pose line in the same order: the frame's time stamp,
its keyframe's time stamp, the good-point count, sigma2 and the 21 upper-triangle entries (row-major) of the 6x6 covariance of the
relative pose frame -> keyframe (api.pair_covariance of the level-0 settings.PairInfo at the final pose; translation 0-2,
rotation 3-5); `nan` for sigma2 and the 21 entries where no covariance exists (a sequence's first frame, too few points, a rank-deficient
system).  Sequential or with --streams; the pose files do not depend on it."""
import os
import sys
import time

import numpy as np


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) < 2:
        print("usage: python -m revo_amd.run_tum <settings.yaml> <dataset.yaml> [device] [--save-model DIR] [--decoders N] "
              "[--streams N [--gpu-decode]] [--exact-sums] [--covariances] [--map VOXEL [--map-window N] [--map-save FILE] [--map-esdf FILE [--map-esdf-pad N]] [--map-views DIR [--map-views-every K] [--map-views-raycast]] [--map-carve [--map-carve-margin M] [--map-carve-views K]] [--surface FILE.ply [--surface-box I0 J0 K0 N0 N1 N2] [--surface-trunc M] [--surface-min-weight K] [--surface-views DIR [--surface-views-every K]] [--surface-track] [--surface-window N] [--surface-follow [--surface-follow-size N0 N1 N2] [--surface-follow-step K] [--surface-store FILE.npz]]] [--streams-surface FILE.ply [--streams-surface-track] [--streams-surface-window N] [--streams-surface-views DIR [--streams-surface-views-every K]] [--surface-box ...] [--surface-trunc M] [--surface-min-weight K]]]")
        return 2
    from . import api, config, ply, synth, tum, vo
    model_dir = None
    if "--save-model" in argv:  # MapDrawer::saveModel (MapDrawer.h:97-170): outputPcl.ply + outputKf.ply
        i = argv.index("--save-model")
        model_dir = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    decoders = None  # PNG decoder processes (tum.DecodePool); 0 = decode on the IO thread itself, like the reference
    if "--decoders" in argv:
        i = argv.index("--decoders")
        decoders = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    map_voxel = None  # api.VoxelMap edge in metres: map_<dataset>.ply
    if "--map" in argv:
        i = argv.index("--map")
        map_voxel = float(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
        if not (np.isfinite(map_voxel) and map_voxel > 0):
            print("--map needs a positive voxel edge in metres")
            return 2
    map_save = None  # the finished map's integer sums as a .rvm file (mapfile): it can be loaded, continued and merged
    if "--map-save" in argv:
        i = argv.index("--map-save")
        map_save = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
        if map_voxel is None:
            print("--map-save writes the voxel map: it needs --map VOXEL")
            return 2
    map_esdf, esdf_pad = None, None  # the finished map's distance field as a .npz (api.DistanceField.save)
    if "--map-esdf-pad" in argv:
        i = argv.index("--map-esdf-pad")
        esdf_pad = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
        if esdf_pad < 0:
            print("--map-esdf-pad needs a number of cells >= 0")
            return 2
    if "--map-esdf" in argv:
        i = argv.index("--map-esdf")
        map_esdf = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
        if map_voxel is None:
            print("--map-esdf writes the voxel map's distance field: it needs --map VOXEL")
            return 2
    elif esdf_pad is not None:
        print("--map-esdf-pad needs --map-esdf FILE")
        return 2
    esdf = None if map_esdf is None else (map_esdf, 8 if esdf_pad is None else esdf_pad)
    map_window = 0  # api.MapWindow: the map holds the last N keyframes only
    if "--map-window" in argv:
        i = argv.index("--map-window")
        map_window = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
        if map_window < 1:
            print("--map-window needs a positive number of keyframes")
            return 2
        if map_voxel is None:
            print("--map-window bounds the voxel map: it needs --map VOXEL")
            return 2
        if "--streams" in argv:
            print("--map-window is not supported together with --streams: the windowed map runs on the sequential driver only "
                  "(drop --streams)")
            return 2
    views_dir, views_every = None, 0  # tum.write_map_views of the finished map: every keyframe's pose, or every K-th frame's
    if "--map-views-every" in argv:
        i = argv.index("--map-views-every")
        views_every = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
        if views_every < 1:
            print("--map-views-every needs a positive number of frames")
            return 2
    views_raycast = "--map-views-raycast" in argv  # the views by api.VoxelMap.raycast in place of render
    if views_raycast:
        argv = [a for a in argv if a != "--map-views-raycast"]
    if "--map-views" in argv:
        i = argv.index("--map-views")
        views_dir = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if (views_dir is not None or views_every) and map_voxel is None:
        print("--map-views renders the voxel map: it needs --map VOXEL")
        return 2
    if views_every and views_dir is None:
        print("--map-views-every needs --map-views DIR")
        return 2
    if views_raycast and views_dir is None:
        print("--map-views-raycast needs --map-views DIR")
        return 2
    map_carve = None  # vo.REVO's carve: free-space carving with every new keyframe
    for opt, key, conv in (("--map-carve-margin", "margin", float), ("--map-carve-views", "min_views", int)):
        if opt in argv:
            i = argv.index(opt)
            try:
                map_carve = dict(map_carve or {}, **{key: conv(argv[i + 1])})
            except (IndexError, ValueError):
                print("%s needs a number: --map-carve-margin a margin >= 0 in metres, --map-carve-views a positive number of views" % opt)
                return 2
            argv = argv[:i] + argv[i + 2:]
    if "--map-carve" in argv:
        argv = [a for a in argv if a != "--map-carve"]
        map_carve = map_carve or {}
    elif map_carve is not None:
        print("--map-carve-margin and --map-carve-views need --map-carve")
        return 2
    if map_carve is not None:
        if map_voxel is None:
            print("--map-carve carves the voxel map: it needs --map VOXEL")
            return 2
        if map_window:
            print("--map-carve is not supported together with --map-window: the window's per-keyframe records must stay subtractable")
            return 2
        if "--streams" in argv:
            print("--map-carve is not supported together with --streams: carving runs on the sequential driver only (drop --streams)")
            return 2
        if not (np.isfinite(map_carve.get("margin", 0.0)) and map_carve.get("margin", 0.0) >= 0) or map_carve.get("min_views", 1) < 1:
            print("--map-carve-margin needs a margin >= 0 in metres, --map-carve-views a positive number of views")
            return 2
    sviews_dir, sviews_every = None, 0  # tum.write_surface_views of the finished surface: every keyframe's pose, or every K-th frame's
    if "--surface-views-every" in argv:
        i = argv.index("--surface-views-every")
        sviews_every = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
        if sviews_every < 1:
            print("--surface-views-every needs a positive number of frames")
            return 2
    if "--surface-views" in argv:
        i = argv.index("--surface-views")
        sviews_dir = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if sviews_every and sviews_dir is None:
        print("--surface-views-every needs --surface-views DIR")
        return 2
    if sviews_dir is not None and "--surface" not in argv:
        print("--surface-views ray-casts the TSDF surface: it needs --surface FILE.ply")
        return 2
    surface_track = "--surface-track" in argv  # vo.REVO's surface_track: every keyframe tracked against the surface before it is fused
    if surface_track:
        argv = [a for a in argv if a != "--surface-track"]
        if "--surface" not in argv:
            print("--surface-track tracks the keyframes against the TSDF surface: it needs --surface FILE.ply")
            return 2
    follow = None  # api.FollowingSurface instead of a fixed box: {"size": [n0, n1, n2], "step": k, "store": file or None}
    if "--surface-follow" in argv:
        argv = [a for a in argv if a != "--surface-follow"]
        follow = {}
        for other, why in (("--surface-box", "the box follows the camera, so there is no box to give (see --surface-follow-size)"),
                           ("--surface-views", "the views are cast from one volume, and a following surface is a box and a store")):
            if other in argv or (other == "--surface-views" and sviews_dir is not None):
                print("--surface-follow is not supported together with %s: %s" % (other, why))
                return 2
        if "--surface" not in argv:
            print("--surface-follow moves the TSDF surface's box: it needs --surface FILE.ply")
            return 2
    for opt, key, k, conv in (("--surface-follow-size", "size", 3, int), ("--surface-follow-step", "step", 1, int), ("--surface-store", "store", 1, str)):
        if opt in argv:
            i = argv.index(opt)
            try:
                got = [conv(x) for x in argv[i + 1:i + 1 + k]]
                if len(got) != k or (conv is int and min(got) < 1):
                    raise ValueError
            except ValueError:
                print("%s needs %s" % (opt, {"size": "three cell counts >= 1: N0 N1 N2", "step": "a number of cells >= 1", "store": "a file name"}[key]))
                return 2
            if follow is None:
                print("%s needs --surface-follow" % opt)
                return 2
            follow[key] = got[0] if k == 1 else got
            argv = argv[:i] + argv[i + 1 + k:]
    surface_window = 0  # api.SurfaceWindow: the surface holds the last N keyframes only
    if "--surface-window" in argv:
        i = argv.index("--surface-window")
        try:
            surface_window = int(argv[i + 1])
        except (IndexError, ValueError):
            surface_window = 0
        argv = argv[:i] + argv[i + 2:]
        if surface_window < 1:
            print("--surface-window needs a positive number of keyframes")
            return 2
        if "--surface" not in argv:
            print("--surface-window bounds the TSDF surface: it needs --surface FILE.ply")
            return 2
        if follow is not None:
            print("--surface-window is not supported together with --surface-follow: a following surface's cells may lie in its store, "
                  "where no view can be taken out of them")
            return 2
        if "--streams" in argv:
            print("--surface-window is not supported together with --streams: the windowed surface runs on the sequential driver only "
                  "(drop --streams)")
            return 2
    ssurface = None  # vo.MultiREVO's surfaces: one SurfaceVolume per dataset, its mesh written at the end of the run
    ssurface_track = "--streams-surface-track" in argv
    if ssurface_track:
        argv = [a for a in argv if a != "--streams-surface-track"]
        if "--streams-surface" not in argv:
            print("--streams-surface-track tracks the keyframes against their stream's TSDF surface: it needs --streams-surface FILE.ply")
            return 2
    ssurface_window = 0  # vo.MultiREVO's surface window: every dataset's surface holds its last N keyframes only
    if "--streams-surface-window" in argv:
        i = argv.index("--streams-surface-window")
        try:
            ssurface_window = int(argv[i + 1])
        except (IndexError, ValueError):
            ssurface_window = 0
        argv = argv[:i] + argv[i + 2:]
        if not 1 <= ssurface_window <= 1024:
            print("--streams-surface-window needs a number of keyframes, 1 .. 1024")
            return 2
        if "--streams-surface" not in argv:
            print("--streams-surface-window bounds every stream's TSDF surface: it needs --streams-surface FILE.ply")
            return 2
    ssviews_dir, ssviews_every = None, 0  # tum.write_surfaces_views of every dataset's finished surface
    if "--streams-surface-views-every" in argv:
        i = argv.index("--streams-surface-views-every")
        try:
            ssviews_every = int(argv[i + 1])
        except (IndexError, ValueError):
            ssviews_every = 0
        argv = argv[:i] + argv[i + 2:]
        if ssviews_every < 1:
            print("--streams-surface-views-every needs a positive number of frames")
            return 2
        if "--streams-surface-views" not in argv:
            print("--streams-surface-views-every needs --streams-surface-views DIR")
            return 2
    if "--streams-surface-views" in argv:
        i = argv.index("--streams-surface-views")
        if i + 1 >= len(argv) or argv[i + 1].startswith("--"):
            print("--streams-surface-views needs a folder name")
            return 2
        ssviews_dir = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
        if "--streams-surface" not in argv:
            print("--streams-surface-views ray-casts every stream's TSDF surface: it needs --streams-surface FILE.ply")
            return 2
    if "--streams-surface" in argv:
        i = argv.index("--streams-surface")
        if i + 1 >= len(argv) or argv[i + 1].startswith("--"):
            print("--streams-surface needs a file name")
            return 2
        ssurface = {"file": argv[i + 1]}
        if ssurface_window:
            ssurface["window"] = ssurface_window
        if ssviews_dir is not None:
            ssurface["views"], ssurface["views_every"] = ssviews_dir, ssviews_every
        argv = argv[:i] + argv[i + 2:]
        if "--streams" not in argv:
            print("--streams-surface gives every dataset of a multi-stream run its surface: it needs --streams N (the sequential driver has --surface)")
            return 2
        if map_voxel is None:
            print("--streams-surface fuses the keyframes over each dataset's voxel map: it needs --map VOXEL")
            return 2
    surface = None  # vo.REVO's surface: the coloured, shaded mesh of the keyframes' TSDF volume, written at the end of the run
    for opt, key, k, conv in (("--surface", "file", 1, str), ("--surface-box", "box", 6, int), ("--surface-trunc", "trunc", 1, float),
                              ("--surface-min-weight", "min_weight", 1, int)):
        if opt in argv:
            i = argv.index(opt)
            try:
                got = [conv(x) for x in argv[i + 1:i + 1 + k]]
                if len(got) != k:
                    raise ValueError
            except ValueError:
                print("%s needs %s" % (opt, {"file": "a file name", "box": "six integers: I0 J0 K0 N0 N1 N2", "trunc": "a distance in metres",
                                             "min_weight": "a number of views"}[key]))
                return 2
            surface = dict(surface or {}, **{key: got[0] if k == 1 else got})
            argv = argv[:i] + argv[i + 1 + k:]
    if ssurface is not None and surface is not None and "file" not in surface:  # the box, trunc and min-weight of --streams-surface
        if any(x < 1 for x in surface.get("box", (0, 0, 0, 1, 1, 1))[3:]) or not surface.get("trunc", 1.0) > 0 or surface.get("min_weight", 1) < 0:
            print("--surface-box needs N0 N1 N2 >= 1, --surface-trunc a distance > 0 in metres, --surface-min-weight a number >= 0")
            return 2
        ssurface.update(surface)
        surface = None
    if surface is not None:
        if "file" not in surface:
            print("--surface-box, --surface-trunc and --surface-min-weight need --surface FILE.ply")
            return 2
        if map_voxel is None:
            print("--surface fuses the keyframes over the voxel map's frame: it needs --map VOXEL")
            return 2
        if map_window and not surface_window:
            print("--surface is not supported together with --map-window: the volumes keep what the window evicts")
            return 2
        if "--streams" in argv:
            print("--surface is not supported together with --streams: the surface runs on the sequential driver only (drop --streams)")
            return 2
        if any(x < 1 for x in surface.get("box", (0, 0, 0, 1, 1, 1))[3:]) or not surface.get("trunc", 1.0) > 0 or surface.get("min_weight", 1) < 0:
            print("--surface-box needs N0 N1 N2 >= 1, --surface-trunc a distance > 0 in metres, --surface-min-weight a number >= 0")
            return 2
    exact_sums = "--exact-sums" in argv  # the tracker's exact-sums mode (both drivers)
    if exact_sums:
        argv = [a for a in argv if a != "--exact-sums"]
    covariances = "--covariances" in argv  # cov_<dataset>.txt: the covariance of every reported relative pose
    if covariances:
        argv = [a for a in argv if a != "--covariances"]
    gpu_decode = "--gpu-decode" in argv  # PNG decoding on the GPU (multi-stream driver only)
    if gpu_decode:
        argv = [a for a in argv if a != "--gpu-decode"]
    streams = 0  # > 0: the Datasets list N at a time through one multi-stream handle
    if "--streams" in argv:
        i = argv.index("--streams")
        streams = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
        if streams < 1:
            print("--streams needs a positive number of streams")
            return 2
        if model_dir is not None:
            print("--save-model is not supported together with --streams: the model export runs on the sequential driver only "
                  "(drop --streams to export the model)")
            return 2
    if gpu_decode and not streams:
        print("--gpu-decode is supported together with --streams only: the GPU decoder feeds the multi-stream driver "
              "(use --streams 1 for a single dataset)")
        return 2
    if gpu_decode and decoders is not None:
        print("--decoders has no effect with --gpu-decode: the PNGs are decoded on the GPU")
    from .settings import OptimizerSettings
    trk_settings, use_edge_filter, sysd = config.load_settings_yaml(argv[0])
    pyr_settings, io = config.load_dataset_yaml(argv[1])
    device = int(argv[2]) if len(argv) > 2 else 0
    trk_settings.optimizerSettings = OptimizerSettings(use_edge_filter=use_edge_filter)
    if streams:
        return _run_streams(streams, pyr_settings, trk_settings, io, sysd, device, decoders, gpu_decode, exact_sums, map_voxel,
                            views_dir, views_every, map_save, covariances, views_raycast, esdf, ssurface, ssurface_track)
    for ds in io["datasets"]:
        folder = os.path.join(io["main_folder"], ds)
        cam = api.CameraPyr(pyr_settings, device=device, exact_sums=exact_sums)
        drawer = ply.ModelExporter() if model_dir else None
        vmap = api.VoxelMap(cam, map_voxel, dense=bool(sysd["do_generate_dense_pcl"])) if map_voxel else None
        if map_window:
            vmap = api.MapWindow(cam, map_voxel, dense=bool(sysd["do_generate_dense_pcl"]), window=map_window)
        surf = None
        if surface is not None:
            if follow is not None:  # the box goes with the camera; what leaves it is kept in surf.store
                surf = api.FollowingSurface(vmap, follow.get("size", (256, 256, 256)), surface.get("trunc"), color=True, step=follow.get("step", 16))
            else:  # the box is decided here and does not move: voxel indices of the first camera's frame
                box = surface.get("box", (-128, -128, -32, 256, 256, 256))
                if surface_window:
                    surf = api.SurfaceWindow(vmap, box[:3], box[3:], window=surface_window, trunc=surface.get("trunc"), color=True)
                else:
                    surf = api.SurfaceVolume(vmap, box[:3], box[3:], surface.get("trunc"), color=True)
        drv = vo.REVO(pyr_settings, trk_settings, cameraPyr=cam, depth_scale_factor=io["depth_scale_factor"],
                      mapDrawer=drawer, generate_dense_pcl=sysd["do_generate_dense_pcl"], voxelMap=vmap, pair_info=covariances, carve=map_carve,
                      surface=surf, surface_track=surface_track or None)
        nd = tum.default_decoders() if decoders is None else decoders
        rows = tum.read_associate(os.path.join(folder, io["associate"]), skip_first_n_frames=io["skip_first_n_frames"],
                                  read_n_images=io["read_n_images"])
        t0 = time.perf_counter()
        if nd >= 1:
            # iowrapperRGBD.cpp:301-333 on `nd` cores: the decoders fill a page-locked ring the IO thread submits from in place
            with tum.DecodePool(folder, rows, pyr_settings.width, pyr_settings.height, workers=nd,
                                use_depth_timestamp=bool(io["use_depth_timestamp"])) as pool:
                res = drv.run(pool)
        else:
            res = drv.run(tum.frames(folder, io["associate"], bool(io["use_depth_timestamp"]),
                                     skip_first_n_frames=io["skip_first_n_frames"], read_n_images=io["read_n_images"]))
        dt = time.perf_counter() - t0
        name = os.path.basename(os.path.normpath(ds)) or "dataset"
        if sysd["do_output_poses"]:
            with open("poses_%s.txt" % name, "w") as f:
                f.write("\n".join(drv.tum_lines()) + "\n")
        if covariances:
            _save_covariances(name, drv.poses, drv.pair_infos)
        print("-----VO Report-----\nFrames Tracked: %d\nKeyframes Tracked: %d\nframes/s (incl. PNG decode, %s): %.1f"
              % (len(res), drv.nKeyFrames, ("%d decoder processes" % nd) if nd >= 1 else "decoded on the IO thread", len(res) / dt))
        if vmap is not None:
            _save_map(vmap, name, _rvm_path(map_save, name, len(io["datasets"]) > 1))
            _save_esdf(vmap, esdf, name, len(io["datasets"]) > 1)
            if map_carve is not None:
                done = [c[2] for c in drv.carves if c[2] is not None]
                print("Map carve: %d voxels (%d points) carved by %d keyframes%s"
                      % (sum(i["voxels_carved"] for i in done), sum(i["points_carved"] for i in done), len(done),
                         (" -- %d keyframes carved NOTHING: their pose's rotation had drifted past the orthogonality rule"
                          % drv.carve_skipped) if drv.carve_skipped else ""))
            if surf is not None:
                if follow is not None:
                    _save_following_surface(surf, drv, surface, follow, name, len(io["datasets"]) > 1)
                else:
                    _save_surface(surf, drv, surface, name, len(io["datasets"]) > 1)
                if surface_track:
                    _save_surface_tracks(drv, name)
                if sviews_dir is not None:
                    _save_surface_views(surf, os.path.join(sviews_dir, name) if len(io["datasets"]) > 1 else sviews_dir, drv.poses,
                                        [kf for _, kf in res], sviews_every, io["depth_scale_factor"], surface.get("min_weight", 1))
            if map_window:
                with open("map_window_%s.txt" % name, "w") as f:
                    for ts, T in zip(vmap.timestamps, vmap.keyframes):
                        f.write("%.9f %s\n" % (ts, " ".join("%.9g" % x for x in T.reshape(16))))
                print("Map window: the last %d of %d keyframes -> map_window_%s.txt" % (len(vmap.keyframes), drv.nKeyFrames, name))
            if views_dir is not None:
                _save_views(vmap, os.path.join(views_dir, name) if len(io["datasets"]) > 1 else views_dir,
                            drv.poses, [kf for _, kf in res], views_every, io["depth_scale_factor"], views_raycast)
        if drawer is not None:
            out = drawer.saveModel(os.path.join(model_dir, name) if len(io["datasets"]) > 1 else model_dir)
            print("model: %d points of %d keyframes -> %s, %s" % (drawer.nPts, len(drawer.vpKfsF), out[0], out[1]))
        _report_ate(folder, drv.poses)
    return 0


def _save_surface(surf, drv, surface, name, per_dataset):
    """--surface FILE.ply: the mesh of the run's volumes with normals and colours (FILE with _<dataset> in front of its extension
    when there are several data sets)."""
    import sys
    mesh = surf.mesh(surface.get("min_weight", 1), normals=True, colors=True)
    out = _rvm_path(surface["file"], name, per_dataset)
    mesh.save_ply(out)
    print("Surface: %d vertices, %d triangles from %d keyframes over the box %s + %s -> %s"
          % (len(mesh.vertices), len(mesh.triangles), surf.views, surf.lo.tolist(), surf.n.tolist(), out))
    blind = sum(1 for c in surf.view_counts() if c["confirmed"] == 0)
    if blind or drv.surface_skipped:
        print("Surface: %d of %d keyframes confirmed no cell of the box (their surfaces lie outside it); %d were not fused for their pose's rotation"
              % (blind, surf.views, drv.surface_skipped), file=sys.stderr)


def _save_following_surface(surf, drv, surface, follow, name, per_dataset):
    """--surface-follow: the mesh of the whole surface (store and box), or a message and the store when it does not fit one volume;
    --surface-store: the store as well, what the box holds at the end included."""
    import sys
    from . import mapfile
    out = _rvm_path(surface["file"], name, per_dataset)
    store_out = _rvm_path(follow["store"], name, per_dataset) if follow.get("store") else None
    try:
        mesh = surf.mesh(surface.get("min_weight", 1), normals=True, colors=True)
        mesh.save_ply(out)
        print("Surface: %d vertices, %d triangles from %d keyframes; the box %s + %s moved %d times, %d cells in the store -> %s"
              % (len(mesh.vertices), len(mesh.triangles), surf.views, surf.lo.tolist(), surf.n.tolist(), surf.shifts, len(surf.store), out))
    except ValueError as e:
        store_out = store_out or os.path.splitext(out)[0] + ".npz"
        print("Surface: no mesh written -- %s" % e, file=sys.stderr)
    if store_out is not None:
        whole = mapfile.SurfaceStore(surf.store.records, surf.store.voxel, surf.store.trunc)
        cur = surf.volume()
        whole.add(mapfile.tsdf_volume_records(cur.cells, cur.color, cur.lo))
        whole.save(store_out)
        print("Surface store: %d cells -> %s (python -m revo_amd.mapfile surface-assemble cuts volumes out of it)" % (len(whole), store_out))
    if drv.surface_skipped:
        print("Surface: %d keyframes were not fused for their pose's rotation" % drv.surface_skipped, file=sys.stderr)


def _save_surface_tracks(drv, name):
    """--surface-track: surface_poses_<dataset>.txt beside the pose file -- every keyframe's pose as it was fused into the surface, in
    the pose file's format, behind one comment line per keyframe with its matched pixels and the tracking's status."""
    from . import vo
    names = ("converged", "iteration_limit", "lost")
    with open("surface_poses_%s.txt" % name, "w") as f:
        f.write("# timestamp matched considered status (lost, iteration_limit: fused at the tracker's pose)\n")
        for ts, _, _, info, status in drv.surface_tracks:
            f.write("# %.6f %d %d %s\n" % (ts, info.matched if info is not None else 0, info.considered if info is not None else 0, names[status]))
        f.write("".join(line + "\n" for line in vo.tum_lines([(ts, T) for ts, _, T, _, _ in drv.surface_tracks])))
    print("Surface track: %d of %d keyframes refined against the surface -> surface_poses_%s.txt"
          % (sum(1 for t in drv.surface_tracks if t[4] == 0), len(drv.surface_tracks), name))


def _rvm_path(map_save, name, per_dataset):
    """--map-save FILE: FILE itself for one sequential dataset, else FILE with _<dataset> in front of its extension."""
    if map_save is None or not per_dataset:
        return map_save
    stem, ext = os.path.splitext(map_save)
    return "%s_%s%s" % (stem, name, ext)


def covariance_lines(poses, pair_infos):
    """One line per pose: 'ts kf_ts good sigma2 c00 c01 .. c55' (21 upper-triangle entries, row-major), %.9e; `nan` for sigma2
    and the 21 entries where api.pair_covariance refuses the record."""
    from . import api
    out = []
    iu = np.triu_indices(6)
    for (ts, _), (info, kf_ts) in zip(poses, pair_infos):
        try:
            cov, s2 = api.pair_covariance(info)
            nums = ["%d" % info.good, "%.9e" % s2] + ["%.9e" % c for c in cov[iu]]
        except api.RevoError:
            nums = ["%d" % info.good] + ["nan"] * 22
        out.append("%.9f %.9f " % (ts, kf_ts) + " ".join(nums))
    return out


def _save_covariances(name, poses, pair_infos):
    lines = covariance_lines(poses, pair_infos)
    with open("cov_%s.txt" % name, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("Covariances: %d lines (%d without a covariance) -> cov_%s.txt" % (len(lines), sum("nan" in ln for ln in lines), name))


def _save_map(vmap, name, rvm=None):
    info = vmap.info()
    path = vmap.save_ply("map_%s.ply" % name)
    if rvm is not None:
        print("Map file: %s" % vmap.save(rvm))
    print("Map: %d voxels of %g m from %d keyframes, %d points fused, %d points dropped (outside +-2048 m or the key range)%s -> %s"
          % (info["voxels"], vmap.voxel, info["keyframes"], info["points_integrated"], info["points_dropped"],
             (", %d keyframes refused (max_voxels)" % info["keyframes_rejected"]) if info["keyframes_rejected"] else "", path))


def _save_esdf(vmap, esdf, name, per_dataset):
    """--map-esdf FILE: the finished map's distance field over its bounds grown by the pad."""
    if esdf is None:
        return
    f = vmap.distance_field(pad=esdf[1])
    path = f.save(_rvm_path(esdf[0], name, per_dataset))
    print("Map distance field: %d x %d x %d cells from %s, largest d2 %d -> %s" % (tuple(f.n) + (f.lo.tolist(), f.info["max_d2"], path)))


def _save_views(vmap, folder, poses, is_kf, every, depth_scale, raycast=False):
    """--map-views: the finished map from the pose of every keyframe (every == 0) or of every `every`-th tracked frame."""
    from . import tum
    sel = poses[::every] if every else [p for p, kf in zip(poses, is_kf) if kf]
    n = tum.write_map_views(folder, vmap, sel, depth_scale=depth_scale, raycast=raycast)
    print("Map views: %d views (%s%s) -> %s" % (n, ("every %d frames" % every) if every else "one per keyframe", ", ray-cast" if raycast else "", folder))


def _save_surface_views(surf, folder, poses, is_kf, every, depth_scale, min_weight):
    """--surface-views: the finished surface from the pose of every keyframe (every == 0) or of every `every`-th tracked frame."""
    from . import tum
    sel = poses[::every] if every else [p for p, kf in zip(poses, is_kf) if kf]
    n = tum.write_surface_views(folder, surf, sel, depth_scale=depth_scale, min_weight=min_weight)
    print("Surface views: %d views (%s) -> %s" % (n, ("every %d frames" % every) if every else "one per keyframe", folder))


def _report_ate(folder, poses):
    gt_file = os.path.join(folder, "groundtruth.txt")  # positions only: ATE (the RPE evaluator needs full poses)
    if os.path.exists(gt_file):
        from . import synth, tum
        gt = tum.read_groundtruth_positions(gt_file)
        est, ref = [], []
        for ts, M in poses:
            if round(ts, 6) in gt:
                est.append(M)
                G = np.eye(4)
                G[:3, 3] = gt[round(ts, 6)]
                ref.append(G)
        if len(est) > 2:
            print("ATE RMSE vs groundtruth.txt: %.4f m over %d poses" % (synth.ate_rmse(est, ref), len(est)))


def _run_streams(streams, pyr_settings, trk_settings, io, sysd, device, decoders, gpu_decode=False, exact_sums=False,
                 map_voxel=None, views_dir=None, views_every=0, map_save=None, covariances=False, views_raycast=False, esdf=None,
                 ssurface=None, ssurface_track=False):
    """The Datasets list `streams` at a time through one vo.MultiREVO: same poses_<dataset>.txt files as the sequential loop.
    ssurface (--streams-surface): every dataset gets a surface on its map, the sequential --surface's box, trunc and files."""
    from . import tum, vo
    names = [os.path.basename(os.path.normpath(ds)) or "dataset" for ds in io["datasets"]]
    folders = [os.path.join(io["main_folder"], ds) for ds in io["datasets"]]
    nd = tum.default_decoders() if decoders is None else decoders
    per = max(1, nd // max(1, min(streams, len(folders)))) if nd >= 1 else 0  # decoders of one running dataset

    group = tum.GpuDecodeGroup(pyr_settings.width, pyr_settings.height, batch=8, device=device,
                               max_sources=min(streams, len(folders))) if gpu_decode else None

    def frames(folder):  # opened when the dataset's stream first asks for a frame, closed when it has none left
        if group is not None:
            rows = tum.read_associate(os.path.join(folder, io["associate"]), skip_first_n_frames=io["skip_first_n_frames"],
                                      read_n_images=io["read_n_images"])
            for f in tum.GpuFrameSource(folder, rows, pyr_settings.width, pyr_settings.height, group,
                                        use_depth_timestamp=bool(io["use_depth_timestamp"])):
                yield f
        elif per >= 1:
            rows = tum.read_associate(os.path.join(folder, io["associate"]), skip_first_n_frames=io["skip_first_n_frames"],
                                      read_n_images=io["read_n_images"])
            with tum.DecodePool(folder, rows, pyr_settings.width, pyr_settings.height, workers=per,
                                use_depth_timestamp=bool(io["use_depth_timestamp"])) as pool:
                for f in pool:
                    yield f
        else:
            for f in tum.frames(folder, io["associate"], bool(io["use_depth_timestamp"]),
                                skip_first_n_frames=io["skip_first_n_frames"], read_n_images=io["read_n_images"]):
                yield f

    surface = None
    if ssurface is not None:  # the box is decided here and does not move: voxel indices of each dataset's first camera frame
        box = ssurface.get("box", (-128, -128, -32, 256, 256, 256))
        surface = dict(lo=box[:3], n=box[3:], trunc=ssurface.get("trunc"), color=True)
        if ssurface.get("window"):
            surface["window"] = ssurface["window"]
    drv = vo.MultiREVO(pyr_settings, streams, trk_settings, device=device, depth_scale_factor=io["depth_scale_factor"],
                       exact_sums=exact_sums, map_voxel=map_voxel, map_dense=bool(sysd["do_generate_dense_pcl"]),
                       pair_info=covariances, surface=surface, surface_track=True if ssurface_track else None)
    t0 = time.perf_counter()
    try:
        res = drv.run([frames(f) for f in folders])
    finally:
        if group is not None:
            group.close()
    dt = time.perf_counter() - t0
    total = 0
    if ssurface is not None and ssurface.get("views") is not None:  # --streams-surface-views: all datasets' views in batched calls
        every = ssurface["views_every"]
        sel = [r.poses[::every] if every else [p for p, (_, kf) in zip(r.poses, r) if kf] for r in res]
        counts = tum.write_surfaces_views([(os.path.join(ssurface["views"], name), r.surface, p) for name, r, p in zip(names, res, sel)],
                                          depth_scale=io["depth_scale_factor"], min_weight=ssurface.get("min_weight", 1))
        for name, n in zip(names, counts):
            print("Surface views: %d views (%s) -> %s" % (n, ("every %d frames" % every) if every else "one per keyframe",
                                                          os.path.join(ssurface["views"], name)))
    for name, folder, r in zip(names, folders, res):
        if sysd["do_output_poses"]:
            with open("poses_%s.txt" % name, "w") as f:
                f.write("\n".join(r.tum_lines()) + "\n")
        if covariances:
            _save_covariances(name, r.poses, r.pair_infos)
        total += len(r)
        print("-----VO Report (%s)-----\nFrames Tracked: %d\nKeyframes Tracked: %d" % (name, len(r), sum(1 for _, kf in r if kf)))
        if r.map is not None:
            _save_map(r.map, name, _rvm_path(map_save, name, True))
            _save_esdf(r.map, esdf, name, True)
            if r.surface is not None:
                _save_surface(r.surface, r, ssurface, name, True)
                if ssurface.get("window"):
                    print("surface window: %d keyframes held, %d evicted (%d refused and left in the volumes)"
                          % (r.surface.views, r.surface_evictions, r.surface_evictions_refused))
                if ssurface_track:
                    _save_surface_tracks(r, name)
            if views_dir is not None:
                _save_views(r.map, os.path.join(views_dir, name), r.poses, [kf for _, kf in r], views_every,
                            io["depth_scale_factor"], views_raycast)
        _report_ate(folder, r.poses)
    print("%d datasets on %d streams: %.1f frames/s (incl. PNG decode, %s)"
          % (len(folders), streams, total / dt,
             ("decoded on the GPU, %d frames on the CPU fallback" % group.fallbacks) if group is not None else
             ("%d decoder processes per dataset" % per) if per else "decoded on this thread"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
