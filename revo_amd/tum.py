"""TUM RGB-D dataset front-end (io/iowrapperRGBD.cpp:257-333) without OpenCV: 'associate.txt'
lines 'ts rgb_path ts depth_path', 8-bit RGB PNGs and 16-bit depth PNGs (metres = raw / 5000).
Decoding uses PIL; the u16 -> float conversion of iowrapperRGBD.cpp:326-327 is fused into the
device-side pyramid build (revo_pyramid_create_u16 / depth_scale_factor)."""
import os

import numpy as np


def read_associate(path, skip_first_n_frames=0, read_n_images=None):
    """-> list of (rgb_ts, rgb_file, depth_ts, depth_file); '#' comments and blank lines ignored."""
    out, n = [], 0
    for line in open(path):
        line = line.strip()
        if not line or line[0] == "#":
            continue
        n += 1
        if n <= skip_first_n_frames:
            continue
        p = line.split()
        if len(p) < 4:
            raise ValueError("bad associate line: %r" % line)
        out.append((float(p[0]), p[1], float(p[2]), p[3]))
        if read_n_images is not None and len(out) > read_n_images:  # `if (nFrames > READ_N_IMAGES) break;` after the
            break                                                      # push: N + 1 frames (iowrapperRGBD.cpp:291)
    return out


def load_frame(folder, rgb_file, depth_file):
    """-> (BGR8 [H,W,3], depth uint16 [H,W]) like cv::imread(rgb) / imread(depth, UNCHANGED)."""
    from PIL import Image
    rgb = np.asarray(Image.open(os.path.join(folder, rgb_file)).convert("RGB"), np.uint8)
    dimg = Image.open(os.path.join(folder, depth_file))
    depth = np.asarray(dimg)
    if depth.dtype != np.uint16:
        depth = depth.astype(np.uint16)
    return np.ascontiguousarray(rgb[..., ::-1]), np.ascontiguousarray(depth)


def frames(folder, associate="associate.txt", use_depth_timestamp=False, **kw):
    """Generator of (bgr, depth_u16, timestamp)."""
    for rts, rf, dts, df in read_associate(os.path.join(folder, associate), **kw):
        bgr, depth = load_frame(folder, rf, df)
        yield bgr, depth, (dts if use_depth_timestamp else rts)


def _decode_worker(shm_name, width, height, folder, tasks, done):
    """One decoder process of DecodePool: (frame index, ring slot, rgb file, depth file) -> pixels in the shared ring."""
    from multiprocessing import shared_memory
    shm = shared_memory.SharedMemory(name=shm_name)
    try:
        nb, nd = width * height * 3, width * height * 2
        while True:
            t = tasks.get()
            if t is None:
                break
            i, slot, rf, df = t
            if rf is None:  # warm(): "this decoder is up"
                done.put((i, None))
                continue
            try:
                bgr, depth = load_frame(folder, rf, df)
                if bgr.shape != (height, width, 3) or depth.shape != (height, width):
                    raise ValueError("frame %d is %s / %s, the ring holds %dx%d frames" % (i, bgr.shape, depth.shape, width, height))
                off = slot * (nb + nd)
                np.frombuffer(shm.buf, np.uint8, nb, off).reshape(height, width, 3)[...] = bgr
                np.frombuffer(shm.buf, np.uint16, width * height, off + nb).reshape(height, width)[...] = depth
                done.put((i, None))
            except BaseException as e:  # surfaced in the consumer
                done.put((i, "%s: %s" % (type(e).__name__, e)))
    finally:
        shm.close()


class DecodePool:
    """IOWrapperRGBD::readNextFrame (iowrapperRGBD.cpp:301-333) on several host cores, so that decoding keeps up with a device
    that tracks thousands of frames per second (one PIL decoder does ~200 640x480 pairs per second: VERDICT r05 missing 5).

    `workers` SPAWNED processes (the caller may hold an initialised HIP runtime) decode the PNG pairs of `entries`
    (read_associate rows) straight into a ring of frame slots in shared memory; the ring is registered with the HIP runtime as
    page-locked memory when a GPU is present (`pin`), so revo_vo_submit(_u16) lets the DMA engine read a slot in place --
    decode -> H2D with no host-side copy at all.  Iterating yields (bgr [H,W,3] u8, depth [H,W] u16, timestamp) IN ORDER; the
    arrays are views of the ring, valid until the NEXT frame is taken from the iterator (revo_vo_submit returns once the
    frame has been read, so the sequential driver satisfies this by construction).  Frames are bit-identical to `frames()`."""

    def __init__(self, folder, entries, width, height, workers=4, ring=None, use_depth_timestamp=False, pin=True):
        import multiprocessing as mp
        from multiprocessing import shared_memory
        self.folder, self.entries = folder, list(entries)
        self.w, self.h = int(width), int(height)
        self.workers = max(1, int(workers))
        self.ring = int(ring) if ring else 2 * self.workers + 2
        self.use_depth_timestamp = bool(use_depth_timestamp)
        self._slot_bytes = self.w * self.h * 5
        self._shm = shared_memory.SharedMemory(create=True, size=self.ring * self._slot_bytes)
        self._pinned = False
        if pin:
            try:
                import ctypes
                import torch
                if torch.cuda.is_available():
                    self._addr = ctypes.addressof(ctypes.c_char.from_buffer(self._shm.buf))
                    rc = torch.cuda.cudart().cudaHostRegister(self._addr, self.ring * self._slot_bytes, 0)
                    self._pinned = (int(rc) == 0)
            except Exception:  # no torch / no device: pageable slots still work (staging copy inside the library)
                self._pinned = False
        ctx = mp.get_context("spawn")
        self._tasks, self._done = ctx.Queue(), ctx.Queue()
        self._procs = [ctx.Process(target=_decode_worker, args=(self._shm.name, self.w, self.h, folder, self._tasks, self._done),
                                   daemon=True) for _ in range(self.workers)]
        for p in self._procs:
            p.start()
        self._closed = False

    @property
    def pinned(self):
        return self._pinned

    def warm(self, timeout=60.0):
        """Blocks until every decoder process has started (spawning a Python interpreter takes a few hundred milliseconds: a
        caller that times a short sequence calls this first; a long run simply amortises it)."""
        for k in range(self.workers):
            self._tasks.put((-1 - k, 0, None, None))
        for _ in range(self.workers):
            self._done.get(timeout=timeout)
        return self

    def _views(self, slot):
        nb = self.w * self.h * 3
        off = slot * self._slot_bytes
        return (np.frombuffer(self._shm.buf, np.uint8, nb, off).reshape(self.h, self.w, 3),
                np.frombuffer(self._shm.buf, np.uint16, self.w * self.h, off + nb).reshape(self.h, self.w))

    def __iter__(self):
        n = len(self.entries)
        issued, ready = 0, {}
        for i in range(n):
            # frame i's slot is the consumer's from now on; frames < i are consumed: slots of frames up to i + ring - 1 are free
            while issued < min(n, i + self.ring):
                rts, rf, dts, df = self.entries[issued]
                self._tasks.put((issued, issued % self.ring, rf, df))
                issued += 1
            while i not in ready:
                j, err = self._done.get()
                if err is not None:
                    raise RuntimeError("decoding frame %d failed: %s" % (j, err))
                ready[j] = True
            del ready[i]
            bgr, depth = self._views(i % self.ring)
            rts, rf, dts, df = self.entries[i]
            yield bgr, depth, (dts if self.use_depth_timestamp else rts)

    def close(self):
        if self._closed:
            return
        self._closed = True
        for _ in self._procs:
            self._tasks.put(None)
        for p in self._procs:
            p.join(5)
            if p.is_alive():
                p.terminate()
        if self._pinned:
            try:
                import torch
                torch.cuda.cudart().cudaHostUnregister(self._addr)
            except Exception:
                pass
        try:
            self._shm.close()
        except Exception:  # (a view of the ring is still alive somewhere: the mapping goes with it)
            pass
        try:
            self._shm.unlink()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuDecodeGroup:
    """Decodes the next `batch` frames of many GpuFrameSources in ONE launch of a png.GpuPngDecoder (one image decode is a
    serial inflate: throughput comes from many images per launch).  A launch covers every source that has taken its last
    decoded batch; it is issued as soon as all running sources have (so in a lockstep run it overlaps the tracking of the
    batch in use), or at once when a source needs a batch nobody asked for yet.  A reader thread loads the file bytes of
    each source's following batch while the current one decodes."""

    def __init__(self, width, height, batch=8, device=0, max_sources=1, decoder=None):
        from concurrent.futures import ThreadPoolExecutor
        from . import png
        import torch
        self.w, self.h, self.batch = int(width), int(height), max(1, int(batch))
        self.device = torch.device("cuda", device)
        self.max_sources = max(1, int(max_sources))
        self.max_images = 2 * self.batch * self.max_sources
        self.raw = png.raw_bytes(self.w, self.h, png.BGR8)
        self.decoder = decoder
        self._cap = 0
        self.stream = torch.cuda.Stream(self.device)
        self._reader = ThreadPoolExecutor(1)
        self._sources = []
        self._inflight = {}  # ticket -> [(source, files ...)]
        self.fallbacks = 0

    def _read(self, src, rows):
        out = []
        for rts, rf, dts, df in rows:
            with open(os.path.join(src.folder, rf), "rb") as f:
                a = f.read()
            with open(os.path.join(src.folder, df), "rb") as f:
                b = f.read()
            out.append((a, b))
        return out

    def _launch(self, srcs):
        from . import png
        jobs = []
        for src in srcs:
            rows, files = src._take_next_files()
            src._requested = True
            for k, (a, b) in enumerate(files):
                jobs.append((src, rows[k], k, a, b))
        if not jobs:
            return
        total = sum(len(a) + len(b) for _, _, _, a, b in jobs)
        if self.decoder is None or total > self._cap:
            for t in list(self._inflight):  # (a bigger decoder: the outstanding batches finish first)
                self._finish(t)
            if self.decoder is not None:
                self.decoder.close()
            self._cap = max(2 * total, 1 << 24)
            self.decoder = png.GpuPngDecoder(self.max_images, self._cap, self.raw, device=self.device.index)
        files, fmts, outs = [], [], []
        for src, row, k, a, b in jobs:
            bgr, depth = src._slot(src._fill_half, k)
            files += [a, b]
            fmts += [png.BGR8, png.U16]
            outs += [bgr, depth]
        t = self.decoder.submit(files, fmts, outs, self.stream)
        self._inflight[t] = jobs
        for src in srcs:
            src._ticket = t
            src._half_of[t] = src._fill_half

    def _finish(self, t):
        """Waits for a launch and decodes on the CPU what the device could not (uploaded into the same slots)."""
        import torch
        jobs = self._inflight.pop(t)
        codes = self.decoder.wait(t)
        for j, (src, row, k, a, b) in enumerate(jobs):
            if codes[2 * j] == 0 and codes[2 * j + 1] == 0:
                continue
            self.fallbacks += 1
            rts, rf, dts, df = row
            bgr, depth = load_frame(src.folder, rf, df)  # (a file PIL cannot read either fails here, as DecodePool does)
            if bgr.shape != (self.h, self.w, 3) or depth.shape != (self.h, self.w):
                raise ValueError("%s: frame is %s / %s, the source holds %dx%d frames" % (rf, bgr.shape, depth.shape, self.w, self.h))
            d_bgr, d_depth = src._slot(src._half_of[t], k)
            with torch.cuda.stream(self.stream):
                d_bgr.copy_(torch.from_numpy(bgr.copy()))
                d_depth.copy_(torch.from_numpy(depth.view(np.int16).copy()).view(torch.uint16))
            self.stream.synchronize()

    def need(self, src):
        """src has used up its batch: make sure its next one is (being) decoded and wait for it."""
        if not src._requested:
            self._launch([s for s in self._sources if s._wants()])
        t = src._ticket
        if t in self._inflight:
            self._finish(t)

    def maybe_prefetch(self):
        live = [s for s in self._sources if not s._exhausted_files()]
        if live and all(s._wants() for s in live):
            self._launch(live)

    def close(self):
        for t in list(self._inflight):
            try:
                self._finish(t)
            except Exception:
                pass
        self._reader.shutdown(wait=True)
        if self.decoder is not None:
            self.decoder.close()


class GpuFrameSource:
    """tum.frames() decoded on the GPU: yields (bgr [H,W,3] uint8, depth [H,W] uint16, timestamp) as device tensors, views
    of a double-buffered ring of 2 x `batch` frames (valid until the next frame is taken; vo.MultiREVO.submit_device copies
    them before that).  The frames of the next batch decode while this batch is tracked.  A file the device reports as
    UNSUPPORTED or CORRUPT is decoded by load_frame and uploaded instead.  `decoder` is a GpuDecodeGroup shared by the
    sources that run together (None: one of its own)."""

    def __init__(self, folder, rows, width, height, decoder=None, batch=8, use_depth_timestamp=False, device=0):
        import torch
        self.folder, self.rows = folder, list(rows)
        self.group = decoder if decoder is not None else GpuDecodeGroup(width, height, batch, device)
        self._own_group = decoder is None
        g = self.group
        self.use_depth_timestamp = bool(use_depth_timestamp)
        self._bgr = torch.empty((2, g.batch, g.h, g.w, 3), dtype=torch.uint8, device=g.device)
        self._depth = torch.empty((2, g.batch, g.h, g.w), dtype=torch.uint16, device=g.device)
        self._next_row = 0          # first row not yet handed to a launch
        self._fill_half = 0         # the half the next launch writes
        self._half_of = {}          # ticket -> half
        self._requested = False     # the next batch is launched (or there is none)
        self._ticket = None
        self._prefetch = None       # future: file bytes of rows[_next_row : _next_row + batch]
        g._sources.append(self)
        self._schedule_read()

    def _slot(self, half, k):
        return self._bgr[half, k], self._depth[half, k]

    def _schedule_read(self):
        rows = self.rows[self._next_row:self._next_row + self.group.batch]
        self._prefetch = (rows, self.group._reader.submit(self.group._read, self, rows)) if rows else None

    def _exhausted_files(self):
        return self._prefetch is None

    def _wants(self):
        return not self._requested and self._prefetch is not None

    def _take_next_files(self):
        rows, fut = self._prefetch
        files = fut.result()
        self._next_row += len(rows)
        self._schedule_read()
        return rows, files

    def __iter__(self):
        g = self.group
        try:
            i = 0
            while i < len(self.rows):
                g.need(self)
                t = self._ticket
                half = self._half_of.pop(t)
                n = min(g.batch, len(self.rows) - i)
                self._requested = False
                self._fill_half = 1 - half
                g.maybe_prefetch()
                for k in range(n):
                    rts, rf, dts, df = self.rows[i + k]
                    bgr, depth = self._slot(half, k)
                    yield bgr, depth, (dts if self.use_depth_timestamp else rts)
                i += n
        finally:
            if self in g._sources:
                g._sources.remove(self)
            if self._own_group:
                g.close()


def usable_cpus():
    """CPUs this process may really use: the affinity mask capped by the cgroup CPU quota (the GPU boxes expose 256 hardware
    threads and grant 16 CPUs: cpu.max = "1600000 100000")."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def default_decoders():
    """Decoder processes for a sequential run: HALF of the CPUs the process may really use (quota-aware), at most 12.  The other
    half is for the driver's own threads (IO thread + consumer loop, system.cpp:96 -- the consumer polls) and for head-room:
    measured on a 16-CPU-quota box (profiles/r06_decode_rates.txt), a pool of 8 decodes 690-820 frames/s, 12 about the same,
    and 16 LESS (420-700: the quota throttles everything, the driver's threads included -- with the tracker running next to
    16 decoders the stream fell to 215 frames/s)."""
    return max(1, min(12, usable_cpus() // 2))


def write_synthetic_dataset(folder, seq, depth_scale=5000.0):
    """Writes a TUM-layout dataset (rgb/*.png, depth/*.png, associate.txt, groundtruth.txt) from
    revo_amd.synth.make_sequence frames: the stand-in for fr1/desk where no data is on disk."""
    from PIL import Image
    os.makedirs(os.path.join(folder, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(folder, "depth"), exist_ok=True)
    with open(os.path.join(folder, "associate.txt"), "w") as fa, open(os.path.join(folder, "groundtruth.txt"), "w") as fg:
        fa.write("# rgb depth (synthetic)\n")
        for bgr, depth, ts, T in seq:
            name = "%.6f.png" % ts
            Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(os.path.join(folder, "rgb", name))
            raw = np.clip(np.rint(depth.astype(np.float64) * depth_scale), 0, 65535).astype(np.uint16)
            Image.fromarray(raw).save(os.path.join(folder, "depth", name))
            fa.write("%.6f rgb/%s %.6f depth/%s\n" % (ts, name, ts, name))
            t = T[:3, 3]
            fg.write("%.6f %.9f %.9f %.9f 0 0 0 1\n" % (ts, t[0], t[1], t[2]))


def read_poses(path):
    """A pose file as vo.tum_lines writes it ('ts tx ty tz qx qy qz qw' per line) -> [(timestamp, 4x4 float32 pose)]: the
    rotation of the normalised quaternion, formed in float64 and rounded once."""
    out = []
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        p = [float(x) for x in line.split()]
        x, y, z, w = np.asarray(p[4:8], np.float64) / np.linalg.norm(p[4:8])
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                              [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                              [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).astype(np.float32)
        T[:3, 3] = np.asarray(p[1:4], np.float32)
        out.append((p[0], T))
    return out


def write_views(folder, poses, render, depth_scale=5000.0, batch=16, what="the voxel map", normals=False):
    """Writes views rendered from `poses` [(timestamp, 4x4 camera -> world)] as a TUM-layout data set: rgb/<ts>.png (8-bit
    colour), depth/<ts>.png (16-bit: metres x depth_scale, rounded to nearest, saturated at 65535, 0 = nothing there),
    associate.txt, and poses.txt in the pose file's format (vo.tum_lines).  render(list of poses) -> (depth images, bgr images)
    or, with normals=True, (depth, bgr, normal images); the normals go to normals/<ts>.npy ([h, w, 3] float32).  The views are
    rendered from the poses as poses.txt states them (read_poses), so the folder describes itself: read_associate / load_frame /
    read_poses give back what was rendered.  -> number of views."""
    from PIL import Image
    from . import vo
    os.makedirs(os.path.join(folder, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(folder, "depth"), exist_ok=True)
    if normals:
        os.makedirs(os.path.join(folder, "normals"), exist_ok=True)
    pose_file = os.path.join(folder, "poses.txt")
    with open(pose_file, "w") as f:
        f.write("".join(line + "\n" for line in vo.tum_lines(poses)))
    poses = read_poses(pose_file)
    with open(os.path.join(folder, "associate.txt"), "w") as fa:
        fa.write("# rgb depth (views of %s at the poses of poses.txt)\n" % what)
        for i in range(0, len(poses), batch):
            part = poses[i:i + batch]
            out = render([T for _, T in part])
            for j, ((ts, _), d, c) in enumerate(zip(part, out[0], out[1])):
                name = "%.6f.png" % ts
                Image.fromarray(np.ascontiguousarray(c[..., ::-1])).save(os.path.join(folder, "rgb", name))
                raw = np.clip(np.rint(d.astype(np.float64) * depth_scale), 0, 65535).astype(np.uint16)
                Image.fromarray(raw).save(os.path.join(folder, "depth", name))
                if normals:
                    np.save(os.path.join(folder, "normals", "%.6f.npy" % ts), np.ascontiguousarray(out[2][j], np.float32))
                fa.write("%.6f rgb/%s %.6f depth/%s\n" % (ts, name, ts, name))
    return len(poses)


def write_map_views(folder, vmap, poses, depth_scale=5000.0, batch=16, splat_max=4, min_count=1, raycast=False):
    """Renders the voxel map `vmap` (api.VoxelMap.render, or with raycast=True api.VoxelMap.raycast: the ray march in place of
    the splat, no footprint and no holes; `batch` views per library call) from `poses` [(timestamp, 4x4 camera -> world)] and
    writes the TUM-layout data set of write_views.  -> number of views."""
    def render(Ts):
        if raycast:
            return vmap.raycast(Ts, min_count=min_count)[:2]
        return vmap.render(Ts, splat_max=splat_max, min_count=min_count)[:2]
    return write_views(folder, poses, render, depth_scale, batch)


def write_surface_views(folder, surface, poses, depth_scale=5000.0, batch=16, normals=False, **ray_kw):
    """Ray-casts a surface -- anything with TsdfVolume.raycast's call: an api.TsdfVolume, an api.SurfaceVolume -- from `poses`
    (revo_map_tsdf_raycast) and writes the TUM-layout data set of write_views; a pixel without colour is black.
    ray_kw: raycast's camera, size, zrange, step, min_weight, max_steps.  -> number of views."""
    def render(Ts):
        r = surface.raycast(Ts, normals=normals, colors=True, **ray_kw)
        bgr = r["bgr"] if r["bgr"] is not None else [np.zeros(d.shape + (3,), np.uint8) for d in r["depth"]]
        return r["depth"], bgr, r["normals"]
    return write_views(folder, poses, render, depth_scale, batch, what="the TSDF surface", normals=normals)


def write_surfaces_views(items, depth_scale=5000.0, calls=256, **ray_kw):
    """write_surface_views for many surfaces at once: items = [(folder, surface, poses), ...], every surface an api.SurfaceVolume.
    The views of all surfaces are ray-cast in batched calls (api.raycast_surfaces, DESIGN 34: `calls` views per call at most, the
    poses as each folder's poses.txt states them) and each folder is then written by write_views, so it holds the files
    write_surface_views writes for that surface alone.  All views are held in host memory until they are written.
    ray_kw: raycast_surfaces' step, min_weight, max_steps.  -> the number of views per item."""
    from . import api, vo
    items = [(folder, surface, list(poses)) for folder, surface, poses in items]
    stated = []
    for folder, _, poses in items:  # the poses as poses.txt will state them
        os.makedirs(folder, exist_ok=True)
        pose_file = os.path.join(folder, "poses.txt")
        with open(pose_file, "w") as f:
            f.write("".join(line + "\n" for line in vo.tum_lines(poses)))
        stated.append([T for _, T in read_poses(pose_file)])
    done = [([], []) for _ in items]  # per item: depth images, bgr images
    at = [0] * len(items)
    while any(a < len(p) for a, p in zip(at, stated)):
        entries, who, room = [], [], int(calls)
        for i, (p, a) in enumerate(zip(stated, at)):
            take = min(len(p) - a, room)
            if take > 0:
                entries.append((items[i][1], np.stack(p[a:a + take])))
                who.append(i)
                at[i] += take
                room -= take
        for i, r in zip(who, api.raycast_surfaces(entries, normals=False, colors=True, **ray_kw)):
            done[i][0].extend(r["depth"])
            done[i][1].extend(r["bgr"] if r["bgr"] is not None else [np.zeros(d.shape + (3,), np.uint8) for d in r["depth"]])
    return [write_views(folder, poses, lambda Ts, d=d: d, depth_scale, max(1, len(poses)), what="the TSDF surface")
            for (folder, _, poses), d in zip(items, done)]


def read_groundtruth_positions(path):
    out = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        p = line.split()
        out[round(float(p[0]), 6)] = np.array([float(p[1]), float(p[2]), float(p[3])])
    return out
