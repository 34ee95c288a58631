"""The voxel map as data: raw voxel records and the .rvm file (include/revo_hip.h revo_map_voxel_raw).

Pure numpy: nothing here needs the GPU or the HIP library, so maps can be inspected, merged and converted anywhere.

A record is one voxel's integer sums, 64 bytes little-endian: key (u64, (kx + 2^20) << 42 | (ky + 2^20) << 21 | (kz + 2^20),
bit 63 clear), count (u64, >= 1), sum_q (3 x i64: x, y, z in 2^-20 m), sum_bgr (3 x u64: B, G, R).

A .rvm file is a 64-byte header -- magic "REVOMAP1", u32 version 1, f32 voxel, i32 dense, u32 zero, u64 voxels,
u64 points_integrated, u64 points_dropped, u64 keyframes, zero padding -- followed by `voxels` records in ascending key order.
Equal maps give equal files.

    python -m revo_amd.mapfile info FILE...            what each file holds
    python -m revo_amd.mapfile merge OUT FILE...       the union of the files' maps (same voxel edge), without a GPU
    python -m revo_amd.mapfile subtract A B -o OUT      map A without map B's sums: undoes `merge A OUT B`, without a GPU
    python -m revo_amd.mapfile coarsen A SHIFT -o OUT   map A with a voxel edge 2^SHIFT times as long (revo_map_coarsen), without a GPU
    python -m revo_amd.mapfile transform A POSE.txt -o OUT [--voxel V] [--min-count N]
                                                        map A seen under a pose (revo_map_pose_raw), without a GPU:
                                                        POSE.txt holds 16 or 12 numbers, a row-major 4x4 or 3x4, A's frame -> OUT's
    python -m revo_amd.mapfile carve A --views DIR -o OUT [--removed R] [--radius N] [--margin M] [--margin-rel F] [--min-views K]
                                                        [--min-count N] [--max-count N] [--camera FX FY CX CY] [--zrange ZMIN ZMAX]
                                                        [--depth-scale S]
                                                        map A without the voxels the views of DIR look through (revo_map_carve,
                                                        DESIGN 19), without a GPU: DIR is a `run_tum --map-views` folder (depth/,
                                                        associate.txt, poses.txt); R gets the removed voxels, so that
                                                        `merge X OUT R` holds A's voxels again
    python -m revo_amd.mapfile esdf A -o OUT.npz [--pad N] [--min-count N] [--clamp D2]
                                                        map A's distance field (revo_map_distance_field), without a GPU:
                                                        the squared distance in cells to the nearest voxel, over the map's bounds
                                                        grown by N cells (default 8); OUT.npz holds d2, lo, n, voxel
    python -m revo_amd.mapfile observe A --views DIR -o SEEN.npz [--pad N] [--radius N] [--margin M] [--margin-rel F]
                                                        [--camera FX FY CX CY] [--zrange ZMIN ZMAX] [--depth-scale S]
                                                        what the views of DIR have looked at (revo_map_observe), without
                                                        a GPU: one byte per cell of A's bounds grown by N cells (default 0), free
                                                        votes and the surface bit; SEEN.npz holds seen, lo, n, voxel
    python -m revo_amd.mapfile frontiers A --seen SEEN.npz -o CELLS.txt [--min-count N] [--min-views K]
                                                        the free cells next to unseen space (revo_map_frontiers), one voxel index
                                                        per line; `esdf` and `plan` take --seen SEEN.npz [--min-views K] too: the
                                                        field then treats unseen space as an obstacle (revo_map_known_field)
    python -m revo_amd.mapfile gain A --seen SEEN.npz --poses POSES.txt --camera FX FY CX CY --size W H [--zrange ZMIN ZMAX]
                                                        [--radius N] [--margin M] [--margin-rel F] [--min-views K] [--min-count N]
                                                        [--miss-depth D] [--max-steps N] -o GAIN.txt
                                                        what a view from each pose of POSES.txt (one row-major 4x4 or 3x4 per line)
                                                        would add to SEEN.npz (revo_map_view_gain), without a GPU: per
                                                        pose the unknown cells it would see free, on a surface, inside the view,
                                                        and the hit pixels of the predicted depth image
    python -m revo_amd.mapfile next-view A --seen SEEN.npz --start X Y Z --clearance M --camera FX FY CX CY --size W H
                                                        [--headings N] [--stride N] [--max-candidates N] [--weight W] [--up X Y Z]
                                                        [the options of gain] -o POSE.txt
                                                        the reachable pose that would reveal most per metre of the way there
    python -m revo_amd.mapfile tsdf A --views DIR [--color] [--trunc M] [--pad N] -o TSDF.npz
                                                        [--camera FX FY CX CY] [--zrange ZMIN ZMAX] [--depth-scale S]
                                                        the views of DIR fused into a truncated signed distance volume over A's
                                                        bounds grown by N cells (revo_map_tsdf_fuse), without a GPU;
                                                        TSDF.npz holds sum, weight, lo, n, voxel, trunc
    python -m revo_amd.mapfile tsdf-unfuse TSDF.npz --views DIR [--only I,J,...] -o OUT.npz
                                                        [--camera FX FY CX CY] [--zrange ZMIN ZMAX] [--depth-scale S]
                                                        views of DIR (all, or those with the indices I, J, ...) taken out of
                                                        the volume again (revo_map_tsdf_unfuse), without a GPU: all or
                                                        nothing; a volume with colour takes DIR's rgb/ images too
    python -m revo_amd.mapfile mesh TSDF.npz [--min-weight K] [--normals] [--colors] -o MESH.ply
                                                        the mesh of the volume's zero level set (revo_map_tsdf_mesh), binary PLY
    python -m revo_amd.mapfile df-align DST SRC [--init POSE.txt] [--max-dist M] [--pad N] -o POSE.txt
                                                        map SRC's points registered against map DST's distance field
                                                        (revo_map_df_align), without a GPU: the pose SRC's frame ->
                                                        DST's as a row-major 4x4; M in metres (default 8 voxels), N the cells the
                                                        field reaches beyond DST's bounds (default ceil(M / voxel) + 2)
    python -m revo_amd.mapfile ply FILE [OUT.ply]      one coloured point per voxel, as map_<dataset>.ply
"""
import struct
import sys

import numpy as np

RAW_DTYPE = np.dtype([("key", "<u8"), ("count", "<u8"), ("sum_q", "<i8", (3,)), ("sum_bgr", "<u8", (3,))])
MAGIC = b"REVOMAP1"
VERSION = 1
HEADER_BYTES = 64
_HEADER = struct.Struct("<8sIfiIQQQQ")  # 56 bytes, then zero padding
HEADER_FIELDS = ("voxel", "dense", "voxels", "points_integrated", "points_dropped", "keyframes")

assert RAW_DTYPE.itemsize == 64


def as_records(a):
    """Records from a structured array of RAW_DTYPE or from their bytes (bytes, or a uint8 array)."""
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(a, np.uint8)
    a = np.asarray(a)
    if a.dtype == RAW_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    if a.dtype != np.uint8 or a.size % RAW_DTYPE.itemsize:
        raise ValueError("voxel records are %d bytes each (RAW_DTYPE)" % RAW_DTYPE.itemsize)
    return np.ascontiguousarray(a).reshape(-1).view(RAW_DTYPE)


def check_records(rec, canonical=True):
    """ValueError unless every record has count >= 1 and key bit 63 clear and (canonical) the keys strictly ascend."""
    if len(rec) == 0:
        return
    if np.any(rec["count"] == 0):
        raise ValueError("a voxel record has count 0")
    if np.any(rec["key"] >> np.uint64(63)):
        raise ValueError("a voxel record's key has bit 63 set")
    if canonical:
        k = rec["key"]
        if np.any(k[1:] == k[:-1]):
            raise ValueError("voxel records with the same key")
        if np.any(k[1:] < k[:-1]):
            raise ValueError("voxel records are not in ascending key order")


def make_header(voxel, dense, records, points_dropped=0, keyframes=0):
    records = as_records(records)
    return {"voxel": float(np.float32(voxel)), "dense": int(dense), "voxels": len(records),
            "points_integrated": int(records["count"].sum(dtype=np.uint64)), "points_dropped": int(points_dropped),
            "keyframes": int(keyframes)}


def pack(header, records):
    """The bytes of a .rvm file.  The header's voxels and points_integrated must say what the records hold."""
    rec = as_records(records)
    check_records(rec)
    if int(header["voxels"]) != len(rec):
        raise ValueError("the header says %d voxels, there are %d records" % (header["voxels"], len(rec)))
    if int(header["points_integrated"]) != int(rec["count"].sum(dtype=np.uint64)):
        raise ValueError("the header's points_integrated is not the sum of the records' counts")
    h = _HEADER.pack(MAGIC, VERSION, float(header["voxel"]), int(header["dense"]), 0, int(header["voxels"]),
                     int(header["points_integrated"]), int(header["points_dropped"]), int(header["keyframes"]))
    return h + bytes(HEADER_BYTES - len(h)) + rec.tobytes()


def unpack(data):
    """(header dict, records) of a .rvm file's bytes; ValueError if anything about them is wrong."""
    data = bytes(data)
    if len(data) < HEADER_BYTES:
        raise ValueError("not a voxel map file: shorter than its header")
    magic, version, voxel, dense, zero, voxels, pts, dropped, kfs = _HEADER.unpack_from(data)
    if magic != MAGIC:
        raise ValueError("not a voxel map file: bad magic")
    if version != VERSION:
        raise ValueError("voxel map file of version %d (this reader knows %d)" % (version, VERSION))
    if len(data) != HEADER_BYTES + RAW_DTYPE.itemsize * voxels:
        raise ValueError("voxel map file of %d bytes, its header says %d voxels" % (len(data), voxels))
    if zero != 0 or any(data[_HEADER.size:HEADER_BYTES]) or dense not in (0, 1) or not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel map file with a malformed header")
    rec = np.frombuffer(data, RAW_DTYPE, count=voxels, offset=HEADER_BYTES).copy()
    check_records(rec)
    if int(rec["count"].sum(dtype=np.uint64)) != pts:
        raise ValueError("the header's points_integrated is not the sum of the records' counts")
    return {"voxel": float(voxel), "dense": int(dense), "voxels": int(voxels), "points_integrated": int(pts),
            "points_dropped": int(dropped), "keyframes": int(kfs)}, rec


def write(path, header, records):
    data = pack(header, records)
    with open(path, "wb") as f:
        f.write(data)
    return path


def read(path):
    with open(path, "rb") as f:
        return unpack(f.read())


def merge_records(a, b):
    """The union of two record sets (keys may repeat, within and across them): per key the integer sums, ascending keys."""
    rec = np.concatenate([as_records(a), as_records(b)])
    check_records(rec, canonical=False)
    keys, inv = np.unique(rec["key"], return_inverse=True)
    out = np.zeros(len(keys), RAW_DTYPE)
    out["key"] = keys
    np.add.at(out["count"], inv, rec["count"])
    np.add.at(out["sum_q"], inv, rec["sum_q"])
    np.add.at(out["sum_bgr"], inv, rec["sum_bgr"])
    return out


def subtract_records(a, b):
    """The records of `a` without the sums of `b`: the inverse of merge_records (keys may repeat in either), ascending keys,
    voxels whose count reaches 0 left out.  ValueError, as revo_map_subtract_raw refuses: a key of b that a does not hold, more
    than a voxel's count, or a voxel left at count 0 with another sum not 0."""
    a, b = as_records(a), as_records(b)
    e = np.zeros(0, RAW_DTYPE)
    a, b = merge_records(a, e), merge_records(b, e)  # canonical: one record per key, checked
    if len(b) == 0:
        return a
    i = np.searchsorted(a["key"], b["key"])
    i[i == len(a)] = 0
    if len(a) == 0 or np.any(a["key"][i] != b["key"]):
        raise ValueError("a voxel record to subtract has a key the map does not hold")
    if np.any(b["count"] > a["count"][i]):
        raise ValueError("the records to subtract take more than a voxel's count")
    out = a.copy()
    out["count"][i] -= b["count"]
    out["sum_q"][i] -= b["sum_q"]
    out["sum_bgr"][i] -= b["sum_bgr"]
    dead = out["count"] == 0
    if np.any(out["sum_q"][dead] != 0) or np.any(out["sum_bgr"][dead] != 0):
        raise ValueError("a voxel would be left with count 0 and a sum that is not 0")
    return out[~dead]


def coarsen_records(records, shift):
    """The records of the map with a voxel edge 2^shift times as long (revo_map_coarsen): every axis index of a key becomes
    floor(k / 2^shift) on the unbiased index; records that meet under one key are added."""
    shift = int(shift)
    if not 1 <= shift <= 20:
        raise ValueError("shift must be 1 .. 20")
    rec = as_records(records).copy()
    check_records(rec, canonical=False)
    key, bias, m = rec["key"], np.int64(1 << 20), np.uint64(0x1fffff)
    ax = [((((key >> np.uint64(sh)) & m).astype(np.int64) - bias) >> np.int64(shift)) + bias for sh in (42, 21, 0)]
    rec["key"] = (ax[0].astype(np.uint64) << np.uint64(42)) | (ax[1].astype(np.uint64) << np.uint64(21)) | ax[2].astype(np.uint64)
    return merge_records(rec, np.zeros(0, RAW_DTYPE))


def coarsen_file(path, shift):
    """(header, records) of the file's map coarsened by `shift`: the voxel edge times 2^shift, the counters unchanged."""
    header, rec = read(path)
    out = coarsen_records(rec, shift)
    voxel = float(np.ldexp(np.float32(header["voxel"]), int(shift)))
    if not np.isfinite(voxel):
        raise ValueError("the coarse voxel edge is not finite")
    return dict(header, voxel=voxel, voxels=len(out)), out


def pose_is_orthogonal(R):
    """The is_orthogonal rule of revo_map_align_eval on a row-major 3x3: |R R^T - I|_F < 1e-5 and det > 0, float32 with every
    operation rounded on its own."""
    R = np.asarray(R, np.float32).reshape(3, 3)
    one, zero = np.float32(1), np.float32(0)
    n2 = zero
    for r in range(3):
        for c in range(3):
            v = (R[r, 0] * R[c, 0] + R[r, 1] * R[c, 1]) + R[r, 2] * R[c, 2]
            v = v - (one if r == c else zero)
            n2 = n2 + v * v
    det = ((R[0, 0] * (R[1, 1] * R[2, 2] - R[1, 2] * R[2, 1]) - R[0, 1] * (R[1, 0] * R[2, 2] - R[1, 2] * R[2, 0]))
           + R[0, 2] * (R[1, 0] * R[2, 1] - R[1, 1] * R[2, 0]))
    return bool(np.sqrt(n2) < np.float32(1e-5) and det > 0)


def _pose_matrix(T):
    T = np.asarray(T, np.float32)
    if T.shape == (3, 4):
        T = np.vstack([T, np.float32([0, 0, 0, 1])])
    if T.shape != (4, 4):
        raise ValueError("a pose is a 4x4 or 3x4 matrix")
    if not np.all(np.isfinite(T)):
        raise ValueError("the pose is not finite")
    if not pose_is_orthogonal(T[:3, :3]):
        raise ValueError("the pose's rotation is not orthogonal")
    return T


def pose_records(records, T, voxel_dst, min_count=1):
    """The records of a map seen under the pose T (4x4 or 3x4, the map's frame -> the destination's) at the destination edge
    voxel_dst: revo_map_pose_raw's canonical form, float32 operation by operation.  Per voxel with count >=
    max(min_count, 1): its point p as to_points gives it, p' = ((R0 px + R1 py) + R2 pz) + t, key = floor(p' / voxel_dst),
    dropped when p' is not finite, some |p'| >= 2048 or some index leaves [-2^20, 2^20 - 1]; else count and colour sums are
    carried and sum_q = count * rint(p' 2^20).  -> (records in ascending key order with equal keys summed, info dict of
    voxels_in, voxels_moved, voxels_dropped, voxels_skipped, points_moved, points_dropped, points_skipped).
    ValueError: a bad record (count 0, key bit 63, count >= 2^32), an edge that is not finite and > 0, a pose that is not
    finite or whose rotation is not orthogonal."""
    rec = as_records(records)
    check_records(rec, canonical=False)
    if np.any(rec["count"] >> np.uint64(32)):
        raise ValueError("a voxel record has a count of 2^32 or more")
    v = np.float32(voxel_dst)
    if not (np.isfinite(v) and v > 0):
        raise ValueError("the destination's voxel edge must be finite and > 0")
    T = _pose_matrix(T)
    sel = rec["count"] >= np.uint64(max(1, int(min_count)))
    r = rec[sel]
    cnt = r["count"]
    p = ((r["sum_q"].astype(np.float64) / cnt.astype(np.float64)[:, None]) * 2.0 ** -20).astype(np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        pt = np.stack([((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3] for i in range(3)], 1).astype(np.float32)
        f = np.floor(pt / v)
        ok = np.all((np.abs(pt) < np.float32(2048.0)) & (f >= -(1 << 20)) & (f <= (1 << 20) - 1), 1)
        k = f[ok].astype(np.int64) + np.int64(1 << 20)
        q = np.rint(pt[ok] * np.float32(1 << 20)).astype(np.int64)
    out = np.zeros(int(ok.sum()), RAW_DTYPE)
    out["key"] = (k[:, 0].astype(np.uint64) << np.uint64(42)) | (k[:, 1].astype(np.uint64) << np.uint64(21)) | k[:, 2].astype(np.uint64)
    out["count"] = cnt[ok]
    out["sum_q"] = cnt[ok].astype(np.int64)[:, None] * q
    out["sum_bgr"] = r["sum_bgr"][ok]
    total = lambda c: int(c.sum(dtype=np.uint64))  # noqa: E731
    info = {"voxels_in": len(rec), "voxels_moved": int(ok.sum()), "voxels_dropped": int((~ok).sum()), "voxels_skipped": int((~sel).sum()),
            "points_moved": total(cnt[ok]), "points_dropped": total(cnt[~ok]), "points_skipped": total(rec["count"][~sel])}
    return merge_records(out, np.zeros(0, RAW_DTYPE)), info


CARVE_CLASSES = ("outside", "unknown", "free", "confirmed", "occluded", "edge")
CARVE_INFO_KEYS = ("voxels_considered", "voxels_carved", "points_carved", "votes")


def carve_view(depth, T_w_c, intrinsics):
    """One view of carve_records, checked as revo_map_carve checks it: depth [h, w] float32 metres (1 .. 2048 each way), T_w_c a
    4x4 or 3x4 camera -> world pose (finite, rotation orthogonal), intrinsics (fx, fy, cx, cy, zmin, zmax) finite with fx, fy > 0
    and 0 <= zmin < zmax.  -> (depth, Rc, tc, k): the world -> camera rotation and translation as revo_map_render forms them."""
    D = np.ascontiguousarray(np.asarray(depth, np.float32))
    if D.ndim != 2 or not (1 <= D.shape[0] <= 2048 and 1 <= D.shape[1] <= 2048):
        raise ValueError("a depth image is h x w with 1 .. 2048 pixels each way")
    T = _pose_matrix(T_w_c)
    k = np.asarray(intrinsics, np.float32).reshape(-1)
    if k.shape != (6,) or not np.all(np.isfinite(k)):
        raise ValueError("the intrinsics are six finite numbers: fx, fy, cx, cy, zmin, zmax")
    if not (k[0] > 0 and k[1] > 0):
        raise ValueError("fx and fy must be > 0")
    if not (k[4] >= 0 and k[4] < k[5]):
        raise ValueError("the depth range needs 0 <= zmin < zmax")
    Rc = T[:3, :3].T.copy()
    t = T[:3, 3]
    tc = np.array([-(((Rc[i, 0] * t[0]) + (Rc[i, 1] * t[1])) + (Rc[i, 2] * t[2])) for i in range(3)], np.float32)
    return D, Rc, tc, k


def carve_classes(p, view, radius, margin, margin_rel, depths=False, pixels=False):
    """The class (index into CARVE_CLASSES) of every point p [N, 3] float32 in one checked view (carve_view): revo_map_carve's
    rule (include/revo_hip.h), float32 operation by operation.  depths: -> (class, z, dc), the camera-space depth of
    every point and the centre pixel's depth (NaN where the class is outside) the classes were decided on.  pixels (with depths):
    -> (class, z, dc, pix), pix the centre pixel's place iv * w + iu (-1 where the class is outside)."""
    D, Rc, tc, k = view
    f32 = np.float32
    fx, fy, cx, cy, zmin, zmax = (f32(x) for x in k)
    r, margin, margin_rel = int(radius), f32(margin), f32(margin_rel)
    h, w = D.shape
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    cls = np.zeros(len(p), np.int64)  # outside
    with np.errstate(all="ignore"):
        x, y, z = (((Rc[i, 0] * px + Rc[i, 1] * py) + Rc[i, 2] * pz) + tc[i] for i in range(3))
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > zmin) & (z < zmax)
        u = (fx * x) / z + cx
        v = (fy * y) / z + cy
        ok &= (np.abs(u) < f32(1 << 20)) & (np.abs(v) < f32(1 << 20))  # NaN / inf fail the comparison
        iu = np.floor(np.where(ok, u, f32(0)) + f32(0.5)).astype(np.int64)
        iv = np.floor(np.where(ok, v, f32(0)) + f32(0.5)).astype(np.int64)
        ok &= (iu - r >= 0) & (iu + r <= w - 1) & (iv - r >= 0) & (iv + r <= h - 1)
        j = np.nonzero(ok)[0]
        z_all = z
        iu, iv, z = iu[j], iv[j], z[j]
        usable = np.ones(len(j), bool)
        dmin = np.full(len(j), np.inf, f32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                d = D[iv + dy, iu + dx]
                good = np.isfinite(d) & (d > zmin) & (d < zmax)
                usable &= good
                dmin = np.where(good, np.minimum(dmin, d), dmin)
        dc = D[iv, iu]
        mc = margin + margin_rel * dc
        c = np.where(z < dmin - (margin + margin_rel * dmin), 2,
                     np.where(np.abs(z - dc) <= mc, 3, np.where(z > dc + mc, 4, 5)))
    cls[j] = np.where(usable, c, 1)
    if depths:
        dc_all = np.full(len(p), np.nan, f32)
        dc_all[j] = dc
        if pixels:
            pix_all = np.full(len(p), -1, np.int64)
            pix_all[j] = iv * w + iu
            return cls, z_all.astype(f32), dc_all, pix_all
        return cls, z_all.astype(f32), dc_all
    return cls


def carve_rule_args(voxel, views, radius, margin, margin_rel):
    """What the per-view rule runs with, checked as revo_map_carve_eval and revo_map_observe check it -> (checked views,
    radius, margin, margin_rel).  margin None: the voxel edge."""
    if not 0 <= int(radius) <= 3:
        raise ValueError("radius must be 0 .. 3")
    margin = np.float32(voxel if margin is None else margin)
    margin_rel = np.float32(margin_rel)
    if not (np.isfinite(margin) and margin >= 0 and np.isfinite(margin_rel) and margin_rel >= 0):
        raise ValueError("margin and margin_rel must be finite and >= 0")
    views = list(views)
    if not 1 <= len(views) <= 64:
        raise ValueError("a carve takes 1 .. 64 views")
    return [carve_view(*v) for v in views], int(radius), margin, margin_rel


def carve_records(records, voxel, views, radius=1, min_views=1, min_count=1, max_count=0, margin=None, margin_rel=0.0):
    """Free-space carving without a GPU: revo_map_carve_eval's contract in vectorised numpy.  views: a list of
    (depth [h, w] float32, T_w_c, (fx, fy, cx, cy, zmin, zmax)).  Per voxel with count >= max(min_count, 1) (and <= max_count
    unless that is 0) and per view its class; a voxel that is `free` in at least max(min_views, 1) views is carved.  margin
    None: the voxel edge.  -> (the carved voxels' records in ascending key order -- subtract_records(records, them) is the carved
    map --, info dict of CARVE_INFO_KEYS, one dict of CARVE_CLASSES counts per view).  ValueError as the library's
    REVO_ERR_INVALID_ARG."""
    rec = as_records(records)
    check_records(rec)
    views, radius, margin, margin_rel = carve_rule_args(voxel, views, radius, margin, margin_rel)
    sel = rec["count"] >= np.uint64(max(1, int(min_count)))
    if int(max_count):
        sel &= rec["count"] <= np.uint64(int(max_count))
    cand = rec[sel]
    p = ((cand["sum_q"].astype(np.float64) / cand["count"].astype(np.float64)[:, None]) * 2.0 ** -20).astype(np.float32).reshape(-1, 3)
    votes = np.zeros(len(cand), np.int64)
    counts = []
    for vw in views:
        cls = carve_classes(p, vw, radius, margin, margin_rel)
        votes += cls == 2
        counts.append({name: int((cls == i).sum()) for i, name in enumerate(CARVE_CLASSES)})
    gone = cand[votes >= max(1, int(min_views))]
    info = {"voxels_considered": len(cand), "voxels_carved": len(gone), "points_carved": int(gone["count"].sum(dtype=np.uint64)),
            "votes": int(votes.sum())}
    return gone.copy(), info, counts


def read_views(views_dir, camera, zrange, depth_scale=5000.0, color=False):
    """The views of a `run_tum --map-views` folder as carve_records and observe_records take them: depth/*.png (16-bit, metres
    x depth_scale), associate.txt and poses.txt (the pose of each depth image by time stamp).  color: each view brings the BGR
    image of rgb/*.png as a fourth entry, as tsdf_records(bgr=) takes it."""
    import os
    from . import tum
    rows = tum.read_associate(os.path.join(views_dir, "associate.txt"))
    poses = {round(ts, 6): T for ts, T in tum.read_poses(os.path.join(views_dir, "poses.txt"))}
    views = []
    for rgb_ts, rgb_file, depth_ts, depth_file in rows:
        T = poses.get(round(float(rgb_ts), 6), poses.get(round(float(depth_ts), 6)))
        if T is None:
            raise ValueError("%s: no pose in poses.txt for the view at %s" % (views_dir, rgb_ts))
        bgr, raw = tum.load_frame(views_dir, rgb_file, depth_file)
        views.append((raw.astype(np.float32) / np.float32(depth_scale), T, tuple(camera) + tuple(zrange)) + ((bgr,) if color else ()))
    if not views:
        raise ValueError("%s holds no views" % views_dir)
    return views


def carve_file(path, views_dir, camera, zrange, depth_scale=5000.0, **params):
    """(header, records, removed header, removed records, info) of the file's map carved with the views of a `run_tum
    --map-views` folder: depth/*.png (16-bit, metres x depth_scale), associate.txt and poses.txt (the pose of each depth
    image by time stamp).  camera (fx, fy, cx, cy) and zrange (zmin, zmax) say how the views were taken.  The removed voxels
    carry no dropped points and no keyframes, so the two headers add up to the file's."""
    header, rec = read(path)
    views = read_views(views_dir, camera, zrange, depth_scale)
    gone = np.zeros(0, RAW_DTYPE)
    info = dict.fromkeys(CARVE_INFO_KEYS, 0)
    if int(params.get("min_views", 1)) <= 1:  # 64 views per carve; with min_views 1 carving in parts is carving at once
        for i in range(0, len(views), 64):
            g, part, _ = carve_records(rec, header["voxel"], views[i:i + 64], **params)
            rec = subtract_records(rec, g)
            gone = merge_records(gone, g)
            # considered: the map's candidates, counted once (the first part sees them all); votes: those cast on voxels still there
            info = dict({k: info[k] + part[k] for k in info}, voxels_considered=part["voxels_considered"] if i == 0 else info["voxels_considered"])
    else:
        if len(views) > 64:
            raise ValueError("a carve with --min-views above 1 takes at most 64 views, %s holds %d" % (views_dir, len(views)))
        gone, info, _ = carve_records(rec, header["voxel"], views, **params)
        rec = subtract_records(rec, gone)
    h = dict(header, voxels=len(rec), points_integrated=header["points_integrated"] - int(gone["count"].sum(dtype=np.uint64)))
    return h, rec, make_header(header["voxel"], header["dense"], gone), gone, info


RAY_STATUS = ("hit", "range", "outside", "exhausted")
RAY_INFO_KEYS = ("rays", "hits", "range", "outside", "exhausted", "cells")
RAY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
RAY_MAX_STEPS = 1 << 20


def _ray_march(o, s0, d, s1, voxel, solid_keys, max_steps):
    """The march of revo_map_raycast / revo_map_cast_rays (include/revo_hip.h) for N rays at once, float32 operation
    by operation: every ray still under way advances one cell per iteration.  o, d [N, 3], s0, s1 [N] float32; solid_keys: the
    ascending keys of the solid voxels.  -> (index into solid_keys or -1, s float32, cells int64, status int64), [N] each."""
    f32 = np.float32
    voxel = f32(voxel)
    o, d = np.asarray(o, f32).reshape(-1, 3), np.asarray(d, f32).reshape(-1, 3)
    s0, s1 = np.asarray(s0, f32).reshape(-1), np.asarray(s1, f32).reshape(-1)
    n = len(o)
    hit = np.full(n, -1, np.int64)
    s_out = np.zeros(n, f32)
    cells = np.zeros(n, np.int64)
    status = np.full(n, 2, np.int64)  # outside
    lo, hi = -(1 << 20), (1 << 20) - 1
    with np.errstate(all="ignore"):
        g = o + s0[:, None] * d
        f = np.floor(g / voxel)
        ok = (s0 < s1) & np.isfinite(s1) & np.all(np.isfinite(g), 1) & np.all((f >= f32(lo)) & (f <= f32(hi)), 1)
        idx = np.nonzero(ok)[0]
        o, d, s1 = o[idx], d[idx], s1[idx]
        k = f[idx].astype(np.int64)
        inv = f32(1) / d
        step = np.where(d > 0, 1, np.where(d < 0, -1, 0)).astype(np.int64)
        step[~np.isfinite(inv)] = 0
        pos = (d > 0).astype(np.int64)
        t = np.where(step != 0, ((k + pos).astype(f32) * voxel - o) * inv, f32(np.inf)).astype(f32)
        s = s0[idx].copy()
        bias = np.int64(1 << 20)
        done = 0
        while len(idx):
            if done == int(max_steps):
                status[idx] = 3
                break
            done += 1
            cells[idx] = done
            s_out[idx] = s
            kb = (k + bias).astype(np.uint64)
            key = (kb[:, 0] << np.uint64(42)) | (kb[:, 1] << np.uint64(21)) | kb[:, 2]
            j = np.searchsorted(solid_keys, key)
            j[j >= len(solid_keys)] = 0
            found = solid_keys[j] == key if len(solid_keys) else np.zeros(len(idx), bool)
            hit[idx[found]] = j[found]
            status[idx[found]] = 0
            a = np.zeros(len(idx), np.int64)
            sn = t[:, 0].copy()
            for ax in (1, 2):
                m = t[:, ax] < sn
                a[m] = ax
                sn[m] = t[m, ax]
            far = ~found & ~(sn < s1)
            status[idx[far]] = 1
            r = np.arange(len(idx))
            kn = k[r, a] + step[r, a]
            out = ~found & ~far & ((kn < lo) | (kn > hi))  # status stays outside
            go = ~found & ~far & ~out
            k[r, a] = kn
            t[r, a] = ((kn + pos[r, a]).astype(f32) * voxel - o[r, a]) * inv[r, a]
            idx, o, s1, k, inv, step, pos, t, s = idx[go], o[go], s1[go], k[go], inv[go], step[go], pos[go], t[go], sn[go]
    return hit, s_out, cells, status


def _ray_info(status, cells):
    return {"rays": int(len(status)), "hits": int((status == 0).sum()), "range": int((status == 1).sum()),
            "outside": int((status == 2).sum()), "exhausted": int((status == 3).sum()), "cells": int(cells.sum())}


def _ray_args(records, voxel, min_count, max_steps):
    rec = as_records(records)
    check_records(rec)
    v = np.float32(voxel)
    if not (np.isfinite(v) and v > 0):
        raise ValueError("the voxel edge must be finite and > 0")
    if not 1 <= int(max_steps) <= RAY_MAX_STEPS:
        raise ValueError("max_steps must be 1 .. 2^20")
    return rec[rec["count"] >= np.uint64(max(1, int(min_count)))], v


def ray_view(T_w_c, intrinsics, size):
    """One view of raycast_records, checked as revo_map_raycast checks it (revo_map_render's rules): T_w_c a finite 4x4 or 3x4
    camera -> world pose, intrinsics (fx, fy, cx, cy, zmin, zmax) finite with fx, fy > 0 and 0 <= zmin < zmax, size (width,
    height), 1 .. 2048 each.  -> (o, R, Rc, tc, k, (w, h)): the rays' origin and rotation, and the world -> camera transform as
    revo_map_render forms it."""
    T = np.asarray(T_w_c, np.float32)
    if T.shape == (3, 4):
        T = np.vstack([T, np.float32([0, 0, 0, 1])])
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise ValueError("a pose is a finite 4x4 or 3x4 matrix")
    w, h = int(size[0]), int(size[1])
    if not (1 <= w <= 2048 and 1 <= h <= 2048):
        raise ValueError("width and height must be 1 .. 2048")
    k = np.asarray(intrinsics, np.float32).reshape(-1)
    if k.shape != (6,) or not np.all(np.isfinite(k)):
        raise ValueError("the intrinsics are six finite numbers: fx, fy, cx, cy, zmin, zmax")
    if not (k[0] > 0 and k[1] > 0):
        raise ValueError("fx and fy must be > 0")
    if not (k[4] >= 0 and k[4] < k[5]):
        raise ValueError("the depth range needs 0 <= zmin < zmax")
    R = T[:3, :3].copy()
    Rc = R.T.copy()
    t = T[:3, 3].copy()
    tc = np.array([-(((Rc[i, 0] * t[0]) + (Rc[i, 1] * t[1])) + (Rc[i, 2] * t[2])) for i in range(3)], np.float32)
    return t, R, Rc, tc, k, (w, h)


def ray_view_rays(view):
    """(o [N, 3], s0 [N], d [N, 3], s1 [N]) of a checked view's pixels in row order: pixel (x, y) casts dcx = (x - cx) / fx,
    dcy = (y - cy) / fy, d_i = ((R_i0 dcx) + (R_i1 dcy)) + R_i2 from the camera's position over [zmin, zmax)."""
    o, R, _, _, k, (w, h) = view
    f32 = np.float32
    xs, ys = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    dcx = ((xs - k[2]) / k[0]).ravel()
    dcy = ((ys - k[3]) / k[1]).ravel()
    d = np.stack([((R[i, 0] * dcx) + (R[i, 1] * dcy)) + R[i, 2] for i in range(3)], 1).astype(f32)
    n = w * h
    return np.broadcast_to(o, (n, 3)).copy(), np.full(n, k[4], f32), d, np.full(n, k[5], f32)


def ray_view_solid(rec, view):
    """The voxels of `rec` (count already selected) that are solid to a checked view: their point as to_points forms it, taken
    to the camera as revo_map_render does, is finite with zmin < z < zmax.  -> (keys, z float32, bgr uint8 [n, 3])."""
    _, _, Rc, tc, k, _ = view
    cnt = rec["count"]
    p = ((rec["sum_q"].astype(np.float64) / cnt.astype(np.float64)[:, None]) * 2.0 ** -20).astype(np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x, y, z = (((Rc[i, 0] * p[:, 0] + Rc[i, 1] * p[:, 1]) + Rc[i, 2] * p[:, 2]) + tc[i] for i in range(3))
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > k[4]) & (z < k[5])
    c = cnt[:, None]
    bgr = ((rec["sum_bgr"] + c // np.uint64(2)) // c).astype(np.uint8).reshape(-1, 3)
    return rec["key"][ok], z[ok].astype(np.float32), bgr[ok]


def raycast_records(records, voxel, views, min_count=1, max_steps=4096):
    """Ray-cast views of a map without a GPU: revo_map_raycast's contract in vectorised numpy.  records: canonical
    (ascending keys); views: a list of (T_w_c, (fx, fy, cx, cy, zmin, zmax), (width, height)).  -> a dict of per-view lists
    depth ([h, w] float32, 0 = miss), bgr ([h, w, 3] uint8), key ([h, w] uint64, all ones = miss), hits, and -- beyond what the
    library returns -- s, cells, status ([h, w] each: the entry parameter of the last cell examined, the cells examined, the
    index into RAY_STATUS), plus info: the call's RAY_INFO_KEYS sums.  ValueError as the library's REVO_ERR_INVALID_ARG."""
    rec, v = _ray_args(records, voxel, min_count, max_steps)
    views = list(views)
    if not 1 <= len(views) <= 64:
        raise ValueError("a ray cast takes 1 .. 64 views")
    views = [ray_view(*vw) for vw in views]
    out = {k: [] for k in ("depth", "bgr", "key", "hits", "s", "cells", "status")}
    total = dict.fromkeys(RAY_INFO_KEYS, 0)
    for vw in views:
        w, h = vw[5]
        keys, z, bgr = ray_view_solid(rec, vw)
        hit, s, cells, status = _ray_march(*ray_view_rays(vw), v, keys, max_steps)
        got = hit >= 0
        j = np.maximum(hit, 0)
        if len(keys) == 0:  # nothing is solid to this view: j has nothing to index
            keys, z, bgr = np.full(1, RAY_EMPTY, np.uint64), np.zeros(1, np.float32), np.zeros((1, 3), np.uint8)
        out["depth"].append(np.where(got, z[j], np.float32(0)).astype(np.float32).reshape(h, w))
        out["bgr"].append(np.where(got[:, None], bgr[j], np.uint8(0)).astype(np.uint8).reshape(h, w, 3))
        out["key"].append(np.where(got, keys[j], RAY_EMPTY).astype(np.uint64).reshape(h, w))
        out["hits"].append(int(got.sum()))
        out["s"].append(s.reshape(h, w))
        out["cells"].append(cells.reshape(h, w))
        out["status"].append(status.reshape(h, w))
        for name, x in _ray_info(status, cells).items():
            total[name] += x
    out["info"] = total
    return out


def cast_rays_records(records, voxel, rays, min_count=1, max_steps=4096):
    """Range queries without a GPU: revo_map_cast_rays' contract in vectorised numpy.  rays: [N, 8] float32 rows of
    o (3), s0, d (3), s1.  A ray that is not finite or has s0 >= s1 comes back `outside` with 0 cells.  -> (key uint64 [N], all
    ones unless a hit; s float32 [N]; cells uint32 [N]; status uint8 [N], the index into RAY_STATUS; info dict of RAY_INFO_KEYS)."""
    rec, v = _ray_args(records, voxel, min_count, max_steps)
    r = np.ascontiguousarray(np.asarray(rays, np.float32)).reshape(-1, 8)
    if not 1 <= len(r) <= 1 << 24:
        raise ValueError("a call takes 1 .. 2^24 rays")
    keys = rec["key"]
    hit, s, cells, status = _ray_march(r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7], v, keys, max_steps)
    key = np.where(hit >= 0, keys[np.maximum(hit, 0)] if len(keys) else RAY_EMPTY, RAY_EMPTY).astype(np.uint64)
    return key, s, cells.astype(np.uint32), status.astype(np.uint8), _ray_info(status, cells)


# ------------------------------------------------------------------------------------------ the distance field --
DF_NONE = np.uint32(0xFFFFFFFF)
DF_MAX_N = 1024
DF_MAX_CELLS = 1 << 27
DF_INFO_KEYS = ("cells", "solid", "outside", "below", "max_d2")
DF_SAMPLE_DTYPE = np.dtype([("dist", "<f4"), ("grad", "<f4", (3,))])
_DF_INF = np.int32(1 << 30)  # above 3 * 1023^2; _DF_INF + 1023^2 fits 32 bits


def key_axes(keys):
    """[N, 3] int64 voxel indices (x, y, z) of packed keys."""
    k = np.asarray(keys, np.uint64)
    m = np.uint64(0x1FFFFF)
    return np.stack([(k >> np.uint64(42)) & m, (k >> np.uint64(21)) & m, k & m], -1).astype(np.int64).reshape(-1, 3) - (1 << 20)


def check_box(lo, n):
    """(lo, n) as int64 [3] arrays; ValueError if the box breaks revo_map_df_box's limits."""
    lo, n = np.asarray(lo, np.int64).reshape(3), np.asarray(n, np.int64).reshape(3)
    if np.any(n < 1) or np.any(n > DF_MAX_N):
        raise ValueError("a distance-field box has 1 .. %d cells per axis, not %s" % (DF_MAX_N, n.tolist()))
    if np.any(lo < -(1 << 20)) or np.any(lo + n - 1 > (1 << 20) - 1):
        raise ValueError("the distance-field box %s + %s leaves the voxel index range [-2^20, 2^20 - 1]" % (lo.tolist(), n.tolist()))
    if int(n[0]) * int(n[1]) * int(n[2]) > DF_MAX_CELLS:
        raise ValueError("the distance-field box %s holds more than 2^27 cells" % (n.tolist(),))
    return lo, n


def bounds_records(records, min_count=1):
    """(lo [3], hi [3], n) of revo_map_bounds: the smallest and largest voxel index per axis over the records with count >=
    max(min_count, 1), and how many there are; zeros when there are none."""
    rec = as_records(records)
    rec = rec[rec["count"] >= np.uint64(max(1, int(min_count)))]
    if len(rec) == 0:
        return np.zeros(3, np.int32), np.zeros(3, np.int32), 0
    k = key_axes(rec["key"])
    return k.min(0).astype(np.int32), k.max(0).astype(np.int32), len(rec)


def padded_box(lo, hi, pad):
    """The box (lo, n) of the index bounds lo .. hi grown by `pad` cells on every side, clipped to the index range."""
    pad = int(pad)
    if pad < 0:
        raise ValueError("pad must be >= 0 cells")
    a = np.maximum(np.asarray(lo, np.int64) - pad, -(1 << 20))
    b = np.minimum(np.asarray(hi, np.int64) + pad, (1 << 20) - 1)
    return check_box(a, b - a + 1)


def _min_plus(g, axis, chunk=1 << 17):
    """d(i) = min_j (i - j)^2 + g(j) along one axis of an int32 array (_DF_INF: no entry; _DF_INF + 1023^2 fits).  Only lines
    with an entry are worked on, `chunk` cells at a time, and the offsets k = |i - j| end once k^2 reaches the largest value
    left in the chunk: nothing can improve any more."""
    g = np.moveaxis(g, axis, 0)
    shape = g.shape
    L = shape[0]
    res = g.reshape(L, -1).copy()
    lines = np.flatnonzero((res < _DF_INF).any(0))
    step = max(1, chunk // L)
    for c in range(0, len(lines), step):
        sel = lines[c:c + step]
        src = np.ascontiguousarray(res[:, sel])
        out, tmp = src.copy(), np.empty_like(src)
        k = 1
        while k < L and k * k < int(out.max()):
            kk = np.int32(k * k)
            np.add(src[:L - k], kk, out=tmp[k:])
            np.minimum(out[k:], tmp[k:], out=out[k:])
            np.add(src[k:], kk, out=tmp[:L - k])
            np.minimum(out[:L - k], tmp[:L - k], out=out[:L - k])
            k += 1
        res[:, sel] = out
    return np.moveaxis(res.reshape(shape), 0, axis)


def distance_field_records(records, lo, n, min_count=1, clamp=0):
    """revo_map_distance_field restated: (d2 uint32 [n0, n1, n2], info dict of DF_INFO_KEYS).  d2[c] is the smallest squared
    distance, in cells, from cell lo + c to a voxel with count >= max(min_count, 1) inside the box (voxels outside it are not
    seen), DF_NONE when the box holds none; with clamp > 0 every other value is min(value, clamp).  Written as the three
    min-plus passes z, y, x over exact integers."""
    lo, n = check_box(lo, n)
    mask, info = solid_cells(records, lo, n, min_count)
    d2, info["max_d2"] = _field_of(mask, clamp)
    return d2, info


def solid_cells(records, lo, n, min_count=1):
    """(bool [n0, n1, n2]: the cells of the box that hold a voxel with count >= max(min_count, 1); the counters cells, solid,
    outside, below of DF_INFO_KEYS)."""
    rec = as_records(records)
    solid = rec["count"] >= np.uint64(max(1, int(min_count)))
    k = key_axes(rec["key"][solid]) - lo
    inside = np.all((k >= 0) & (k < n), axis=1)
    k = k[inside]
    mask = np.zeros(tuple(int(x) for x in n), bool)
    mask[k[:, 0], k[:, 1], k[:, 2]] = True
    return mask, {"cells": int(mask.size), "solid": int(inside.sum()), "outside": int(solid.sum() - inside.sum()), "below": int((~solid).sum())}


def _field_of(obstacles, clamp):
    """(d2, max_d2) of revo_map_distance_field's definition over a bool volume of obstacle cells."""
    g = np.where(obstacles, np.int32(0), _DF_INF)
    for axis in (2, 1, 0):
        g = _min_plus(g, axis)
    none = g >= _DF_INF
    g = g.astype(np.uint32)
    if int(clamp) > 0:
        g = np.minimum(g, np.uint32(min(int(clamp), 0xFFFFFFFF)))
    return np.where(none, DF_NONE, g), int(g[~none].max()) if (~none).any() else 0


SEEN_INFO_KEYS = ("cells", "cells_free", "cells_surface", "votes", "newly_known")
KNOWN_INFO_KEYS = DF_INFO_KEYS + ("unknown", "known_free")
SEEN_VOTES, SEEN_SURFACE = np.uint8(0x7F), np.uint8(0x80)


def seen_centres(lo, n, voxel):
    """[cells, 3] float32: the centres of the box's cells in the volume's order (z fastest), ((float32)(lo + a) + 0.5) * voxel
    with the product rounded once."""
    ax = [(np.arange(int(lo[i]), int(lo[i]) + int(n[i])).astype(np.float32) + np.float32(0.5)) * np.float32(voxel) for i in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def seen_update(seen_in, f, s):
    """The byte rule of revo_map_observe: ((in | s << 7) & 0x80) | min(127, (in & 0x7F) + f), elementwise -> uint8."""
    b = np.asarray(seen_in, np.uint8).astype(np.int64)
    return (((b | (np.asarray(s, np.int64) << 7)) & 0x80) | np.minimum(127, (b & 0x7F) + np.asarray(f, np.int64))).astype(np.uint8)


def observe_records(voxel, lo, n, views, radius=1, margin=None, margin_rel=0.0, seen=None, chunk=1 << 20):
    """The seen volume without a GPU: revo_map_observe's contract in vectorised numpy, through carve_classes -- the
    class rule carve_records uses.  views: as carve_records takes them; seen: a uint8 [n0, n1, n2] volume to accumulate into
    (it is not changed), None for a fresh one.  -> (seen uint8 [n0, n1, n2], info dict of SEEN_INFO_KEYS, one dict of
    CARVE_CLASSES counts per view).  ValueError as the library's REVO_ERR_INVALID_ARG."""
    lo, n = check_box(lo, n)
    views, radius, margin, margin_rel = carve_rule_args(voxel, views, radius, margin, margin_rel)
    shape = tuple(int(x) for x in n)
    if seen is None:
        before = np.zeros(shape, np.uint8)
    else:
        before = np.asarray(seen)
        if before.dtype != np.uint8 or before.shape != shape:
            raise ValueError("the volume to accumulate into is a uint8 array of the box's shape")
    p = seen_centres(lo, n, voxel)
    f, s = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
    counts = [dict.fromkeys(CARVE_CLASSES, 0) for _ in views]
    for a in range(0, len(p), int(chunk)):
        for vw, cnt in zip(views, counts):
            cls = carve_classes(p[a:a + chunk], vw, radius, margin, margin_rel)
            f[a:a + chunk] += cls == 2
            s[a:a + chunk] |= cls == 3
            for i, name in enumerate(CARVE_CLASSES):
                cnt[name] += int((cls == i).sum())
    out = seen_update(before.reshape(-1), f, s).reshape(shape)
    info = {"cells": int(out.size), "cells_free": int(((out & SEEN_VOTES) != 0).sum()), "cells_surface": int(((out & SEEN_SURFACE) != 0).sum()),
            "votes": int(f.sum()), "newly_known": int(((before == 0) & (out != 0)).sum())}
    return out, info, counts


def seen_free(seen, min_views=1):
    """bool: the cells with at least max(min_views, 1) free votes."""
    return (np.asarray(seen, np.uint8) & SEEN_VOTES) >= max(1, int(min_views))


def seen_known(seen, min_views=1, solid=None):
    """bool: the known cells -- free, with the surface bit, or (solid: a bool volume) solid."""
    k = seen_free(seen, min_views) | ((np.asarray(seen, np.uint8) & SEEN_SURFACE) != 0)
    return k if solid is None else k | np.asarray(solid, bool)


def _seen_volume(seen, n):
    seen = np.asarray(seen)
    if seen.dtype != np.uint8 or seen.shape != tuple(int(x) for x in n):
        raise ValueError("the seen volume is a uint8 array of the box's shape")
    return seen


def known_field_records(records, lo, n, seen, min_count=1, clamp=0, min_views=1):
    """revo_map_known_field restated: distance_field_records over the obstacle set solid + unknown -> (d2 uint32 [n0, n1, n2],
    info dict of KNOWN_INFO_KEYS)."""
    lo, n = check_box(lo, n)
    seen = _seen_volume(seen, n)
    solid, info = solid_cells(records, lo, n, min_count)
    unknown = ~seen_known(seen, min_views, solid)
    d2, info["max_d2"] = _field_of(solid | unknown, clamp)
    info["unknown"] = int(unknown.sum())
    info["known_free"] = info["cells"] - info["solid"] - info["unknown"]
    return d2, info


def frontier_records(records, lo, n, seen, min_count=1, min_views=1):
    """revo_map_frontiers restated: [k, 3] int32 absolute voxel indices, in ascending order of the cell's place in the box, of
    the cells that are not solid, have >= max(min_views, 1) free votes and have a face neighbour inside the box that is unknown."""
    lo, n = check_box(lo, n)
    seen = _seen_volume(seen, n)
    solid, _ = solid_cells(records, lo, n, min_count)
    unknown = ~seen_known(seen, min_views, solid)
    near = np.zeros(unknown.shape, bool)
    for axis in range(3):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[axis], b[axis] = slice(1, None), slice(None, -1)
        near[tuple(a)] |= unknown[tuple(b)]
        near[tuple(b)] |= unknown[tuple(a)]
    cells = np.argwhere(~solid & seen_free(seen, min_views) & near)
    return (cells + lo).astype(np.int32).reshape(-1, 3)


def explore_records(records, lo, n, voxel, seen, start, clearance, min_count=1, min_views=1, max_len=4096):
    """The whole route without a GPU: the known field, the frontiers, the cost-to-go with the frontiers as goals at the
    clearance (metres), and the path from `start` (a voxel index) -> (d2, frontiers, cost, plan info, (cells, status, cost))."""
    d2, _ = known_field_records(records, lo, n, seen, min_count, 0, min_views)
    fr = frontier_records(records, lo, n, seen, min_count, min_views)
    if len(fr) == 0:
        raise ValueError("the seen volume has no frontier cell")
    cost, info = plan_records(d2, lo, n, plan_seeds(fr), plan_r2(clearance, voxel))
    if info["seeds_used"] == 0:  # a frontier cell touches unseen space: d2 = 1 in the known field
        raise ValueError("no frontier cell keeps the clearance: unseen space counts against it, so the route needs r2 = 1 (at most one voxel edge)")
    return d2, fr, cost, info, plan_paths(cost, lo, n, np.asarray(start, np.int64).reshape(1, 3), max_len)[0]


GAIN_DTYPE = np.dtype([("unknown_free", "<u4"), ("unknown_surface", "<u4"), ("unknown_inside", "<u4"), ("hits", "<u4"), ("reserved", "<u4", (4,))])
GAIN_INFO_KEYS = ("poses", "cells", "unknown", "unknown_free", "unknown_surface", "unknown_inside", "rays", "ray_hits")
GAIN_MAX_POSES = 4096
assert GAIN_DTYPE.itemsize == 32


class GainRecords(np.ndarray):
    """The per-pose records of a view-gain call (GAIN_DTYPE) with the call's counters in `.info` (GAIN_INFO_KEYS)."""
    info = None

    def __array_finalize__(self, obj):
        self.info = getattr(obj, "info", None)


def gain_result(records, info):
    out = np.ascontiguousarray(records, GAIN_DTYPE).view(GainRecords)
    out.info = dict(info)
    return out


def gain_poses(poses):
    """[k, 4, 4] float32 of one pose or 1 .. 4096 poses given as 4x4 or 3x4 matrices; no rule of a pose is checked here."""
    T = np.asarray(poses, np.float32)
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[1:] not in ((4, 4), (3, 4)) or not 1 <= len(T) <= GAIN_MAX_POSES:
        raise ValueError("view gain takes 1 .. 4096 poses, 4x4 or 3x4 each")
    if T.shape[1] == 3:
        T = np.concatenate([T, np.broadcast_to(np.float32([0, 0, 0, 1]), (len(T), 1, 4))], 1)
    return np.ascontiguousarray(T)


def gain_pose_ok(T):
    """revo_map_carve_eval's pose rules: finite, rotation orthogonal."""
    return bool(np.all(np.isfinite(T))) and pose_is_orthogonal(T[:3, :3])


def gain_records(records, voxel, lo, n, seen, view, poses, radius=1, min_views=1, margin=None, margin_rel=0.0, miss_depth=0.0,
                 min_count=1, max_steps=4096, device_poses=False):
    """What each of `poses` would add to a seen volume, without a GPU: revo_map_view_gain's contract in vectorised
    numpy, through raycast_records (the predicted depth image), carve_classes (a centre's class in it) and seen_known (which
    cells are unknown).  view: ((fx, fy, cx, cy, zmin, zmax), (width, height)); poses: what gain_poses takes.  -> GainRecords:
    GAIN_DTYPE per pose, and .info.  device_poses: a pose that breaks the pose rules gives an all-zero record, as the library
    treats poses in device memory; otherwise it is a ValueError, like every REVO_ERR_INVALID_ARG of the library."""
    lo, n = check_box(lo, n)
    seen = _seen_volume(seen, n)
    rec, v = _ray_args(records, voxel, min_count, max_steps)
    k, size = view
    T = gain_poses(poses)
    cam = ray_view(np.eye(4, dtype=np.float32), k, size)
    k = cam[4]
    if not 0 <= int(radius) <= 3:
        raise ValueError("radius must be 0 .. 3")
    margin, margin_rel, miss = np.float32(v if margin is None else margin), np.float32(margin_rel), np.float32(miss_depth)
    if not (np.isfinite(margin) and margin >= 0 and np.isfinite(margin_rel) and margin_rel >= 0):
        raise ValueError("margin and margin_rel must be finite and >= 0")
    if miss != 0 and not (miss > k[4] and miss < k[5]):
        raise ValueError("miss_depth must be 0 or inside (zmin, zmax)")
    good = [gain_pose_ok(M) for M in T]
    if not device_poses and not all(good):
        raise ValueError("pose %d is not finite or its rotation is not orthogonal" % good.index(False))
    solid, _ = solid_cells(rec, lo, n, 1)
    unknown = ~seen_known(seen, min_views, solid)
    p = seen_centres(lo, n, v)[unknown.reshape(-1)]
    out = np.zeros(len(T), GAIN_DTYPE)
    info = dict.fromkeys(GAIN_INFO_KEYS, 0)
    info.update(poses=len(T), cells=int(unknown.size), unknown=int(unknown.sum()))
    idx = [i for i, g in enumerate(good) if g]
    for a in range(0, len(idx), 64):
        part = idx[a:a + 64]
        cast = raycast_records(rec, v, [(T[i], k, size) for i in part], 1, max_steps)
        info["rays"] += cast["info"]["rays"]
        for i, D, hits in zip(part, cast["depth"], cast["hits"]):
            if miss != 0:
                D = np.where(D == 0, miss, D)
            cls = carve_classes(p, carve_view(D, T[i], k), int(radius), margin, margin_rel)
            out[i] = (int((cls == 2).sum()), int((cls == 3).sum()), int((cls != 0).sum()), hits, (0, 0, 0, 0))
    for name, field in (("unknown_free", "unknown_free"), ("unknown_surface", "unknown_surface"), ("unknown_inside", "unknown_inside"), ("ray_hits", "hits")):
        info[name] = int(out[field].sum(dtype=np.uint64))
    return gain_result(out, info)


def next_view_poses(cells, voxel, headings=8, up=(0.0, -1.0, 0.0)):
    """[len(cells) * headings, 4, 4] float32 camera -> world poses: at the centre of every cell (absolute voxel indices), `headings`
    yaws 2 pi j / headings about `up`.  The camera looks along its +z with its image's y axis pointing against `up`; yaw 0 looks
    along the world's +z made perpendicular to `up` (the world's +x where `up` is within 0.1 of the z axis).  Computed in
    float64 and rounded once."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    headings = int(headings)
    u = np.asarray(up, np.float64).reshape(3)
    if headings < 1 or not np.all(np.isfinite(u)) or not np.linalg.norm(u) > 0:
        raise ValueError("headings must be >= 1 and up a finite direction")
    u = u / np.linalg.norm(u)
    ref = np.array([0.0, 0.0, 1.0]) if abs(u[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    f0 = ref - ref.dot(u) * u
    f0 /= np.linalg.norm(f0)
    s0 = np.cross(u, f0)
    T = np.zeros((len(cells), headings, 4, 4), np.float64)
    for j in range(headings):
        th = 2.0 * np.pi * j / headings
        z = np.cos(th) * f0 + np.sin(th) * s0
        y = -u
        T[:, j, :3, 0], T[:, j, :3, 1], T[:, j, :3, 2] = np.cross(y, z), y, z
    T[:, :, :3, 3] = (((cells.astype(np.float32) + np.float32(0.5)) * np.float32(voxel)).astype(np.float64))[:, None, :]
    T[:, :, 3, 3] = 1.0
    return T.reshape(-1, 4, 4).astype(np.float32)


def next_view_candidates(cost, lo, stride=4, headings=8, max_candidates=1024):
    """[k, 3] int64 absolute voxel indices: the reachable cells of a cost field (cost != PLAN_NONE) whose absolute index is a
    multiple of `stride` on every axis, in ascending order of the cell's place in the box, at most max_candidates // headings."""
    stride, headings = int(stride), int(headings)
    if stride < 1 or headings < 1 or int(max_candidates) < headings:
        raise ValueError("stride and headings must be >= 1 and max_candidates at least one position's headings")
    lo = np.asarray(lo, np.int64).reshape(3)
    c = np.argwhere(np.asarray(cost) != PLAN_NONE) + lo
    c = c[np.all(c % stride == 0, axis=1)]
    return c[:int(max_candidates) // headings]


def next_view_choice(gain, cost_at, voxel, headings, weight=1.0):
    """(scores float64 [poses], best index): unknown_free / (1 + weight * metres) with metres = cost * voxel / 3 of the pose's
    position; the best is the first of the largest."""
    metres = np.repeat(np.asarray(cost_at, np.float64), int(headings)) * float(np.float32(voxel)) / 3.0
    scores = np.asarray(gain["unknown_free"], np.float64) / (1.0 + float(weight) * metres)
    return scores, int(np.argmax(scores))


def next_view_records(records, voxel, lo, n, seen, start, clearance, view, headings=8, up=(0.0, -1.0, 0.0), stride=4, max_candidates=1024,
                      weight=1.0, min_count=1, max_len=4096, **gain_params):
    """Where to look next, without a GPU: the known field of `seen`, the cost-to-go from `start` (a voxel index; the
    plan with `start` as its only seed) at the clearance (metres), the candidate positions next_view_candidates picks from it,
    `headings` yaws at each, their view gain, and the best score -> dict: pose (4x4), cell, heading, record, index, scores,
    poses, cells, gain (GainRecords), cost, path ((cells, status, cost) from the position back to `start`).  ValueError when no
    candidate is reachable."""
    lo, n = check_box(lo, n)
    min_views = gain_params.get("min_views", 1)
    d2, _ = known_field_records(records, lo, n, seen, min_count, 0, min_views)
    cost, pinfo = plan_records(d2, lo, n, plan_seeds(np.asarray(start, np.int64).reshape(1, 3)), plan_r2(clearance, voxel))
    cells = next_view_candidates(cost, lo, stride, headings, max_candidates)
    if len(cells) == 0:
        raise ValueError("no candidate position is reachable from the start (%d seeds used, %d cells reachable)" % (pinfo["seeds_used"], pinfo["reachable"]))
    poses = next_view_poses(cells, voxel, headings, up)
    gain = gain_records(records, voxel, lo, n, seen, view, poses, min_count=min_count, **gain_params)
    at = tuple((cells - lo).T)
    scores, best = next_view_choice(gain, cost[at], voxel, headings, weight)
    cell = cells[best // int(headings)]
    return {"pose": poses[best], "cell": cell.astype(np.int32), "heading": best % int(headings), "record": gain[best], "index": best, "scores": scores,
            "poses": poses, "cells": cells.astype(np.int32), "gain": gain, "cost": cost, "path": plan_paths(cost, lo, n, cell.reshape(1, 3), max_len)[0]}


def read_poses(path):
    """[k, 4, 4] float32: one pose per line of a text file, 16 or 12 numbers each (a row-major 4x4 or 3x4); '#' starts a comment."""
    out = []
    with open(path) as f:
        for ln in f:
            a = [float(x) for x in ln.split("#")[0].replace(",", " ").split()]
            if not a:
                continue
            if len(a) not in (12, 16):
                raise ValueError("%s: a line holds %d numbers; a pose is 16 (4x4) or 12 (3x4), row-major" % (path, len(a)))
            out.append(_pose_matrix(np.float32(a).reshape(-1, 4)))
    if not out:
        raise ValueError("%s holds no pose" % path)
    return np.stack(out)


def write_seen(path, seen, lo, voxel):
    """The .npz of a seen volume: seen (uint8 [n0, n1, n2]), lo, n (int32 [3]), voxel (float32)."""
    seen = np.ascontiguousarray(seen, np.uint8)
    with open(path, "wb") as f:
        np.savez(f, seen=seen, lo=np.asarray(lo, np.int32).reshape(3), n=np.asarray(seen.shape, np.int32), voxel=np.float32(voxel))
    return path


def read_seen(path):
    """(seen, lo, voxel) of a file write_seen wrote; ValueError if its arrays do not fit together."""
    with np.load(path) as z:
        if not all(k in z.files for k in ("seen", "lo", "n", "voxel")):
            raise ValueError("%s is not a seen-volume file (seen, lo, n, voxel)" % path)
        seen, lo, n, voxel = z["seen"], z["lo"], z["n"], z["voxel"]
    if seen.dtype != np.uint8 or seen.ndim != 3 or lo.shape != (3,) or list(seen.shape) != [int(x) for x in n]:
        raise ValueError("%s: a seen volume is a 3-D uint8 array of the shape its n states" % path)
    check_box(lo, n)
    return seen, lo.astype(np.int32), float(np.float32(voxel))


def _seen_for(path, voxel):
    """The seen volume of a file for a map of edge `voxel`."""
    seen, lo, v = read_seen(path)
    if np.float32(v).tobytes() != np.float32(voxel).tobytes():
        raise ValueError("%s was observed at voxels of %g m, the map has %g m" % (path, v, voxel))
    return seen, lo, np.asarray(seen.shape, np.int64)


def observe_file(path, views_dir, camera, zrange, depth_scale=5000.0, pad=0, **params):
    """(seen, lo, voxel, info) of the views of a `run_tum --map-views` folder over the bounds of the file's map grown by `pad`
    cells; more than 64 views accumulate in parts of 64."""
    header, rec = read(path)
    views = read_views(views_dir, camera, zrange, depth_scale)
    lo, hi, _ = bounds_records(rec)
    lo, n = padded_box(lo, hi, pad)
    seen, info = None, None
    for i in range(0, len(views), 64):
        seen, part, _ = observe_records(header["voxel"], lo, n, views[i:i + 64], seen=seen, **params)
        info = part if info is None else dict(part, votes=info["votes"] + part["votes"], newly_known=info["newly_known"] + part["newly_known"])
    return seen, lo.astype(np.int32), header["voxel"], info


TSDF_CELL_DTYPE = np.dtype([("sum", "<i4"), ("weight", "<u4")])  # revo_map_tsdf_cell
TSDF_INFO_KEYS = ("cells", "updates", "cells_weighted", "cells_inside", "saturated")
TSDF_COLOR_DTYPE = np.dtype([("sum_b", "<u4"), ("sum_g", "<u4"), ("sum_r", "<u4"), ("weight", "<u4")])  # revo_map_tsdf_color
TSDF_COLOR_INFO_KEYS = ("color_updates", "cells_colored")
MESH_INFO_KEYS = ("cells", "valid", "inside", "cubes", "cubes_active", "vertices", "triangles")
TSDF_W_MAX = 1 << 20
# the Kuhn tetrahedra of a cube: the corner numbers (dx + 2 dy + 4 dz) of v0 .. v3, per permutation of (x, y, z) in lexicographic order
TSDF_TETRA = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
# bit `case` (bit i of the case: v_i inside): the case's triangles are listed with their last two vertices swapped
TSDF_SWAP = (0x4D24, 0x32DA, 0x32DA, 0x4D24, 0x4D24, 0x32DA)


def tsdf_trunc(voxel, trunc=None):
    """The truncation distance a fuse runs with, checked as revo_map_tsdf_fuse checks it (None: 4 x the voxel edge) -> float32."""
    t = np.float32(4.0) * np.float32(voxel) if trunc is None else np.float32(trunc)
    if not (np.isfinite(t) and t > 0):
        raise ValueError("trunc must be finite and > 0")
    return t


def _tsdf_volume(cells, n=None):
    cells = np.asarray(cells)
    if cells.dtype != TSDF_CELL_DTYPE or cells.ndim != 3 or (n is not None and cells.shape != tuple(int(x) for x in n)):
        raise ValueError("a TSDF volume is a 3-D array of (sum int32, weight uint32) cells of the box's shape")
    return cells


def _tsdf_color_volume(color, shape):
    color = np.asarray(color)
    if color.dtype != TSDF_COLOR_DTYPE or color.shape != tuple(int(x) for x in shape):
        raise ValueError("a colour volume is a 3-D array of (sum_b, sum_g, sum_r, weight uint32) cells of the TSDF volume's shape")
    return color


def tsdf_bgr_images(views, bgr):
    """The colour images of a fuse's checked views (carve_view), checked as revo_map_tsdf_fuse_color checks them: one [h, w, 3]
    uint8 image per view, of the view's size."""
    bgr = list(bgr)
    if len(bgr) != len(views):
        raise ValueError("a colour fuse takes one colour image per view")
    out = []
    for i, (vw, im) in enumerate(zip(views, bgr)):
        if im is None:
            raise ValueError("view %d: a raw view needs a colour image" % i)
        im = np.asarray(im)
        if im.dtype != np.uint8 or im.shape != vw[0].shape + (3,):
            raise ValueError("view %d: a colour image is [h, w, 3] uint8 of the depth image's size" % i)
        out.append(np.ascontiguousarray(im).reshape(-1, 3))
    return out


def tsdf_records(voxel, lo, n, views, trunc=None, tsdf=None, chunk=1 << 20, bgr=None, color=None):
    """The TSDF volume without a GPU: revo_map_tsdf_fuse's contract in vectorised numpy, through carve_classes at
    radius 0 with margin = trunc.  views: as carve_records takes them; tsdf: a volume to accumulate into (it is not changed),
    None for a fresh one.  -> (cells TSDF_CELL_DTYPE [n0, n1, n2], info dict of TSDF_INFO_KEYS, one dict of CARVE_CLASSES counts
    per view).  ValueError as the library's REVO_ERR_INVALID_ARG.
    bgr: one [h, w, 3] uint8 colour image per view -- revo_map_tsdf_fuse_color's contract; color: the colour volume to
    accumulate into beside tsdf.  -> (cells, info, counts, colour cells TSDF_COLOR_DTYPE, dict of TSDF_COLOR_INFO_KEYS)."""
    lo, n = check_box(lo, n)
    trunc = tsdf_trunc(voxel, trunc)
    views, _, _, _ = carve_rule_args(voxel, views, 0, trunc, 0.0)
    shape = tuple(int(x) for x in n)
    before = np.zeros(shape, TSDF_CELL_DTYPE) if tsdf is None else _tsdf_volume(tsdf, n)
    if bgr is None and color is not None:
        raise ValueError("a colour volume is accumulated into with colour images")
    if bgr is not None:
        images = tsdf_bgr_images(views, bgr)
        if (tsdf is None) != (color is None):
            raise ValueError("a colour fuse accumulates into both volumes or into none")
        cbefore = np.zeros(shape, TSDF_COLOR_DTYPE) if color is None else _tsdf_color_volume(color, shape)
        csum = np.stack([cbefore[k].reshape(-1).astype(np.int64) for k in ("sum_b", "sum_g", "sum_r")], 1)
        cw = cbefore["weight"].reshape(-1).astype(np.int64)
        color_updates = 0
    p = seen_centres(lo, n, voxel)
    s = before["sum"].reshape(-1).astype(np.int64)
    w = before["weight"].reshape(-1).astype(np.int64)
    counts = [dict.fromkeys(CARVE_CLASSES, 0) for _ in views]
    updates = saturated = 0
    for a in range(0, len(p), int(chunk)):
        sl = slice(a, a + int(chunk))
        for vi, (vw, cnt) in enumerate(zip(views, counts)):  # in their order: a full weight drops the later ones
            cls, z, dc, pix = carve_classes(p[sl], vw, 0, trunc, np.float32(0), depths=True, pixels=True)
            with np.errstate(all="ignore"):
                q = np.rint(((dc - z) / trunc) * np.float32(1024))
            q = np.where(cls == 2, 1024, np.where(cls == 3, q, 0)).astype(np.int64)
            hit = (cls == 2) | (cls == 3)
            full = w[sl] >= TSDF_W_MAX
            take = hit & ~full
            s[sl] += np.where(take, q, 0)
            w[sl] += take
            updates += int(take.sum())
            saturated += int((hit & full).sum())
            if bgr is not None:  # the colour update goes with a CONFIRMED update that took place
                took = np.nonzero(take & (cls == 3))[0]
                csum[sl][took] += images[vi][pix[took]]
                cw[sl][took] += 1
                color_updates += len(took)
            for i, name in enumerate(CARVE_CLASSES):
                cnt[name] += int((cls == i).sum())
    out = np.zeros(shape, TSDF_CELL_DTYPE)
    out["sum"], out["weight"] = s.reshape(shape), w.reshape(shape)
    info = {"cells": int(out.size), "updates": updates, "cells_weighted": int((w > 0).sum()), "cells_inside": int(((w > 0) & (s < 0)).sum()),
            "saturated": saturated}
    if bgr is not None:
        cout = np.zeros(shape, TSDF_COLOR_DTYPE)
        for k, name in enumerate(("sum_b", "sum_g", "sum_r")):
            cout[name] = csum[:, k].reshape(shape)
        cout["weight"] = cw.reshape(shape)
        return out, info, counts, cout, {"color_updates": color_updates, "cells_colored": int((cw > 0).sum())}
    return out, info, counts


TSDF_UNFUSE_INFO_KEYS = ("cells", "updates", "cells_weighted", "cells_inside", "misfits", "color_updates", "cells_colored")


class TsdfUnfuseRefused(ValueError):
    """An unfuse that was refused (the library's REVO_ERR_INVALID_ARG for cells that do not FIT): nothing was changed.  misfits:
    how many cells; info: the dict of TSDF_UNFUSE_INFO_KEYS, the volumes as they stand."""

    def __init__(self, misfits, info=None, counts=None):
        super().__init__("%d cells do not fit: a view that is not in them, a full weight, or sums no fuse can reach" % misfits)
        self.misfits = int(misfits)
        self.info = info
        self.counts = counts  # one dict of CARVE_CLASSES counts per view: the fuse's, refused or not


def tsdf_unfuse_records(cells, color, lo, voxel, views, trunc=None, bgr=None, chunk=1 << 20):
    """Views taken out of a TSDF volume again without a GPU: revo_map_tsdf_unfuse's contract per cell, from
    tsdf_records' pieces (carve_classes at radius 0 with margin = trunc, the same quantum).  cells: the volume of the box at lo;
    color: its colour volume or None (bgr: one image per view, given exactly with a colour volume); trunc: what the views were
    fused with (None or 0: 4 x the voxel edge).  All or nothing: -> (cells', color', info dict of TSDF_UNFUSE_INFO_KEYS, one dict of
    CARVE_CLASSES counts per view), the inputs unchanged; TsdfUnfuseRefused, carrying `misfits`, when a cell does not FIT;
    ValueError as the library's other REVO_ERR_INVALID_ARG."""
    cells = _tsdf_volume(cells)
    lo, n = check_box(lo, cells.shape)
    trunc = tsdf_trunc(voxel, None if trunc is None or trunc == 0 else trunc)
    views, _, _, _ = carve_rule_args(voxel, views, 0, trunc, 0.0)
    if (color is None) != (bgr is None):
        raise ValueError("a colour volume is unfused with colour images, and only with them")
    if color is not None:
        color = _tsdf_color_volume(color, cells.shape)
        images = tsdf_bgr_images(views, bgr)
        cs = np.stack([color[k].reshape(-1).astype(np.int64) for k in ("sum_b", "sum_g", "sum_r")], 1)
        cw = color["weight"].reshape(-1).astype(np.int64)
    p = seen_centres(lo, n, voxel)
    s = cells["sum"].reshape(-1).astype(np.int64)
    w = cells["weight"].reshape(-1).astype(np.int64)
    k, kc, Q = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
    C3 = np.zeros((len(p), 3), np.int64)
    counts = [dict.fromkeys(CARVE_CLASSES, 0) for _ in views]
    for a in range(0, len(p), int(chunk)):
        sl = slice(a, a + int(chunk))
        for vi, (vw, cnt) in enumerate(zip(views, counts)):
            cls, z, dc, pix = carve_classes(p[sl], vw, 0, trunc, np.float32(0), depths=True, pixels=True)
            with np.errstate(all="ignore"):
                q = np.rint(((dc - z) / trunc) * np.float32(1024))
            Q[sl] += np.where(cls == 2, 1024, np.where(cls == 3, q, 0)).astype(np.int64)
            k[sl] += (cls == 2) | (cls == 3)
            kc[sl] += cls == 3
            if color is not None:
                took = np.nonzero(cls == 3)[0]
                C3[sl][took] += images[vi][pix[took]]
            for i, name in enumerate(CARVE_CLASSES):
                cnt[name] += int((cls == i).sum())
    w1, s1 = w - k, s - Q
    fits = (w < TSDF_W_MAX) & (w1 >= 0) & (np.abs(s1) <= 1024 * w1)
    if color is not None:
        c1, cs1 = cw - kc, cs - C3
        fits &= (c1 >= 0) & np.all(cs1 >= 0, axis=1) & (c1 <= w1) & np.all(cs1 <= 255 * c1[:, None], axis=1)
    hit = k > 0
    misfits = int((hit & ~fits).sum())
    if misfits:
        info = {"cells": int(cells.size), "updates": 0, "cells_weighted": int((w > 0).sum()), "cells_inside": int(((w > 0) & (s < 0)).sum()),
                "misfits": misfits, "color_updates": 0, "cells_colored": 0 if color is None else int((cw > 0).sum())}
        raise TsdfUnfuseRefused(misfits, info, counts)
    w1, s1 = np.where(hit, w1, w), np.where(hit, s1, s)
    out = np.zeros(cells.shape, TSDF_CELL_DTYPE)
    out["sum"], out["weight"] = s1.reshape(cells.shape), w1.reshape(cells.shape)
    info = {"cells": int(cells.size), "updates": int(k.sum()), "cells_weighted": int((w1 > 0).sum()), "cells_inside": int(((w1 > 0) & (s1 < 0)).sum()),
            "misfits": 0, "color_updates": 0, "cells_colored": 0}
    cout = None
    if color is not None:
        c1, cs1 = np.where(hit, c1, cw), np.where(hit[:, None], cs1, cs)
        cout = np.zeros(cells.shape, TSDF_COLOR_DTYPE)
        for i, name in enumerate(("sum_b", "sum_g", "sum_r")):
            cout[name] = cs1[:, i].reshape(cells.shape)
        cout["weight"] = c1.reshape(cells.shape)
        info["color_updates"], info["cells_colored"] = int(kc.sum()), int((c1 > 0).sum())
    return out, cout, info, counts


def tsdf_unfuse_many_records(jobs):
    """revo_map_tsdf_unfuse_many's contract without a GPU: per job, tsdf_unfuse_records for that job alone, with a
    refusal captured as that job's result instead of raised -- every other job is applied all the same.  A job is a dict: cells,
    lo, voxel, view (one view as tsdf_unfuse_records takes them) and optionally color with bgr (the view's image) and trunc.
    -> one dict per job: cells and color (the inputs themselves for a refused job: no byte changed), info (the dict of
    TSDF_UNFUSE_INFO_KEYS; a refused job's is the refusal's), counts (the view's CARVE_CLASSES counts, refused or not) and status
    (0, or -1, the library's REVO_ERR_INVALID_ARG, for a refused job).  ValueError as the library's argument errors: the call as
    a whole, before any job's result."""
    jobs = list(jobs)
    if not 1 <= len(jobs) <= 1024:
        raise ValueError("1 .. 1024 jobs")
    out = []
    for job in jobs:
        color, bgr = job.get("color"), job.get("bgr")
        if color is None and bgr is not None:
            raise ValueError("bgr goes with a colour volume")
        args = (job["cells"], color, job["lo"], job["voxel"], [tuple(job["view"])], job.get("trunc"))
        try:
            cells, col, info, counts = tsdf_unfuse_records(*args, bgr=None if color is None else [bgr])
            out.append({"cells": cells, "color": col, "info": info, "counts": counts[0], "status": 0})
        except TsdfUnfuseRefused as e:
            out.append({"cells": job["cells"], "color": color, "info": e.info, "counts": e.counts[0], "status": -1})
    return out


def tsdf_unfuse_file(path, views_dir, camera, zrange, depth_scale=5000.0, only=None):
    """(cells, lo, voxel, trunc, info, colour cells or None) of a saved volume with views of a `run_tum --map-views` /
    `--surface-views` folder taken out again (only: the indices of the views to take, default all; more than 64 go in parts of
    64, each part all or nothing).  A volume with colour takes the folder's rgb/ images too."""
    cells, lo, voxel, trunc, col = read_tsdf(path, color=True)
    views = read_views(views_dir, camera, zrange, depth_scale, color=col is not None)
    if only is not None:
        bad = [i for i in only if not 0 <= int(i) < len(views)]
        if bad:
            raise ValueError("the folder holds %d views: there is no view %s" % (len(views), ", ".join(str(i) for i in bad)))
        views = [views[int(i)] for i in only]
    if not views:
        raise ValueError("no view to take out")
    info = None
    for i in range(0, len(views), 64):
        part = views[i:i + 64]
        cells, col, pinfo, _ = tsdf_unfuse_records(cells, col, lo, voxel, [v[:3] for v in part], trunc,
                                                   bgr=[v[3] for v in part] if col is not None else None)
        if info is not None:
            pinfo = dict(pinfo, **{k: info[k] + pinfo[k] for k in ("updates", "color_updates")})
        info = pinfo
    return cells, lo, voxel, trunc, info, col


def tsdf_sdf(cells, trunc):
    """The signed distance in metres, float64 [n0, n1, n2]: sum / weight * trunc / 1024, NaN where the weight is 0."""
    cells = _tsdf_volume(cells)
    with np.errstate(all="ignore"):
        return np.where(cells["weight"] > 0, cells["sum"].astype(np.float64) / cells["weight"] * float(np.float32(trunc)) / 1024.0, np.nan)


class Mesh:
    """A triangle mesh (revo_map_tsdf_mesh, mesh_records): vertices [V, 3] float32 metres, triangles [T, 3] uint32 vertex
    indices, both in the contract's canonical order; info: the call's counts (MESH_INFO_KEYS), None for a loaded mesh.
    normals: None or [V, 3] float32 unit normals, colors: None or [V, 4] uint8 B, G, R, k (revo_map_tsdf_mesh_attr)."""

    def __init__(self, vertices, triangles, info=None, normals=None, colors=None):
        self.vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
        self.triangles = np.asarray(triangles, np.uint32).reshape(-1, 3)
        self.info = info
        self.normals = None if normals is None else np.asarray(normals, np.float32).reshape(-1, 3)
        self.colors = None if colors is None else np.asarray(colors, np.uint8).reshape(-1, 4)
        for a in (self.normals, self.colors):
            if a is not None and len(a) != len(self.vertices):
                raise ValueError("a mesh has one normal and one colour per vertex")

    def save_ply(self, path):
        from . import ply
        return ply.write_mesh_ply(path, self.vertices, self.triangles, self.normals, self.colors)

    @classmethod
    def load_ply(cls, path):
        from . import ply
        v, t, normals, colors = ply.read_mesh_ply(path, attributes=True)
        return cls(v, t, None, normals, colors)


def _tsdf_case_triangles(case):
    """The triangles of a case (bit i: v_i inside) as edges (i, j), i < j, before the swap."""
    ins = [i for i in range(4) if (case >> i) & 1]
    out = [i for i in range(4) if not (case >> i) & 1]
    e = lambda a, b: (min(a, b), max(a, b))  # noqa: E731
    if len(ins) in (0, 4):
        return []
    if len(ins) in (1, 3):
        a = ins[0] if len(ins) == 1 else out[0]
        b, c, d = [i for i in range(4) if i != a]
        return [(e(a, b), e(a, c), e(a, d))]
    (a, b), (c, d) = ins, out
    return [(e(a, c), e(a, d), e(b, d)), (e(a, c), e(b, d), e(b, c))]


def mesh_records(cells, lo, voxel, min_weight=1, _edges=None):
    """The mesh of a TSDF volume without a GPU: revo_map_tsdf_mesh's contract in vectorised numpy -> Mesh.
    _edges: a dict that takes the vertices' edges (mesh_attr_records)."""
    cells = _tsdf_volume(cells)
    n = np.asarray(cells.shape, np.int64)
    lo, _ = check_box(lo, n)
    f32 = np.float32
    voxel = f32(voxel)
    mw = max(1, int(min_weight))
    s, w = cells["sum"].astype(np.int64), cells["weight"].astype(np.int64)
    valid = w >= mw
    inside = valid & (s < 0)
    info = dict.fromkeys(MESH_INFO_KEYS, 0)
    info.update(cells=int(cells.size), valid=int(valid.sum()), inside=int(inside.sum()), cubes=int(np.prod(n - 1)))
    off = lambda v: (v & 1, (v >> 1) & 1, (v >> 2) & 1)  # noqa: E731

    def shifted(a, d, fill=False):
        """a[c + d] where that is inside the box, `fill` elsewhere (d: an offset of -1 .. 1 per axis)."""
        out = np.full(a.shape, fill, a.dtype)
        src = tuple(slice(max(0, d[i]), a.shape[i] + min(0, d[i])) for i in range(3))
        dst = tuple(slice(max(0, -d[i]), a.shape[i] + min(0, -d[i])) for i in range(3))
        out[dst] = a[src]
        return out

    active = np.ones(cells.shape, bool)
    for v in range(8):
        active &= shifted(valid, off(v))
    info["cubes_active"] = int(active.sum())
    # the edges that carry a vertex: bit per type, in the order (cell, type)
    carries = np.zeros(cells.shape + (7,), bool)
    for t in range(7):
        d = t + 1
        owner = np.zeros(cells.shape, bool)
        for o in range(8):
            if not (o & d):
                owner |= shifted(active, tuple(-x for x in off(o)))
        carries[..., t] = (inside != shifted(inside, off(d))) & owner
    flat = carries.reshape(-1, 7)
    cell_i, type_i = np.nonzero(flat)
    index = np.cumsum(flat.reshape(-1)).reshape(-1, 7) - 1  # the vertex of (cell, type), where it has one
    ix, iy, iz = np.unravel_index(cell_i, cells.shape)
    d = type_i + 1
    dx, dy, dz = d & 1, (d >> 1) & 1, (d >> 2) & 1
    n0 = s[ix, iy, iz] * w[ix + dx, iy + dy, iz + dz]
    n1 = s[ix + dx, iy + dy, iz + dz] * w[ix, iy, iz]
    a = (n0.astype(np.float64) / (n0 - n1).astype(np.float64)).astype(f32)
    vertices = np.empty((len(cell_i), 3), f32)
    for axis, (c, along) in enumerate(((ix, dx), (iy, dy), (iz, dz))):
        vertices[:, axis] = (((int(lo[axis]) + c).astype(f32) + f32(0.5)) + np.where(along == 1, a, f32(0))) * voxel
    if _edges is not None:
        _edges.update(c0=(ix, iy, iz), d=(dx, dy, dz), a=a, valid=valid, shifted=shifted)
    # the triangles: per active cube (ascending place), tetrahedron and k
    cubes = np.nonzero(active.reshape(-1))[0]
    cx, cy, cz = np.unravel_index(cubes, cells.shape)
    place = lambda v: ((cx + off(v)[0]) * int(n[1]) + cy + off(v)[1]) * int(n[2]) + cz + off(v)[2]  # noqa: E731
    tri = np.zeros((len(cubes), 6, 2, 3), np.int64)
    have = np.zeros((len(cubes), 6, 2), bool)
    corner_in = [inside.reshape(-1)[place(v)] for v in range(8)]
    for k, tc in enumerate(TSDF_TETRA):
        case = sum(corner_in[tc[i]].astype(np.int64) << i for i in range(4))
        for code in range(1, 15):
            sel = np.nonzero(case == code)[0]
            if not len(sel):
                continue
            for j, t3 in enumerate(_tsdf_case_triangles(code)):
                if (TSDF_SWAP[k] >> code) & 1:
                    t3 = (t3[0], t3[2], t3[1])
                for q, (i0, i1) in enumerate(t3):
                    tri[sel, k, j, q] = index[place(tc[i0])[sel], (tc[i0] ^ tc[i1]) - 1]
                have[sel, k, j] = True
    triangles = tri[have].astype(np.uint32).reshape(-1, 3)
    info["vertices"], info["triangles"] = len(vertices), len(triangles)
    return Mesh(vertices, triangles, info)


def mesh_attr_records(tsdf, color, lo, voxel, min_weight=1):
    """mesh_records with the vertices' normals and colours: revo_map_tsdf_mesh_attr's contract in vectorised numpy,
    float32 operation by operation -> Mesh.  color: the colour volume, or None (then the mesh has no colours)."""
    f32 = np.float32
    e = {}
    m = mesh_records(tsdf, lo, voxel, min_weight, _edges=e)
    cells = _tsdf_volume(tsdf)
    valid, shifted = e["valid"], e["shifted"]
    (ix, iy, iz), (dx, dy, dz), a = e["c0"], e["d"], e["a"]
    with np.errstate(all="ignore"):
        f = np.where(valid, cells["sum"].astype(f32) / cells["weight"].astype(f32), f32(0)).astype(f32)
        grad = np.zeros(cells.shape + (3,), f32)
        for axis in range(3):
            dm, dp = [0, 0, 0], [0, 0, 0]
            dm[axis], dp[axis] = -1, 1
            vm, vp = shifted(valid, dm), shifted(valid, dp)
            fm, fp = shifted(f, dm, f32(0)), shifted(f, dp, f32(0))
            grad[..., axis] = np.where(vm & vp, (fp - fm) * f32(0.5), np.where(vp, fp - f, np.where(vm, f - fm, f32(0))))
        g0, g1 = grad[ix, iy, iz], grad[ix + dx, iy + dy, iz + dz]
        g = (g0 + a[:, None] * (g1 - g0)).astype(f32)
        l2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        ok = np.isfinite(l2) & (l2 > 0)
        m.normals = np.where(ok[:, None], g / np.sqrt(l2)[:, None], f32(0)).astype(f32).reshape(-1, 3)
        if color is not None:
            color = _tsdf_color_volume(color, cells.shape)
            cw = color["weight"]
            w0, w1 = cw[ix, iy, iz], cw[ix + dx, iy + dy, iz + dz]
            out = np.zeros((len(a), 4), np.uint8)
            for k, name in enumerate(("sum_b", "sum_g", "sum_r")):
                mean = color[name].astype(f32) / cw.astype(f32)
                m0, m1 = mean[ix, iy, iz], mean[ix + dx, iy + dy, iz + dz]
                v = np.where((w0 > 0) & (w1 > 0), m0 + a * (m1 - m0), np.where(w0 > 0, m0, np.where(w1 > 0, m1, f32(0)))).astype(f32)
                out[:, k] = np.rint(np.minimum(np.maximum(v, f32(0)), f32(255))).astype(np.uint8)
            out[:, 3] = (w0 > 0).astype(np.uint8) + (w1 > 0).astype(np.uint8)
            m.colors = out
    return m


def write_tsdf(path, cells, lo, voxel, trunc, color=None):
    """The .npz of a TSDF volume: sum (int32 [n0, n1, n2]), weight (uint32), lo, n (int32 [3]), voxel, trunc (float32); with a
    colour volume also color_sum (uint32 [n0, n1, n2, 3]: B, G, R) and color_weight (uint32)."""
    cells = _tsdf_volume(cells)
    extra = {}
    if color is not None:
        color = _tsdf_color_volume(color, cells.shape)
        extra = {"color_sum": np.stack([color[k] for k in ("sum_b", "sum_g", "sum_r")], -1), "color_weight": np.ascontiguousarray(color["weight"])}
    with open(path, "wb") as f:
        np.savez(f, sum=np.ascontiguousarray(cells["sum"]), weight=np.ascontiguousarray(cells["weight"]), lo=np.asarray(lo, np.int32).reshape(3),
                 n=np.asarray(cells.shape, np.int32), voxel=np.float32(voxel), trunc=np.float32(trunc), **extra)
    return path


def read_tsdf(path, color=False):
    """(cells, lo, voxel, trunc) of a file write_tsdf wrote; ValueError if its arrays do not fit together.  color: a fifth entry,
    the file's colour volume or None."""
    if color:
        base = read_tsdf(path)
        with np.load(path) as z:
            if "color_sum" not in z.files and "color_weight" not in z.files:
                return base + (None,)
            if not ("color_sum" in z.files and "color_weight" in z.files):
                raise ValueError("%s: a colour volume is color_sum and color_weight" % path)
            cs, cw = z["color_sum"], z["color_weight"]
        if cs.dtype != np.uint32 or cw.dtype != np.uint32 or cw.shape != base[0].shape or cs.shape != base[0].shape + (3,):
            raise ValueError("%s: a colour volume is a uint32 color_sum [n0, n1, n2, 3] and a uint32 color_weight" % path)
        col = np.zeros(cw.shape, TSDF_COLOR_DTYPE)
        col["sum_b"], col["sum_g"], col["sum_r"], col["weight"] = cs[..., 0], cs[..., 1], cs[..., 2], cw
        return base + (col,)
    with np.load(path) as z:
        if not all(k in z.files for k in ("sum", "weight", "lo", "n", "voxel", "trunc")):
            raise ValueError("%s is not a TSDF file (sum, weight, lo, n, voxel, trunc)" % path)
        s, w, lo, n, voxel, trunc = (z[k] for k in ("sum", "weight", "lo", "n", "voxel", "trunc"))
    if s.dtype != np.int32 or w.dtype != np.uint32 or s.ndim != 3 or s.shape != w.shape or lo.shape != (3,) or list(s.shape) != [int(x) for x in n]:
        raise ValueError("%s: a TSDF volume is an int32 sum and a uint32 weight of the shape its n states" % path)
    check_box(lo, n)
    cells = np.zeros(s.shape, TSDF_CELL_DTYPE)
    cells["sum"], cells["weight"] = s, w
    return cells, lo.astype(np.int32), float(np.float32(voxel)), float(tsdf_trunc(voxel, trunc))


def tsdf_file(path, views_dir, camera, zrange, depth_scale=5000.0, pad=0, trunc=None, color=False):
    """(cells, lo, voxel, trunc, info) of the views of a `run_tum --map-views` folder over the bounds of the file's map grown by
    `pad` cells; more than 64 views accumulate in parts of 64.  color: the folder's rgb/ images are fused too -> (cells, lo,
    voxel, trunc, info, colour cells); info then holds TSDF_COLOR_INFO_KEYS as well."""
    header, rec = read(path)
    views = read_views(views_dir, camera, zrange, depth_scale, color=color)
    lo, hi, _ = bounds_records(rec)
    lo, n = padded_box(lo, hi, pad)
    cells, info, col = None, None, None
    for i in range(0, len(views), 64):
        part_views = views[i:i + 64]
        if color:
            cells, part, _, col, cpart = tsdf_records(header["voxel"], lo, n, [v[:3] for v in part_views], trunc, tsdf=cells,
                                                       bgr=[v[3] for v in part_views], color=col)
            part = dict(part, **cpart)
        else:
            cells, part, _ = tsdf_records(header["voxel"], lo, n, part_views, trunc, tsdf=cells)
        if info is not None:
            part = dict(part, **{k: info[k] + part[k] for k in ("updates", "saturated", "color_updates") if k in part})
        info = part
    out = (cells, lo.astype(np.int32), header["voxel"], float(tsdf_trunc(header["voxel"], trunc)), info)
    return out + (col,) if color else out


# -------------------------------------------------------------------------------- views of the surface --
TSDF_RAY_STATUS = ("hit", "range", "backface", "exhausted")
TSDF_RAY_INFO_KEYS = ("rays", "hits", "range", "backface", "exhausted", "samples", "uncolored")
TSDF_RAY_MAX_STEPS = 1 << 20


def tsdf_ray_params(voxel, step=None, min_weight=1, max_steps=4096):
    """The parameters a surface ray cast runs with, checked as revo_map_tsdf_raycast checks them -> (step float32, min_weight,
    max_steps): step None or 0 is the voxel edge, min_weight 0 counts as 1, max_steps 0 is 4096."""
    v = np.float32(voxel)
    if not (np.isfinite(v) and v > 0):
        raise ValueError("the voxel edge must be finite and > 0")
    st = np.float32(0 if step is None else step)
    if not np.isfinite(st) or st < 0:
        raise ValueError("step must be finite and >= 0 (0: the voxel edge)")
    if not 0 <= int(max_steps) <= TSDF_RAY_MAX_STEPS:
        raise ValueError("max_steps must be 0 (4096) or 1 .. 2^20")
    if not 0 <= int(min_weight) < 1 << 32:
        raise ValueError("min_weight is a number of views >= 0")
    return (v if st == 0 else st), max(1, int(min_weight)), int(max_steps) or 4096


def _tsdf_ray_march(f, valid, lo, voxel, o, d, zmin, zmax, step, max_steps):
    """The plain march of revo_map_tsdf_raycast (include/revo_hip.h) for the N rays of one view at once, float32
    operation by operation: every ray still under way takes sample k in iteration k.  f, valid: the field and the validity of
    the cells; o, d [N, 3] float32.  -> dict of [N] arrays: status, k (the sample that ended the ray), and for the hits a, sp
    (the previous sample's depth), gp, g ([N, 3]: the two gradients), c0, c1 (the two colour cells' places)."""
    f32 = np.float32
    n = len(o)
    nx, ny, nz = f.shape
    ff, vv = f.reshape(-1), valid.reshape(-1)
    last = ff.size - 1
    out = {"status": np.full(n, 3, np.int64), "k": np.full(n, int(max_steps), np.int64), "a": np.zeros(n, f32), "sp": np.zeros(n, f32),
           "gp": np.zeros((n, 3), f32), "g": np.zeros((n, 3), f32), "c0": np.zeros(n, np.int64), "c1": np.zeros(n, np.int64)}
    centre = np.asarray(lo, np.int64).astype(f32) + f32(0.5)
    top = (np.asarray(f.shape, np.int64) - 2).astype(f32)
    offs = {(dx, dy, dz): (dx * ny + dy) * nz + dz for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
    L = lambda x0, x1, a: x0 + a * (x1 - x0)  # noqa: E731
    B = lambda v00, v01, v10, v11, r0, r1: L(L(v00, v01, r0), L(v10, v11, r0), r1)  # noqa: E731
    idx = np.arange(n)
    pv, pF, pS, pG, pC = np.zeros(n, bool), np.zeros(n, f32), np.zeros(n, f32), np.zeros((n, 3), f32), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for k in range(int(max_steps)):
            if not len(idx):
                break
            s = f32(zmin + f32(k) * step)
            if not s < zmax:  # every ray of a view shares its samples' depths
                out["status"][idx], out["k"][idx] = 1, k
                break
            g = o[idx] + s * d[idx]
            u = g / voxel - centre
            b = np.floor(u)
            r = (u - b).astype(f32)
            inbox = np.all(np.isfinite(u) & (b >= 0) & (b <= top), 1)
            bi = np.where(inbox[:, None], b, 0).astype(np.int64)
            c = (bi[:, 0] * ny + bi[:, 1]) * nz + bi[:, 2]
            at = {key: np.minimum(c + off, last) for key, off in offs.items()}
            val = inbox.copy()
            for a_ in at.values():
                val &= vv[a_]
            q = {key: ff[a_] for key, a_ in at.items()}
            rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
            F = L(B(q[0, 0, 0], q[0, 0, 1], q[0, 1, 0], q[0, 1, 1], rz, ry), B(q[1, 0, 0], q[1, 0, 1], q[1, 1, 0], q[1, 1, 1], rz, ry), rx)
            G = np.stack([B(q[1, 0, 0] - q[0, 0, 0], q[1, 0, 1] - q[0, 0, 1], q[1, 1, 0] - q[0, 1, 0], q[1, 1, 1] - q[0, 1, 1], rz, ry),
                          B(q[0, 1, 0] - q[0, 0, 0], q[0, 1, 1] - q[0, 0, 1], q[1, 1, 0] - q[1, 0, 0], q[1, 1, 1] - q[1, 0, 1], rz, rx),
                          B(q[0, 0, 1] - q[0, 0, 0], q[0, 1, 1] - q[0, 1, 0], q[1, 0, 1] - q[1, 0, 0], q[1, 1, 1] - q[1, 1, 0], ry, rx)], 1).astype(f32)
            near = bi + (r >= f32(0.5))
            cc = (near[:, 0] * ny + near[:, 1]) * nz + near[:, 2]
            both = val & pv
            hit = both & (pF >= 0) & (F < 0)
            back = both & (pF < 0) & (F >= 0)
            h = idx[hit]
            out["status"][h], out["k"][h] = 0, k
            out["a"][h] = pF[hit] / (pF[hit] - F[hit])
            out["sp"][h], out["gp"][h], out["g"][h], out["c0"][h], out["c1"][h] = pS[hit], pG[hit], G[hit], pC[hit], cc[hit]
            out["status"][idx[back]], out["k"][idx[back]] = 2, k
            go = ~(hit | back)
            idx, pv, pF, pS, pG, pC = idx[go], val[go], F[go].astype(f32), np.full(int(go.sum()), s, f32), G[go], cc[go]
    return out


def tsdf_raycast_records(tsdf, color, lo, voxel, views, step=None, min_weight=1, max_steps=4096):
    """Depth, normal and colour views of a TSDF volume without a GPU: revo_map_tsdf_raycast's contract in vectorised
    numpy.  tsdf: the volume; color: the colour volume or None (then no bgr comes back and uncolored is 0); lo: the box's first
    voxel index; views: a list of (T_w_c, (fx, fy, cx, cy, zmin, zmax), (width, height)), 1 .. 64.  -> a dict of per-view lists
    depth ([h, w] float32, 0 = miss), normals ([h, w, 3] float32), bgr ([h, w, 3] uint8, or None without a colour volume), hits,
    and -- beyond what the library returns -- status ([h, w]: the index into TSDF_RAY_STATUS), samples ([h, w]: the samples the
    ray counts) and colored ([h, w]: a hit's k), plus info: the call's TSDF_RAY_INFO_KEYS sums.  ValueError as the library's
    REVO_ERR_INVALID_ARG."""
    f32 = np.float32
    cells = _tsdf_volume(tsdf)
    lo, _ = check_box(lo, np.asarray(cells.shape, np.int64))
    if color is not None:
        color = _tsdf_color_volume(color, cells.shape)
    st, mw, ms = tsdf_ray_params(voxel, step, min_weight, max_steps)
    views = list(views)
    if not 1 <= len(views) <= 64:
        raise ValueError("a ray cast takes 1 .. 64 views")
    views = [ray_view(*vw) for vw in views]
    voxel = f32(voxel)
    valid = cells["weight"] >= mw
    with np.errstate(all="ignore"):
        f = np.where(valid, cells["sum"].astype(f32) / cells["weight"].astype(f32), f32(0)).astype(f32)
        if color is not None:
            cw = color["weight"].reshape(-1)
            mean = [(color[name].astype(f32) / color["weight"].astype(f32)).astype(f32).reshape(-1) for name in ("sum_b", "sum_g", "sum_r")]
    out = {k: [] for k in ("depth", "normals", "bgr", "hits", "status", "samples", "colored")}
    total = dict.fromkeys(TSDF_RAY_INFO_KEYS, 0)
    for vw in views:
        w, h = vw[5]
        o, _, d, _ = ray_view_rays(vw)
        m = _tsdf_ray_march(f, valid, lo, voxel, o, d, vw[4][4], vw[4][5], st, ms)
        status, k, a = m["status"], m["k"], m["a"]
        got = status == 0
        samples = np.where(got | (status == 2), k + 1, k)
        with np.errstate(all="ignore"):
            depth = np.where(got, m["sp"] + a * st, f32(0)).astype(f32)
            g = (m["gp"] + a[:, None] * (m["g"] - m["gp"])).astype(f32)
            l2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            ok = got & np.isfinite(l2) & (l2 > 0)
            normals = np.where(ok[:, None], g / np.sqrt(l2)[:, None], f32(0)).astype(f32)
            colored = np.zeros(len(a), np.int64)
            bgr = None
            if color is not None:
                w0, w1 = cw[m["c0"]], cw[m["c1"]]
                bgr = np.zeros((len(a), 3), np.uint8)
                for ch in range(3):
                    m0, m1 = mean[ch][m["c0"]], mean[ch][m["c1"]]
                    v = np.where((w0 > 0) & (w1 > 0), m0 + a * (m1 - m0), np.where(w0 > 0, m0, np.where(w1 > 0, m1, f32(0)))).astype(f32)
                    bgr[:, ch] = np.where(got, np.rint(np.minimum(np.maximum(v, f32(0)), f32(255))), 0).astype(np.uint8)
                colored = np.where(got, (w0 > 0).astype(np.int64) + (w1 > 0).astype(np.int64), 0)
        out["depth"].append(depth.reshape(h, w))
        out["normals"].append(normals.reshape(h, w, 3))
        out["bgr"].append(None if bgr is None else bgr.reshape(h, w, 3))
        out["hits"].append(int(got.sum()))
        out["status"].append(status.reshape(h, w))
        out["samples"].append(samples.reshape(h, w))
        out["colored"].append(colored.reshape(h, w))
        for i, name in enumerate(TSDF_RAY_STATUS):
            total[name if name != "hit" else "hits"] += int((status == i).sum())
        total["rays"] += len(status)
        total["samples"] += int(samples.sum())
        total["uncolored"] += int((got & (colored == 0)).sum()) if color is not None else 0
    out["info"] = total
    return out


def tsdf_raycast_many_records(jobs):
    """revo_map_tsdf_raycast_many's contract without a GPU: per job, tsdf_raycast_records for that job alone.  A job is a
    dict: cells, lo, voxel, views (1 .. 64, as tsdf_raycast_records takes them) and optionally color, step, min_weight and
    max_steps.  Jobs may share a volume: it is only read.  1 .. 1024 jobs with at most 4096 views between them.  -> one
    tsdf_raycast_records dict per job.  ValueError as the library's argument errors: the call as a whole, before any job's result."""
    jobs = list(jobs)
    if not 1 <= len(jobs) <= 1024:
        raise ValueError("1 .. 1024 jobs")
    views = [list(job["views"]) for job in jobs]
    if any(not 1 <= len(v) <= 64 for v in views):
        raise ValueError("a job takes 1 .. 64 views")
    if sum(len(v) for v in views) > 4096:
        raise ValueError("at most 4096 views in one call")
    for job, v in zip(jobs, views):  # every job's own rules first: the call is refused as a whole
        cells = _tsdf_volume(job["cells"])
        check_box(job["lo"], np.asarray(cells.shape, np.int64))
        if job.get("color") is not None:
            _tsdf_color_volume(job["color"], cells.shape)
        tsdf_ray_params(job["voxel"], job.get("step"), job.get("min_weight", 1), job.get("max_steps", 4096))
        for vw in v:
            ray_view(*vw)
    return [tsdf_raycast_records(job["cells"], job.get("color"), job["lo"], job["voxel"], v, job.get("step"), job.get("min_weight", 1),
                                 job.get("max_steps", 4096)) for job, v in zip(jobs, views)]


def df_sample(d2, lo, voxel, points):
    """revo_map_df_sample restated: a DF_SAMPLE_DTYPE array, one entry per point ([N, 3] float32 metres).  All arithmetic is
    float32, every operation rounded on its own.  dist -1: outside the box (or not finite); +inf: the cell holds DF_NONE."""
    F = np.float32
    d2 = np.asarray(d2, np.uint32)
    n = np.asarray(d2.shape, np.int64)
    lo = np.asarray(lo, np.int64).reshape(3)
    p = np.asarray(points, F).reshape(-1, 3)
    out = np.zeros(len(p), DF_SAMPLE_DTYPE)
    with np.errstate(all="ignore"):
        f = np.floor(p / F(voxel))
        inside = np.all(np.isfinite(p) & np.isfinite(f) & (f >= lo.astype(F)) & (f <= (lo + n - 1).astype(F)), axis=1)
        a = np.where(inside[:, None], f, lo.astype(F)).astype(np.int64) - lo
        v = d2[a[:, 0], a[:, 1], a[:, 2]]
        none = v == DF_NONE
        root = np.sqrt(d2.astype(F))
        dist = root[a[:, 0], a[:, 1], a[:, 2]] * F(voxel)
        out["dist"] = np.where(inside, np.where(none, F(np.inf), dist), F(-1))
        for i in range(3):
            lo_, hi_ = a.copy(), a.copy()
            lo_[:, i] = np.maximum(a[:, i] - 1, 0)
            hi_[:, i] = np.minimum(a[:, i] + 1, n[i] - 1)
            span = hi_[:, i] - lo_[:, i]
            diff = root[hi_[:, 0], hi_[:, 1], hi_[:, 2]] - root[lo_[:, 0], lo_[:, 1], lo_[:, 2]]
            grad = np.where(span == 0, F(0), diff / np.maximum(span, 1).astype(F))
            out["grad"][:, i] = np.where(inside & ~none, grad, F(0))
    return out


DF_ALIGN_DTYPE = np.dtype([("S", "<f4", (28,)), ("matched", "<u8"), ("considered", "<u8"), ("skipped", "<u8"), ("centre", "<f4", (3,)),
                           ("max_dist", "<f4"), ("R", "<f4", (9,)), ("T", "<f4", (3,)), ("flags", "<i4"), ("reserved", "<i4")])
ALIGN_CONVERGED, ALIGN_ITER_LIMIT, ALIGN_LOST = 0, 1, 2
assert DF_ALIGN_DTYPE.itemsize == 208


def sum_exact_f32(terms):
    """The float32 nearest the exact sum of float32 terms, ties to even: what a record's S holds.  math.fsum gives the double
    nearest the exact sum; only when that double is the midpoint of two adjacent floats can the second rounding go wrong, and
    then rational arithmetic decides."""
    import math
    from fractions import Fraction
    t = np.asarray(terms, np.float32).astype(np.float64).tolist()
    d = math.fsum(t) + 0.0  # an empty or all-zero sum is +0
    f = np.float32(d)
    if float(f) == d or not math.isfinite(d):
        return f
    g = np.nextafter(f, np.float32(math.inf if d > float(f) else -math.inf))
    if d != (float(f) + float(g)) / 2.0:
        return f
    exact, mid = sum((Fraction(x) for x in t), Fraction(0)), Fraction(d)
    lo_, hi_ = (f, g) if float(f) < float(g) else (g, f)
    if exact != mid:
        return lo_ if exact < mid else hi_
    return lo_ if (int(lo_.view(np.uint32)) & 1) == 0 else hi_


def df_align_terms(d2, lo, voxel, points, T, max_dist, centre):
    """The per-point part of revo_map_df_align_eval at one pose T (4x4 float32, finite, orthogonal), float32 with every
    operation rounded on its own -> (the 28 float32 term arrays of the accepted points, matched, skipped)."""
    F = np.float32
    d2 = np.asarray(d2, np.uint32)
    n = np.asarray(d2.shape, np.int64)
    lo = np.asarray(lo, np.int64).reshape(3)
    p = np.asarray(points, F).reshape(-1, 3)
    T = np.asarray(T, F)
    v, c = F(voxel), np.asarray(centre, F).reshape(3)
    with np.errstate(all="ignore"):
        pt = np.stack([((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3] for i in range(3)], 1).astype(F).reshape(-1, 3)
        g = (pt / v - F(0.5)).astype(F)
        f = np.floor(g)
        w = (g - f).astype(F)
        a = (f - lo.astype(F)).astype(F)
        ok = np.all(np.isfinite(pt) & np.isfinite(g) & (a >= F(0)) & (a <= (n - 2).astype(F)), axis=1)
    idx = np.flatnonzero(ok)
    a, w, pt = a[idx].astype(np.int64), w[idx], pt[idx]
    corner = {(i, j, k): d2[a[:, 0] + i, a[:, 1] + j, a[:, 2] + k] for i in (0, 1) for j in (0, 1) for k in (0, 1)}
    some = np.zeros(len(idx), bool)
    for q in corner.values():
        some |= q == DF_NONE
    keep = ~some
    w, pt = w[keep], pt[keep]
    s = {k: np.sqrt(q[keep].astype(F)) for k, q in corner.items()}
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    lerp = lambda x0, x1, t: x0 + t * (x1 - x0)  # noqa: E731
    m = {(i, j): lerp(s[i, j, 0], s[i, j, 1], wz) for i in (0, 1) for j in (0, 1)}
    dz = {(i, j): s[i, j, 1] - s[i, j, 0] for i in (0, 1) for j in (0, 1)}
    l_ = [lerp(m[i, 0], m[i, 1], wy) for i in (0, 1)]
    h_ = [m[i, 1] - m[i, 0] for i in (0, 1)]
    k_ = [lerp(dz[i, 0], dz[i, 1], wy) for i in (0, 1)]
    cc = lerp(l_[0], l_[1], wx)
    gx, gy, gz = l_[1] - l_[0], lerp(h_[0], h_[1], wx), lerp(k_[0], k_[1], wx)
    e = cc * v
    acc = e <= F(max_dist)
    pt, e, gx, gy, gz = pt[acc], e[acc], gx[acc], gy[acc], gz[acc]
    u = pt - c
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    J = [gx, gy, gz, uy * gz - uz * gy, uz * gx - ux * gz, ux * gy - uy * gx]
    terms = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * e for i in range(6)] + [e * e]
    assert all(t.dtype == F for t in terms)
    return terms, int(acc.sum()), int(len(p) - len(keep) + some.sum())


def df_align_records(d2, lo, n, voxel, points, poses, max_dist, centre):
    """revo_map_df_align_eval restated: a DF_ALIGN_DTYPE array, one record per pose (4x4, or [N, 4, 4]), of the
    points ([N, 3] float32, source frame) against the field d2 (uint32, shape n) of the box at lo with the edge `voxel`."""
    F = np.float32
    lo, n = check_box(lo, n)
    d2 = np.asarray(d2, np.uint32).reshape(tuple(int(x) for x in n))
    p = np.asarray(points, F).reshape(-1, 3)
    md, c = F(max_dist), np.asarray(centre, F).reshape(3)
    if not (np.isfinite(md) and md > 0) or not np.all(np.isfinite(c)):
        raise ValueError("max_dist must be finite and > 0, the centre finite")
    if not 1 <= len(p) <= 1 << 24:
        raise ValueError("1 .. 2^24 points")
    Ts = np.asarray(poses, F).reshape(-1, 4, 4)
    out = np.zeros(len(Ts), DF_ALIGN_DTYPE)
    for r, T in zip(out, Ts):
        r["centre"], r["max_dist"] = c, md
        r["R"], r["T"] = np.ascontiguousarray(T[:3, :3].T).reshape(9), T[:3, 3]  # column-major, as given (a NaN keeps its bits)
        if not np.all(np.isfinite(T[:3, :4])) or not pose_is_orthogonal(T[:3, :3]):
            r["flags"] = 1
            continue
        terms, matched, skipped = df_align_terms(d2, lo, voxel, p, T, md, c)
        r["S"] = [sum_exact_f32(t) for t in terms]
        r["matched"], r["considered"], r["skipped"] = matched, len(p), skipped
    return out


def df_align_system(rec):
    """revo_map_df_align_system: (H [6, 6], g [6]) float64 of a record; H from its upper triangle S[0..20], g = S[21..26]."""
    S = np.asarray(rec["S"], np.float64).reshape(28)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = S[:21]
    return H + np.triu(H, 1).T, S[21:27].copy()


def _align_solve(H, g):
    """H x = -g by the Cholesky factorisation and pivot rule of the library's registration loops (revo_align_host.h), in its
    order of operations; None: rank-deficient."""
    import math
    L = [[0.0] * 6 for _ in range(6)]
    H, g = [[float(x) for x in row] for row in H], [float(x) for x in g]
    for j in range(6):
        p = H[j][j]
        for k in range(j):
            p -= L[j][k] * L[j][k]
        if not (p > 64.0 * 2.220446049250313e-16 * H[j][j]) or not math.isfinite(p):
            return None
        L[j][j] = math.sqrt(p)
        for i in range(j + 1, 6):
            v = H[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = -g[i]
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k][i] * x[k]
        x[i] = v / L[i][i]
    return x if all(math.isfinite(a) for a in x) else None


def _mul4(A, B):
    """Row-major 4 x 4 product, every entry summed over k in index order from 0.0 (mat4_mul of revo_align_host.h)."""
    out = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            v = 0.0
            for k in range(4):
                v += A[i][k] * B[k][j]
            out[i][j] = v
    return out


def _se3_exp(x):
    """expm(hat(x)), x = (v, w), as revo_align_host.h forms it -> 4 x 4 nested lists."""
    import math
    v, w = x[:3], x[3:]
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    W2 = [W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j] for i in range(3) for j in range(3)]
    a, b, c, d = 1.0, 0.0, 0.5, 0.0
    if not th < 1e-10:
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th)
        c, d = b, (th - math.sin(th)) / (th * th * th)
    E = [[0.0] * 4 for _ in range(4)]
    E[3][3] = 1.0
    for i in range(3):
        t = 0.0
        for j in range(3):
            eye = 1.0 if i == j else 0.0
            E[i][j] = eye + a * W[3 * i + j] + b * W2[3 * i + j]
            t += (eye + c * W[3 * i + j] + d * W2[3 * i + j]) * v[j]
        E[i][3] = t
    return E


def df_align(d2, lo, n, voxel, points, T_init=None, max_dist=None, centre=None, max_iters=30, eps_t=1e-6, eps_r=1e-6, min_matched=12):
    """revo_map_df_align restated: Gauss-Newton in double over df_align_records' records -> (T 4x4 float32, the record at T,
    iterations, status).  centre defaults to the mean of the points under T_init, rounded to float32."""
    F = np.float32
    p = np.asarray(points, F).reshape(-1, 3)
    T0 = np.eye(4, dtype=F) if T_init is None else np.asarray(T_init, F).reshape(4, 4)
    if not np.all(np.isfinite(T0)):
        raise ValueError("T_init is not finite")
    if int(max_iters) < 1:
        raise ValueError("max_iters must be >= 1")
    if centre is None:
        centre = df_align_centre(p, T0)
    evaluate = lambda T: df_align_records(d2, lo, n, voxel, p, np.array(T, np.float64).astype(F), max_dist, centre)[0]  # noqa: E731
    return _gauss_newton(evaluate, T0, centre, max_iters, eps_t, eps_r, min_matched)


def _gauss_newton(evaluate, T0, centre, max_iters, eps_t, eps_r, min_matched):
    """align_loop_over of revo_align_host.h in its order of operations: Gauss-Newton in double over the records evaluate(T) gives
    (T: 4 x 4 nested lists of doubles, rounded to float32 by evaluate) -> (T 4x4 float32, the record at T, iterations, status)."""
    F = np.float32
    c = [float(x) for x in np.asarray(centre, F).reshape(3)]
    Cp = [[1.0, 0.0, 0.0, c[0]], [0.0, 1.0, 0.0, c[1]], [0.0, 0.0, 1.0, c[2]], [0.0, 0.0, 0.0, 1.0]]
    Cm = [[1.0, 0.0, 0.0, -c[0]], [0.0, 1.0, 0.0, -c[1]], [0.0, 0.0, 1.0, -c[2]], [0.0, 0.0, 0.0, 1.0]]
    T = [[float(x) for x in row] for row in T0]
    Tsys, status, it = T, ALIGN_ITER_LIMIT, 0
    while it < int(max_iters):
        rec = evaluate(T)
        x = _align_solve(*df_align_system(rec)) if not (rec["flags"] & 1) and rec["matched"] >= min_matched else None
        if x is None:
            status, T = ALIGN_LOST, Tsys
            break
        it += 1
        Tsys = T
        T = _mul4(_mul4(_mul4(Cp, _se3_exp(x)), Cm), T)
        if max(abs(a) for a in x[:3]) < eps_t and max(abs(a) for a in x[3:]) < eps_r:
            status = ALIGN_CONVERGED
            break
    Tf = np.array(T, np.float64).astype(F)
    return Tf, evaluate(Tf), it, status


def df_align_centre(points, T_init):
    """The default rotation centre: the mean of the points under T_init in float64, rounded to float32 (api.align_maps' rule)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    T = np.asarray(T_init, np.float32).astype(np.float64)
    return (T[:3, :3] @ p.mean(0) + T[:3, 3]).astype(np.float32) if len(p) else np.zeros(3, np.float32)


def df_align_files(dst_path, src_path, T_init=None, max_dist=None, pad=None, min_count=1, **opts):
    """`mapfile df-align`: the map of src_path (its voxels' points) registered against the distance field of dst_path's map,
    built over its bounds grown by `pad` cells (default ceil(max_dist / voxel) + 2); max_dist defaults to 8 voxels.
    -> (T, record, iterations, status)."""
    import math
    h, rec = read(dst_path)
    _, src = read(src_path)
    voxel = np.float32(h["voxel"])
    max_dist = float(8 * voxel) if max_dist is None else float(max_dist)
    pad = int(math.ceil(float(np.float32(max_dist) / voxel))) + 2 if pad is None else int(pad)  # the ratio in float32: 0.24 / 0.02 is 12
    lo, hi, k = bounds_records(rec, min_count)
    if k == 0 or len(src) == 0:
        raise ValueError("df-align needs voxels in both maps")
    lo, n = padded_box(lo, hi, pad)
    d2, _ = distance_field_records(rec, lo, n, min_count)
    return df_align(d2, lo, n, voxel, to_points(src, min_count)[0], T_init, max_dist, **opts)


# --------------------------------------------------------------------- tracking a depth frame against the surface --
TSDF_TRACK_DTYPE = DF_ALIGN_DTYPE   # revo_map_tsdf_track_info has revo_map_df_align_info's layout
TSDF_TRACK_MAX_POSES = 4096
TSDF_TRACK_CLASSES = ("skipped", "gated", "accepted")


def tsdf_track_params(trunc, max_dist=None, stride=1, min_weight=1, centre=None):
    """The parameters a surface tracking call runs with, checked as revo_map_tsdf_track_eval checks them -> (trunc, max_dist
    float32, stride, min_weight, centre float32 [3]): max_dist None or 0 is trunc / 2, stride 0 is 1, min_weight 0 counts as 1,
    centre None is the origin."""
    F = np.float32
    tr = F(trunc)
    if not (np.isfinite(tr) and tr > 0):
        raise ValueError("trunc must be finite and > 0")
    md = F(0 if max_dist is None else max_dist)
    if not np.isfinite(md) or md < 0 or md > tr:
        raise ValueError("max_dist must be 0 (trunc / 2) or finite with 0 < max_dist <= trunc")
    if not 0 <= int(stride) <= 8:
        raise ValueError("stride must be 0 (1) or 1 .. 8")
    if not 0 <= int(min_weight) < 1 << 32:
        raise ValueError("min_weight is a number of views >= 0")
    c = np.zeros(3, F) if centre is None else np.asarray(centre, F).reshape(3)
    if not np.all(np.isfinite(c)):
        raise ValueError("the centre is not finite")
    return tr, (tr * F(0.5) if md == 0 else md), max(1, int(stride)), max(1, int(min_weight)), c


def tsdf_track_centre(lo, n, voxel):
    """The default rotation centre of TsdfVolume.track: the middle of the volume's box in metres, (lo + n / 2) * voxel in float64,
    rounded to float32."""
    lo, n = np.asarray(lo, np.float64).reshape(3), np.asarray(n, np.float64).reshape(3)
    return ((lo + n / 2.0) * float(np.float32(voxel))).astype(np.float32)


def tsdf_track_terms(cells, lo, voxel, trunc, depth, camera, zrange, T, max_dist, stride, min_weight, centre, classes=False):
    """The per-pixel part of revo_map_tsdf_track_eval at one pose T (4x4 float32, finite, orthogonal) with checked parameters,
    float32 with every operation rounded on its own -> (the 28 float32 term arrays of the accepted pixels, matched, considered,
    skipped[, the class of every visited pixel, row by row: an index into TSDF_TRACK_CLASSES])."""
    F = np.float32
    n = np.asarray(cells.shape, np.int64)
    lo = np.asarray(lo, np.int64).reshape(3)
    D = np.asarray(depth, F)
    h, w = D.shape
    fx, fy, cx, cy = (F(x) for x in camera)
    zmin, zmax = F(zrange[0]), F(zrange[1])
    T = np.asarray(T, F)
    v, c, kq = F(voxel), np.asarray(centre, F).reshape(3), F(trunc) / F(1024.0)
    ys, xs = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    cls = np.zeros(len(xs), np.int64)
    L = lambda x0, x1, a: x0 + a * (x1 - x0)  # noqa: E731
    B = lambda v00, v01, v10, v11, r0, r1: L(L(v00, v01, r0), L(v10, v11, r0), r1)  # noqa: E731
    with np.errstate(all="ignore"):
        d = D[ys, xs]
        idx = np.flatnonzero(np.isfinite(d) & (d > zmin) & (d < zmax))
        d = d[idx]
        dcx, dcy = (xs[idx].astype(F) - cx) / fx, (ys[idx].astype(F) - cy) / fy
        pcx, pcy, pcz = dcx * d, dcy * d, d
        pt = np.stack([((T[i, 0] * pcx + T[i, 1] * pcy) + T[i, 2] * pcz) + T[i, 3] for i in range(3)], 1).astype(F).reshape(-1, 3)
        u = (pt / v - (lo.astype(F) + F(0.5))).astype(F)
        b = np.floor(u)
        r = (u - b).astype(F)
        inbox = np.all(np.isfinite(u) & (b >= 0) & (b <= (n - 2).astype(F)), axis=1)
        idx, pt, r, b = idx[inbox], pt[inbox], r[inbox], b[inbox].astype(np.int64)
        corner = {(i, j, k): cells[b[:, 0] + i, b[:, 1] + j, b[:, 2] + k] for i in (0, 1) for j in (0, 1) for k in (0, 1)}
        valid = np.ones(len(idx), bool)
        for q in corner.values():
            valid &= q["weight"] >= min_weight
        idx, pt, r = idx[valid], pt[valid], r[valid]
        q = {key: (x["sum"][valid].astype(F) / x["weight"][valid].astype(F)).astype(F) for key, x in corner.items()}
        rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
        Fv = L(B(q[0, 0, 0], q[0, 0, 1], q[0, 1, 0], q[0, 1, 1], rz, ry), B(q[1, 0, 0], q[1, 0, 1], q[1, 1, 0], q[1, 1, 1], rz, ry), rx)
        G = [B(q[1, 0, 0] - q[0, 0, 0], q[1, 0, 1] - q[0, 0, 1], q[1, 1, 0] - q[0, 1, 0], q[1, 1, 1] - q[0, 1, 1], rz, ry),
             B(q[0, 1, 0] - q[0, 0, 0], q[0, 1, 1] - q[0, 0, 1], q[1, 1, 0] - q[1, 0, 0], q[1, 1, 1] - q[1, 0, 1], rz, rx),
             B(q[0, 0, 1] - q[0, 0, 0], q[0, 1, 1] - q[0, 1, 0], q[1, 0, 1] - q[1, 0, 0], q[1, 1, 1] - q[1, 1, 0], ry, rx)]
        e = Fv * kq
        gx, gy, gz = ((a * kq) / v for a in G)
        acc = np.abs(e) <= F(max_dist)
        cls[idx] = np.where(acc, 2, 1)
        pt, e, gx, gy, gz = pt[acc], e[acc], gx[acc], gy[acc], gz[acc]
        uu = pt - c
        ux, uy, uz = uu[:, 0], uu[:, 1], uu[:, 2]
        J = [gx, gy, gz, uy * gz - uz * gy, uz * gx - ux * gz, ux * gy - uy * gx]
        terms = [J[i] * J[j] for i in range(6) for j in range(i, 6)] + [J[i] * e for i in range(6)] + [e * e]
    assert all(t.dtype == F for t in terms)
    out = (terms, int(acc.sum()), len(xs), int(len(xs) - len(idx)))
    return out + (cls,) if classes else out


def tsdf_track_records(tsdf, lo, voxel, trunc, depth, camera, zrange, poses, max_dist=None, stride=1, min_weight=1, centre=None):
    """revo_map_tsdf_track_eval restated in vectorised numpy: a TSDF_TRACK_DTYPE array, one record per pose (4x4 T_w_c,
    or [N, 4, 4]; 1 .. 4096), of the depth image ([h, w] float32 metres, camera (fx, fy, cx, cy), zrange (zmin, zmax)) against the
    volume tsdf of the box at lo with the edge `voxel` and the truncation distance trunc.  The sums are formed as df_align_records
    forms them.  ValueError as the library's REVO_ERR_INVALID_ARG."""
    F = np.float32
    cells = _tsdf_volume(tsdf)
    lo, _ = check_box(lo, np.asarray(cells.shape, np.int64))
    if not (np.isfinite(F(voxel)) and F(voxel) > 0):
        raise ValueError("the voxel edge must be finite and > 0")
    tr, md, st, mw, c = tsdf_track_params(trunc, max_dist, stride, min_weight, centre)
    D = np.asarray(depth, F)
    if D.ndim != 2 or not (1 <= D.shape[0] <= 2048 and 1 <= D.shape[1] <= 2048):
        raise ValueError("a depth image is [h, w] float32 with width and height 1 .. 2048")
    k = [F(x) for x in tuple(camera)[:4]] + [F(x) for x in zrange]
    if len(k) != 6 or not all(np.isfinite(x) for x in k) or not (k[0] > 0 and k[1] > 0) or not (k[4] >= 0 and k[4] < k[5]):
        raise ValueError("the camera needs finite intrinsics with fx, fy > 0 and a depth range 0 <= zmin < zmax")
    Ts = np.asarray(poses, F).reshape(-1, 4, 4)
    if not 1 <= len(Ts) <= TSDF_TRACK_MAX_POSES:
        raise ValueError("1 .. 4096 poses")
    out = np.zeros(len(Ts), TSDF_TRACK_DTYPE)
    for r, T in zip(out, Ts):
        r["centre"], r["max_dist"] = c, md
        r["R"], r["T"] = np.ascontiguousarray(T[:3, :3].T).reshape(9), T[:3, 3]  # column-major, as given (a NaN keeps its bits)
        if not np.all(np.isfinite(T[:3, :4])) or not pose_is_orthogonal(T[:3, :3]):
            r["flags"] = 1
            continue
        terms, matched, considered, skipped = tsdf_track_terms(cells, lo, voxel, tr, D, k[:4], k[4:], T, md, st, mw, c)
        r["S"] = [sum_exact_f32(t) for t in terms]
        r["matched"], r["considered"], r["skipped"] = matched, considered, skipped
    return out


def tsdf_track(tsdf, lo, voxel, trunc, depth, camera, zrange, T_init, max_dist=None, stride=1, min_weight=1, centre=None, max_iters=30,
               eps_t=1e-6, eps_r=1e-6, min_matched=12):
    """revo_map_tsdf_track restated: Gauss-Newton in double over tsdf_track_records' records from T_init -> (T 4x4 float32, the record
    at T, iterations, status).  centre None: tsdf_track_centre, the middle of the box."""
    F = np.float32
    cells = _tsdf_volume(tsdf)
    T0 = np.asarray(T_init, F).reshape(4, 4)
    if not np.all(np.isfinite(T0)):
        raise ValueError("T_init is not finite")
    if int(max_iters) < 1:
        raise ValueError("max_iters must be >= 1")
    if centre is None:
        centre = tsdf_track_centre(lo, cells.shape, voxel)
    evaluate = lambda T: tsdf_track_records(cells, lo, voxel, trunc, depth, camera, zrange, np.array(T, np.float64).astype(F), max_dist, stride,  # noqa: E731
                                            min_weight, centre)[0]
    return _gauss_newton(evaluate, T0, centre, max_iters, eps_t, eps_r, min_matched)


def tsdf_track_file(path, views_dir, camera, zrange, depth_scale=5000.0, **params):
    """`mapfile surface-track`: every frame of a `run_tum --map-views` / `--surface-views` folder (or one `mapfile surface-views`
    wrote) tracked against the volume of the .npz `path` from the pose poses.txt lists for it -> [(time stamp, listed pose, refined
    pose, record, iterations, status)].  params: tsdf_track's."""
    import os
    from . import tum
    cells, lo, voxel, trunc, _ = read_tsdf(path, color=True)
    stamps = [float(r[0]) for r in tum.read_associate(os.path.join(views_dir, "associate.txt"))]
    out = []
    for ts, (depth, T0, _) in zip(stamps, read_views(views_dir, camera, zrange, depth_scale)):
        out.append((ts, T0) + tsdf_track(cells, lo, voxel, trunc, depth, camera, zrange, T0, **params))
    return out


# ----------------------------------------------------------------------------- a box that follows the camera --
TSDF_RECORD_DTYPE = np.dtype([("key", "<u8"), ("sum", "<i4"), ("weight", "<u4"), ("sum_b", "<u4"), ("sum_g", "<u4"), ("sum_r", "<u4"),
                              ("color_weight", "<u4")])  # revo_map_tsdf_record
TSDF_SHIFT_INFO_KEYS = ("cells", "staying", "leaving", "records", "dropped")
TSDF_REFILL_INFO_KEYS = ("records", "applied", "outside")
TSDF_SUM_MAX = 1 << 30          # |sum| of a cell that FITS
TSDF_COLOR_MAX = 255 << 20      # a colour sum of a cell that FITS
SURFACE_ASSEMBLE_MAX_N = DF_MAX_N
SURFACE_ASSEMBLE_MAX_CELLS = DF_MAX_CELLS
_RECORD_COLOR = (("sum_b", "sum_b"), ("sum_g", "sum_g"), ("sum_r", "sum_r"), ("color_weight", "weight"))  # record field, colour cell field


def pack_keys(idx):
    """The packed keys (uint64) of [N, 3] voxel indices, each in [-2^20, 2^20 - 1]: 21 bits per axis biased by 2^20, x highest."""
    k = (np.asarray(idx, np.int64).reshape(-1, 3) + (1 << 20)).astype(np.uint64)
    return (k[:, 0] << np.uint64(42)) | (k[:, 1] << np.uint64(21)) | k[:, 2]


def tsdf_record_array(records):
    """records as a 1-D TSDF_RECORD_DTYPE array (an array of that dtype, or bytes of whole records)."""
    if isinstance(records, (bytes, bytearray, memoryview)):
        records = np.frombuffer(bytes(records), TSDF_RECORD_DTYPE)
    rec = np.asarray(records)
    if rec.dtype != TSDF_RECORD_DTYPE or rec.ndim != 1:
        raise ValueError("surface records are a 1-D array of TSDF_RECORD_DTYPE")
    return rec


def _tsdf_cells_nonempty(cells, color):
    ne = (cells["sum"] != 0) | (cells["weight"] != 0)
    if color is not None:
        for k in ("sum_b", "sum_g", "sum_r", "weight"):
            ne |= color[k] != 0
    return ne


def _tsdf_cells_to_records(idx, cells, color):
    """The records of the cells at the voxel indices idx [N, 3] (cells, color: [N] arrays; color may be None), in key order."""
    rec = np.zeros(len(cells), TSDF_RECORD_DTYPE)
    rec["key"] = pack_keys(idx)
    rec["sum"], rec["weight"] = cells["sum"], cells["weight"]
    if color is not None:
        for rk, ck in _RECORD_COLOR:
            rec[rk] = color[ck]
    return rec[np.argsort(rec["key"], kind="stable")]


def tsdf_volume_records(cells, color, lo):
    """Every cell of the box (lo, cells.shape) that is not EMPTY, as TSDF_RECORD_DTYPE in ascending key order."""
    cells = _tsdf_volume(cells)
    if color is not None:
        color = _tsdf_color_volume(color, cells.shape)
    lo, _ = check_box(lo, cells.shape)
    mask = _tsdf_cells_nonempty(cells, color)
    return _tsdf_cells_to_records(np.argwhere(mask) + lo, cells[mask], None if color is None else color[mask])


def tsdf_shift_records(cells, color, lo, delta):
    """revo_map_tsdf_shift's contract in numpy: the volumes of the box (lo, cells.shape) moved into the volumes of the box
    (lo + delta, same shape).  color: the colour volume or None.  -> (cells2, color2, records, info): the destination volumes (an
    entering cell is zero), the leaving cells that are not EMPTY as TSDF_RECORD_DTYPE in ascending key order, and the dict of
    TSDF_SHIFT_INFO_KEYS (dropped is 0: the records are returned).  ValueError as the library's REVO_ERR_INVALID_ARG."""
    cells = _tsdf_volume(cells)
    if color is not None:
        color = _tsdf_color_volume(color, cells.shape)
    lo, n = check_box(lo, cells.shape)
    d = np.asarray(delta, np.int64).reshape(3)
    check_box(lo + d, n)
    out = np.zeros(cells.shape, TSDF_CELL_DTYPE)
    cout = None if color is None else np.zeros(cells.shape, TSDF_COLOR_DTYPE)
    leaving = np.ones(cells.shape, bool)
    if np.all(np.abs(d) < n):
        src = tuple(slice(int(max(0, d[k])), int(min(n[k], n[k] + d[k]))) for k in range(3))
        dst = tuple(slice(int(max(0, -d[k])), int(min(n[k], n[k] - d[k]))) for k in range(3))
        out[dst] = cells[src]
        if color is not None:
            cout[dst] = color[src]
        leaving[src] = False
    mask = leaving & _tsdf_cells_nonempty(cells, color)
    idx = np.argwhere(mask) + lo
    rec = _tsdf_cells_to_records(idx, cells[mask], None if color is None else color[mask])
    total = int(cells.size)
    n_leaving = int(leaving.sum())
    info = {"cells": total, "staying": total - n_leaving, "leaving": n_leaving, "records": len(rec), "dropped": 0}
    return out, cout, rec, info


def tsdf_refill_records(cells, color, lo, records):
    """revo_map_tsdf_refill's contract in numpy: every record whose key lies inside the box (lo, cells.shape) added to its cell.
    -> (cells2, color2, info dict of TSDF_REFILL_INFO_KEYS); the inputs are not changed.  ValueError where the library refuses: keys
    that are not strictly ascending (or with bit 63 set), colour words without a colour volume, a cell that would not FIT."""
    cells = _tsdf_volume(cells)
    if color is not None:
        color = _tsdf_color_volume(color, cells.shape)
    lo, n = check_box(lo, cells.shape)
    rec = tsdf_record_array(records)
    key = rec["key"]
    if np.any(key >> np.uint64(63)) or np.any(key[1:] <= key[:-1]):
        raise ValueError("surface records must be in strictly ascending key order")
    if color is None and any(np.any(rec[rk] != 0) for rk, _ in _RECORD_COLOR):
        raise ValueError("a record carries colour words and there is no colour volume")
    c = key_axes(key) - lo
    inside = np.all((c >= 0) & (c < n), axis=1)
    ci = tuple(c[inside].T)
    r = rec[inside]
    s = cells["sum"][ci].astype(np.int64) + r["sum"].astype(np.int64)
    w = cells["weight"][ci].astype(np.int64) + r["weight"].astype(np.int64)
    bad = (np.abs(s) > TSDF_SUM_MAX) | (w > TSDF_W_MAX)
    cs = {}
    if color is not None:
        for rk, ck in _RECORD_COLOR:
            cs[ck] = color[ck][ci].astype(np.int64) + r[rk].astype(np.int64)
            bad |= cs[ck] > (TSDF_W_MAX if ck == "weight" else TSDF_COLOR_MAX)
    if np.any(bad):
        raise ValueError("a cell would pass the sums a fuse can reach")
    out = cells.copy()
    out["sum"][ci] = s.astype(np.int32)
    out["weight"][ci] = w.astype(np.uint32)
    cout = None
    if color is not None:
        cout = color.copy()
        for ck, v in cs.items():
            cout[ck][ci] = v.astype(np.uint32)
    return out, cout, {"records": len(rec), "applied": int(inside.sum()), "outside": int(len(rec) - inside.sum())}


def follow_lo(T_w_c, n, voxel, ahead, step):
    """The following policy, one pure function: the first voxel index of the box of n cells that a camera at T_w_c (4x4,
    the float32 pose; computed in float64) should be in -- centred `ahead` metres along the camera's z axis, snapped down to a
    multiple of `step` cells per axis, and clamped so the box stays inside the index range [-2^20, 2^20 - 1]."""
    T = np.asarray(np.asarray(T_w_c, np.float32).reshape(4, 4), np.float64)
    n = np.asarray(n, np.int64).reshape(3)
    step = int(step)
    if step < 1:
        raise ValueError("step must be >= 1 cell")
    if not np.all(np.isfinite(T)):
        raise ValueError("the pose is not finite")
    v = float(np.float32(voxel))
    p = T[:3, 3] + float(ahead) * T[:3, 2]
    want = np.floor(p / v).astype(np.int64) - n // 2
    lo = step * np.floor_divide(want, step)
    return np.clip(lo, -(1 << 20), (1 << 20) - n).astype(np.int64)


class SurfaceStore:
    """Everything that has left a following surface's box: TSDF_RECORD_DTYPE records, sparse, in ascending key order
    with unique keys.  voxel, trunc: what the records were fused with (None until known); they travel with save / load."""

    def __init__(self, records=None, voxel=None, trunc=None):
        self.records = np.zeros(0, TSDF_RECORD_DTYPE)
        self.voxel = None if voxel is None else float(np.float32(voxel))
        self.trunc = None if trunc is None else float(np.float32(trunc))
        if records is not None:
            self.add(records)

    def __len__(self):
        return len(self.records)

    def add(self, records):
        """Records into the store; records with equal keys (in the store or among themselves) are summed field by field.  All or
        nothing: ValueError, with the store unchanged, when a key has bit 63 set or a summed cell would not FIT."""
        rec = tsdf_record_array(records)
        if len(rec) == 0:
            return
        if np.any(rec["key"] >> np.uint64(63)):
            raise ValueError("a surface record's key has bit 63 set")
        both = np.concatenate([self.records, rec])
        keys, inv = np.unique(both["key"], return_inverse=True)
        out = np.zeros(len(keys), TSDF_RECORD_DTYPE)
        out["key"] = keys
        for k in TSDF_RECORD_DTYPE.names[1:]:
            acc = np.zeros(len(keys), np.int64)
            np.add.at(acc, inv, both[k].astype(np.int64))
            limit = TSDF_SUM_MAX if k == "sum" else TSDF_W_MAX if k in ("weight", "color_weight") else TSDF_COLOR_MAX
            if np.any(np.abs(acc) > limit):
                raise ValueError("a cell of the store would pass the sums a fuse can reach")
            out[k] = acc.astype(TSDF_RECORD_DTYPE[k])
        self.records = out

    def _inside(self, lo, n):
        lo, n = check_box(lo, n)
        c = key_axes(self.records["key"]) - lo
        return np.all((c >= 0) & (c < n), axis=1)

    def take(self, lo, n):
        """The records inside the box (lo, n), in key order; they leave the store."""
        inside = self._inside(lo, n)
        out = self.records[inside]
        self.records = self.records[~inside]
        return out

    def bounds(self):
        """(lo [3], n [3]) int64 of the smallest box that holds every record, or None for an empty store."""
        if len(self.records) == 0:
            return None
        k = key_axes(self.records["key"])
        return k.min(0), k.max(0) - k.min(0) + 1

    def check(self, voxel=None, trunc=None):
        """ValueError when the store's voxel edge or truncation distance is known, given, and another."""
        for mine, given, name in ((self.voxel, voxel, "voxel edge"), (self.trunc, trunc, "truncation distance")):
            if mine is not None and given is not None and np.float32(mine) != np.float32(given):
                raise ValueError("the store's %s is %g, not %g" % (name, mine, given))

    def volume(self, lo, n, voxel=None, trunc=None):
        """(cells, color) dense over the box (lo, n): the store's records inside it, zeros elsewhere; the store keeps them.  voxel,
        trunc: checked against the store's where both are known (check)."""
        self.check(voxel, trunc)
        lo, n = check_box(lo, n)
        shape = tuple(int(x) for x in n)
        cells, color = np.zeros(shape, TSDF_CELL_DTYPE), np.zeros(shape, TSDF_COLOR_DTYPE)
        inside = self._inside(lo, n)
        r = self.records[inside]
        ci = tuple((key_axes(r["key"]) - lo).T)
        cells["sum"][ci], cells["weight"][ci] = r["sum"], r["weight"]
        for rk, ck in _RECORD_COLOR:
            color[ck][ci] = r[rk]
        return cells, color

    def save(self, path):
        """The .npz of a store: records (TSDF_RECORD_DTYPE), voxel and trunc (float32; NaN when not known)."""
        with open(path, "wb") as f:
            np.savez(f, records=self.records, voxel=np.float32(np.nan if self.voxel is None else self.voxel),
                     trunc=np.float32(np.nan if self.trunc is None else self.trunc))
        return path

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if not all(k in z.files for k in ("records", "voxel", "trunc")):
                raise ValueError("%s is not a surface store (records, voxel, trunc)" % path)
            rec, voxel, trunc = z["records"], float(z["voxel"]), float(z["trunc"])
        if rec.dtype != TSDF_RECORD_DTYPE or rec.ndim != 1:
            raise ValueError("%s: the records are not TSDF_RECORD_DTYPE" % path)
        if np.any(rec["key"] >> np.uint64(63)) or np.any(rec["key"][1:] <= rec["key"][:-1]):
            raise ValueError("%s: the records are not in strictly ascending key order" % path)
        s = cls(None, None if np.isnan(voxel) else voxel, None if np.isnan(trunc) else trunc)
        s.records = rec
        return s


def surface_assemble_box(bounds, lo=None, n=None):
    """The box a store (and what goes with it) is assembled over: (lo, n) as given, or the bounds; ValueError with a message when
    there is nothing to assemble or the box is larger than a volume may be (1024 cells per axis, 2^27 cells)."""
    if (lo is None) != (n is None):
        raise ValueError("give both lo and n, or neither (the store's bounds)")
    if lo is None:
        if bounds is None:
            raise ValueError("the store is empty: there is no surface to assemble")
        lo, n = bounds
    lo, n = np.asarray(lo, np.int64).reshape(3), np.asarray(n, np.int64).reshape(3)
    if np.any(n > SURFACE_ASSEMBLE_MAX_N):
        raise ValueError("the surface spans %s cells: an axis of more than %d cells does not fit one volume (give a smaller box; the "
                         "store keeps everything)" % (n.tolist(), SURFACE_ASSEMBLE_MAX_N))
    if np.all(n >= 1) and int(n[0]) * int(n[1]) * int(n[2]) > SURFACE_ASSEMBLE_MAX_CELLS:
        raise ValueError("the surface spans %s cells: more than 2^27 cells do not fit one volume (give a smaller box; the store keeps "
                         "everything)" % (n.tolist(),))
    return check_box(lo, n)


def surface_assemble_file(path, box=None):
    """`mapfile surface-assemble`: (cells, color, lo, voxel, trunc) of the store file `path` over box = (lo, n), by default its bounds."""
    store = SurfaceStore.load(path)
    if store.voxel is None or store.trunc is None:
        raise ValueError("%s does not state its voxel edge and truncation distance" % path)
    lo, n = surface_assemble_box(store.bounds(), *(box if box is not None else (None, None)))
    cells, color = store.volume(lo, n)
    return cells, color, lo.astype(np.int32), store.voxel, store.trunc


# ---------------------------------------------------------------------------------- planning through the map --
PLAN_NONE = np.uint32(0xFFFFFFFF)
PLAN_INFO_KEYS = ("cells", "free", "reachable", "max_cost", "seeds_used", "seeds_outside", "seeds_blocked")
PLAN_STATUS = ("reached", "unreachable", "outside", "truncated")
PLAN_REACHED, PLAN_UNREACHABLE, PLAN_OUTSIDE, PLAN_TRUNCATED = 0, 1, 2, 3
PLAN_MAX_SEEDS = PLAN_MAX_STARTS = PLAN_MAX_LEN = 1 << 20
PLAN_MAX_COST0 = 1 << 24
_PLAN_INF = np.int32(1 << 30)
# the 26 moves in revo_map_plan_paths' order: dx outermost, then dy, then dz, each -1, 0, 1, the cell itself skipped
PLAN_MOVES = tuple((dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))


def plan_r2(clearance, voxel):
    """The squared clearance in cells of a clearance in metres: max(1, ceil((clearance / voxel)^2))."""
    if not (np.isfinite(clearance) and clearance >= 0):
        raise ValueError("the clearance must be finite and >= 0 metres")
    return max(1, int(np.ceil((float(clearance) / float(np.float32(voxel))) ** 2)))


def plan_seeds(seeds, voxel=None):
    """[k, 4] int64 (cell x, y, z, cost0) of goals given as [k, 3] or [k, 4] integers (voxel indices, cost0 0 by default) or as
    [k, 3] floating-point metres (floor(p / voxel), float32 like revo_map_df_sample)."""
    s = np.asarray(seeds)
    if s.ndim == 1:
        s = s.reshape(1, -1)
    if s.ndim != 2 or s.shape[1] not in (3, 4) or len(s) < 1 or len(s) > PLAN_MAX_SEEDS:
        raise ValueError("goals are 1 .. 2^20 rows of 3 (a cell or a point) or 4 (a cell and its cost0) numbers")
    if s.dtype.kind == "f":
        if s.shape[1] != 3 or voxel is None or not np.isfinite(s).all():
            raise ValueError("goals in metres are finite [k, 3] points of a field with a voxel edge")
        s = np.floor(s.astype(np.float32) / np.float32(voxel)).astype(np.int64)
    s = s.astype(np.int64)
    if s.shape[1] == 3:
        s = np.concatenate([s, np.zeros((len(s), 1), np.int64)], 1)
    if np.any(s[:, 3] < 0) or np.any(s[:, 3] > PLAN_MAX_COST0):
        raise ValueError("a goal's cost0 is 0 .. 2^24")
    if np.any(np.abs(s[:, :3]) >= 1 << 31):
        raise ValueError("a goal's cell does not fit 32 bits")
    return s


def plan_records(d2, lo, n, seeds, r2):
    """revo_map_plan restated: (cost uint32 [n0, n1, n2], info dict of PLAN_INFO_KEYS).  A cell is free iff d2 >= r2; cost is
    the cheapest way from a used seed over free cells by the 26 moves at the weights 3, 4, 5, plus the seed's cost0; PLAN_NONE
    where a cell is not free or not reached.  Written as whole-array min-plus sweeps over the 26 moves until nothing changes."""
    lo, n = check_box(lo, n)
    d2 = np.asarray(d2, np.uint32)
    if d2.shape != tuple(int(x) for x in n):
        raise ValueError("the field's shape %s is not the box's %s" % (d2.shape, n.tolist()))
    r2 = int(r2)
    if r2 < 1 or r2 > 0xFFFFFFFF:
        raise ValueError("r2 must be 1 .. 2^32 - 1")
    s = plan_seeds(seeds)
    free = d2 >= np.uint32(r2)
    c = s[:, :3] - lo
    inside = np.all((c >= 0) & (c < n), axis=1)
    ci = c[inside]
    on_free = free[ci[:, 0], ci[:, 1], ci[:, 2]]
    # one halo cell on every side holds "not free": a move out of the box is a move onto a blocked cell
    g = np.full(tuple(int(x) + 2 for x in n), _PLAN_INF, np.int32)
    core = g[1:-1, 1:-1, 1:-1]
    np.minimum.at(core, tuple(ci[on_free].T), s[inside][on_free, 3].astype(np.int32))
    moves = [(m, 2 + sum(1 for x in m if x)) for m in PLAN_MOVES if all(x == 0 or n[a] > 1 for a, x in enumerate(m))]
    changed = bool(on_free.any())
    while changed:
        changed = False
        for (dx, dy, dz), w in moves:
            nb = g[1 + dx:g.shape[0] - 1 + dx, 1 + dy:g.shape[1] - 1 + dy, 1 + dz:g.shape[2] - 1 + dz] + np.int32(w)
            lower = free & (nb < core)
            if lower.any():
                core[lower] = nb[lower]
                changed = True
    reached = core < _PLAN_INF
    cost = np.where(reached, core.astype(np.int64), np.int64(PLAN_NONE)).astype(np.uint32)
    info = {"cells": int(cost.size), "free": int(free.sum()), "reachable": int(reached.sum()), "max_cost": int(core[reached].max()) if reached.any() else 0,
            "seeds_used": int(on_free.sum()), "seeds_outside": int((~inside).sum()), "seeds_blocked": int((~on_free).sum())}
    return cost, info


def plan_paths(cost, lo, n, starts, max_len=4096):
    """revo_map_plan_paths restated: a list of (cells int32 [length, 3] absolute voxel indices, status, cost) per start.  From a
    cell the next one is the first of PLAN_MOVES inside the box with cost[nb] != PLAN_NONE and cost[nb] + w == cost[c]."""
    lo, n = check_box(lo, n)
    cost = np.asarray(cost, np.uint32)
    if cost.shape != tuple(int(x) for x in n):
        raise ValueError("the cost field's shape %s is not the box's %s" % (cost.shape, n.tolist()))
    st = np.asarray(starts, np.int64).reshape(-1, 3)
    max_len = int(max_len)
    if len(st) < 1 or len(st) > PLAN_MAX_STARTS or max_len < 1 or max_len > PLAN_MAX_LEN:
        raise ValueError("1 .. 2^20 starts and a max_len of 1 .. 2^20 cells")
    c64 = cost.astype(np.int64)
    none = int(PLAN_NONE)
    out = []
    for p in st:
        c = p - lo
        if np.any(c < 0) or np.any(c >= n):
            out.append((np.zeros((0, 3), np.int32), PLAN_OUTSIDE, none))
            continue
        x, y, z = (int(v) for v in c)
        v = int(c64[x, y, z])
        if v == none:
            out.append((np.zeros((0, 3), np.int32), PLAN_UNREACHABLE, none))
            continue
        cells, v0 = [], v
        while True:
            cells.append((x, y, z))
            nxt = None
            for dx, dy, dz in PLAN_MOVES:
                ux, uy, uz = x + dx, y + dy, z + dz
                if 0 <= ux < n[0] and 0 <= uy < n[1] and 0 <= uz < n[2]:
                    u = int(c64[ux, uy, uz])
                    if u != none and u + 2 + (dx != 0) + (dy != 0) + (dz != 0) == v:
                        nxt = (ux, uy, uz, u)
                        break
            if nxt is None:
                status = PLAN_REACHED
                break
            if len(cells) == max_len:
                status = PLAN_TRUNCATED
                break
            x, y, z, v = nxt
        out.append(((np.asarray(cells, np.int64) + lo).astype(np.int32), status, v0))
    return out


def plan_path_points(cells, voxel):
    """[length, 3] float32 metres: the centres of a path's cells."""
    return ((np.asarray(cells, np.float64).reshape(-1, 3) + 0.5) * float(np.float32(voxel))).astype(np.float32)


def write_cost(path, cost, lo, voxel, r2):
    """The .npz of a cost field: cost (uint32 [n0, n1, n2]), lo, n (int32 [3]), voxel (float32), r2 (uint32)."""
    cost = np.ascontiguousarray(cost, np.uint32)
    with open(path, "wb") as f:
        np.savez(f, cost=cost, lo=np.asarray(lo, np.int32).reshape(3), n=np.asarray(cost.shape, np.int32), voxel=np.float32(voxel), r2=np.uint32(r2))
    return path


def read_cost(path):
    """(cost, lo, voxel, r2) of a file write_cost wrote; ValueError if its arrays do not fit together."""
    with np.load(path) as z:
        if not all(k in z.files for k in ("cost", "lo", "n", "voxel", "r2")):
            raise ValueError("%s is not a cost-field file (cost, lo, n, voxel, r2)" % path)
        cost, lo, n, voxel, r2 = z["cost"], z["lo"], z["n"], z["voxel"], z["r2"]
    if cost.dtype != np.uint32 or cost.ndim != 3 or lo.shape != (3,) or list(cost.shape) != [int(x) for x in n]:
        raise ValueError("%s: a cost field is a 3-D uint32 array of the shape its n states" % path)
    check_box(lo, n)
    return cost, lo.astype(np.int32), float(np.float32(voxel)), int(r2)


def plan_file(path, goals, starts, clearance, pad=None, max_len=1 << 20, min_count=1, seen=None, min_views=1):
    """Plans through the file's map: the distance field over its bounds grown by `pad` cells (by default the clearance in
    cells plus 2), the cost field from `goals` at the clearance (metres), and the paths from `starts` (both voxel indices)
    -> (cost, lo, voxel, r2, info, paths).  With seen (a write_seen file) the field is the known field over that volume's
    box: the way keeps the clearance from unseen space too."""
    header, rec = read(path)
    voxel = header["voxel"]
    r2 = plan_r2(clearance, voxel)
    if seen is not None:
        vol, lo, n = _seen_for(seen, voxel)
        d2, _ = known_field_records(rec, lo, n, vol, min_count, 0, min_views)
    else:
        lo, hi, _ = bounds_records(rec, min_count)
        lo, n = padded_box(lo, hi, int(np.ceil(np.sqrt(r2))) + 2 if pad is None else pad)
        d2, _ = distance_field_records(rec, lo, n, min_count)
    cost, info = plan_records(d2, lo, n, goals, r2)
    return cost, lo.astype(np.int32), voxel, r2, info, plan_paths(cost, lo, n, starts, max_len)


def write_field(path, d2, lo, voxel):
    """The .npz of a distance field: d2 (uint32 [n0, n1, n2]), lo, n (int32 [3]), voxel (float32)."""
    d2 = np.ascontiguousarray(d2, np.uint32)
    with open(path, "wb") as f:
        np.savez(f, d2=d2, lo=np.asarray(lo, np.int32).reshape(3), n=np.asarray(d2.shape, np.int32), voxel=np.float32(voxel))
    return path


def read_field(path):
    """(d2, lo, voxel) of a file write_field wrote; ValueError if its arrays do not fit together."""
    with np.load(path) as z:
        if not all(k in z.files for k in ("d2", "lo", "n", "voxel")):
            raise ValueError("%s is not a distance-field file (d2, lo, n, voxel)" % path)
        d2, lo, n, voxel = z["d2"], z["lo"], z["n"], z["voxel"]
    if d2.dtype != np.uint32 or d2.ndim != 3 or lo.shape != (3,) or list(d2.shape) != [int(x) for x in n]:
        raise ValueError("%s: a distance field is a 3-D uint32 array of the shape its n states" % path)
    check_box(lo, n)
    return d2, lo.astype(np.int32), float(np.float32(voxel))


def esdf_file(path, pad=8, min_count=1, clamp=0, seen=None, min_views=1):
    """(d2, lo, voxel, info) of the file's map over its bounds grown by `pad` cells; with seen (a write_seen file) the known
    field over that volume's box."""
    header, rec = read(path)
    if seen is not None:
        vol, lo, n = _seen_for(seen, header["voxel"])
        d2, info = known_field_records(rec, lo, n, vol, min_count, clamp, min_views)
        return d2, lo.astype(np.int32), header["voxel"], info
    lo, hi, _ = bounds_records(rec, min_count)
    lo, n = padded_box(lo, hi, pad)
    d2, info = distance_field_records(rec, lo, n, min_count, clamp)
    return d2, lo.astype(np.int32), header["voxel"], info


def read_pose(path):
    """A pose from a text file of 16 or 12 numbers: a row-major 4x4 or 3x4."""
    with open(path) as f:
        a = [float(x) for x in f.read().replace(",", " ").split()]
    if len(a) not in (12, 16):
        raise ValueError("%s holds %d numbers; a pose is 16 (4x4) or 12 (3x4), row-major" % (path, len(a)))
    return _pose_matrix(np.float32(a).reshape(-1, 4))


def transform_file(path, T, voxel=None, min_count=1):
    """(header, records, info) of the file's map under the pose T at the edge `voxel` (the file's by default): the header
    carries that edge, the file's cloud mode and keyframes, and its dropped points plus those the move dropped."""
    header, rec = read(path)
    voxel = header["voxel"] if voxel is None else float(np.float32(voxel))
    out, info = pose_records(rec, T, voxel, min_count)
    h = make_header(voxel, header["dense"], out, header["points_dropped"] + info["points_dropped"], header["keyframes"])
    return h, out, info


def to_points(records, min_count=1):
    """(xyz N x 3 float32, rgb N x 3 uint8 as R,G,B, count N uint32) of the records with count >= max(min_count, 1), in their
    order -- what revo_map_extract gives: xyz = float32(float64(sum_q) / float64(count) * 2^-20), colour = (sum + count // 2)
    // count."""
    rec = as_records(records)
    rec = rec[rec["count"] >= np.uint64(max(1, int(min_count)))]
    cnt = rec["count"]
    xyz = ((rec["sum_q"].astype(np.float64) / cnt.astype(np.float64)[:, None]) * 2.0 ** -20).astype(np.float32)
    c = cnt[:, None]
    bgr = ((rec["sum_bgr"] + c // np.uint64(2)) // c).astype(np.uint8)
    return xyz.reshape(-1, 3), np.ascontiguousarray(bgr[:, ::-1]).reshape(-1, 3), cnt.astype(np.uint32)


def merge_files(paths):
    """(header, records) of the union of the files' maps: same voxel edge; dense of the first; counters added."""
    header, rec = read(paths[0])
    for p in paths[1:]:
        h, r = read(p)
        if np.float32(h["voxel"]).tobytes() != np.float32(header["voxel"]).tobytes():
            raise ValueError("%s has voxels of %g m, %s of %g m" % (p, h["voxel"], paths[0], header["voxel"]))
        rec = merge_records(rec, r)
        header = dict(header, voxels=len(rec), points_integrated=header["points_integrated"] + h["points_integrated"],
                      points_dropped=header["points_dropped"] + h["points_dropped"], keyframes=header["keyframes"] + h["keyframes"])
    return header, rec


def subtract_files(path_a, path_b):
    """(header, records) of map A without map B: same voxel edge; dense of A; B's counters leave A's (ValueError if larger)."""
    header, rec = read(path_a)
    h, r = read(path_b)
    if np.float32(h["voxel"]).tobytes() != np.float32(header["voxel"]).tobytes():
        raise ValueError("%s has voxels of %g m, %s of %g m" % (path_b, h["voxel"], path_a, header["voxel"]))
    for k in ("points_dropped", "keyframes"):
        if h[k] > header[k]:
            raise ValueError("%s counts %d %s, %s only %d" % (path_b, h[k], k, path_a, header[k]))
    rec = subtract_records(rec, r)
    return dict(header, voxels=len(rec), points_integrated=header["points_integrated"] - h["points_integrated"],
                points_dropped=header["points_dropped"] - h["points_dropped"], keyframes=header["keyframes"] - h["keyframes"]), rec


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    cmd, args = (argv[0], argv[1:]) if argv else (None, [])
    try:
        if cmd == "info" and args:
            for p in args:
                h, _ = read(p)
                print("%s: %d voxels of %g m (%s clouds) from %d keyframes, %d points fused, %d points dropped"
                      % (p, h["voxels"], h["voxel"], "dense" if h["dense"] else "edge", h["keyframes"], h["points_integrated"],
                         h["points_dropped"]))
            return 0
        if cmd == "merge" and len(args) >= 2:
            h, rec = merge_files(args[1:])
            write(args[0], h, rec)
            print("%s: %d voxels from %d files" % (args[0], len(rec), len(args) - 1))
            return 0
        if cmd == "subtract" and len(args) == 4 and "-o" in args[:3]:
            i = args.index("-o")
            out = args[i + 1]
            a, b = args[:i] + args[i + 2:]
            h, rec = subtract_files(a, b)
            write(out, h, rec)
            print("%s: %d voxels (%s without %s)" % (out, len(rec), a, b))
            return 0
        if cmd == "coarsen" and len(args) == 4 and "-o" in args[:3]:
            i = args.index("-o")
            out = args[i + 1]
            a, shift = args[:i] + args[i + 2:]
            h, rec = coarsen_file(a, int(shift))
            write(out, h, rec)
            print("%s: %d voxels of %g m (%s coarsened by %d)" % (out, len(rec), h["voxel"], a, int(shift)))
            return 0
        if cmd == "transform" and "-o" in args:
            opt = {"-o": None, "--voxel": None, "--min-count": "1"}
            pos, i = [], 0
            while i < len(args):
                if args[i] in opt and i + 1 < len(args):
                    opt[args[i]] = args[i + 1]
                    i += 2
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 2 and opt["-o"] is not None:
                h, rec, info = transform_file(pos[0], read_pose(pos[1]), None if opt["--voxel"] is None else float(opt["--voxel"]),
                                              int(opt["--min-count"]))
                write(opt["-o"], h, rec)
                print("%s: %d voxels of %g m (%s under %s: %d voxels moved, %d dropped, %d skipped)"
                      % (opt["-o"], len(rec), h["voxel"], pos[0], pos[1], info["voxels_moved"], info["voxels_dropped"], info["voxels_skipped"]))
                return 0
        if cmd == "carve" and "-o" in args and "--views" in args:
            opt = {"-o": 1, "--views": 1, "--removed": 1, "--radius": 1, "--margin": 1, "--margin-rel": 1, "--min-views": 1,
                   "--min-count": 1, "--max-count": 1, "--camera": 4, "--zrange": 2, "--depth-scale": 1}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1:
                params = {name: conv(val[o][0]) for o, name, conv in (("--radius", "radius", int), ("--margin", "margin", float),
                                                                       ("--margin-rel", "margin_rel", float), ("--min-views", "min_views", int),
                                                                       ("--min-count", "min_count", int), ("--max-count", "max_count", int))
                          if o in val}
                camera = [float(x) for x in val.get("--camera", (525.0, 525.0, 319.5, 239.5))]  # the TUM default camera
                zrange = [float(x) for x in val.get("--zrange", (0.1, 5.2))]
                h, rec, hg, gone, info = carve_file(pos[0], val["--views"][0], camera, zrange, float(val.get("--depth-scale", [5000.0])[0]),
                                                    **params)
                write(val["-o"][0], h, rec)
                if "--removed" in val:
                    write(val["--removed"][0], hg, gone)
                print("%s: %d voxels (%s carved with the views of %s: %d voxels, %d points removed)"
                      % (val["-o"][0], len(rec), pos[0], val["--views"][0], len(gone), int(gone["count"].sum(dtype=np.uint64))))
                return 0
        if cmd == "observe" and "-o" in args and "--views" in args:
            opt = {"-o": 1, "--views": 1, "--pad": 1, "--radius": 1, "--margin": 1, "--margin-rel": 1, "--camera": 4, "--zrange": 2, "--depth-scale": 1}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1:
                params = {name: conv(val[o][0]) for o, name, conv in (("--radius", "radius", int), ("--margin", "margin", float),
                                                                       ("--margin-rel", "margin_rel", float), ("--pad", "pad", int)) if o in val}
                camera = [float(x) for x in val.get("--camera", (525.0, 525.0, 319.5, 239.5))]  # the TUM default camera
                zrange = [float(x) for x in val.get("--zrange", (0.1, 5.2))]
                seen, lo, voxel, info = observe_file(pos[0], val["--views"][0], camera, zrange, float(val.get("--depth-scale", [5000.0])[0]), **params)
                write_seen(val["-o"][0], seen, lo, voxel)
                print("%s: %d x %d x %d cells from %s (the views of %s over %s): %d free, %d with a surface"
                      % ((val["-o"][0],) + seen.shape + (lo.tolist(), val["--views"][0], pos[0], info["cells_free"], info["cells_surface"])))
                return 0
        if cmd == "frontiers" and "-o" in args and "--seen" in args:
            opt = {"-o": None, "--seen": None, "--min-count": "1", "--min-views": "1"}
            pos, i = [], 0
            while i < len(args):
                if args[i] in opt and i + 1 < len(args):
                    opt[args[i]] = args[i + 1]
                    i += 2
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1 and opt["-o"] is not None and opt["--seen"] is not None:
                header, rec = read(pos[0])
                vol, lo, n = _seen_for(opt["--seen"], header["voxel"])
                cells = frontier_records(rec, lo, n, vol, int(opt["--min-count"]), int(opt["--min-views"]))
                with open(opt["-o"], "w") as f:
                    f.write("".join("%d %d %d\n" % tuple(c) for c in cells.tolist()))
                print("%s: %d frontier cells of %s seen through %s" % (opt["-o"], len(cells), pos[0], opt["--seen"]))
                return 0
        if cmd == "esdf" and "-o" in args:
            opt = {"-o": None, "--pad": "8", "--min-count": "1", "--clamp": "0", "--seen": None, "--min-views": "1"}
            pos, i = [], 0
            while i < len(args):
                if args[i] in opt and i + 1 < len(args):
                    opt[args[i]] = args[i + 1]
                    i += 2
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1 and opt["-o"] is not None:
                d2, lo, voxel, info = esdf_file(pos[0], int(opt["--pad"]), int(opt["--min-count"]), int(opt["--clamp"]), opt["--seen"],
                                                int(opt["--min-views"]))
                write_field(opt["-o"], d2, lo, voxel)
                print("%s: %d x %d x %d cells from %s (%s), %d voxels in the box%s, largest d2 %d"
                      % ((opt["-o"],) + d2.shape + (lo.tolist(), pos[0], info["solid"],
                                                    ", %d unknown cells" % info["unknown"] if "unknown" in info else "", info["max_d2"])))
                return 0
        if cmd == "df-align" and "-o" in args:
            opt = {"-o": None, "--init": None, "--max-dist": None, "--pad": None}
            pos, i = [], 0
            while i < len(args):
                if args[i] in opt and i + 1 < len(args):
                    opt[args[i]] = args[i + 1]
                    i += 2
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 2 and opt["-o"] is not None:
                T, rec, it, status = df_align_files(pos[0], pos[1], None if opt["--init"] is None else read_pose(opt["--init"]),
                                                    None if opt["--max-dist"] is None else float(opt["--max-dist"]),
                                                    None if opt["--pad"] is None else int(opt["--pad"]))
                with open(opt["-o"], "w") as f:
                    f.write("".join(" ".join("%.9g" % x for x in row) + "\n" for row in T))
                print("%s: %s after %d iterations, %d of %d points matched (%d skipped), rms residual %.4g m"
                      % (opt["-o"], ("converged", "iteration limit", "lost")[status], it, rec["matched"], rec["considered"], rec["skipped"],
                         float(np.sqrt(rec["S"][27] / max(int(rec["matched"]), 1)))))
                return 0 if status != ALIGN_LOST else 1
        if cmd == "plan" and "-o" in args:
            opt = {"-o": 1, "--goal": 3, "--start": 3, "--clearance": 1, "--pad": 1, "--cost": 1, "--seen": 1, "--min-views": 1}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val.setdefault(args[i], []).append(args[i + 1:i + 1 + k])
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1 and all(k in val for k in ("-o", "--goal", "--start", "--clearance")):
                goals = [[int(x) for x in g] for g in val["--goal"]]
                starts = [[int(x) for x in s] for s in val["--start"]]
                cost, lo, voxel, r2, info, paths = plan_file(pos[0], goals, starts, float(val["--clearance"][-1][0]),
                                                             None if "--pad" not in val else int(val["--pad"][-1][0]),
                                                             seen=val["--seen"][-1][0] if "--seen" in val else None,
                                                             min_views=int(val.get("--min-views", [["1"]])[-1][0]))
                if "--cost" in val:
                    write_cost(val["--cost"][-1][0], cost, lo, voxel, r2)
                if info["seeds_used"] == 0:
                    raise ValueError("no goal lies on a free cell of the box (%d outside it, %d closer than the clearance to a surface)"
                                     % (info["seeds_outside"], info["seeds_blocked"]))
                if not any(st in (PLAN_REACHED, PLAN_TRUNCATED) for _, st, _ in paths):
                    raise ValueError("no start reaches a goal: %s" % ", ".join(PLAN_STATUS[st] for _, st, _ in paths))
                with open(val["-o"][-1][0], "w") as f:
                    for j, (cells, st, c) in enumerate(paths):
                        f.write("# path %d from %s: %s, cost %s, %d cells, %.9g m (chamfer)\n"
                                % (j, starts[j], PLAN_STATUS[st], "none" if c == int(PLAN_NONE) else c, len(cells),
                                   0.0 if c == int(PLAN_NONE) else c * voxel / 3.0))
                        f.write("".join(" ".join("%.9g" % x for x in p) + "\n" for p in plan_path_points(cells, voxel)))
                print("%s: %d paths (%s) through %d x %d x %d cells at r2 = %d: %d free, %d reachable, largest cost %d"
                      % ((val["-o"][-1][0], len(paths), ", ".join(PLAN_STATUS[st] for _, st, _ in paths)) + cost.shape
                         + (r2, info["free"], info["reachable"], info["max_cost"])))
                return 0
        if cmd in ("gain", "next-view") and "-o" in args and "--seen" in args:
            opt = {"-o": 1, "--seen": 1, "--poses": 1, "--camera": 4, "--size": 2, "--zrange": 2, "--radius": 1, "--margin": 1, "--margin-rel": 1,
                   "--min-views": 1, "--min-count": 1, "--miss-depth": 1, "--max-steps": 1, "--start": 3, "--clearance": 1, "--headings": 1,
                   "--stride": 1, "--max-candidates": 1, "--weight": 1, "--up": 3}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            need = ("--poses",) if cmd == "gain" else ("--start", "--clearance")
            if len(pos) == 1 and all(k in val for k in need + ("--camera", "--size")):
                params = {name: conv(val[o][0]) for o, name, conv in (("--radius", "radius", int), ("--margin", "margin", float),
                                                                       ("--margin-rel", "margin_rel", float), ("--min-views", "min_views", int),
                                                                       ("--min-count", "min_count", int), ("--miss-depth", "miss_depth", float),
                                                                       ("--max-steps", "max_steps", int)) if o in val}
                view = ([float(x) for x in val["--camera"]] + [float(x) for x in val.get("--zrange", (0.1, 5.2))], [int(x) for x in val["--size"]])
                header, rec = read(pos[0])
                vol, lo, n = _seen_for(val["--seen"][0], header["voxel"])
                if cmd == "gain":
                    g = gain_records(rec, header["voxel"], lo, n, vol, view, read_poses(val["--poses"][0]), **params)
                    with open(val["-o"][0], "w") as f:
                        f.write("# unknown_free unknown_surface unknown_inside hits\n")
                        f.write("".join("%d %d %d %d\n" % (r["unknown_free"], r["unknown_surface"], r["unknown_inside"], r["hits"]) for r in g))
                    print("%s: %d poses over %d unknown of %d cells: %d free, %d surface, %d inside the views; %d of %d rays hit"
                          % (val["-o"][0], len(g), g.info["unknown"], g.info["cells"], g.info["unknown_free"], g.info["unknown_surface"],
                             g.info["unknown_inside"], g.info["ray_hits"], g.info["rays"]))
                    return 0
                extra = {name: conv(val[o][0]) for o, name, conv in (("--headings", "headings", int), ("--stride", "stride", int),
                                                                      ("--max-candidates", "max_candidates", int), ("--weight", "weight", float)) if o in val}
                if "--up" in val:
                    extra["up"] = [float(x) for x in val["--up"]]
                r = next_view_records(rec, header["voxel"], lo, n, vol, [int(x) for x in val["--start"]], float(val["--clearance"][0]), view,
                                      **extra, **params)
                with open(val["-o"][0], "w") as f:
                    f.write("".join(" ".join("%.9g" % x for x in row) + "\n" for row in r["pose"]))
                print("%s: the best of %d poses at %d positions: cell %s heading %d, %d unknown cells seen free, score %.6g, %d cells from the start"
                      % (val["-o"][0], len(r["poses"]), len(r["cells"]), r["cell"].tolist(), r["heading"], int(r["record"]["unknown_free"]),
                         r["scores"][r["index"]], len(r["path"][0])))
                return 0
        if cmd in ("tsdf", "mesh") and "-o" in args:
            opt = {"-o": 1, "--views": 1, "--pad": 1, "--trunc": 1, "--camera": 4, "--zrange": 2, "--depth-scale": 1, "--min-weight": 1}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            flags = {f for f in ("--color", "--normals", "--colors") if f in pos}
            pos = [a for a in pos if a not in flags]
            if cmd == "tsdf" and len(pos) == 1 and "--views" in val:
                camera = [float(x) for x in val.get("--camera", (525.0, 525.0, 319.5, 239.5))]  # the TUM default camera
                zrange = [float(x) for x in val.get("--zrange", (0.1, 5.2))]
                res = tsdf_file(pos[0], val["--views"][0], camera, zrange, float(val.get("--depth-scale", [5000.0])[0]),
                                int(val.get("--pad", [0])[0]), float(val["--trunc"][0]) if "--trunc" in val else None, color="--color" in flags)
                cells, lo, voxel, trunc, info = res[:5]
                write_tsdf(val["-o"][0], cells, lo, voxel, trunc, res[5] if "--color" in flags else None)
                print("%s: %d x %d x %d cells from %s (the views of %s over %s), trunc %g m: %d with a weight, %d inside%s"
                      % ((val["-o"][0],) + cells.shape + (lo.tolist(), val["--views"][0], pos[0], trunc, info["cells_weighted"], info["cells_inside"],
                                                          ", %d coloured" % info["cells_colored"] if "--color" in flags else "")))
                return 0
            if cmd == "mesh" and len(pos) == 1:
                cells, lo, voxel, _, col = read_tsdf(pos[0], color=True)
                mw = int(val.get("--min-weight", [1])[0])
                if "--colors" in flags and col is None:
                    raise ValueError("%s holds no colour volume (mapfile tsdf --color writes one)" % pos[0])
                if flags:
                    m = mesh_attr_records(cells, col if "--colors" in flags else None, lo, voxel, mw)
                    if "--normals" not in flags:
                        m.normals = None
                else:
                    m = mesh_records(cells, lo, voxel, mw)
                m.save_ply(val["-o"][0])
                print("%s: %d vertices, %d triangles from %d active cubes of %s" % (val["-o"][0], len(m.vertices), len(m.triangles),
                                                                                   m.info["cubes_active"], pos[0]))
                return 0
        if cmd == "surface-views" and "-o" in args and "--poses" in args:
            opt = {"-o": 1, "--poses": 1, "--camera": 4, "--size": 2, "--zrange": 2, "--step": 1, "--min-weight": 1, "--max-steps": 1, "--depth-scale": 1}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            with_normals = "--normals" in pos
            pos = [a for a in pos if a != "--normals"]
            if len(pos) == 1 and "--camera" in val and "--size" in val:
                from . import api, tum
                vol = api.TsdfVolume.load(pos[0])
                poses = [(float(j), T) for j, T in enumerate(read_poses(val["--poses"][0]))]  # the time stamps: the poses' numbers
                n = tum.write_surface_views(val["-o"][0], vol, poses, depth_scale=float(val.get("--depth-scale", [5000.0])[0]), batch=64,
                                            normals=with_normals, camera=[float(x) for x in val["--camera"]], size=[int(x) for x in val["--size"]],
                                            zrange=[float(x) for x in val.get("--zrange", (0.1, 5.2))],
                                            step=float(val["--step"][0]) if "--step" in val else None, min_weight=int(val.get("--min-weight", [1])[0]),
                                            max_steps=int(val.get("--max-steps", [4096])[0]))
                print("%s: %d views of the surface in %s (%s colour%s)" % (val["-o"][0], n, pos[0], "with" if vol.color is not None else "without",
                                                                           ", normals" if with_normals else ""))
                return 0
        if cmd == "surface-track" and "-o" in args and "--views" in args:
            opt = {"-o": 1, "--views": 1, "--stride": 1, "--max-dist": 1, "--min-weight": 1, "--camera": 4, "--zrange": 2, "--depth-scale": 1}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1:
                from . import vo
                params = {name: conv(val[o][0]) for o, name, conv in (("--stride", "stride", int), ("--max-dist", "max_dist", float),
                                                                       ("--min-weight", "min_weight", int)) if o in val}
                camera = [float(x) for x in val.get("--camera", (525.0, 525.0, 319.5, 239.5))]  # the TUM default camera
                zrange = [float(x) for x in val.get("--zrange", (0.1, 5.2))]
                res = tsdf_track_file(pos[0], val["--views"][0], camera, zrange, float(val.get("--depth-scale", [5000.0])[0]), **params)
                names = ("converged", "iteration limit", "lost")
                with open(val["-o"][0], "w") as f:
                    f.write("# timestamp matched considered skipped iterations status\n")
                    for ts, _, _, rec, it, status in res:
                        f.write("# %.6f %d %d %d %d %s\n" % (ts, rec["matched"], rec["considered"], rec["skipped"], it, names[status].replace(" ", "_")))
                    f.write("".join(line + "\n" for line in vo.tum_lines([(ts, T) for ts, _, T, _, _, _ in res])))
                print("%s: %d frames of %s tracked against %s: %d converged, %d lost, %d matched pixels"
                      % (val["-o"][0], len(res), val["--views"][0], pos[0], sum(r[5] == ALIGN_CONVERGED for r in res),
                         sum(r[5] == ALIGN_LOST for r in res), sum(int(r[3]["matched"]) for r in res)))
                return 0
        if cmd == "tsdf-unfuse" and "-o" in args and "--views" in args:
            opt = {"-o": 1, "--views": 1, "--only": 1, "--camera": 4, "--zrange": 2, "--depth-scale": 1}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1:
                only = [int(x) for x in val["--only"][0].split(",")] if "--only" in val else None
                camera = [float(x) for x in val.get("--camera", (525.0, 525.0, 319.5, 239.5))]  # the TUM default camera
                zrange = [float(x) for x in val.get("--zrange", (0.1, 5.2))]
                try:
                    cells, lo, voxel, trunc, info, col = tsdf_unfuse_file(pos[0], val["--views"][0], camera, zrange,
                                                                          float(val.get("--depth-scale", [5000.0])[0]), only)
                except TsdfUnfuseRefused as e:
                    print("%s: refused, nothing written: %s" % (pos[0], e))
                    return 1
                write_tsdf(val["-o"][0], cells, lo, voxel, trunc, col)
                print("%s: %d updates%s of %s taken out of %s: %d cells weighted, %d inside"
                      % (val["-o"][0], info["updates"], " and %d colour updates" % info["color_updates"] if col is not None else "",
                         val["--views"][0], pos[0], info["cells_weighted"], info["cells_inside"]))
                return 0
        if cmd == "surface-assemble" and "-o" in args:
            opt = {"-o": 1, "--box": 6}
            val, pos, i = {}, [], 0
            while i < len(args):
                k = opt.get(args[i])
                if k and len(args[i + 1:i + 1 + k]) == k:
                    val[args[i]] = args[i + 1:i + 1 + k]
                    i += 1 + k
                else:
                    pos.append(args[i])
                    i += 1
            if len(pos) == 1:
                box = None
                if "--box" in val:
                    b = [int(x) for x in val["--box"]]
                    box = (b[:3], b[3:])
                cells, color, lo, voxel, trunc = surface_assemble_file(pos[0], box)
                write_tsdf(val["-o"][0], cells, lo, voxel, trunc, color)
                print("%s: %d x %d x %d cells from %s of the store %s: %d with a weight"
                      % ((val["-o"][0],) + cells.shape + (lo.tolist(), pos[0], int((cells["weight"] > 0).sum()))))
                return 0
        if cmd == "ply" and len(args) in (1, 2):
            from . import ply
            out = args[1] if len(args) == 2 else (args[0][:-4] if args[0].endswith(".rvm") else args[0]) + ".ply"
            _, rec = read(args[0])
            ply.write_voxel_ply(out, *to_points(rec))
            print("%s: %d voxels -> %s" % (args[0], len(rec), out))
            return 0
    except (ValueError, OSError) as e:
        print("mapfile: %s" % e)
        return 1
    print("usage: python -m revo_amd.mapfile info FILE... | merge OUT FILE... | subtract A B -o OUT | coarsen A SHIFT -o OUT | "
          "transform A POSE.txt -o OUT [--voxel V] [--min-count N] | carve A --views DIR -o OUT [--removed R] [--radius N] [--margin M] "
          "[--margin-rel F] [--min-views K] [--min-count N] [--max-count N] [--camera FX FY CX CY] [--zrange ZMIN ZMAX] [--depth-scale S] | "
          "observe A --views DIR -o SEEN.npz [--pad N] [--radius N] [--margin M] [--margin-rel F] [--camera FX FY CX CY] [--zrange ZMIN ZMAX] "
          "[--depth-scale S] | frontiers A --seen SEEN.npz -o CELLS.txt [--min-count N] [--min-views K] | "
          "esdf A -o OUT.npz [--pad N] [--min-count N] [--clamp D2] [--seen SEEN.npz] [--min-views K] | df-align DST SRC [--init POSE.txt] [--max-dist M] [--pad N] -o POSE.txt | "
          "plan A --goal X Y Z [--goal ...] --start X Y Z [--start ...] --clearance M [--pad N] [--seen SEEN.npz] [--min-views K] -o PATH.txt "
          "[--cost OUT.npz] | "
          "gain A --seen SEEN.npz --poses POSES.txt --camera FX FY CX CY --size W H [--zrange ZMIN ZMAX] [--radius N] [--margin M] [--margin-rel F] "
          "[--min-views K] [--min-count N] [--miss-depth D] [--max-steps N] -o GAIN.txt | "
          "next-view A --seen SEEN.npz --start X Y Z --clearance M --camera FX FY CX CY --size W H [--headings N] [--stride N] [--max-candidates N] "
          "[--weight W] [--up X Y Z] [the options of gain] -o POSE.txt | "
          "tsdf-unfuse TSDF.npz --views DIR [--only I,J,...] -o OUT.npz [--camera FX FY CX CY] [--zrange ZMIN ZMAX] [--depth-scale S] | "
          "tsdf A --views DIR -o TSDF.npz [--color] [--trunc M] [--pad N] [--camera FX FY CX CY] [--zrange ZMIN ZMAX] [--depth-scale S] | "
          "mesh TSDF.npz -o MESH.ply [--min-weight K] [--normals] [--colors] | "
          "surface-views TSDF.npz --poses POSES.txt --camera FX FY CX CY --size W H [--zrange ZMIN ZMAX] [--step M] [--min-weight K] [--max-steps N] "
          "[--depth-scale S] [--normals] -o DIR | "
          "surface-track TSDF.npz --views DIR [--stride K] [--max-dist M] [--min-weight K] [--camera FX FY CX CY] [--zrange ZMIN ZMAX] "
          "[--depth-scale S] -o POSES.txt | "
          "surface-assemble STORE.npz [--box I0 J0 K0 N0 N1 N2] -o TSDF.npz | "
          "ply FILE [OUT.ply]")
    return 2


if __name__ == "__main__":
    sys.exit(main())
