"""The voxel map's raw records (include/revo_hip.h revo_map_voxel_raw) restated from tests/voxel_map_ref.py: per voxel
the packed key, the count, the sums of the 2^-20 m fixed-point coordinates and the sums of the colour bytes as B, G, R (the
restatement keeps colours as R, G, B), in ascending key order.  Written without revo_amd.mapfile, which is checked against it."""
import struct

import numpy as np

import voxel_map_ref as ref

DTYPE = np.dtype([("key", "<u8"), ("count", "<u8"), ("sum_q", "<i8", (3,)), ("sum_bgr", "<u8", (3,))])


def records_from_points(xyz, rgb, T, voxel):
    """Records of the points (keyframe frame, colours R,G,B) at pose T: keys_and_fixed and pack_keys, then per-key sums."""
    ok, k, q = ref.keys_and_fixed(ref.world_points(xyz, T), ref.F(voxel))
    return _sum(ref.pack_keys(k[ok]), q[ok], np.asarray(rgb, np.int64)[ok])


def records_of(r):
    """Records of a voxel_map_ref.VoxelMapRef."""
    if not r.keys:
        return np.zeros(0, DTYPE)
    return _sum(np.concatenate(r.keys), np.concatenate(r.q), np.concatenate(r.rgb))


def _sum(keys, q, rgb):
    uk, inv = np.unique(keys, return_inverse=True)
    out = np.zeros(len(uk), DTYPE)
    out["key"] = uk
    out["count"] = np.bincount(inv, minlength=len(uk))
    sq = np.zeros((len(uk), 3), np.int64)
    sc = np.zeros((len(uk), 3), np.int64)
    np.add.at(sq, inv, q)
    np.add.at(sc, inv, rgb)
    out["sum_q"] = sq
    out["sum_bgr"] = sc[:, ::-1]
    return out


def file_bytes(voxel, dense, rec, points_dropped, keyframes):
    """A .rvm file's bytes, field by field."""
    out = b"REVOMAP1" + struct.pack("<I", 1) + struct.pack("<f", voxel) + struct.pack("<i", dense) + struct.pack("<I", 0)
    out += struct.pack("<4Q", len(rec), int(rec["count"].sum()), points_dropped, keyframes) + bytes(8)
    assert len(out) == 64
    for r in rec:
        out += struct.pack("<2Q", int(r["key"]), int(r["count"])) + struct.pack("<3q", *[int(x) for x in r["sum_q"]])
        out += struct.pack("<3Q", *[int(x) for x in r["sum_bgr"]])
    return out
