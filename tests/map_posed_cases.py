"""Hand-made voxel records shared by the posed-map tests (test_map_posed_cpu.py, test_gpu_map_posed.py): means on the 2^-20 m
grid with few significant bits, so a pose that is exact in float32 moves them exactly.  Test infrastructure only."""
import numpy as np

import voxel_map_ref as ref
from map_records_ref import DTYPE

F = np.float32
I4 = np.eye(4, dtype=F)
V6 = 2.0 ** -6
SHIFT = (3, -2, 5)  # voxels of edge 2^-6


def translation(t):
    T = I4.copy()
    T[:3, 3] = t
    return T


def records_at(q, count, voxel, seed=0):
    """One record per row of q (N x 3 integers, the voxel's mean in 2^-20 m): key = floor(mean / voxel) in float32, sum_q =
    count * q, colours from the seed; rows that share a key with an earlier one are left out; ascending keys."""
    q = np.asarray(q, np.int64).reshape(-1, 3)
    count = np.broadcast_to(np.asarray(count, np.int64), (len(q),)).copy()
    p = (q.astype(np.float64) * 2.0 ** -20).astype(F)
    assert np.all(p.astype(np.float64) * 2.0 ** 20 == q)  # at most 24 significant bits
    ok, k, _ = ref.keys_and_fixed(p, F(voxel))
    assert ok.all()
    keys = ref.pack_keys(k)
    _, first = np.unique(keys, return_index=True)
    rng = np.random.default_rng(seed)
    rec = np.zeros(len(first), DTYPE)
    rec["key"], rec["count"] = keys[first], count[first]
    rec["sum_q"] = q[first] * count[first][:, None]
    rec["sum_bgr"] = rng.integers(0, 256, (len(first), 3)) * count[first][:, None]
    return rec[np.argsort(rec["key"])]


def singles(n=300, voxel=0.02, seed=11):
    """Count-1 voxels whose q has at most 24 significant bits: the identity pose gives them back byte for byte."""
    rng = np.random.default_rng(seed)
    return records_at(rng.integers(-(1 << 22), 1 << 22, (n, 3)), 1, voxel, seed)


def counted(n=300, seed=12):
    """Voxels of edge 2^-6 with counts 1 .. 5 and |q| < 2^21: a translation by whole voxels moves them exactly."""
    rng = np.random.default_rng(seed)
    return records_at(rng.integers(-(1 << 21), 1 << 21, (n, 3)), rng.integers(1, 6, n), V6, seed)


def shifted(rec, shift=SHIFT):
    """counted() moved by `shift` voxels of edge 2^-6: the keys shifted, sum_q moved by shift * 2^14 per point."""
    out = rec.copy()
    k = np.asarray(shift, np.int64)
    out["key"] = (rec["key"].astype(np.int64) + (k[0] << 42) + (k[1] << 21) + k[2]).astype(np.uint64)
    out["sum_q"] = rec["sum_q"] + rec["count"].astype(np.int64)[:, None] * (k << 14)
    return out[np.argsort(out["key"])]


def edge_cases():
    """(records of edge 2^-8, pose, destination edge 2^-10): under the pose voxel 0 stays in range, voxel 1 is pushed past
    2048 m, voxel 2 past index 2^20 - 1 (1024 m at the destination's edge) but not past 2048 m; counts 3, 5, 7."""
    q = np.array([[1 << 20, 2 << 20, 3 << 20], [2047 << 20, 0, 0], [(1023 << 20) + (1 << 19), 1 << 20, 0]], np.int64)
    return records_at(q, [3, 5, 7], 2.0 ** -8, 13), translation([1.5, 0.0, 0.0]), 2.0 ** -10


def last_index():
    """(records of edge 2^-9, pose): a voxel that lands in index 2^20 - 1 on x, the last one."""
    v = 2.0 ** -9
    q = np.array([[int(((1 << 20) - 2) * v * 2 ** 20) + (1 << 10), 1 << 12, -(1 << 12)]], np.int64)
    return records_at(q, [2], v, 14), translation([v, 0.0, 0.0])
