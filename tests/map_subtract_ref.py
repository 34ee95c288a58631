"""The difference of two voxel record sets (include/revo_hip.h revo_map_subtract_raw), restated with Python integers
and a dict, without revo_amd.mapfile (which is checked against it): per key the counts and sums of `b` leave those of `a`; a
voxel whose count reaches 0 is gone.  Also the host-side search for keys that share a home slot of the device's hash table."""
import numpy as np

from map_records_ref import DTYPE

M64 = (1 << 64) - 1


def _table(rec):
    t = {}
    for r in rec:
        v = t.setdefault(int(r["key"]), [0] * 7)
        v[0] += int(r["count"])
        for i in range(3):
            v[1 + i] += int(r["sum_q"][i])
            v[4 + i] += int(r["sum_bgr"][i])
    return t


def _records(t):
    out = np.zeros(len(t), DTYPE)
    for j, k in enumerate(sorted(t)):
        v = t[k]
        out[j] = (k, v[0], v[1:4], v[4:7])
    return out


def union(a, b):
    return _records(_table(np.concatenate([a, b])))


def difference(a, b):
    """Records of a without b (keys may repeat in either), ascending keys; ValueError where the library refuses."""
    ta, tb = _table(a), _table(b)
    for r in b:
        if int(r["count"]) == 0 or int(r["key"]) >> 63:
            raise ValueError("bad record")
    for k, v in tb.items():
        if k not in ta:
            raise ValueError("missing key")
        w = ta[k]
        if v[0] > w[0]:
            raise ValueError("count too large")
        for i in range(7):
            w[i] -= v[i]
        if w[0] == 0:
            if any(w[1:]):
                raise ValueError("count 0 with a sum left")
            del ta[k]
    return _records(ta)


def splitmix64(k):
    """map_hash of revo_map_impl.h."""
    k &= M64
    k ^= k >> 30
    k = (k * 0xbf58476d1ce4e5b9) & M64
    k ^= k >> 27
    k = (k * 0x94d049bb133111eb) & M64
    return k ^ (k >> 31)


def splitmix64_np(k):
    k = np.asarray(k, np.uint64).copy()
    k ^= k >> np.uint64(30)
    k *= np.uint64(0xbf58476d1ce4e5b9)
    k ^= k >> np.uint64(27)
    k *= np.uint64(0x94d049bb133111eb)
    return k ^ (k >> np.uint64(31))


def keys_with_home(home, mask, n, start=1):
    """The first n 63-bit keys >= start whose hash & mask == home (a vectorised search in blocks)."""
    out, base, step = [], int(start), 1 << 18
    while len(out) < n:
        k = np.arange(base, base + step, dtype=np.uint64)
        hit = k[(splitmix64_np(k) & np.uint64(mask)) == np.uint64(home)]
        out.extend(int(x) for x in hit)
        base += step
    out = out[:n]
    assert all(splitmix64(k) & mask == home for k in out)
    return out


def random_records(rng, keys):
    """One record per key with counts, signed coordinate sums and colour sums as a map could hold them."""
    rec = np.zeros(len(keys), DTYPE)
    rec["key"] = np.asarray(keys, np.uint64)
    rec["count"] = rng.integers(1, 50, len(keys))
    rec["sum_q"] = rng.integers(-(1 << 40), 1 << 40, (len(keys), 3))
    rec["sum_bgr"] = rng.integers(0, 255 * 50, (len(keys), 3))
    return rec
