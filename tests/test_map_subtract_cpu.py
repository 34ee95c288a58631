"""revo_amd/mapfile.py subtract_records and the `subtract` command -- the numpy inverse of merge_records -- against the
restatement (tests/map_subtract_ref.py), and the C ABI's two new declarations.  No GPU: the device's subtraction is checked
against the same restatement in tests/test_gpu_map_subtract.py."""
import os

import numpy as np
import pytest

import map_records_ref as mrr
import map_subtract_ref as msr
from revo_amd import mapfile
from test_mapfile_cpu import _header, _map

HERE = os.path.dirname(os.path.abspath(__file__))


def test_header_declares_and_library_exports_both_functions():
    from revo_amd import _lib
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    assert re.search(r"int\s+revo_map_subtract_raw\(revo_map\*\s*m,\s*const revo_map_voxel_raw\*\s*src,\s*size_t n,\s*int device_in,"
                     r"\s*size_t points_dropped,\s*int32_t keyframes\);", txt)
    assert re.search(r"int\s+revo_map_subtract\(revo_map\*\s*dst,\s*revo_map\*\s*src\);", txt)
    for name in ("revo_map_subtract_raw", "revo_map_subtract"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    L = _lib.lib()
    assert L.revo_map_subtract_raw(None, None, 0, 0, 0, 0) == -1 and L.revo_map_subtract(None, None) == -1  # no device needed


def test_subtract_records_inverts_merge_records():
    # overlapping keys: two maps of the same scene region
    a, b = mrr.records_of(_map([11, 13], 0.15)), mrr.records_of(_map([12, 14], 0.15))
    assert len(np.intersect1d(a["key"], b["key"])) > 100 and len(np.setdiff1d(b["key"], a["key"])) > 100
    whole = mapfile.merge_records(a, b)
    assert mapfile.subtract_records(whole, b).tobytes() == a.tobytes() == msr.difference(whole, b).tobytes()
    assert mapfile.subtract_records(whole, a).tobytes() == b.tobytes()
    # keys may repeat in what is subtracted, and in what it is subtracted from
    half = len(b) // 2
    twice = np.concatenate([b[half:], b[:half], a])
    assert len(mapfile.subtract_records(np.concatenate([a, b]), twice)) == 0
    three = mapfile.merge_records(whole, b)
    assert mapfile.subtract_records(three, np.concatenate([b, b])).tobytes() == a.tobytes()
    # disjoint keys: far apart, no voxel shared
    c = a.copy()
    c["key"] += np.uint64(1 << 50)
    both = mapfile.merge_records(a, c)
    assert len(both) == len(a) + len(c)
    assert mapfile.subtract_records(both, c).tobytes() == a.tobytes()
    assert mapfile.subtract_records(both, a).tobytes() == c.tobytes()
    # nothing, and everything
    e = np.zeros(0, mapfile.RAW_DTYPE)
    assert mapfile.subtract_records(a, e).tobytes() == a.tobytes()
    assert mapfile.subtract_records(a, a).tobytes() == b""
    assert mapfile.subtract_records(e, e).tobytes() == b""


def test_golden_map_without_a_half_of_itself():
    h, rec = mapfile.read(os.path.join(HERE, "golden", "small_map.rvm"))
    assert len(rec) == 5
    half = rec[::2]
    rest = mapfile.subtract_records(rec, half)
    assert rest.tobytes() == rec[1::2].tobytes() == msr.difference(rec, half).tobytes()
    assert mapfile.merge_records(rest, half).tobytes() == rec.tobytes()
    # a part of a voxel: the one with three points loses one of them
    v = rec[rec["count"] == 3].copy()
    assert len(v) == 1
    q = [int(np.rint(np.float32(x) * np.float32(1 << 20))) for x in (0.1, 0.1, 1.0)]
    v["count"], v["sum_q"], v["sum_bgr"] = 1, [q], [[30, 20, 10]]
    got = mapfile.subtract_records(rec, v)
    assert len(got) == 5 and got.tobytes() == msr.difference(rec, v).tobytes()
    assert int(got[got["key"] == v["key"][0]]["count"][0]) == 2
    assert mapfile.merge_records(got, v).tobytes() == rec.tobytes()


def test_every_refusal_raises():
    a = mrr.records_of(_map([5], 0.15))
    assert np.any(a["count"] > 1)

    def refused(b):
        with pytest.raises(ValueError):
            mapfile.subtract_records(a, b)
        with pytest.raises(ValueError):
            msr.difference(a, b)

    missing = a[:3].copy()
    missing["key"][2] = a["key"].max() + np.uint64(1)
    refused(missing)                                   # a key the map does not hold
    below = a[:3].copy()
    below["key"][0] = a["key"].min() - np.uint64(1)
    refused(below)
    more = a[:3].copy()
    more["count"][1] += 1
    refused(more)                                      # a count too large
    refused(np.concatenate([a[:3], a[2:3]]))           # two records that fit one by one, not together
    left = a[:3].copy()
    left["sum_q"][0, 1] += 1
    refused(left)                                      # count 0 with a sum left
    left = a[:3].copy()
    left["sum_bgr"][2, 0] -= 1
    refused(left)
    zero = a[:3].copy()
    zero["count"][0] = 0
    refused(zero)                                      # the records themselves
    high = a[:3].copy()
    high["key"][0] |= np.uint64(1 << 63)
    refused(high)
    with pytest.raises(ValueError):
        mapfile.subtract_records(np.zeros(0, mapfile.RAW_DTYPE), a[:1])
    # a part of a voxel may leave any sums: that is the caller's responsibility
    i = int(np.argmax(a["count"] > 1))
    part = a[i:i + 1].copy()
    part["count"] = 1
    assert len(mapfile.subtract_records(a, part)) == len(a)


def test_command_line_round_trip(tmp_path, capsys):
    ra, rb = _map([31, 32]), _map([33])
    pa, pb, pw, po = (str(tmp_path / n) for n in ("a.rvm", "b.rvm", "whole.rvm", "out.rvm"))
    for r, p in ((ra, pa), (rb, pb)):
        rec = mrr.records_of(r)
        mapfile.write(p, _header(r, rec), rec)
    assert mapfile.main(["merge", pw, pa, pb]) == 0
    assert mapfile.main(["subtract", pw, pb, "-o", po]) == 0
    assert open(po, "rb").read() == open(pa, "rb").read()
    assert "%d voxels" % ra.voxels() in capsys.readouterr().out
    assert mapfile.main(["subtract", "-o", po, pw, pa]) == 0
    assert open(po, "rb").read() == open(pb, "rb").read()
    h, _ = mapfile.read(po)
    assert h["keyframes"] == 1 and h["points_dropped"] == rb.points_dropped
    # a map without itself is a header alone
    assert mapfile.main(["subtract", pa, pa, "-o", po]) == 0
    h, rec = mapfile.read(po)
    assert os.path.getsize(po) == 64 and len(rec) == 0 and h["keyframes"] == 0 and h["points_integrated"] == 0
    # refusals: records that are not there, counters too large, another voxel edge, a missing file, a wrong call
    os.remove(po)
    assert mapfile.main(["subtract", pa, pb, "-o", po]) == 1 and not os.path.exists(po)
    rec = mrr.records_of(rb)
    for counters in ({"keyframes": 4}, {"points_dropped": ra.points_dropped + rb.points_dropped + 1}):
        mapfile.write(pb, dict(_header(rb, rec), **counters), rec)
        assert mapfile.main(["subtract", pw, pb, "-o", po]) == 1 and not os.path.exists(po)
    other = mrr.records_of(_map([34], 0.1))
    mapfile.write(pb, mapfile.make_header(0.1, 1, other), other)
    assert mapfile.main(["subtract", pw, pb, "-o", po]) == 1
    assert mapfile.main(["subtract", pw, str(tmp_path / "missing.rvm"), "-o", po]) == 1
    assert mapfile.main(["subtract", pw, pb]) == 2 and mapfile.main(["subtract", pw, pb, po]) == 2
