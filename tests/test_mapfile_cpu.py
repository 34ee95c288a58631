"""revo_amd/mapfile.py -- raw voxel records, the .rvm file, the numpy union -- against the restatement (tests/voxel_map_ref.py
through tests/map_records_ref.py).  No GPU: the device's export, merge, save and load are checked against the same restatement
in tests/test_gpu_map_merge.py."""
import os
import struct

import numpy as np
import pytest

import map_records_ref as mrr
import voxel_map_ref as ref
from revo_amd import mapfile

HERE = os.path.dirname(os.path.abspath(__file__))
I4 = np.eye(4, dtype=np.float32)


def _cloud(seed, n=4000):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(0.3, 4.0, n)], 1).astype(np.float32)
    return xyz, rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _pose(seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 0.5)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    T[:3, 3] = rng.uniform(-1, 1, 3)
    return T


def _map(seeds, voxel=0.05):
    r = ref.VoxelMapRef(voxel)
    for sd in seeds:
        r.integrate(*_cloud(sd), _pose(sd))
    return r


def _header(r, rec, dense=1):
    return mapfile.make_header(r.voxel, dense, rec, r.points_dropped, r.keyframes)


def test_record_layout_matches_the_header_struct():
    from revo_amd import _lib
    import re
    txt = open(_lib.HEADER).read()
    body = re.search(r"typedef struct revo_map_voxel_raw \{(.*?)\} revo_map_voxel_raw;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert decls == [["uint64_t", "key"], ["uint64_t", "count"], ["int64_t", "sum_q[3]"], ["uint64_t", "sum_bgr[3]"]]
    assert mapfile.RAW_DTYPE == mrr.DTYPE and mapfile.RAW_DTYPE.itemsize == 64
    assert [mapfile.RAW_DTYPE.fields[n][1] for n in ("key", "count", "sum_q", "sum_bgr")] == [0, 8, 16, 40]
    for name in ("revo_map_export_raw", "revo_map_merge_raw", "revo_map_merge", "revo_map_voxel_size"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)


def test_write_then_read_round_trips(tmp_path):
    r = _map([1, 2, 3])
    rec = mrr.records_of(r)
    assert len(rec) == r.voxels() > 1000 and int(rec["count"].sum()) == r.points_integrated
    assert np.any(rec["count"] > 1) and np.any(rec["sum_q"] < 0)
    h = _header(r, rec)
    p = str(tmp_path / "m.rvm")
    mapfile.write(p, h, rec)
    data = open(p, "rb").read()
    assert data == mrr.file_bytes(r.voxel, 1, rec, r.points_dropped, r.keyframes)
    h2, rec2 = mapfile.read(p)
    assert h2 == h and h2["keyframes"] == 3 and h2["voxel"] == float(np.float32(0.05))
    assert rec2.dtype == mapfile.RAW_DTYPE and rec2.tobytes() == rec.tobytes()
    # an empty map is a header alone
    e = np.zeros(0, mapfile.RAW_DTYPE)
    mapfile.write(p, mapfile.make_header(0.01, 0, e), e)
    h3, rec3 = mapfile.read(p)
    assert os.path.getsize(p) == 64 and h3["voxels"] == 0 and len(rec3) == 0


def test_malformed_files_raise(tmp_path):
    r = _map([4])
    rec = mrr.records_of(r)[:50]
    good = mapfile.pack(_header(r, rec), rec)
    p = tmp_path / "m.rvm"

    def refused(data):
        p.write_bytes(data)
        with pytest.raises(ValueError):
            mapfile.read(str(p))

    p.write_bytes(good)
    mapfile.read(str(p))
    refused(b"REVOMAP2" + good[8:])                               # magic
    refused(good[:8] + struct.pack("<I", 2) + good[12:])          # version
    refused(good[:-1])                                            # size
    refused(good + bytes(64))
    refused(good[:40])

    def with_records(rr, pts=None):
        pts = int(rr["count"].sum()) if pts is None else pts
        return good[:24] + struct.pack("<2Q", len(rr), pts) + good[40:64] + rr.tobytes()

    assert with_records(rec) == good
    swapped = rec.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    refused(with_records(swapped))                                # unsorted keys
    dup = rec.copy()
    dup["key"][7] = dup["key"][6]
    refused(with_records(dup))                                    # duplicate keys
    zero = rec.copy()
    zero["count"][9] = 0
    refused(with_records(zero))                                   # count == 0
    high = rec.copy()
    high["key"][-1] |= np.uint64(1 << 63)
    refused(with_records(high))                                   # key bit 63
    refused(with_records(rec, int(rec["count"].sum()) + 1))       # sum of counts != points_integrated
    # the writer refuses what the reader would
    for bad in (swapped, dup, zero, high):
        with pytest.raises(ValueError):
            mapfile.pack(dict(_header(r, rec), points_integrated=int(bad["count"].sum())), bad)
    with pytest.raises(ValueError):
        mapfile.pack(dict(_header(r, rec), voxels=len(rec) + 1), rec)


def test_merge_records_of_two_halves_is_the_whole():
    whole = mrr.records_of(_map([11, 12, 13, 14], 0.15))
    a, b = mrr.records_of(_map([11, 13], 0.15)), mrr.records_of(_map([12, 14], 0.15))
    assert len(np.intersect1d(a["key"], b["key"])) > 100 and len(whole) < len(a) + len(b)
    assert mapfile.merge_records(a, b).tobytes() == whole.tobytes()
    assert mapfile.merge_records(b, a).tobytes() == whole.tobytes()
    # keys may repeat inside an input: a concatenation merges like its parts
    e = np.zeros(0, mapfile.RAW_DTYPE)
    assert mapfile.merge_records(np.concatenate([b, a, e]), e).tobytes() == whole.tobytes()
    assert mapfile.merge_records(a, e).tobytes() == a.tobytes()
    bad = a.copy()
    bad["count"][0] = 0
    with pytest.raises(ValueError):
        mapfile.merge_records(bad, b)


def test_to_points_is_the_extraction_byte_for_byte():
    for voxel in (0.004, 0.05, 0.6):
        r = _map([21, 22, 23], voxel)
        rec = mrr.records_of(r)
        for mc in (1, 3):
            got, want = mapfile.to_points(rec, mc), r.points(mc)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    xyz, rgb, cnt = mapfile.to_points(np.zeros(0, mapfile.RAW_DTYPE))
    assert xyz.shape == (0, 3) and rgb.shape == (0, 3) and cnt.shape == (0,)


def test_golden_file_pins_the_byte_layout(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_small_map", os.path.join(HERE, "golden", "gen_small_map.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    data = open(os.path.join(HERE, "golden", "small_map.rvm"), "rb").read()
    assert len(data) == 64 + 64 * 5 < 1024
    rec = mrr.records_from_points(*gen.points(), I4, gen.VOXEL)
    assert data == mrr.file_bytes(gen.VOXEL, gen.DENSE, rec, gen.DROPPED, gen.KEYFRAMES)
    h, got = mapfile.read(os.path.join(HERE, "golden", "small_map.rvm"))
    assert h == {"voxel": 0.25, "dense": 1, "voxels": 5, "points_integrated": 7, "points_dropped": 1, "keyframes": 2}
    assert got.tobytes() == rec.tobytes()
    assert mapfile.pack(h, got) == data
    # spelled out: the voxel of (0.1, 0.1, 1.0), (0.2, 0.05, 1.1), (0.15, 0.12, 1.2) at 0.25 m is (0, 0, 4)
    v = got[got["key"] == np.uint64(((1 << 20) << 42) | ((1 << 20) << 21) | ((1 << 20) + 4))]
    assert len(v) == 1 and int(v["count"][0]) == 3
    q = [int(np.rint(np.float32(x) * np.float32(1 << 20))) for x in (0.1, 0.2, 0.15)]
    assert int(v["sum_q"][0, 0]) == sum(q) and v["sum_bgr"][0].tolist() == [30 + 7 + 200, 20 + 0 + 9, 10 + 250 + 9]


def test_command_line(tmp_path, capsys):
    from revo_amd import ply
    ra, rb, rw = _map([31, 32]), _map([33]), _map([31, 32, 33])
    pa, pb, po = (str(tmp_path / n) for n in ("a.rvm", "b.rvm", "out.rvm"))
    for r, p in ((ra, pa), (rb, pb)):
        rec = mrr.records_of(r)
        mapfile.write(p, _header(r, rec), rec)
    assert mapfile.main(["merge", po, pa, pb]) == 0
    rec = mrr.records_of(rw)
    assert open(po, "rb").read() == mapfile.pack(_header(rw, rec), rec)
    assert mapfile.main(["info", pa, po]) == 0
    assert "%d voxels" % rw.voxels() in capsys.readouterr().out
    assert mapfile.main(["ply", po]) == 0
    got = ply.read_voxel_ply(str(tmp_path / "out.ply"))
    for g, w in zip(got, rw.points()):
        assert g.tobytes() == w.tobytes()
    other = mrr.records_of(_map([34], 0.1))
    mapfile.write(pb, mapfile.make_header(0.1, 1, other), other)
    assert mapfile.main(["merge", po, pa, pb]) == 1  # voxel edges differ
    assert mapfile.main(["info", str(tmp_path / "missing.rvm")]) == 1
    assert mapfile.main([]) == 2
