"""Taking voxels out of the map again (revo_map_subtract_raw / revo_map_subtract, api.VoxelMap.subtract*, api.MapWindow, run_tum
--map-window) against maps built without the removed keyframes and against the restatement of the difference
(tests/map_subtract_ref.py).  Everything compared is bytes and integers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_records_ref as mrr  # noqa: E402
import map_subtract_ref as msr  # noqa: E402
from revo_amd import mapfile  # noqa: E402
from revo_amd._lib import vp  # noqa: E402
from test_gpu_voxel_map import S320, BIASES, _keyframes, _poses, _restate  # noqa: E402
from revo_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARG, CAPACITY = -1, -5
COUNTERS = ("voxels", "points_integrated", "points_dropped", "keyframes")


@pytest.fixture(scope="module")
def kfs():
    """One context, five 320x240 keyframes and their poses; keyframe 1 stands so far out that some of its points are dropped."""
    from revo_amd import api
    cam, pyrs = _keyframes(api, S320, [1101, 1102, 1103, 1104, 1105])
    Ts = _poses(5, 31)
    Ts[1][:3, 3] = [2047.5, -2047.2, 3.0]
    return cam, pyrs, Ts


def _build(kfs, idx, voxel, dense, **kw):
    from revo_amd import api
    cam, pyrs, Ts = kfs
    m = api.VoxelMap(cam, voxel, dense=dense, **kw)
    for i in idx:
        m.integrate(pyrs[i], Ts[i])
    return m


def _state(m):
    info = m.info()
    return m.export_raw().tobytes(), tuple(info[k] for k in COUNTERS)


def _whole(m):
    """Everything a refused call must leave alone."""
    return m.export_raw().tobytes(), m.info()


def _dev(rec):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).cuda()


def _hand_made(m, rec, keyframes=1):
    m.merge_raw(rec, 0, keyframes)
    assert m.export_raw().tobytes() == msr.union(rec, rec[:0]).tobytes()


# ------------------------------------------------------------------------------------------------ 1. inverse of the whole --
@pytest.mark.parametrize("voxel", [0.01, 0.05], ids=["1cm", "5cm"])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_subtract_is_the_inverse_of_the_whole(kfs, voxel, dense):
    import torch
    full = _build(kfs, [0, 1, 2, 3], voxel, dense)
    one, two = _build(kfs, [1], voxel, dense), _build(kfs, [2], voxel, dense)
    want, all4 = _state(_build(kfs, [0, 2, 3], voxel, dense)), _state(full)
    rec, i1, i2 = one.export_raw(), one.info(), two.info()
    assert want[1][0] < all4[1][0] and (not dense or i1["points_dropped"] > 0)
    assert len(np.intersect1d(full.export_raw()["key"], rec["key"])) == len(rec)
    # from the host export
    full.subtract_raw(rec, i1["points_dropped"], 1)
    assert _state(full) == want
    full.merge(one)
    assert _state(full) == all4
    # from a device export (unspecified order)
    buf = torch.empty(64 * len(rec) + 64, dtype=torch.uint8, device="cuda")
    assert one.export_raw_into(buf) == len(rec)
    full.subtract_raw(buf, i1["points_dropped"], 1, n=len(rec))
    assert _state(full) == want
    full.merge_raw(buf, i1["points_dropped"], 1, n=len(rec))
    assert _state(full) == all4
    # straight from the other map's table
    before = _state(one)
    full.subtract(one)
    assert _state(full) == want and _state(one) == before
    full.merge(one)
    # two exports concatenated: the keys of voxels both keyframes touch repeat
    both = np.concatenate([two.export_raw(), rec])
    full.subtract_raw(both, i1["points_dropped"] + i2["points_dropped"], 2)
    assert _state(full) == _state(_build(kfs, [0, 3], voxel, dense))
    full.subtract_raw(_dev(both[:0]))  # n == 0: a no-op
    full.merge_raw(_dev(both), i1["points_dropped"] + i2["points_dropped"], 2)
    assert _state(full) == all4


# ------------------------------------------------------------------------------------------------------ 2. probe chains --
def test_probe_chains_survive_a_removal():
    """40 keys that share one home slot of the smallest table (1024 slots) form one probe chain; every second one goes."""
    from revo_amd import api
    rng = np.random.default_rng(7)
    cluster = msr.keys_with_home(777, 1023, 40)
    others = [int(k) for k in np.unique(rng.integers(1 << 20, 1 << 62, 300, dtype=np.uint64)) if int(k) not in cluster]
    rec = msr.random_records(rng, cluster + others)
    rec = rec[rng.permutation(len(rec))]
    cam = api.CameraPyr(S320)
    m = api.VoxelMap(cam, 0.05, initial_voxels=1)
    _hand_made(m, rec)
    assert m.info()["capacity"] == 1024
    original = _whole(m)
    ck = np.isin(rec["key"], np.asarray(cluster[::2], np.uint64))
    removed, kept_chain = rec[ck], rec[np.isin(rec["key"], np.asarray(cluster[1::2], np.uint64))]
    assert len(removed) == 20 and len(kept_chain) == 20
    for rnd in range(2):  # a second subtraction of the same records succeeds again
        m.subtract_raw(removed if rnd else _dev(removed))
        want = msr.difference(rec, removed)
        assert m.export_raw().tobytes() == want.tobytes() == mapfile.subtract_records(rec, removed).tobytes()
        assert m.info()["voxels"] == len(rec) - 20 and m.info()["capacity"] == 1024
        # every key left in the chain is still found from its hash: adding to it must not insert it a second time
        m.merge_raw(kept_chain)
        assert m.export_raw().tobytes() == msr.union(want, kept_chain).tobytes()
        m.subtract_raw(kept_chain)
        assert m.export_raw().tobytes() == want.tobytes()
        m.merge_raw(removed)
        got = _whole(m)
        assert got[0] == original[0] and got[1]["voxels"] == original[1]["voxels"]
        assert got[1]["points_integrated"] == original[1]["points_integrated"]
    # the whole chain and nothing else, then the rest
    chain = rec[np.isin(rec["key"], np.asarray(cluster, np.uint64))]
    m.subtract_raw(_dev(chain))
    assert m.export_raw().tobytes() == msr.difference(rec, chain).tobytes()
    m.subtract_raw(msr.difference(rec, chain), 0, 1)
    assert m.info()["voxels"] == 0 and len(m.export_raw()) == 0 and m.info()["keyframes"] == 0


# ------------------------------------------------------------------------------------------------------ 3. launch edges --
@pytest.mark.parametrize("device_in", [0, 1], ids=["host", "device"])
def test_launch_edges(kfs, device_in):
    from revo_amd import api
    cam, pyrs, Ts = kfs
    rng = np.random.default_rng(11)
    keys = [int(k) for k in np.unique(rng.integers(1, 1 << 62, 700, dtype=np.uint64))]
    rec = msr.random_records(rng, keys)
    m = api.VoxelMap(cam, 0.05, dense=True)
    _hand_made(m, rec)
    give = (lambda r: _dev(r)) if device_in else (lambda r: r)
    for n in (1, 63, 64, 65, 255, 256, 257):
        part = rec[rng.permutation(len(rec))[:n]]
        m.subtract_raw(give(part))
        assert m.export_raw().tobytes() == msr.difference(rec, part).tobytes(), n
        assert m.info()["voxels"] == len(rec) - n
        m.merge_raw(give(part))
        assert m.export_raw().tobytes() == rec.tobytes(), n
    # one key in the last thread of a block and the first of the next: two parts of one voxel
    batch = rec[:300].copy()
    j = int(np.argmax(batch["count"] >= 2))
    batch[[j, 255]] = batch[[255, j]]
    ab = batch[[255, 255]].copy()
    ab["count"] = [1, int(batch["count"][255]) - 1]
    ab["sum_q"][0], ab["sum_bgr"][0] = [5, -7, 9], [1, 2, 3]
    ab["sum_q"][1], ab["sum_bgr"][1] = batch["sum_q"][255] - ab["sum_q"][0], batch["sum_bgr"][255] - ab["sum_bgr"][0]
    batch = np.concatenate([batch[:255], ab, batch[257:]])
    assert batch[255]["key"] == batch[256]["key"] and len(batch) == 300 and ab["count"][1] >= 1
    m.subtract_raw(give(batch))
    assert m.export_raw().tobytes() == msr.difference(rec, batch).tobytes()
    m.merge_raw(give(batch))
    # everything: an empty map, equal to a fresh one, and a following integration gives the restatement's bytes
    m.subtract_raw(give(m.export_raw()), 0, 1)
    fresh = api.VoxelMap(cam, 0.05, dense=True)
    assert len(m.export_raw()) == 0 and _state(m) == _state(fresh) == (b"", (0, 0, 0, 0))
    assert m.points()[0].shape == (0, 3) and m.render(Ts[0])[2] == 0
    m.integrate(pyrs[0], Ts[0])
    r = _restate(pyrs[:1], Ts[:1], 0.05, True)
    assert m.export_raw().tobytes() == mrr.records_of(r).tobytes() and m.info()["voxels"] == r.voxels()


# --------------------------------------------------------------------------------------------------------- 4. refusals --
def test_every_refusal_leaves_the_map_bit_identical(kfs):
    from revo_amd import _lib, api
    cam, pyrs, Ts = kfs
    L = _lib.lib()
    n01 = _build(kfs, [0, 1], 0.05, True).info()["voxels"]
    m = _build(kfs, [0, 1], 0.05, True, max_voxels=n01 + 5)
    with pytest.raises(_lib.RevoError):  # one refused integration, so keyframes_rejected is not 0
        m.integrate(pyrs[2], Ts[2])
    assert m.info()["keyframes_rejected"] == 1
    one = _build(kfs, [1], 0.05, True)
    rec, i1 = one.export_raw(), one.info()
    before = _whole(m)
    assert len(rec) > 2000 and i1["points_dropped"] > 0 and before[1]["points_dropped"] == i1["points_dropped"]
    full = m.export_raw()
    big = int(np.argmax(full["count"] >= 4))
    assert full["count"][big] >= 4

    def refused(r, dropped=0, keyframes=0):
        r = np.ascontiguousarray(r)
        for dev in (0, 1):
            d = _dev(r) if dev else None
            src = d.data_ptr() if dev else r.ctypes.data
            assert L.revo_map_subtract_raw(m._h, vp(src), len(r), dev, dropped, keyframes) == INVALID_ARG
            assert L.revo_last_error()
            assert _whole(m) == before

    bad = rec.copy()
    bad["key"][-1] = full["key"].max() + np.uint64(1)
    refused(bad, i1["points_dropped"], 1)                 # a missing key, the last record of a large batch
    bad = rec.copy()
    bad["count"][len(rec) // 2] = full["count"][np.searchsorted(full["key"], rec["key"][len(rec) // 2])] + np.uint64(1)
    refused(bad)                                          # one more than the voxel has
    c = int(full["count"][big])
    two = full[[big, big]].copy()                         # each fits, together they do not; in different blocks
    two["count"] = [c - 1, 2]
    two["sum_q"], two["sum_bgr"] = 0, 0
    two = np.concatenate([two[:1], rec[:399], two[1:]])
    assert full["key"][big] not in rec["key"][:399]
    refused(two)
    bad = rec.copy()
    j = int(np.argmax(bad["count"] == full["count"][np.searchsorted(full["key"], bad["key"])]))  # a voxel only keyframe 1 holds
    bad["sum_q"][j, 2] += 1
    refused(bad, i1["points_dropped"], 1)                 # count reaching 0 with sum_q off by 1
    bad = rec.copy()
    bad["sum_bgr"][j, 0] -= np.uint64(1)
    refused(bad)
    bad = rec.copy()
    bad["count"][7] = 0
    refused(bad)                                          # a record with count 0
    bad = rec.copy()
    bad["key"][300] |= np.uint64(1 << 63)
    refused(bad)                                          # key bit 63
    refused(rec, i1["points_dropped"] + 1, 1)             # more dropped points than the map counts
    refused(rec, i1["points_dropped"], 3)                 # more keyframes than the map counts
    # map against map
    assert L.revo_map_subtract(m._h, m._h) == INVALID_ARG and _whole(m) == before
    other = api.VoxelMap(cam, 0.02, dense=True)
    assert L.revo_map_subtract(m._h, other._h) == INVALID_ARG and b"voxel" in L.revo_last_error()
    assert L.revo_map_subtract(m._h, None) == INVALID_ARG and L.revo_map_subtract(None, one._h) == INVALID_ARG
    three = _build(kfs, [1, 2], 0.05, True)               # keyframe 2 is not in m
    assert L.revo_map_subtract(m._h, three._h) == INVALID_ARG and _whole(m) == before
    # argument errors
    d = _dev(rec)
    assert L.revo_map_subtract_raw(m._h, vp(d.data_ptr() + 8), len(rec) - 1, 1, 0, 0) == INVALID_ARG  # misaligned
    assert L.revo_map_subtract_raw(m._h, None, len(rec), 0, 0, 0) == INVALID_ARG
    assert L.revo_map_subtract_raw(m._h, vp(rec.ctypes.data), len(rec), 2, 0, 0) == INVALID_ARG
    assert L.revo_map_subtract_raw(m._h, vp(rec.ctypes.data), len(rec), 0, 0, -1) == INVALID_ARG
    assert L.revo_map_subtract_raw(m._h, None, 0, 0, 5, 5) == 0  # n == 0: a no-op
    assert _whole(m) == before
    # and the map is as usable as before: the same records, this time as they are
    m.subtract(one)
    assert _state(m) == _state(_build(kfs, [0], 0.05, True)) and m.info()["keyframes_rejected"] == before[1]["keyframes_rejected"]


# ------------------------------------------------------------------------------------------------ 5. invariants afterwards --
def test_max_voxels_rollback_and_growth_after_a_subtraction(kfs):
    from revo_amd import _lib
    cam, pyrs, Ts = kfs
    v = {idx: _build(kfs, idx, 0.01, True).info()["voxels"] for idx in ((0, 1), (0, 2), (0, 1, 2))}
    limit = max(v[0, 1], v[0, 2]) + 10
    assert limit < v[0, 1, 2]
    m = _build(kfs, [0, 1], 0.01, True, max_voxels=limit, initial_voxels=16)
    one = _build(kfs, [1], 0.01, True)
    with pytest.raises(_lib.RevoError) as e:
        m.integrate(pyrs[2], Ts[2])
    assert e.value.code == CAPACITY
    m.subtract(one)                          # frees voxels: they count against max_voxels no more
    assert _state(m) == _state(_build(kfs, [0], 0.01, True))
    m.integrate(pyrs[2], Ts[2])              # fits now
    want = _state(_build(kfs, [0, 2], 0.01, True))
    assert _state(m) == want
    with pytest.raises(_lib.RevoError) as e:  # does not fit: inserted, refused, rolled back over a table that had deletions
        m.integrate(pyrs[1], Ts[1])
    assert e.value.code == CAPACITY
    assert _state(m) == want and m.info()["keyframes_rejected"] == 2
    m.subtract_raw(_build(kfs, [2], 0.01, True).export_raw(), 0, 1)
    m.integrate(pyrs[1], Ts[1])
    assert _state(m) == _state(_build(kfs, [0, 1], 0.01, True))
    # growth by a large integration after a subtraction (5 cm voxels: the two keyframes leave the table at its first size)
    from revo_amd import api
    g = api.VoxelMap(cam, 0.05, dense=True, initial_voxels=16)
    for i in (0, 1):
        g.integrate(pyrs[i], Ts[i])
        g.sync()
    g.subtract_raw(_build(kfs, [0], 0.05, True).export_raw(), 0, 1)
    cap, rehashes = g.info()["capacity"], g.info()["rehashes"]
    g.integrate_many(pyrs[2:], Ts[2:])
    assert g.info()["capacity"] > cap and g.info()["rehashes"] > rehashes
    r = _restate(pyrs[1:], Ts[1:], 0.05, True)
    assert g.export_raw().tobytes() == mrr.records_of(r).tobytes()
    assert g.info()["points_dropped"] == r.points_dropped and g.info()["keyframes"] == 4


def test_render_of_the_reduced_map(kfs):
    cam, pyrs, Ts = kfs
    c0 = cam.at(0)
    camera = (c0.fx / 2, c0.fy / 2, c0.cx / 2, c0.cy / 2, 160, 120)
    for voxel, dense in ((0.01, True), (0.05, False)):
        m = _build(kfs, [0, 1, 2, 3], voxel, dense)
        m.subtract(_build(kfs, [1], voxel, dense))
        got = m.render(Ts[0], camera=camera)
        want = _build(kfs, [0, 2, 3], voxel, dense).render(Ts[0], camera=camera)
        assert got[2] == want[2] > 100
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        for a, b in zip(m.points(), _build(kfs, [0, 2, 3], voxel, dense).points()):
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------- 6. MapWindow --
@pytest.mark.parametrize("voxel,dense", [(0.01, True), (0.05, False)], ids=["1cm-dense", "5cm-edges"])
def test_map_window_holds_the_last_keyframes(kfs, voxel, dense):
    from revo_amd import api
    cam, pyrs, Ts = kfs
    w = api.MapWindow(cam, voxel, dense=dense, window=2)
    for n, (p, T) in enumerate(zip(pyrs, Ts)):
        w.integrate(p, T)
        assert len(w.keyframes) == min(n + 1, 2) and w.info()["keyframes"] == min(n + 1, 2)
    assert _state(w) == _state(_build(kfs, [3, 4], voxel, dense))
    assert [T.tobytes() for T in w.keyframes] == [Ts[3].tobytes(), Ts[4].tobytes()]
    assert w.voxel == w.map.voxel and w.dense == dense
    for window in (5, 8):
        w = api.MapWindow(cam, voxel, dense=dense, window=window)
        for p, T in zip(pyrs, Ts):
            w.integrate(p, T)
        assert _state(w) == _state(_build(kfs, [0, 1, 2, 3, 4], voxel, dense)) and len(w.keyframes) == 5
    with pytest.raises(ValueError):
        api.MapWindow(cam, voxel, window=0)


def test_run_tum_map_window(tmp_path, monkeypatch):
    """The data set of test_run_tum_map_save."""
    from revo_amd import api, run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    name = "rgbd_synth_a"
    folder = str(tmp_path / "data" / name)
    tum.write_synthetic_dataset(folder, synth.make_sequence(41, S320, 20, max_t=0.01, max_rot_deg=0.4, bias=BIASES[1]))
    _tum_yaml(tmp_path, S320, [name])
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--map", "0.05"]
    for sub, extra in (("plain", ["--map-save", "f.rvm"]), ("window", ["--map-window", "2", "--map-save", "f.rvm"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    assert run_tum.main(args + ["--map-window", "2", "--streams", "2"]) == 2  # sequential driver only
    assert run_tum.main(args + ["--map-window", "0"]) == 2
    plain, window = tmp_path / "plain", tmp_path / "window"
    assert (plain / ("poses_%s.txt" % name)).read_bytes() == (window / ("poses_%s.txt" % name)).read_bytes()
    h, rec = mapfile.read(str(window / "f.rvm"))
    rows = [[float(x) for x in ln.split()] for ln in (window / ("map_window_%s.txt" % name)).read_text().splitlines()]
    nkf = mapfile.read(str(plain / "f.rvm"))[0]["keyframes"]
    print("keyframes of the run: %d, in the window: %d" % (nkf, len(rows)))
    assert nkf >= 1 and len(rows) == min(2, nkf) == h["keyframes"] and h["voxels"] > 100
    # the same map from the data set's frames at the two reported keyframe poses
    data = list(tum.frames(folder, "associate.txt", True))
    cam = api.CameraPyr(S320)
    m = api.VoxelMap(cam, 0.05, dense=bool(h["dense"]))
    for row in rows:
        f = [f for f in data if abs(f[2] - row[0]) < 1e-6]
        assert len(f) == 1
        pyr = api.ImgPyramidRGBD(S320, cam, f[0][0], f[0][1], f[0][2], depth_scale_factor=5000.0)
        m.integrate(pyr, np.array(row[1:], np.float32).reshape(4, 4))
    assert m.export_raw().tobytes() == rec.tobytes()
    info = m.info()
    assert {k: h[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}
    if nkf > 2:  # then the plain run's map holds more than the window
        assert (plain / ("map_%s.ply" % name)).read_bytes() != (window / ("map_%s.ply" % name)).read_bytes()
