"""The voxel map as data (revo_map_export_raw / revo_map_merge_raw / revo_map_merge, api.VoxelMap.save / load,
parallel.allmerge_map, run_tum --map-save): the exported records are the restatement's byte for byte
(tests/voxel_map_ref.py through tests/map_records_ref.py), a map merged from parts is the map of the whole, a refused merge
changes nothing, and a map that was saved, loaded and continued -- or built by two ranks -- gives the uninterrupted map's file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile, synth  # noqa: E402

from test_gpu_voxel_map import S320, S640, BIASES, INVALID_ARG, CAPACITY, _poses, _keyframes, _restate, _bytes  # noqa: E402
from test_gpu_configs import SAME_PARTITION  # noqa: E402
import map_records_ref as mrr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("voxels", "points_integrated", "points_dropped", "keyframes")


def _build(api, cam, pyrs, Ts, idx, voxel, dense, **kw):
    m = api.VoxelMap(cam, voxel, dense=dense, **kw)
    for i in idx:
        m.integrate(pyrs[i], Ts[i])
    return m


def _raw(m):
    return m.export_raw().tobytes()


@pytest.mark.parametrize("s", [S320, S640], ids=["320x240", "640x480"])
@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_export_matches_the_restatement(s, dense):
    import torch
    from revo_amd import _lib, api
    cam, pyrs = _keyframes(api, s, [1001, 1002, 1003])
    Ts = _poses(3, 21)
    for voxel in (0.002, 0.02):
        m = _build(api, cam, pyrs, Ts, range(3), voxel, dense)
        want = mrr.records_of(_restate(pyrs, Ts, voxel, dense))
        rec = m.export_raw()
        assert rec.dtype == mapfile.RAW_DTYPE and len(rec) == len(want) > 100
        assert rec.tobytes() == want.tobytes()
        assert np.all(rec["key"][1:] > rec["key"][:-1])
        info = m.info()
        assert int(rec["count"].sum()) == info["points_integrated"] and len(rec) == info["voxels"]
        assert m.voxel == float(np.float32(voxel)) and m.dense == dense
        # the device export: the same set of records, in any order
        d = torch.zeros(64 * (len(rec) + 3), dtype=torch.uint8, device="cuda")
        assert m.export_raw_into(d) == len(rec)
        got = mapfile.as_records(d.cpu().numpy()[:64 * len(rec)])
        assert got[np.argsort(got["key"], kind="stable")].tobytes() == want.tobytes()
        assert not d[64 * len(rec):].any()
        # counting, and an output that is too small
        L, n = _lib.lib(), C.c_size_t()
        assert L.revo_map_export_raw(m._h, None, 0, C.byref(n), 0) == 0 and n.value == len(rec)
        small = np.full(len(rec) - 1, 0x55, np.uint8).repeat(64)
        assert L.revo_map_export_raw(m._h, small.ctypes.data_as(C.c_void_p), len(rec) - 1, C.byref(n), 0) == CAPACITY
        assert n.value == len(rec) and np.all(small == 0x55)


@pytest.mark.parametrize("dense", [False, True], ids=["edges", "dense"])
def test_split_and_merge_equals_the_whole(dense):
    import torch
    from revo_amd import api
    # three scenes, each seen twice from poses a few millimetres apart: both halves see every scene, so they share voxels
    cam, pyrs = _keyframes(api, S320, [1011, 1012, 1013, 1011, 1012, 1013])
    Ts = [synth.se3_exp(np.array([0.003 * i, 0.002 * i, 0, 0, 0.001 * i, 0])).astype(np.float32) for i in range(6)]
    voxel = 0.01
    whole = _build(api, cam, pyrs, Ts, range(6), voxel, dense)
    want = _raw(whole)
    assert want == mrr.records_of(_restate(pyrs, Ts, voxel, dense)).tobytes()
    A = _build(api, cam, pyrs, Ts, (0, 2, 4), voxel, dense)
    B = _build(api, cam, pyrs, Ts, (1, 3, 5), voxel, dense)
    ra, rb = A.export_raw(), B.export_raw()
    ia, ib = A.info(), B.info()
    shared = len(np.intersect1d(ra["key"], rb["key"]))
    assert shared > 100 and len(ra) + len(rb) - shared == whole.info()["voxels"]  # the halves really share voxels
    A.merge(B)
    assert _raw(A) == want
    assert _bytes(A.points()) == _bytes(whole.points())
    views_a, views_w = A.render(Ts[:2]), whole.render(Ts[:2])
    for k in range(2):
        assert views_a[0][k].tobytes() == views_w[0][k].tobytes() and views_a[1][k].tobytes() == views_w[1][k].tobytes()
        assert views_a[2][k] == views_w[2][k] > 100
    info = A.info()
    for k in COUNTERS[1:]:
        assert info[k] == ia[k] + ib[k] == whole.info()[k], k
    assert info["voxels"] == whole.info()["voxels"] and info["keyframes_rejected"] == 0
    assert _raw(B) == rb.tobytes() and B.info() == ib  # the source is unchanged
    # the other direction
    A2 = _build(api, cam, pyrs, Ts, (0, 2, 4), voxel, dense)
    B.merge(A2)
    assert _raw(B) == want
    # into an empty map from host exports; the source's cloud mode need not be the destination's
    E = api.VoxelMap(cam, voxel, dense=not dense)
    E.merge_raw(ra, ia["points_dropped"], ia["keyframes"])
    assert _raw(E) == ra.tobytes()
    E.merge_raw(rb.tobytes(), ib["points_dropped"], ib["keyframes"])
    assert _raw(E) == want and all(E.info()[k] == whole.info()[k] for k in COUNTERS)
    # from device exports
    D = api.VoxelMap(cam, voxel, dense=dense)
    for src, n in ((A2, len(ra)), (_build(api, cam, pyrs, Ts, (1, 3, 5), voxel, dense), len(rb))):
        d = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        assert src.export_raw_into(d) == n
        D.merge_raw(d, keyframes=3)
    assert _raw(D) == want and D.info()["keyframes"] == 6
    # one call with the concatenation: keys occur twice in it
    cat = np.concatenate([ra, rb])
    for dev in (False, True):
        M = api.VoxelMap(cam, voxel, dense=dense)
        M.merge_raw(torch.from_numpy(cat.view(np.uint8).copy()).cuda() if dev else cat, 0, 6)
        assert _raw(M) == want and all(M.info()[k] == whole.info()[k] for k in COUNTERS), dev
    M.merge_raw(cat[:0])  # no records: nothing happens
    assert _raw(M) == want


def test_growth_during_a_merge():
    from revo_amd import api
    cam, pyrs = _keyframes(api, S320, [1021, 1022, 1023, 1024])
    Ts = _poses(4, 23)
    want = _raw(_build(api, cam, pyrs, Ts, range(4), 0.005, True))
    src = _build(api, cam, pyrs, Ts, range(4), 0.005, True)
    for how in ("merge", "merge_raw"):
        m = api.VoxelMap(cam, 0.005, dense=True, initial_voxels=1024)
        assert m.info()["capacity"] == 2048
        if how == "merge":
            m.merge(src)
        else:
            m.merge_raw(src.export_raw(), 0, 4)
        info = m.info()
        assert info["rehashes"] > 0 and info["capacity"] >= 2 * info["voxels"] and _raw(m) == want, how


def test_capacity_is_all_or_nothing():
    import torch
    from revo_amd import api
    from revo_amd._lib import RevoError
    cam, pyrs = _keyframes(api, S320, [1031, 1032, 1033])
    Ts = _poses(3, 24)
    B = _build(api, cam, pyrs, Ts, (1,), 0.01, True)
    rb = B.export_raw()
    na = _restate(pyrs[:1], Ts[:1], 0.01, True).voxels()
    nab = _restate(pyrs[:2], Ts[:2], 0.01, True).voxels()
    cap = (na + nab) // 2
    assert na < cap < nab
    A = _build(api, cam, pyrs, Ts, (0,), 0.01, True, max_voxels=cap)
    before, info0 = _raw(A), A.info()
    d_rb = torch.from_numpy(rb.view(np.uint8).copy()).cuda()
    for k, call in enumerate((lambda: A.merge(B), lambda: A.merge_raw(rb, 0, 1), lambda: A.merge_raw(d_rb, 0, 1))):
        with pytest.raises(RevoError) as e:
            call()
        assert e.value.code == CAPACITY
        info = A.info()
        assert _raw(A) == before and info["keyframes_rejected"] == k + 1
        assert all(info[c] == info0[c] for c in COUNTERS), info
    # the map stays usable: an integration that fits goes in and matches the restatement
    A.integrate(pyrs[0], Ts[0])
    r = _restate([pyrs[0], pyrs[0]], [Ts[0], Ts[0]], 0.01, True)
    assert _raw(A) == mrr.records_of(r).tobytes() and A.info()["keyframes"] == 2
    # and so does a merge that fits: the map's own voxels again
    A.merge_raw(mapfile.as_records(before), 0, 1)
    r.integrate_pcl(pyrs[0].generateColoredPcl(0, True), Ts[0])
    assert _raw(A) == mrr.records_of(r).tobytes() and A.info()["points_integrated"] == r.points_integrated


def test_refusals_leave_the_map_unchanged():
    import torch
    from revo_amd import _lib, api
    L = _lib.lib()
    cam, pyrs = _keyframes(api, S320, [1041, 1042])
    Ts = _poses(2, 25)
    A = _build(api, cam, pyrs, Ts, (0,), 0.01, True)
    B = _build(api, cam, pyrs, Ts, (1,), 0.01, True)
    before, info0 = _raw(A), A.info()
    rb = B.export_raw()
    vp = C.c_void_p

    def unchanged(rejected):
        info = A.info()
        assert _raw(A) == before and all(info[c] == info0[c] for c in COUNTERS) and info["keyframes_rejected"] == rejected

    zero, high = rb.copy(), rb.copy()
    zero["count"][len(rb) // 2] = 0
    high["key"][-1] |= np.uint64(1 << 63)
    rejected = 0
    for bad in (zero, high):
        d_bad = torch.from_numpy(bad.view(np.uint8).copy()).cuda()
        for src, dev in ((bad.ctypes.data, 0), (d_bad.data_ptr(), 1)):
            assert L.revo_map_merge_raw(A._h, vp(src), len(bad), dev, 0, 2) == INVALID_ARG
            rejected += 2  # a refused merge counts its keyframes, like a refused integration
            unchanged(rejected)
    other = _build(api, cam, pyrs, Ts, (1,), 0.02, True)
    assert L.revo_map_merge(A._h, other._h) == INVALID_ARG and b"voxel" in L.revo_last_error()
    assert L.revo_map_merge(A._h, A._h) == INVALID_ARG
    assert L.revo_map_merge(A._h, None) == INVALID_ARG and L.revo_map_merge(None, B._h) == INVALID_ARG
    d_rb = torch.from_numpy(np.concatenate([np.zeros(8, np.uint8), rb.view(np.uint8)])).cuda()
    assert d_rb.data_ptr() % 16 == 0
    assert L.revo_map_merge_raw(A._h, vp(d_rb.data_ptr() + 8), len(rb), 1, 0, 1) == INVALID_ARG  # misaligned
    assert b"aligned" in L.revo_last_error()
    assert L.revo_map_merge_raw(A._h, None, len(rb), 0, 0, 1) == INVALID_ARG
    assert L.revo_map_merge_raw(A._h, None, len(rb), 1, 0, 1) == INVALID_ARG
    assert L.revo_map_merge_raw(None, vp(rb.ctypes.data), len(rb), 0, 0, 1) == INVALID_ARG
    assert L.revo_map_merge_raw(A._h, vp(rb.ctypes.data), len(rb), 2, 0, 1) == INVALID_ARG
    assert L.revo_map_merge_raw(A._h, vp(rb.ctypes.data), len(rb), 0, 0, -1) == INVALID_ARG
    n = C.c_size_t()
    assert L.revo_map_export_raw(A._h, vp(d_rb.data_ptr() + 8), len(rb), C.byref(n), 1) == INVALID_ARG
    assert L.revo_map_export_raw(A._h, None, 0, None, 0) == INVALID_ARG
    assert L.revo_map_voxel_size(None, None, None) == INVALID_ARG
    unchanged(rejected)  # argument errors count nothing
    assert _raw(B) == rb.tobytes()
    # after all of it the map still merges
    A.merge(B)
    assert _raw(A) == mrr.records_of(_restate(pyrs, Ts, 0.01, True)).tobytes()


_SAVE_SCRIPT = """import sys, numpy as np
sys.path[:0] = [%r, %r]
from revo_amd import api, synth
from test_gpu_voxel_map import S320, _keyframes, _poses
cam, pyrs = _keyframes(api, S320, [1051, 1052, 1053, 1054, 1055, 1056])
Ts = _poses(6, 26)
m = api.VoxelMap(cam, 0.01, dense=True)
for i in range(int(sys.argv[2])):
    m.integrate(pyrs[i], Ts[i])
m.save(sys.argv[1])
"""


def test_checkpoint_save_load_continue(tmp_path):
    from revo_amd import api
    script = tmp_path / "save_map.py"
    script.write_text(_SAVE_SCRIPT % (ROOT, os.path.dirname(os.path.abspath(__file__))))
    outs = []
    for k in range(2):  # two processes of the same run write the same file
        p = str(tmp_path / ("six%d.rvm" % k))
        subprocess.run([sys.executable, str(script), p, "6"], check=True, timeout=300)
        outs.append(open(p, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 64 * 1000
    half = str(tmp_path / "half.rvm")
    subprocess.run([sys.executable, str(script), half, "3"], check=True, timeout=300)
    cam, pyrs = _keyframes(api, S320, [1051, 1052, 1053, 1054, 1055, 1056])
    Ts = _poses(6, 26)
    m = api.VoxelMap.load(cam, half)
    assert m.voxel == float(np.float32(0.01)) and m.dense is True and m.info()["keyframes"] == 3
    again = str(tmp_path / "again.rvm")
    m.save(again)
    assert open(again, "rb").read() == open(half, "rb").read()
    for i in (3, 4, 5):
        m.integrate(pyrs[i], Ts[i])
    m.save(again)
    assert open(again, "rb").read() == outs[0]
    r = _restate(pyrs, Ts, 0.01, True)
    h, rec = mapfile.read(again)
    assert rec.tobytes() == mrr.records_of(r).tobytes()
    assert h == mapfile.make_header(0.01, 1, rec, r.points_dropped, 6)
    # a small table at load time grows
    small = api.VoxelMap.load(cam, again, initial_voxels=16)
    assert _raw(small) == rec.tobytes()


def test_run_tum_map_save(tmp_path, monkeypatch):
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    from revo_amd import ply, run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    names = ["rgbd_synth_a"]
    tum.write_synthetic_dataset(str(tmp_path / "data" / names[0]),
                                synth.make_sequence(41, S320, 20, max_t=0.01, max_rot_deg=0.4, bias=BIASES[1]))
    _tum_yaml(tmp_path, S320, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--map", "0.01"]
    for sub, extra in (("plain", []), ("saved", ["--map-save", "f.rvm"]), ("streams", ["--streams", "2", "--map-save", "f.rvm"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    plain, saved, streams = (tmp_path / n for n in ("plain", "saved", "streams"))
    assert not (plain / "f.rvm").exists()
    for f in ("poses_rgbd_synth_a.txt", "map_rgbd_synth_a.ply"):  # neither depends on the option
        assert (plain / f).read_bytes() == (saved / f).read_bytes() == (streams / f).read_bytes()
    h, rec = mapfile.read(str(saved / "f.rvm"))
    assert h["voxels"] > 100 and h["keyframes"] >= 1 and h["voxel"] == float(np.float32(0.01))
    want = ply.read_voxel_ply(str(saved / "map_rgbd_synth_a.ply"))
    for g, w in zip(mapfile.to_points(rec), want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert (streams / "f_rgbd_synth_a.rvm").read_bytes() == (saved / "f.rvm").read_bytes()  # one file per dataset there


_RANK_SCRIPT = """import os, sys, numpy as np
sys.path[:0] = [%r, %r]
import torch, torch.distributed as dist
from revo_amd import api, parallel
from test_gpu_voxel_map import S320, _keyframes, _poses
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
seeds = list(range(1061, 1069))
mine = parallel.shard_pairs(len(seeds), rank, world)
cam, pyrs = _keyframes(api, S320, [seeds[i] for i in mine])
Ts = _poses(len(seeds), 27)
m = api.VoxelMap(cam, 0.01, dense=True)
for p, i in zip(pyrs, mine):
    m.integrate(p, Ts[i])
assert m.info()["keyframes"] == len(mine)
parallel.allmerge_map(m, world)
m.save(os.path.join(sys.argv[1], "rank%%d.rvm" %% rank))
dist.barrier()
dist.destroy_process_group()
"""


def test_two_ranks_allmerge_to_the_single_process_map(tmp_path):
    from revo_amd import api, parallel
    script = tmp_path / "rank_map.py"
    script.write_text(_RANK_SCRIPT % (ROOT, os.path.dirname(os.path.abspath(__file__))))
    codes = parallel.spawn_ranks(str(script), [str(tmp_path)], 2, timeout=300)
    assert codes == [0, 0], codes
    cam, pyrs = _keyframes(api, S320, list(range(1061, 1069)))
    Ts = _poses(8, 27)
    m = _build(api, cam, pyrs, Ts, range(8), 0.01, True)
    single = str(tmp_path / "single.rvm")
    m.save(single)
    want = open(single, "rb").read()
    assert mapfile.read(single)[0]["keyframes"] == 8
    for r in range(2):
        assert (tmp_path / ("rank%d.rvm" % r)).read_bytes() == want, r
    # without a process group, or alone, there is nothing to merge
    before = _raw(m)
    assert parallel.allmerge_map(m, 1) is m and parallel.allmerge_map(m, 2) is m and _raw(m) == before
