"""Planning through the map on the device (revo_map_plan / revo_map_plan_paths / revo_map_plan_last, api.DistanceField.plan,
api.CostField, api.VoxelMap.plan_into / plan_paths_into): costs and the info record bit for bit the specification
tests/map_plan_ref.py (a heapq Dijkstra) from host and device fields and outputs on every shared case -- tile rims, partial
tiles, the moves across tile faces, edges and corners, the seed rules, runs of many rounds -- and revo_amd.mapfile's restatement
on a 64^3 box of the scene map's field; the same bytes on every run; the round limit; paths bit for bit from 256 starts with
all four statuses; every argument rule with the outputs untouched; and the API with the window."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import mapfile  # noqa: E402
from revo_amd.settings import MapDfBox, PLAN_NONE  # noqa: E402

import map_plan_cases as pc  # noqa: E402
import map_plan_ref as pr  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402

RAW = mapfile.RAW_DTYPE
INVALID_ARG, CAPACITY = -1, -5
V = 2.0 ** -6
SENTINEL = 0x07070707
SEED_DTYPE = np.dtype([("cell", "<i4", (3,)), ("cost0", "<u4")])


def _box(lo, n):
    return MapDfBox((C.c_int32 * 3)(*[int(x) for x in lo]), (C.c_int32 * 3)(*[int(x) for x in n]))


@functools.lru_cache(maxsize=None)
def _map():
    """The field and the cost are arguments: the map gives the context, the stream and the voxel edge only."""
    return tr._hand(np.zeros(0, RAW), V)


@functools.lru_cache(maxsize=None)
def _spec(name):
    c = [x for x in pc.cached_cases() if x["name"] == name][0]
    return pr.plan(c["d2"], c["lo"], c["seeds"], c["r2"])


def _seeds(seeds):
    rec = np.zeros(len(seeds), SEED_DTYPE)
    s = np.asarray(seeds, np.int64).reshape(-1, 4)
    rec["cell"], rec["cost0"] = s[:, :3], s[:, 3]
    return rec


def _plan(d2, lo, seeds, r2, device=False, max_rounds=0, m=None):
    """revo_map_plan into sentinel-filled host or device outputs, from a host or device field -> (rc, cost, info dict or the
    raw sentinel words)."""
    from revo_amd import _lib
    m = m or _map()
    L = _lib.lib()
    box = _box(lo, d2.shape)
    rec = _seeds(seeds)
    if device:
        import torch
        dev = "cuda:%d" % m.cameraPyr.device
        f = torch.from_numpy(np.ascontiguousarray(d2).view(np.int32)).to(dev)
        c = torch.full(d2.shape, SENTINEL, dtype=torch.int32, device=dev)
        i = torch.full((8,), 9, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        rc = L.revo_map_plan(m._h, C.byref(box), C.c_void_p(f.data_ptr()), 1, r2, len(rec), rec.ctypes.data_as(C.c_void_p), max_rounds,
                             C.c_void_p(c.data_ptr()), 1, C.c_void_p(i.data_ptr()))
        m.sync()
        assert f.cpu().numpy().view(np.uint32).tobytes() == d2.tobytes()  # the field is not written
        cost, words = c.cpu().numpy().view(np.uint32), i.cpu().numpy().view(np.uint64)
    else:
        cost = np.full(d2.shape, SENTINEL, np.uint32)
        words = np.full(8, 9, np.uint64)
        keep = d2.copy()
        rc = L.revo_map_plan(m._h, C.byref(box), d2.ctypes.data_as(C.c_void_p), 0, r2, len(rec), rec.ctypes.data_as(C.c_void_p), max_rounds,
                             cost.ctypes.data_as(C.c_void_p), 0, words.ctypes.data_as(C.c_void_p))
        assert d2.tobytes() == keep.tobytes()
    if rc:
        return rc, cost, words
    assert words[7] == 0
    return rc, cost, dict(zip(mapfile.PLAN_INFO_KEYS, (int(x) for x in words[:7])))


@pytest.mark.parametrize("case", pc.cached_cases(), ids=lambda c: c["name"])
def test_cases_bit_exact(case):
    want = _spec(case["name"])
    for device in (False, True):
        rc, cost, info = _plan(case["d2"], case["lo"], case["seeds"], case["r2"], device)
        ms, rounds = _map().last_plan()
        print("%s (%s): %s, %d rounds, %.3f ms" % (case["name"], "device" if device else "host", info, rounds, ms))
        assert rc == 0 and cost.dtype == np.uint32 and cost.shape == want[0].shape
        assert cost.tobytes() == want[0].tobytes(), (case["name"], device, int(np.sum(cost != want[0])))
        assert info == want[1], (case["name"], device, info, want[1])
        assert ms > 0 and (rounds >= 1) == (want[1]["seeds_used"] > 0)
        if case["name"].startswith("a line"):
            assert cost[-1, 0, 0] == 3 * 1023 and rounds >= 128  # a tile cannot be reached before the 127 in front of it have run
        if case["name"].startswith("the 40"):
            assert rounds > 10  # ten corridors, each a round at the very least


@functools.lru_cache(maxsize=None)
def _scene_field():
    """A 64^3 box of the scene map's field around its median voxel, built on the device (test_gpu_map_field.py holds that
    field to the restatement), with a free cell of it as the seed."""
    rec = tr._scene_records()
    k = mapfile.key_axes(rec["key"])
    lo = np.median(k, 0).astype(np.int64) - 32
    m = tr._hand(rec, tr.VOXEL)
    f = m.distance_field(lo=lo, n=(64, 64, 64))
    assert f.info["solid"] >= 500
    return m, f


@pytest.mark.parametrize("r2", [1, 9])
def test_the_scene_field(r2):
    m, f = _scene_field()
    free = np.argwhere(f.d2 >= r2)
    seeds = [tuple(int(v) for v in free[len(free) // 2] + f.lo) + (0,), tuple(int(v) for v in free[7] + f.lo) + (1000,)]
    want = mapfile.plan_records(f.d2, f.lo, f.n, seeds, r2)
    assert 1000 < want[1]["reachable"] <= want[1]["free"] < want[1]["cells"]
    for device in (False, True):
        rc, cost, info = _plan(f.d2, f.lo, seeds, r2, device, m=m)
        print("scene 64^3 at r2 = %d (%s): %s, %d rounds, %.3f ms" % ((r2, "device" if device else "host", info) + m.last_plan()[::-1]))
        assert rc == 0 and cost.tobytes() == want[0].tobytes() and info == want[1]


def test_same_bytes_on_every_run():
    case = pc.seed_rules_case()
    runs = [_plan(case["d2"], case["lo"], case["seeds"], 1, device) for device in (False, True, False, True)]
    assert len({r[1].tobytes() + repr(r[2]).encode() for r in runs}) == 1 and runs[0][0] == 0
    rev = _plan(case["d2"], case["lo"], case["seeds"][::-1], 1, True)  # the order of the seeds does not matter
    assert rev[1].tobytes() == runs[0][1].tobytes() and rev[2] == runs[0][2]


def test_the_round_limit():
    """The serpentine's corridors are narrower than a tile, so a path re-enters tiles: one round cannot settle it."""
    from revo_amd import _lib
    s = pc.serpentine()
    for device in (False, True):
        rc, cost, words = _plan(s["d2"], s["lo"], s["seeds"], 1, device, max_rounds=1)
        assert rc == CAPACITY and b"rounds" in _lib.lib().revo_last_error() and np.all(words == 9)  # info is not written
    want = _spec(s["name"])
    rounds = _map().last_plan()[1]
    assert rounds == 1
    # a limit with room is no error (the rounds a run takes depend on which halo reads saw a neighbour's write-back of the same
    # round, so twice what one run took); the map is as usable as before
    rc, cost, info = _plan(s["d2"], s["lo"], s["seeds"], 1, True)
    need = _map().last_plan()[1]
    assert rc == 0 and cost.tobytes() == want[0].tobytes() and need > 10
    rc, cost, info = _plan(s["d2"], s["lo"], s["seeds"], 1, False, max_rounds=2 * need)
    assert rc == 0 and cost.tobytes() == want[0].tobytes() and info == want[1]
    # an open box of one tile settles in one round, so a limit of 1 is enough there
    n = (8, 8, 8)
    rc, cost, info = _plan(pc.open_box(n), (0, 0, 0), [(3, 3, 3, 0)], 1, True, max_rounds=1)
    assert rc == 0 and info["reachable"] == 512 and cost[7, 7, 7] == 20


def _paths(cost, lo, starts, max_len, device=False):
    """revo_map_plan_paths into sentinel-filled outputs from a host or device cost field -> (rc, cells, records [k, 4])."""
    from revo_amd import _lib
    m = _map()
    L = _lib.lib()
    box = _box(lo, cost.shape)
    st = np.ascontiguousarray(np.asarray(starts, np.int64).reshape(-1, 3).astype(np.int32))
    k = len(st)
    if device:
        import torch
        dev = "cuda:%d" % m.cameraPyr.device
        c = torch.from_numpy(np.ascontiguousarray(cost).view(np.int32)).to(dev)
        cells = torch.full((k, max_len, 3), SENTINEL, dtype=torch.int32, device=dev)
        rec = torch.full((k, 4), SENTINEL, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = L.revo_map_plan_paths(m._h, C.byref(box), C.c_void_p(c.data_ptr()), 1, k, st.ctypes.data_as(C.c_void_p), max_len,
                                   C.c_void_p(cells.data_ptr()), C.c_void_p(rec.data_ptr()), 1)
        m.sync()
        return rc, cells.cpu().numpy(), rec.cpu().numpy().view(np.uint32)
    cells = np.full((k, max_len, 3), SENTINEL, np.int32)
    rec = np.full((k, 4), SENTINEL, np.uint32)
    rc = L.revo_map_plan_paths(m._h, C.byref(box), cost.ctypes.data_as(C.c_void_p), 0, k, st.ctypes.data_as(C.c_void_p), max_len,
                               cells.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), 0)
    return rc, cells, rec


def _same_paths(got, want, max_len):
    rc, cells, rec = got
    assert rc == 0 and len(rec) == len(want)
    for i, (w_cells, status, c0) in enumerate(want):
        assert rec[i].tolist() == [len(w_cells), status, c0, 0], (i, rec[i], status)
        assert [tuple(r) for r in cells[i, :len(w_cells)].tolist()] == w_cells, i
        assert np.all(cells[i, len(w_cells):] == SENTINEL), i  # entries past length are not written
    return {w[1] for w in want}


@pytest.mark.parametrize("name", ["random 33 x 20 x 11, 35 % blocked, seed 1", "the seed rules", "the 40 x 40 x 8 serpentine"])
def test_paths_bit_exact(name):
    case = [c for c in pc.cached_cases() if c["name"] == name][0]
    cost = _spec(name)[0]
    starts = pc.starts_for(case, 256)
    longest = 0
    for max_len in (512, 7):
        want = pr.paths(cost, case["lo"], starts, max_len)
        longest = max(longest, max(len(w[0]) for w in want))
        for device in (False, True):
            seen = _same_paths(_paths(cost, case["lo"], starts, max_len, device), want, max_len)
        if not name.startswith("the 40"):
            assert seen == ({0, 1, 2, 3} if max_len == 7 else {0, 1, 2}), (name, max_len, seen)
    assert 7 < longest < 512
    # max_len exactly the longest path's length and one less, and one start alone
    full = pr.paths(cost, case["lo"], starts, 512)
    j = max(range(len(full)), key=lambda i: len(full[i][0]))
    for ml, status in ((longest, pr.REACHED), (longest - 1, pr.TRUNCATED)):
        want = pr.paths(cost, case["lo"], starts, ml)
        assert want[j][1] == status and len(want[j][0]) == ml
        for device in (False, True):
            _same_paths(_paths(cost, case["lo"], starts, ml, device), want, ml)
        _same_paths(_paths(cost, case["lo"], [starts[j]], ml, True), [want[j]], ml)


def test_argument_errors_write_nothing():
    import torch
    from revo_amd import _lib
    L = _lib.lib()
    m = _map()
    n = (4, 3, 5)
    d2 = np.full(n, 4, np.uint32)
    cost = np.full(n, SENTINEL, np.uint32)
    info = np.full(8, 9, np.uint64)
    seeds = _seeds([(0, 0, 0, 0), (1, 2, 3, 1 << 24)])
    good = _box((0, 0, 0), n)
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    vp = C.c_void_p
    fp, sp, cp, ip = d2.ctypes.data_as(vp), seeds.ctypes.data_as(vp), cost.ctypes.data_as(vp), info.ctypes.data_as(vp)

    def call(box=good, f=fp, df=0, r2=1, ns=2, s=sp, mr=0, c=cp, dout=0, i=ip, mm=m):
        return L.revo_map_plan(mm._h if mm is not None else None, C.byref(box) if box is not None else None, f, df, r2, ns, s, mr, c, dout, i)

    R = 1 << 20
    bad_boxes = [_box((0, 0, 0), (0, 3, 5)), _box((0, 0, 0), (4, -1, 5)), _box((0, 0, 0), (4, 3, 1025)), _box((0, 0, 0), (1024, 1024, 129)),
                 _box((-R - 1, 0, 0), n), _box((0, R - 2, 0), n), _box((0, 0, R), (1, 1, 1)), _box((-(1 << 31), 0, 0), n), _box(((1 << 31) - 1, 0, 0), n)]
    for j, b in enumerate(bad_boxes):
        assert call(b) == INVALID_ARG and L.revo_last_error(), j
    over = _seeds([(0, 0, 0, 0), (1, 2, 3, (1 << 24) + 1)])
    assert [call(mm=None), call(box=None), call(f=None), call(s=None), call(c=None), call(r2=0), call(ns=0), call(ns=(1 << 20) + 1), call(df=2), call(df=-1),
            call(dout=2), call(s=over.ctypes.data_as(vp)), call(f=vp(base + 4), df=1), call(c=vp(base + 1024 + 8), dout=1, i=None),
            call(c=vp(base + 1024), dout=1, i=vp(base + 2048 + 8)), call(bad_boxes[0], f=vp(base), df=1, c=vp(base + 1024), dout=1, i=None)] == [INVALID_ARG] * 16
    m.sync()
    assert not t.cpu().numpy().any() and np.all(cost == SENTINEL) and np.all(info == 9)
    # revo_map_plan_paths
    field = np.full(n, 6, np.uint32)
    starts = np.zeros((3, 3), np.int32)
    cells = np.full((3, 8, 3), SENTINEL, np.int32)
    rec = np.full((3, 4), SENTINEL, np.uint32)
    kp, stp, clp, rp = field.ctypes.data_as(vp), starts.ctypes.data_as(vp), cells.ctypes.data_as(vp), rec.ctypes.data_as(vp)

    def pcall(box=good, k=kp, dk=0, ns=3, s=stp, ml=8, c=clp, r=rp, dout=0, mm=m):
        return L.revo_map_plan_paths(mm._h if mm is not None else None, C.byref(box) if box is not None else None, k, dk, ns, s, ml, c, r, dout)

    assert [pcall(mm=None), pcall(box=None), pcall(k=None), pcall(s=None), pcall(c=None), pcall(r=None), pcall(ns=0), pcall(ns=(1 << 20) + 1), pcall(ml=0),
            pcall(ml=(1 << 20) + 1), pcall(dk=2), pcall(dout=-1), pcall(k=vp(base + 4), dk=1), pcall(c=vp(base + 1024 + 4), r=vp(base + 2048), dout=1),
            pcall(c=vp(base + 1024), r=vp(base + 2048 + 8), dout=1)] == [INVALID_ARG] * 15
    for j, b in enumerate(bad_boxes):
        assert pcall(b) == INVALID_ARG, j
    m.sync()
    assert not t.cpu().numpy().any() and np.all(cells == SENTINEL) and np.all(rec == SENTINEL)
    # the time of a map that has planned nothing is an error; then the good calls work, info may be NULL
    ms, rounds = C.c_float(), C.c_uint32()
    fresh = tr._hand(np.zeros(0, RAW), V)
    assert L.revo_map_plan_last(fresh._h, C.byref(ms), C.byref(rounds)) == INVALID_ARG and L.revo_map_plan_last(None, C.byref(ms), C.byref(rounds)) == INVALID_ARG
    assert call(mm=fresh) == 0 and call(mm=fresh, i=None) == 0
    assert L.revo_map_plan_last(fresh._h, None, None) == INVALID_ARG and L.revo_map_plan_last(fresh._h, C.byref(ms), None) == 0 and ms.value > 0
    assert L.revo_map_plan_last(fresh._h, None, C.byref(rounds)) == 0 and rounds.value == 1
    want = pr.plan(d2, (0, 0, 0), [(0, 0, 0, 0), (1, 2, 3, 1 << 24)], 1)
    assert cost.tobytes() == want[0].tobytes() and info.tolist() == [want[1][k] for k in pr.INFO_KEYS] + [0]
    assert pcall(k=cp) == 0 and rec[:, 1].tolist() == [0, 0, 0] and rec[0].tolist() == [1, 0, 0, 0]
    fresh.close()


def test_the_api_and_the_window():
    import torch
    import map_field_cases as fc
    api, cam = tr._scene()[:2]
    c = fc.random_case(seed=11, n=(20, 12, 9), voxels=40)
    rec = fc.records(c["cells"]).astype(RAW)
    m = tr._hand(rec, fc.V)
    f = m.distance_field(lo=c["lo"], n=c["n"])
    free = np.argwhere(f.d2 >= 2) + f.lo
    goals, starts = free[:2], np.concatenate([free[-3:], [f.lo - 1], mapfile.key_axes(rec["key"])[:1]])
    cf = f.plan(goals, r2=2)
    want = pr.plan(f.d2, f.lo, [tuple(g) + (0,) for g in goals.tolist()], 2)
    assert cf.cost.tobytes() == want[0].tobytes() and cf.info == want[1] and cf.r2 == 2 and m.last_plan()[0] > 0 and m.last_plan()[1] >= 1
    wp = pr.paths(want[0], f.lo, starts, 4096)
    p = cf.path(starts)
    assert [([tuple(r) for r in a[0].tolist()], a[1], a[2]) for a in p] == wp and [a[1] for a in p] == [0, 0, 0, 2, 1]
    assert np.array_equal(cf.path_points(starts)[0][0], mapfile.plan_path_points(p[0][0], fc.V))
    assert f.plan((goals + 0.5) * fc.V, clearance=1.2 * fc.V).cost.tobytes() == cf.cost.tobytes()  # metres; ceil(1.44) = 2
    with pytest.raises(ValueError, match="clamp"):
        m.distance_field(lo=c["lo"], n=c["n"], clamp=3).plan(goals, r2=4)
    # a closed map's field goes through mapfile: the same bytes
    g = api.DistanceField(f.d2, f.lo, f.voxel)
    assert g.plan(goals, r2=2).cost.tobytes() == cf.cost.tobytes()
    # between device tensors
    d_d2 = torch.from_numpy(f.d2.view(np.int32)).cuda()
    d_cost = torch.full(tuple(c["n"]), 7, dtype=torch.int32, device="cuda")
    d_info = torch.zeros(8, dtype=torch.int64, device="cuda")
    m.plan_into(d_cost, d_d2, c["lo"], c["n"], goals, 2, d_info=d_info)
    assert d_cost.cpu().numpy().view(np.uint32).tobytes() == cf.cost.tobytes() and d_info.cpu().numpy().tolist()[:7] == [cf.info[k] for k in pr.INFO_KEYS]
    d_cells = torch.full((len(starts), 64, 3), 7, dtype=torch.int32, device="cuda")
    d_paths = torch.zeros((len(starts), 4), dtype=torch.int32, device="cuda")
    m.plan_paths_into(d_cells, d_paths, d_cost, c["lo"], starts, 64, wait=False)
    m.sync()
    assert d_paths.cpu().numpy().tolist() == [[len(w[0]), w[1], w[2] if w[2] != PLAN_NONE else -1, 0] for w in wp]
    assert d_cells.cpu().numpy()[0, :len(wp[0][0])].tolist() == [list(r) for r in wp[0][0]] and np.all(d_cells.cpu().numpy()[0, len(wp[0][0]):] == 7)
    with pytest.raises(ValueError):
        m.plan_into(d_cost[:-1], d_d2, c["lo"], c["n"], goals, 2)
    with pytest.raises(_lib_error()):
        m.plan(f, goals, 0)
    # MapWindow forwards to its inner map
    w = api.MapWindow(cam, fc.V, window=2)
    w.map.merge_raw(rec)
    wf = w.distance_field(lo=c["lo"], n=c["n"])
    wc = wf.plan(goals, r2=2)
    assert wc.cost.tobytes() == cf.cost.tobytes() and [a[0].tolist() for a in wc.path(starts)] == [a[0].tolist() for a in p] and w.last_plan()[1] >= 1
    w.close()
    m.close()


def _lib_error():
    from revo_amd import _lib
    return _lib.RevoError
