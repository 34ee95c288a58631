"""Batched TSDF ray casts on the device (revo_map_tsdf_raycast_many, api.VoxelMap.surface_raycast_many_into, api.raycast_surfaces,
vo.MultiREVO.surface_views, run_tum --streams-surface-views).  The single call is the specification, byte for byte: every
job's images, hits and info are compared with revo_map_tsdf_raycast on the same device volumes, each output inside a
sentinel-filled arena whose other bytes must stay as they were.  The shapes are those of map_tsdf_ray_cases.py."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import _lib, api, mapfile  # noqa: E402
from revo_amd.settings import MapTsdfRayJob, MapTsdfRayParams  # noqa: E402

import map_carve_cases as cc  # noqa: E402
import map_seen_cases as sc  # noqa: E402
import map_tsdf_cases as tc  # noqa: E402
import map_tsdf_ray_cases as rc  # noqa: E402
import test_gpu_map_raycast as tr  # noqa: E402
import test_gpu_map_surface as ts  # noqa: E402
import test_gpu_map_tsdf as tt  # noqa: E402

F = np.float32
INVALID_ARG = -1
FILL, GAP = 0x2B, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
BORDER = ("9x9x17 block border z", "17x9x9 block border x", "9x17x9 block border y", "tilted plane 20x20x20", "far wall 5x5x33", "far wall 33x5x5")


def _spec(c, share=None, **kw):
    """A job from a case of map_tsdf_ray_cases: its volumes on the device (share: the spec whose device volumes it reads), its
    views and parameters, and which optional outputs it asks for."""
    s = dict(cells=c["cells"], color=c["color"], lo=c["lo"], views=list(c["views"]), step=c["step"], min_weight=c["min_weight"], max_steps=c["max_steps"],
             normals=True, colors=c["color"] is not None, hits=True, info=True, keep_color=False, map=None)
    s.update(kw)
    if share is not None:
        s["d_tsdf"], s["d_color"] = share["d_tsdf"], share["d_color"]
    else:
        s["d_tsdf"] = tt._as_tensor(s["cells"])
        s["d_color"] = ts._col_tensor(s["color"]) if s["color"] is not None else None
    return s


class Arena:
    """A job's outputs in one sentinel-filled device buffer, GAP bytes of it in front of, between and behind them."""

    def __init__(self, spec):
        import torch
        n = len(spec["views"])
        parts = []
        for i, (_, _, (w, h)) in enumerate(spec["views"]):
            parts.append((("depth", i), w * h * 4))
            if spec["normals"]:
                parts.append((("normals", i), w * h * 12))
            if spec["colors"]:
                parts.append((("bgr", i), w * h * 3))
        if spec["hits"]:
            parts.append((("hits", 0), 4 * n))
        if spec["info"]:
            parts.append((("info", 0), 64))
        off, self.at = GAP, {}
        for key, b in parts:
            self.at[key] = (off, b)
            off += (b + 15) // 16 * 16 + GAP
        self.buf = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")

    def ptr(self, name, i=0):
        return self.buf.data_ptr() + self.at[(name, i)][0] if (name, i) in self.at else None

    def rows(self, name, n):
        return (vp * n)(*[self.ptr(name, i) for i in range(n)]) if (name, 0) in self.at else None

    def host(self):
        return self.buf.cpu().numpy()

    def around_untouched(self, host):
        keep = np.ones(len(host), bool)
        for off, b in self.at.values():
            keep[off:off + b] = False
        return bool(np.all(host[keep] == FILL))

    def info(self, host):
        off, _ = self.at[("info", 0)]
        return dict(zip(mapfile.TSDF_RAY_INFO_KEYS, host[off:off + 56].view(np.uint64).tolist()))


def _prm(s):
    return MapTsdfRayParams(0.0 if s["step"] is None else float(s["step"]), int(s["min_weight"]), int(s["max_steps"]), 0)


def _color_ptr(s):
    return s["d_color"].data_ptr() if s["d_color"] is not None and (s["colors"] or s["keep_color"]) else None


def _single(m, s):
    """The job through revo_map_tsdf_raycast on the same device volumes -> the bytes of its arena."""
    a = Arena(s)
    n = len(s["views"])
    v, box, prm = tr._views(s["views"]), tt._box(s["lo"], s["cells"].shape), _prm(s)
    m.sync()
    code = _lib.lib().revo_map_tsdf_raycast((s["map"] or m)._h, C.byref(box), vp(s["d_tsdf"].data_ptr()), _color_ptr(s), 1, n, v, C.byref(prm),
                                            a.rows("depth", n), a.rows("normals", n), a.rows("bgr", n), a.ptr("hits"), 1, a.ptr("info"))
    assert code == 0, _lib.lib().revo_last_error()
    m.sync()
    host = a.host()
    assert a.around_untouched(host)
    return host


def _jobs(specs, arenas):
    """-> (the revo_map_tsdf_ray_job array, per job its (MapView array, depth rows, normal rows, bgr rows): what a refusal test mutates)."""
    arr = (MapTsdfRayJob * max(len(specs), 1))()
    parts = []
    for j, s, a in zip(arr, specs, arenas):
        n = len(s["views"])
        v = tr._views(s["views"])
        rows = [a.rows(name, n) for name in ("depth", "normals", "bgr")]
        j.map = s["map"]._h if s["map"] is not None else None
        j.box = tt._box(s["lo"], s["cells"].shape)
        j.prm = _prm(s)
        j.tsdf, j.color = s["d_tsdf"].data_ptr(), _color_ptr(s)
        j.n_views, j.views = n, C.addressof(v)
        j.depth, j.normal, j.bgr = (C.addressof(r) if r is not None else None for r in rows)
        j.hits, j.info = a.ptr("hits"), a.ptr("info")
        parts.append((v, rows[0], rows[1], rows[2]))
    return arr, parts


def _many(m, specs, mutate=None, n_jobs=None):
    import torch
    arenas = [Arena(s) for s in specs]
    arr, parts = _jobs(specs, arenas)
    keep = mutate(arr, parts) if mutate is not None else None
    torch.cuda.synchronize()
    code = _lib.lib().revo_map_tsdf_raycast_many(m._h, len(specs) if n_jobs is None else n_jobs, arr)
    m.sync()
    del keep
    return code, [a.host() for a in arenas], arenas


def _check(m, specs, what, want=None):
    want = [_single(m, s) for s in specs] if want is None else want
    code, got, arenas = _many(m, specs)
    assert code == 0, (what, _lib.lib().revo_last_error())
    for i, (g, w, a) in enumerate(zip(got, want, arenas)):
        assert a.around_untouched(g), (what, "job", i, "bytes around an output were written")
        if g.tobytes() != w.tobytes():
            bad = [key for key, (off, b) in a.at.items() if g[off:off + b].tobytes() != w[off:off + b].tobytes()]
            raise AssertionError((what, "job", i, "differs from the single call in", bad))
    return want


def _table():
    return [_spec(c, map=None if i % 2 else "m") for i, c in enumerate(rc.cases().values())]


def _with_map(specs, m):
    for s in specs:
        if s["map"] == "m":
            s["map"] = m
    return specs


# ------------------------------------------------------------------------------------------------------------ the whole table --
@functools.lru_cache(maxsize=None)
def _table_reference():
    """The table's jobs on a map of their own (with voxels in the boxes: they play no part) and the single calls' bytes for them,
    computed once for the tests that need them."""
    m = tt._map(sc.records_at([(0, 0, 8), (-4, -3, 6)]))
    specs = _with_map(_table(), m)
    return m, specs, [_single(m, s) for s in specs]


def test_the_whole_table_in_one_call():
    """Every case of the table as the jobs of one call -- mixed boxes, lo < 0, with and without colour, each job's own step, min_weight
    and max_steps, 1 x 1 and 16 x 12 views in one job, a 64-view job -- then the same jobs reversed, and jobs alone."""
    m, specs, want = _table_reference()
    before = m.export_raw().tobytes()
    names = list(rc.cases())
    assert any(s["color"] is None for s in specs) and any(s["color"] is not None for s in specs) and max(len(s["views"]) for s in specs) == 64
    assert len({(s["step"], s["min_weight"], s["max_steps"]) for s in specs}) >= 6 and any(min(s["lo"]) < 0 for s in specs)
    _check(m, specs, "the table", want)
    hits = 0
    for name, s, w in zip(names, specs, want):
        info = Arena(s).info(w)
        kind = rc.cases()[name]["kind"]
        assert (info["hits"] > 0) if kind == "hit" else (info["hits"] == 0) if kind == "miss" else True, (name, info)
        hits += info["hits"]
    print("the table: %d jobs, %d views, %d hits" % (len(specs), sum(len(s["views"]) for s in specs), hits))
    _check(m, specs[::-1], "the table reversed", want[::-1])
    for i in (0, names.index("64 views"), names.index("sphere"), len(specs) - 1):
        _check(m, [specs[i]], "job %d alone" % i, [want[i]])
    assert m.export_raw().tobytes() == before


def test_the_finish_does_not_show(monkeypatch):
    """REVO_MAP_TSDF_RAY_MANY_TICKET=1 hands the counters over by a ticket per job in place of the trailing launch (the variant
    profiles/multi_surface_ray_rates.py measures): the same bytes, for jobs of one view and of many."""
    m, specs, want = _table_reference()
    monkeypatch.setenv("REVO_MAP_TSDF_RAY_MANY_TICKET", "1")
    _check(m, specs, "the table, a ticket per job", want)


def test_the_masks_block_borders_in_a_batch():
    """The cases built for the mask's block border -- the sign change between the cells 7 and 8 along each axis, the tilted plane and
    the long boxes -- between volumes of other sizes, in two orders: a mask laid out at the wrong offset loses marks and hits."""
    m = tt._map()
    small = rc.cases()["2x2x2"]
    specs = []
    for name in BORDER:
        specs += [_spec(rc.cases()[name]), _spec(small)]
    want = _check(m, specs, "block borders")
    assert all(Arena(s).info(w)["hits"] > 0 for s, w in zip(specs, want))
    order = [2 * i for i in (3, 0, 5, 1, 4, 2)] + [1, 3]
    _check(m, [specs[i] for i in order], "block borders, another order", [want[i] for i in order])
    m.close()


# -------------------------------------------------------------------------------------------------------------- shared volumes --
def test_jobs_that_share_a_volume():
    """Two and five jobs on one volume with the same and with different min_weight (a shared mask, separate masks), and 65 views of
    one volume as two jobs, equal to a 64-view single call and a 1-view single call."""
    m = tt._map()
    c = rc.cases()["min_weight 1"]
    poses = [rc.I4, rc.at(rc.I4, 0.05, -0.03, 0.02), rc.at(rc.I4, -0.06, 0.02, -0.05), rc.at(rc.I4, 0.0, 0.04, 0.1), rc.at(rc.I4, 0.02, 0.0, -0.1)]
    first = _spec(c, views=[(poses[0], rc.KC, rc.SIZE)])
    for weights in ((1, 1), (1, 3), (1, 0, 3, 3, 2)):  # 0 counts as 1: one mask for both
        specs = [first if i == 0 else _spec(c, share=first, views=[(poses[i], rc.KC, rc.SIZE)]) for i in range(len(weights))]
        for s, mw in zip(specs, weights):
            s["min_weight"] = mw
        want = _check(m, specs, ("shared", weights))
        infos = [Arena(s).info(w) for s, w in zip(specs, want)]
        assert all(i["rays"] == 192 for i in infos) and sum(i["hits"] for i in infos) > 0
        if 3 in weights:  # the masks differ: the volume has cells of weight 1 and 2
            assert infos[0] != infos[list(weights).index(3)]
    c = rc.cases()["64 views"]
    a = _spec(c)
    b = _spec(c, share=a, views=[(rc.at(rc.I4, 0.03, 0.03, 0.03), c["views"][0][1], (2, 2))])
    want = _check(m, [a, b], "65 views of one volume")
    assert Arena(a).info(want[0])["rays"] == 256 and Arena(b).info(want[1])["rays"] == 4 and Arena(b).info(want[1])["hits"] > 0
    m.close()


# --------------------------------------------------------------------------------------------------------------------- limits --
def _pixel_jobs(n_jobs, n_views, seed):
    """n_jobs jobs on 2 x 2 x 2 volumes of their own, n_views 1 x 1 views each, every view from a pose of its own."""
    c = rc.cases()["2x2x2"]
    rng = np.random.default_rng(seed)
    k = (8.5, 8.5, 0.0, 0.0, rc.ZMIN, rc.ZMAX)
    specs = []
    for j in range(n_jobs):
        cells = c["cells"].copy()
        cells["sum"][:, :, 0] += j  # every volume its own bytes
        views = [(rc.at(rc.I4, *rng.uniform(-0.04, 0.04, 3)), k, (1, 1)) for _ in range(n_views)]
        specs.append(_spec(dict(c, cells=cells, color=None), views=views, normals=j % 2 == 0))
    return specs


def test_1024_jobs():
    m = tt._map()
    specs = _pixel_jobs(1024, 1, 1024)
    want = _check(m, specs, "1024 jobs")
    hits = sum(Arena(s).info(w)["hits"] for s, w in zip(specs, want))
    print("1024 jobs: %d hits" % hits)
    assert 0 < hits <= 1024
    assert _many(m, specs + specs[:1])[0] == INVALID_ARG  # 1025 jobs
    m.close()


def test_4096_views_and_one_more():
    m = tt._map()
    specs = _pixel_jobs(64, 64, 4096)
    want = _check(m, specs, "64 jobs x 64 views")
    assert sum(Arena(s).info(w)["rays"] for s, w in zip(specs, want)) == 4096 and sum(Arena(s).info(w)["hits"] for s, w in zip(specs, want)) > 0
    more = specs + _pixel_jobs(1, 1, 4097)
    code, got, _ = _many(m, more)
    assert code == INVALID_ARG and all(bool(np.all(g == FILL)) for g in got)
    m.close()


# ---------------------------------------------------------------------------------------------------------- the mask's switch --
CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_multi_surface_ray as t
print("digests", " ".join(t._table_digests()))
"""


def _table_digests():
    m = tt._map()
    code, got, _ = _many(m, _with_map(_table(), m))
    assert code == 0
    return [hashlib.sha256(g.tobytes()).hexdigest() for g in got]


def test_the_block_mask_does_not_show():
    """REVO_MAP_TSDF_RAY_MASK=0 in a fresh child process: the plain march gives the same bytes, `samples` included."""
    env = dict(os.environ)
    env["REVO_MAP_TSDF_RAY_MASK"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    plain = [ln.split()[1:] for ln in r.stdout.decode().splitlines() if ln.startswith("digests ")]
    want = [hashlib.sha256(w.tobytes()).hexdigest() for w in _table_reference()[2]]
    assert os.environ.get("REVO_MAP_TSDF_RAY_MASK", "1") != "0" and plain == [want]


# ------------------------------------------------------------------------------------------------------------ optional outputs --
def test_optional_outputs_left_null_in_some_jobs():
    c = rc.cases()["inside and outside the box"]
    m = tt._map()
    first = _spec(c)
    specs = [first]
    for normals, colors, hits, info in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False),
                                        (False, False, False, False)):
        specs.append(_spec(c, share=first, normals=normals, colors=colors, hits=hits, info=info))
    specs.append(_spec(c, share=first, colors=False, keep_color=True))  # the colour volume given, the colour images not: uncolored still counts
    want = _check(m, specs, "optional outputs")
    assert Arena(specs[-1]).info(want[-1]) == Arena(first).info(want[0]) and Arena(first).info(want[0])["hits"] > 0
    assert Arena(specs[2]).info(want[2])["uncolored"] == 0
    m.close()


# ------------------------------------------------------------------------------------------------------------ argument errors --
def test_argument_errors_write_nothing():
    import torch
    m = tt._map()
    L = _lib.lib()
    other = api.VoxelMap(api.CameraPyr(cc.settings320()), tc.V)  # a map of another context
    host = np.zeros(4096, np.uint8)
    host_ptr = (host.ctypes.data + 15) // 16 * 16
    spare = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    nan_T = [float("nan")] * 16

    def specs():
        return [_spec(rc.cases()["3x5x7 lo < 0"]), _spec(rc.cases()["1x1 and 16x12"]), _spec(rc.cases()["sphere"])]

    def refused(mutate, what, n_jobs=None):
        code, got, _ = _many(m, specs(), mutate, n_jobs)
        assert code == INVALID_ARG, (what, code)
        assert all(bool(np.all(g == FILL)) for g in got), (what, "something was written")

    def set_(i, **kw):
        def f(arr, parts):
            for k, v in kw.items():
                setattr(arr[i], k, v)
        return f

    def row_(i, which, view, value):  # which: 1 depth, 2 normal, 3 bgr
        def f(arr, parts):
            parts[i][which][view] = value
        return f

    def view_(i, view, **kw):
        def f(arr, parts):
            for k, v in kw.items():
                if k == "T_w_c":
                    parts[i][0][view].T_w_c[:] = v
                else:
                    setattr(parts[i][0][view], k, v)
        return f

    def prm_(i, **kw):
        def f(arr, parts):
            for k, v in kw.items():
                setattr(arr[i].prm, k, v)
        return f

    # across the call
    refused(lambda arr, parts: setattr(arr[1], "info", arr[0].info), "two jobs with one info record")
    refused(lambda arr, parts: row_(2, 1, 0, parts[0][1][0])(arr, parts), "two jobs with one depth image")
    refused(lambda arr, parts: row_(1, 1, 1, parts[1][2][1] + 16)(arr, parts), "a depth image inside the same view's normal image")
    refused(lambda arr, parts: setattr(arr[2], "hits", parts[0][1][0] + 16), "hit words inside another job's depth image")
    refused(lambda arr, parts: setattr(arr[0], "info", arr[2].tsdf + 64), "an info record inside another job's volume")
    refused(lambda arr, parts: row_(2, 1, 0, arr[2].color)(arr, parts), "a depth image on the job's own colour volume")
    # in a job
    refused(row_(0, 1, 0, host_ptr), "a host depth image")
    refused(row_(2, 3, 0, host_ptr), "a host colour image")
    refused(set_(1, tsdf=host_ptr), "a host volume")
    refused(set_(1, hits=host_ptr), "host hit words")
    refused(set_(0, info=host_ptr), "a host info record")
    refused(set_(1, map=other._h), "a map of another context")
    refused(set_(0, reserved=1), "a reserved word")
    refused(prm_(2, reserved=1), "the parameters' reserved word")
    refused(set_(2, color=None), "bgr without color")
    refused(view_(2, 0, width=0), "a broken view in the last job only")
    refused(view_(2, 0, T_w_c=nan_T), "a pose that is not finite in the last job only")
    refused(view_(1, 1, height=2049), "a view too tall")
    refused(view_(0, 0, fx=-1.0), "a negative focal length")
    refused(row_(1, 1, 1, None), "a NULL depth[i]")
    refused(row_(1, 2, 0, None), "a NULL normal[i] of a given array")
    refused(lambda arr, parts: row_(0, 1, 0, spare.data_ptr() + 4)(arr, parts), "a misaligned depth image")
    refused(lambda arr, parts: setattr(arr[0], "hits", spare.data_ptr() + 8), "misaligned hit words")
    refused(lambda arr, parts: setattr(arr[1], "tsdf", arr[1].tsdf + 8), "a misaligned volume")
    refused(set_(0, tsdf=None), "a NULL volume")
    refused(set_(1, views=None), "NULL views")
    refused(set_(2, depth=None), "NULL depth")
    refused(set_(0, n_views=0), "no view")
    refused(set_(1, n_views=65), "65 views in a job")
    refused(set_(1, n_views=-1), "a negative number of views")
    refused(prm_(0, step=-0.125), "a negative step")
    refused(prm_(1, step=float("nan")), "a step that is no number")
    refused(prm_(2, max_steps=(1 << 20) + 1), "too many steps")
    refused(lambda arr, parts: setattr(arr[1].box, "n", (C.c_int32 * 3)(0, 5, 7)), "a box rule")
    refused(lambda arr, parts: setattr(arr[0].box, "lo", (C.c_int32 * 3)((1 << 20) - 1, 0, 0)), "a box that leaves the index range")
    refused(lambda arr, parts: None, "no job", n_jobs=0)
    refused(lambda arr, parts: None, "a negative number of jobs", n_jobs=-1)
    refused(lambda arr, parts: None, "1025 jobs", n_jobs=1025)
    arenas = [Arena(s) for s in specs()]
    assert L.revo_map_tsdf_raycast_many(None, 3, _jobs(specs(), arenas)[0]) == INVALID_ARG and L.revo_map_tsdf_raycast_many(m._h, 3, None) == INVALID_ARG
    # touching ranges are no overlap: job 1's info right behind job 0's
    def touching(arr, parts):
        arr[1].info = spare.data_ptr() + 64
        arr[0].info = spare.data_ptr()
        arr[2].hits = spare.data_ptr() + 128
    code, _, _ = _many(m, specs(), touching)
    assert code == 0, L.revo_last_error()
    _check(m, specs(), "the same jobs untouched")
    # the API's own checks
    s = specs()[0]
    d_depth = torch.zeros((12, 16), dtype=torch.float32, device="cuda")
    job = dict(d_tsdf=s["d_tsdf"], lo=s["lo"], poses=rc.I4, camera=rc.KC[:4], size=rc.SIZE, zrange=rc.KC[4:], d_depth=d_depth)
    m.surface_raycast_many_into([job])
    with pytest.raises(ValueError):
        m.surface_raycast_many_into([dict(job, d_bgr=torch.zeros((12, 16, 3), dtype=torch.uint8, device="cuda"))])  # d_bgr needs d_color
    with pytest.raises(ValueError):
        m.surface_raycast_many_into([dict(job, d_depth=d_depth[:6])])
    with pytest.raises(ValueError):
        m.surface_raycast_many_into([dict(job, d_depth=d_depth.cpu())])
    with pytest.raises(ValueError):
        m.surface_raycast_many_into([dict(job, map=other, poses=np.zeros((65, 4, 4), F))])
    with pytest.raises(api.RevoError):
        m.surface_raycast_many_into([])
    with pytest.raises(api.RevoError):
        m.surface_raycast_many_into([dict(job, step=-1.0)])
    other.close()
    m.close()


# ------------------------------------------------------------------------------------------------------------------ the API --
KW = dict(camera=sc.KC[:4], size=rc.SIZE, zrange=sc.KC[4:])
def _boxes():
    """The wall's box (map_tsdf_cases), and the same box one cell shorter on two sides."""
    lo, n = tuple(int(x) for x in tc.wall()["lo"]), tuple(int(x) for x in tc.wall()["n"])
    return ((lo, n), ((lo[0] + 1, lo[1], lo[2]), (n[0] - 1, n[1] - 1, n[2])))


def _raw_views():
    """The wall's depth image from five poses near the first, each with a colour image of its own, on the device."""
    import torch
    rng = np.random.default_rng(34)
    d = np.ascontiguousarray(tc.wall()["views"][0][0], F)
    poses = [rc.I4, rc.at(rc.I4, 0.1, 0.0, 0.0), rc.at(rc.I4, 0.0, 0.05, 0.0), rc.at(rc.I4, -0.05, 0.0, 0.02), rc.at(rc.I4, 0.0, -0.05, -0.02)]
    return [(torch.from_numpy(d).cuda(), T, sc.KC, torch.from_numpy(rng.integers(0, 256, d.shape + (3,), dtype=np.uint8)).cuda()) for T in poses]


def _same_views(got, want, what):
    single = not isinstance(want["depth"], list)
    wrap = (lambda a: [a]) if single else (lambda a: a)
    assert len(wrap(got["depth"])) == len(wrap(want["depth"])), what
    for key in ("depth", "normals", "bgr"):
        assert (got[key] is None) == (want[key] is None), (what, key)
        if want[key] is not None:
            for i, (g, w) in enumerate(zip(wrap(got[key]), wrap(want[key]))):
                assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, key, i)
    assert got["hits"] == want["hits"] and got["info"] == want["info"], (what, got["info"], want["info"])


def test_fuse_then_raycast_without_a_wait():
    """api.fuse_surfaces followed by api.raycast_surfaces on the same handle with no synchronisation in between: per surface what
    SurfaceVolume.raycast gives."""
    m = tt._map()
    views = _raw_views()
    surfs = [api.SurfaceVolume(m, lo, n) for lo, n in _boxes()] + [api.SurfaceVolume(m, *_boxes()[1], color=False)]
    tilted = rc.at(rc.I4, 0.1, 0.0, 0.0)
    poses = [rc.I4, tilted, rc.at(rc.I4, 0.0, 0.05, -0.1)]
    for rnd in range(2):
        api.fuse_surfaces([(s, views[rnd + i] if s.d_color is not None else views[rnd + i][:3]) for i, s in enumerate(surfs)])  # only enqueued
    entries = [(surfs[0], poses) + tuple(KW.values()), (surfs[1], tilted) + tuple(KW.values()), (surfs[2], poses[:2]) + tuple(KW.values())]
    dev = api.raycast_surfaces(entries, device=True)  # enqueued behind the fuses: nothing has been waited for
    got = api.raycast_surfaces(entries)
    want = [s.raycast(e[1], **KW) for s, e in zip(surfs, entries)]
    print("hits per entry:", [w["info"]["hits"] for w in want])
    assert all(w["info"]["hits"] > 0 for w in want) and want[2]["bgr"] is None and got[1]["depth"].shape == (12, 16)
    for i, (g, w, d) in enumerate(zip(got, want, dev)):
        _same_views(g, w, ("entry", i))
        n = 1 if i == 1 else len(w["depth"])
        assert d["depth"].cpu().numpy().tobytes() == np.stack(w["depth"] if i != 1 else [w["depth"]]).tobytes() and tuple(d["hits"].shape) == (n,)
        assert d["info"].cpu().numpy().tolist()[:7] == [w["info"][k] for k in mapfile.TSDF_RAY_INFO_KEYS]
    fine = api.raycast_surfaces([(surfs[0], tilted) + tuple(KW.values())], step=0.05, normals=False, colors=False)[0]
    _same_views(fine, surfs[0].raycast(tilted, step=0.05, normals=False, colors=False, **KW), "its parameters")
    assert api.raycast_surfaces([]) == []
    m.close()


def test_windows_a_following_surface_and_130_poses():
    import torch
    m = tt._map()
    views = _raw_views()
    win = api.SurfaceWindow(m, *_boxes()[1], window=2)
    for v in views[:3]:
        win.integrate(v)
    rng = np.random.default_rng(130)
    poses = np.stack([rc.at(rc.I4, *rng.uniform(-0.1, 0.1, 3)) for _ in range(130)])
    plain = api.SurfaceVolume(m, *_boxes()[0])
    plain.integrate(views[0])
    got = api.raycast_surfaces([(win, poses) + tuple(KW.values()), (plain, poses[:3]) + tuple(KW.values())])
    parts = [win.raycast(poses[a:a + 64], **KW) for a in (0, 64, 128)]
    want = {k: sum((p[k] for p in parts), []) for k in ("depth", "normals", "bgr", "hits")}
    want["info"] = {k: sum(p["info"][k] for p in parts) for k in mapfile.TSDF_RAY_INFO_KEYS}
    print("130 poses:", want["info"])
    assert len(want["depth"]) == 130 and want["info"]["hits"] > 0
    _same_views(got[0], want, "130 poses of a window")
    _same_views(got[1], plain.raycast(poses[:3], **KW), "beside them")
    dev = api.raycast_surfaces([(win, poses) + tuple(KW.values())], device=True)[0]
    assert tuple(dev["depth"].shape) == (130, 12, 16) and dev["hits"].cpu().numpy().tolist() == want["hits"]
    assert dev["info"].cpu().numpy().tolist()[:7] == [want["info"][k] for k in mapfile.TSDF_RAY_INFO_KEYS]
    # MapWindow forwards the call: the window's voxels play no part
    mw = api.MapWindow(m.cameraPyr, tc.V, window=2)
    d_depth = torch.zeros((3, 12, 16), dtype=torch.float32, device="cuda")
    mw.surface_raycast_many_into([dict(d_tsdf=plain.d_tsdf, lo=plain.lo, poses=poses[:3], d_depth=d_depth, **KW)])
    assert d_depth.cpu().numpy().tobytes() == np.stack(got[1]["depth"]).tobytes()
    on_window = api.SurfaceVolume(mw, *_boxes()[0])
    on_window.integrate(views[0])
    _same_views(api.raycast_surfaces([(on_window, poses[:3]) + tuple(KW.values())])[0], got[1], "a surface on a MapWindow")
    with pytest.raises(NotImplementedError):
        api.raycast_surfaces([(plain, poses[:3]) + tuple(KW.values()), (api.FollowingSurface(m, (8, 8, 8)), poses[:1]) + tuple(KW.values())])
    mw.close()
    m.close()


# ------------------------------------------------------------------------------------------------------------------ drivers --
def test_multirevo_surface_views(monkeypatch):
    """vo.MultiREVO.surface_views on the three 160 x 120 streams of test_gpu_multi_surface, under SAME_PARTITION as that test runs:
    per stream the views of vo.REVO(surface=) + SurfaceVolume.raycast on that sequence alone."""
    import torch
    import test_gpu_multi_surface as ms
    from lm_settings_cases import S160
    from revo_amd import vo
    from test_gpu_configs import SAME_PARTITION
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    single = ms._single_driver(False)
    seqs = ms._driver_sequences()
    mv = vo.MultiREVO(S160, 3)
    vms = [api.VoxelMap(mv.camPyr, ms.DRIVER_VOXEL, dense=True) for _ in range(3)]
    surfs = [api.SurfaceVolume(vm, **ms.DRIVER_BOX) for vm in vms]
    for s in range(3):
        mv.attach_map(s, vms[s])
        mv.attach_surface(s, surfs[s])
    its, done = [iter(q) for q in seqs], [False] * 3
    while not all(done) or any(mv.pending(s) > 0 for s in range(3)):  # the streams stay attached: no reset at a sequence's end
        frames = []
        for s in range(3):
            if not done[s] and mv.pending(s) < mv.max_queue:
                f = next(its[s], None)
                done[s] = f is None
                if f is not None:
                    frames.append((s, f[0], f[1], f[2]))
        if frames:
            mv.submit(frames)
        if any(mv.pending(s) > 0 for s in range(3)):
            mv.step()
    poses = [[T for _, T, _, _ in s["kfs"]] for s in single]
    assert all(len(p) >= 3 for p in poses)
    got = mv.surface_views({0: poses[0], 2: (poses[2],)}, normals=True)  # behind the last step's fuse; stream 1 in a call of its own
    got.update(mv.surface_views([None, poses[1][0], None]))
    assert sorted(got) == [0, 1, 2] and got[1]["depth"].shape == (S160.height, S160.width)
    with pytest.raises(ValueError):
        mv.surface_views({3: poses[0]})
    for i, s in enumerate(single):
        assert ms._volume_bytes(surfs[i]) == s["volume"], i
        alone = api.SurfaceVolume(vms[i], **ms.DRIVER_BOX)  # the single driver's volumes, seen through SurfaceVolume.raycast
        alone.d_tsdf.copy_(torch.from_numpy(np.frombuffer(s["volume"][0], np.int32).reshape(tuple(alone.d_tsdf.shape)).copy()))
        alone.d_color.copy_(torch.from_numpy(np.frombuffer(s["volume"][1], np.int32).reshape(tuple(alone.d_color.shape)).copy()))
        want = alone.raycast(poses[i] if i != 1 else poses[1][0])
        print("stream", i, "views", len(poses[i]) if i != 1 else 1, want["info"])
        assert want["info"]["hits"] > 1000, i
        _same_views(got[i], want, ("stream", i))
    for vm in vms:
        vm.close()


def test_run_tum_streams_surface_views_writes_the_sequential_files(tmp_path, monkeypatch, capsys):
    """run_tum --streams 3 --streams-surface --streams-surface-views DIR on three datasets: every file of DIR/<dataset>/ is the
    sequential --surface --surface-views run's of that dataset (under SAME_PARTITION, which makes the two drivers' poses equal)."""
    from lm_settings_cases import S160
    from revo_amd import run_tum, synth, tum
    from test_gpu_configs import SAME_PARTITION
    from test_gpu_voxel_map import BIASES
    from test_gpu_vo_multi import _tum_yaml
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)
    names = ["rgbd_synth_a", "rgbd_synth_b", "rgbd_synth_c"]
    for k, (n, lens) in enumerate(zip(names, (12, 16, 9))):
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), synth.make_sequence(41 + 2 * k, S160, lens, max_t=0.01, max_rot_deg=0.4, bias=BIASES[k % 3]))
    _tum_yaml(tmp_path, S160, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--map", "0.05"]
    box = ["--surface-box", "-40", "-40", "0", "80", "80", "100", "--surface-trunc", "0.2"]
    runs = (("seq", ["--surface", "surface.ply", "--surface-views", "views", "--surface-views-every", "4"]),
            ("multi", ["--streams", "3", "--streams-surface", "surface.ply", "--streams-surface-views", "views", "--streams-surface-views-every", "4"]),
            ("seqk", ["--surface", "surface.ply", "--surface-views", "views"]),
            ("multik", ["--streams", "3", "--streams-surface", "surface.ply", "--streams-surface-views", "views"]))
    for sub, extra in runs:
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra + box) == 0, sub
    assert "Surface views: 3 views (every 4 frames)" in capsys.readouterr().out
    for a, b in (("seq", "multi"), ("seqk", "multik")):
        for n in names:
            fa, fb = tmp_path / a / "views" / n, tmp_path / b / "views" / n
            files = sorted(str(p.relative_to(fa)) for p in fa.rglob("*") if p.is_file())
            assert files == sorted(str(p.relative_to(fb)) for p in fb.rglob("*") if p.is_file()) and len(files) >= 4, (a, n, files)
            for f in files:
                assert (fa / f).read_bytes() == (fb / f).read_bytes(), (a, n, f)
            rows = tum.read_associate(str(fb / "associate.txt"))
            assert len(rows) >= 1 and (tum.load_frame(str(fb), rows[0][1], rows[0][3])[1] > 0).sum() > 1000, (b, n)
