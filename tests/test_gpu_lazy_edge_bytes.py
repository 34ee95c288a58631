"""GPU: a batch that defers the end of its build (the default) ends its hysteresis at the edge BITMAPS; the byte planes edgesPyr /
edgesOrigPyr come into being when somebody reads them through a view (ensure_edge_bytes), fill-in and the EDT's column pass
work on the bitmaps at every width.  Whoever asks and whenever, every plane, list and histogram a view returns and every
tracker record are the bits an eager build (REVO_DEFER=0, a fresh handle) of the same input gives.

Geometry: 160 x 128 x 4 levels (level widths 160 / 80 / 40 / 20: three levels are no multiple of 32 wide and take the partial
last word of the column pass; 160 x 120 x 4 is not a geometry the library accepts, its coarsest level has 300 pixels, no
multiple of 16) and 640 x 480 x 4 (the bench geometry)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, TrackerSettings, PLANE_EDGES, PLANE_EDGES_ORIG  # noqa: E402

N_PAIRS, LEVELS = 2, 4
GEOMS = {
    "160x128": dict(size=(160, 128), hist_patch=(10, 5, 0, 0, 0, 0)),
    "640x480": dict(size=(640, 480), hist_patch=(20, 10, 5, 0, 0, 0)),
}
_frames, _reference, _fill_pct = {}, {}, {}


def _settings(geom, **kw):
    g = GEOMS[geom]
    return ImgPyramidSettings.scaled(g["size"][0], g["size"][1], LEVELS, hist_patch=g["hist_patch"], **kw)


def _input(geom, seed0=700):
    """2 pairs of synthetic frames: (bgr [4,h,w,3], depth [4,h,w]) on the host, rendered once per geometry and seed"""
    key = (geom, seed0)
    if key not in _frames:
        s = _settings(geom)
        pairs = [synth.make_pair(seed0 + i, s) for i in range(N_PAIRS)]
        bgr = np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])
        dep = np.stack([p[k][1] for p in pairs for k in ("ref", "curr")]).astype(np.float32)
        _frames[key] = (bgr, dep)
    return _frames[key]


def _to_device(bgr, dep):
    import torch
    return torch.from_numpy(bgr).cuda(), torch.from_numpy(dep).cuda()


def _read_all(bt, s):
    """everything a view returns that depends on the edges: byte planes, histogram, both edge lists, the keyframes' DT planes"""
    out = {}
    for f in range(2 * bt.n_pairs):
        v = bt.frame(f, s)
        for lvl in range(LEVELS):
            out[("edges", f, lvl)] = v.returnEdges(lvl)
            out[("edges_orig", f, lvl)] = v.returnOrigEdges(lvl)
            out[("hist", f, lvl)] = v.returnHist(lvl)
            out[("list_tiled", f, lvl)] = v.edges3DTiled(lvl)
            out[("list", f, lvl)] = v.return3DEdges(lvl)
            if f % 2 == 0:
                out[("dt", f, lvl)] = v.returnDistTransform(lvl)
    return out


def _records(bt, side=None):
    import torch
    rec = torch.zeros(bt.n_pairs * 96, dtype=torch.uint8, device="cuda")
    if side is not None:
        bt.prepare(stream=side.cuda_stream)
        side.synchronize()
    bt.track_only(rec.data_ptr())
    bt.sync()
    return rec.cpu().numpy().tobytes()


def _eager(api, monkeypatch, geom, pct, seed0=700):
    """the reference: the same input through a batch that defers nothing, planes AND records; once per (geometry, nPercentage, input)"""
    key = (geom, pct, seed0)
    if key not in _reference:
        s = _settings(geom, **({} if pct is None else {"n_percentage": pct}))
        cam = api.CameraPyr(s)
        api.TrackerNew(TrackerSettings(), s, cam)
        d_bgr, d_dep = _to_device(*_input(geom, seed0))
        monkeypatch.setenv("REVO_DEFER", "0")  # read when the batch is created
        bt = api.BatchTracker(cam, N_PAIRS)
        monkeypatch.delenv("REVO_DEFER")
        bt.build(d_bgr.data_ptr(), d_dep.data_ptr())
        rec = _records(bt)
        _reference[key] = (_read_all(bt, s), rec)
    return _reference[key]


def _assert_same(tag, got, want):
    assert got.keys() == want.keys()
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %s of frame %d level %d differs" % ((tag,) + k)


def _lazy_against_eager(api, monkeypatch, geom, pct, cam_env=None):
    import torch
    want, want_rec = _eager(api, monkeypatch, geom, pct)
    for k, v in (cam_env or {}).items():
        monkeypatch.setenv(k, v)  # read when the context is created
    s = _settings(geom, **({} if pct is None else {"n_percentage": pct}))
    cam = api.CameraPyr(s)
    for k in (cam_env or {}):
        monkeypatch.delenv(k)
    api.TrackerNew(TrackerSettings(), s, cam)
    d_bgr, d_dep = _to_device(*_input(geom))
    side = torch.cuda.Stream()
    # the accessor is the batch's first consumer: the byte planes are asked for in front of the deferred work
    first = api.BatchTracker(cam, N_PAIRS)
    first.build(d_bgr.data_ptr(), d_dep.data_ptr())
    got = _read_all(first, s)
    _assert_same("read before tracking", got, want)
    assert _records(first) == want_rec, "records after the planes were read"
    # ... and behind prepare on a second stream + a tracker grid
    second = api.BatchTracker(cam, N_PAIRS)
    second.build(d_bgr.data_ptr(), d_dep.data_ptr())
    assert _records(second, side) == want_rec, "records of the deferred build"
    _assert_same("read after tracking", _read_all(second, s), want)
    # the same batch rebuilt with other frames and back: no byte of an earlier expansion may survive a rebuild
    o_bgr, o_dep = _to_device(*_input(geom, 740))
    second.build(o_bgr.data_ptr(), o_dep.data_ptr())
    other = second.frame(1, s).returnEdges(0)
    assert not np.array_equal(other, want[("edges", 1, 0)]), "the two inputs must differ"
    second.build(d_bgr.data_ptr(), d_dep.data_ptr())
    _assert_same("read after two rebuilds", _read_all(second, s), want)
    return got


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_same_planes_as_an_immediate_build(monkeypatch, geom):
    from revo_amd import api
    got = _lazy_against_eager(api, monkeypatch, geom, None)
    assert any(got[("edges", f, 0)].any() for f in range(2 * N_PAIRS))


def _pick_fill_pct(ro, geom):
    """the smallest nPercentage of the list at which the REFERENCE's fill-in adds pixels to some (level, frame) of the input"""
    if geom not in _fill_pct:
        bgr, dep = _input(geom)
        _fill_pct[geom] = None
        for pct in (0.5, 0.7, 0.9, 1.01):
            s = _settings(geom, n_percentage=pct)
            added = 0
            for f in range(bgr.shape[0]):
                o = ro.Pyramid(s, bgr[f], dep[f])
                for lvl in range(1, LEVELS):
                    added += int(np.count_nonzero(o.read(PLANE_EDGES, lvl) != o.read(PLANE_EDGES_ORIG, lvl)))
            print("%s nPercentage %.2f: the reference's fill-in adds %d pixels" % (geom, pct, added))
            if added:
                _fill_pct[geom] = pct
                break
    return _fill_pct[geom]


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_same_planes_with_fill_in_active(monkeypatch, geom):
    from revo_amd import api
    from oracle import ro
    pct = _pick_fill_pct(ro, geom)
    assert pct is not None, "no nPercentage of the list makes the reference fill in"
    got = _lazy_against_eager(api, monkeypatch, geom, pct)
    s = _settings(geom)
    opened, added = 0, 0
    for f in range(2 * N_PAIRS):
        for lvl in range(1, LEVELS):
            if not (s.hist_patch[lvl] > 0 and s.hist_patch[lvl - 1] > 0):
                continue
            h = got[("hist", f, lvl)]
            frac = np.float32(np.count_nonzero(h)) / np.float32(h.size)  # hist_nz over the tiles, as k_fill's gate has it
            opened += bool(frac < np.float32(pct))
            added += int(np.count_nonzero(got[("edges", f, lvl)] != got[("edges_orig", f, lvl)]))
    print("%s nPercentage %.2f: gate open on %d (level, frame), %d pixels filled in" % (geom, pct, opened, added))
    assert opened >= 1 and added >= 1


def test_pipelined_records_and_a_slot_that_was_never_expanded(monkeypatch):
    """depth 4, 2 pairs, 160 x 128: six steps rebuild two slots whose byte planes nobody asked for; then a slot whose planes
    were read is rebuilt as well"""
    import torch
    from revo_amd import api
    geom = "160x128"
    s = _settings(geom)
    seeds = (700, 740, 780)
    refs = [_eager(api, monkeypatch, geom, None, sd) for sd in seeds]
    cam = api.CameraPyr(s)
    api.TrackerNew(TrackerSettings(), s, cam)
    inputs = [_to_device(*_input(geom, sd)) for sd in seeds]
    # a fresh BatchTracker, step by step
    alone = api.BatchTracker(cam, N_PAIRS)
    for (d_bgr, d_dep), (_, want_rec) in zip(inputs, refs):
        alone.build(d_bgr.data_ptr(), d_dep.data_ptr())
        assert _records(alone) == want_rec
    pipe = api.Pipeline(cam, N_PAIRS, depth=4)
    outs, tickets = [], []

    def submit(n):
        for _ in range(n):
            t = len(tickets)
            d_bgr, d_dep = inputs[t % len(inputs)]
            outs.append(torch.zeros(N_PAIRS * 96, dtype=torch.uint8, device="cuda"))
            tickets.append(pipe.submit(d_bgr.data_ptr(), d_dep.data_ptr(), outs[-1].data_ptr())[0])

    def slot_planes(t):
        got = {}
        for f in range(2 * N_PAIRS):
            v = pipe.batch_frame(tickets[t], f, s)
            for lvl in range(LEVELS):
                got[("edges", f, lvl)] = v.returnEdges(lvl)
                got[("edges_orig", f, lvl)] = v.returnOrigEdges(lvl)
        want = {k: a for k, a in refs[t % len(inputs)][0].items() if k[0] in ("edges", "edges_orig")}
        _assert_same("slot of step %d" % (t + 1), got, want)

    submit(6)
    pipe.wait(tickets[-1])
    slot_planes(5)   # slot 1: built twice, never expanded before
    submit(4)        # ... and every slot once more, the expanded one included
    pipe.wait(tickets[-1])
    slot_planes(9)   # slot 1 again
    pipe.drain()
    for t, o in enumerate(outs):
        assert o.cpu().numpy().tobytes() == refs[t % len(inputs)][1], "step %d differs from the batch alone" % (t + 1)
    pipe.close()


def test_forced_banded_hysteresis(monkeypatch):
    """REVO_HYST_BANDED=1 with bands of 160 bitmap words: seven bands at level 0 of 160 x 128, two at level 1 -- k_hyst_out ends
    at the bitmaps too"""
    from revo_amd import api
    _lazy_against_eager(api, monkeypatch, "160x128", None, cam_env={"REVO_HYST_BANDED": "1", "REVO_HYST_BAND_WORDS": "160"})
