"""The host core's handles share one context's streams, pools and marks (revo_host_impl.h: FrameSet's "built" and "released"
marks, the deferred work of a batch build, the job slots of host-buffer batches, the step sets of revo_mdev).  ONE context
runs single-frame pyramids, a BatchTracker, a HostBatchTracker and a MultiREVO with their calls interleaved: every output is
byte for byte what the same calls give alone on a fresh context.  Then lifetimes: handles outlive CameraPyr.close().

160x120, 3 levels, the seeded pairs of lm_settings_cases.py; exact sums wherever tracker records are compared (float-mode sums
are not run-to-run identical).  No assertion about timing."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import TrackerSettings  # noqa: E402

from lm_settings_cases import S160 as S, SEEDS  # noqa: E402

I4 = np.eye(4, dtype=np.float32)
# stream 1 of the MultiREVO: three frames of a slow pan, then one 15 frames further on (the vote asks for a new keyframe)
PAN = [0.004, 0, 0, 0, np.deg2rad(1.5), 0]


@functools.lru_cache(maxsize=None)
def _pairs():
    return [synth.make_pair(seed, S) for seed in list(SEEDS)[:5]]


@functools.lru_cache(maxsize=None)
def _sequences():
    a = synth.make_sequence(31, S, 4, max_t=0.01, max_rot_deg=0.4)
    b = synth.make_sequence(32, S, 19, max_t=0.01, max_rot_deg=0.4, bias=PAN)
    return [[(f[0], f[1], f[2]) for f in a], [(f[0], f[1], f[2]) for f in (b[0], b[1], b[2], b[18])]]


def _context():
    from revo_amd import api
    cam = api.CameraPyr(S, exact_sums=True)
    return cam, api.TrackerNew(TrackerSettings(), S, cam)


def _planes(p):
    return [f(lvl) for lvl in range(3) for f in (p.returnGray, p.returnDepth, p.returnEdges, p.edges3DTiled)]


def _record(r):
    return (r["R"].tobytes(), r["T"].tobytes(), r["err"], r["good"], r["bad"], r["status"], r["evals"].tobytes(), r["flags"])


# Every feature is a generator over one context: it yields between its calls (where the interleaved run lets the others in)
# and leaves its outputs in `out`.
def _frames(cam, trk, out):
    """Single-frame pyramids created, read, tracked, voted on and destroyed, then created again: round 2 and 3 rebuild the
    pooled sets of the round before behind both of their "released" marks -- pageable rows, page-locked rows, pageable."""
    import torch
    from revo_amd import api
    for rnd, pinned in enumerate((False, True, False)):
        pair = _pairs()[rnd]
        pyr = []
        for k, (bgr, depth) in enumerate((pair["ref"], pair["curr"])):
            bgr, depth = np.ascontiguousarray(bgr, np.uint8), np.ascontiguousarray(depth, np.float32)
            if pinned:
                bgr, depth = torch.from_numpy(bgr).pin_memory().numpy(), torch.from_numpy(depth).pin_memory().numpy()
            pyr.append(api.ImgPyramidRGBD(S, cam, bgr, depth, timestamp=float(2 * rnd + k)))
            yield
        ref, cur = pyr
        out += _planes(ref) + _planes(cur)
        yield
        ref.makeKeyframe()
        out += [ref.returnDistTransform(lvl) for lvl in range(3)]
        st, R, T, err = trk.trackFrames(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), ref, cur)
        out += [np.array([st]), R, T, np.array([err], np.float32), trk.last_evals.copy()]
        yield
        trk.addOldPclAndPose(ref, trk.histogramLevel, I4, float(rnd))  # a past cloud: round 3's vote reads three of them
        M = I4.copy()
        M[:3, :3], M[:3, 3] = R, T
        yield
        st, h4, o4 = trk.assessTrackingQuality(M, cur, return_hist=True)
        out += [np.array([st]), h4, o4]
        del ref, cur, pyr  # both sets go back to the pool
        yield
    assert trk.pastSize() == 3


def _batch(cam, trk, out):
    """A batch of 2 pairs built on one stream and tracked on another, rebuilt with other frames and tracked again; an even
    view is read before the first grid (the accessor runs the deferred work) and after the second (the tracker ran it)."""
    import torch
    from revo_amd import api
    bt = api.BatchTracker(cam, 2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    rec = torch.zeros(2 * 96, dtype=torch.uint8, device="cuda")
    sets = []
    for ps in (_pairs()[0:2], _pairs()[2:4]):
        bgr = np.stack([p[k][0] for p in ps for k in ("ref", "curr")])
        dep = np.stack([p[k][1] for p in ps for k in ("ref", "curr")]).astype(np.float32)
        sets.append((torch.from_numpy(bgr).cuda(), torch.from_numpy(dep).cuda()))
    torch.cuda.synchronize()

    def even_view():
        v = bt.frame(2, S)
        return [v.edges3DTiled(0), v.returnDepth(2), v.returnDistTransform(1)]

    for k, (d_bgr, d_dep) in enumerate(sets):
        bt.build(d_bgr.data_ptr(), d_dep.data_ptr(), stream=sa.cuda_stream)
        yield
        if k == 0:
            out += even_view()
            yield
        bt.track_only(rec.data_ptr(), stream=sb.cuda_stream)
        yield
        bt.sync(stream=sb.cuda_stream)
        out.append(rec.cpu().numpy().copy())
        yield
    out += even_view()


def _host(cam, trk, out):
    """Host-buffer jobs of 2, 3 and 2 pairs (the third takes the first one's slot again), then raw-depth jobs of 2 and 3 pairs:
    a third slot, and a fourth shape that evicts a free one.  The first job's rows are padded (strided copies), the others lie
    back to back in one slab per plane type (merged copies)."""
    from revo_amd import api

    def padded(a):
        big = np.zeros((a.shape[0], a.shape[1] + 8) + a.shape[2:], a.dtype)
        big[:, :a.shape[1]] = a
        return big[:, :a.shape[1]]

    def slab(ps, u16):
        bgr = np.stack([p[k][0] for p in ps for k in ("ref", "curr")])
        dep = np.stack([p[k][1] for p in ps for k in ("ref", "curr")]).astype(np.float32)
        if u16:
            dep = np.round(np.nan_to_num(dep) * 5000.0).astype(np.uint16)
        return [((bgr[2 * i], dep[2 * i]), (bgr[2 * i + 1], dep[2 * i + 1])) for i in range(len(ps))]

    P = _pairs()
    f32, u16 = api.HostBatchTracker(cam), api.HostBatchTracker(cam, depth_scale_factor=5000.0)
    jobs = [(f32, [tuple((padded(b), padded(d.astype(np.float32))) for b, d in (p["ref"], p["curr"])) for p in P[0:2]]),
            (f32, slab(P[2:5], False)), (f32, slab(P[1:3], False)), (u16, slab(P[0:2], True)), (u16, slab(P[2:5], True))]
    for hb, pairs in jobs:
        job = hb.submit(pairs)
        yield
        out += [_record(r) for r in hb.wait(job)]
        yield


def _multi(cam, trk, out):
    """Two streams stepped four frames; stream 1's fourth frame makes its vote ask for a new keyframe: promotions, cloud
    copies, votes and the re-track all run."""
    from revo_amd import vo
    m = vo.MultiREVO(S, 2, cameraPyr=cam)
    seqs = _sequences()
    for k in range(4):
        m.submit([(s, *seqs[s][k]) for s in range(2)])
        yield
        out += [(s, M.tobytes(), kf, ts) for s, M, kf, ts in m.step()]
        yield
    while m.pending(0) or m.pending(1):
        out += [(s, M.tobytes(), kf, ts) for s, M, kf, ts in m.step()]
        yield
    assert (m.nKeyFrames(0), m.nKeyFrames(1)) == (1, 2)
    kf, T = m.keyframe(1)
    out += [T, kf.returnDistTransform(0), kf.edges3DTiled(1)]


FEATURES = {"frames": _frames, "batch": _batch, "host": _host, "multi": _multi}


def _same(a, b):
    assert len(a) == len(b) and len(a) > 0
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), i
        else:
            assert x == y, i


@functools.lru_cache(maxsize=None)
def _alone(name):
    """The feature's outputs on a fresh context of its own.  Do not modify."""
    cam, trk = _context()
    out = []
    for _ in FEATURES[name](cam, trk, out):
        pass
    cam.close()
    return out


def test_interleaved_on_one_context_every_output_is_what_the_call_gives_alone():
    cam, trk = _context()
    outs = {name: [] for name in FEATURES}
    live = [(name, FEATURES[name](cam, trk, outs[name])) for name in FEATURES]
    while live:  # round robin: one call of every feature in turn
        for item in list(live):
            if next(item[1], "done") == "done":
                live.remove(item)
    cam.close()
    for name in FEATURES:
        _same(outs[name], _alone(name))
    assert any(r[3] > 0 for r in outs["host"]) and np.any(outs["batch"][3] != outs["batch"][4])  # real records, two builds


def test_handles_outlive_the_context_owner_and_a_new_context_works_after_them():
    import torch
    from revo_amd import api, vo
    P, seqs = _pairs(), _sequences()

    def run(close_early):
        cam, trk = _context()
        pyr = api.ImgPyramidRGBD(S, cam, *P[0]["ref"])
        bt = api.BatchTracker(cam, 2)
        bgr = torch.from_numpy(np.stack([p[k][0] for p in P[0:2] for k in ("ref", "curr")])).cuda()
        dep = torch.from_numpy(np.stack([p[k][1] for p in P[0:2] for k in ("ref", "curr")]).astype(np.float32)).cuda()
        rec = torch.zeros(2 * 96, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bt.track(bgr.data_ptr(), dep.data_ptr(), rec.data_ptr())
        bt.sync()
        m = vo.MultiREVO(S, 2, cameraPyr=cam)
        for k in range(2):
            m.submit([(s, *seqs[s][k]) for s in range(2)])
            m.step()
        if close_early:
            cam.close()  # the owner's reference goes; the three handles keep the context alive
        out = _planes(pyr)
        bt.track_only(rec.data_ptr())
        bt.sync()
        out.append(rec.cpu().numpy().copy())
        m.submit([(s, *seqs[s][2]) for s in range(2)])
        out += [(s, M.tobytes(), kf, ts) for s, M, kf, ts in m.step()]
        del pyr, bt, m
        cam.close()
        return out

    _same(run(True), run(False))
    _same(_alone("frames")[:24], _frames_first_round())  # after the last handle has gone: a new context on the device works


def _frames_first_round():
    cam, trk = _context()
    out = []
    g = _frames(cam, trk, out)
    while len(out) < 24:
        next(g)
    g.close()
    cam.close()
    return out[:24]
