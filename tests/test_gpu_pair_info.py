"""revo_pair_info on the MI355X (k_pair_info): the record against its numpy specification (tests/pair_info_ref.py), the
batch, pipeline, revo_vo and revo_vo_multi paths against the single-pair call, the refusals, and run_tum --covariances."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import (ImgPyramidSettings, OptimizerSettings, TrackerSettings, PairInfo, PAIR_INFO_CHUNK,  # noqa: E402
                               pair_info_groups)

import pair_info_ref as pr  # noqa: E402

S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
S640 = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
REC, INFO = 96, 192
OS = OptimizerSettings()


def _ctx(s, exact=False):
    from revo_amd import api
    cam = api.CameraPyr(s, exact_sums=exact)
    return cam, api.TrackerNew(TrackerSettings(), s, cam)


def _pyrs(s, cam, p):
    from revo_amd import api
    ref = api.ImgPyramidRGBD(s, cam, *p["ref"])
    cur = api.ImgPyramidRGBD(s, cam, *p["curr"])
    ref.makeKeyframe()
    return ref, cur


def _spec(s, cam, ref, cur, R, T, lvl):
    c = cam.at(lvl)
    return pr.pair_info(ref.returnOptimizationStructure(lvl), cur.return3DEdges(lvl), (c.fx, c.fy, c.cx, c.cy, c.width, c.height),
                        R, T, OS.edge_distance_lvl[lvl], OS.use_edge_filter, OS.huber_edge, level=lvl)


def _poses(p, Rc, Tc):
    gt = p["T_ref_curr"]
    return [(np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3]), (Rc, Tc)]


def _dev_pairs(pairs):
    import torch
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")])).cuda()
    return bgr, dep


def _split(t, size):
    buf = t.cpu().numpy().tobytes()
    return [buf[i:i + size] for i in range(0, len(buf), size)]


def _rot(rec):
    return np.array(list(rec.R), np.float32).reshape(3, 3).T, np.array(list(rec.T), np.float32)


@pytest.fixture(scope="module")
def pairs320():
    return synth.make_pairs(range(700, 704), S320)


def test_spec_every_level_three_poses(pairs320):
    """4 seeded pairs x 3 levels x 3 poses through revo_tracker_pair_info: the 192 bytes are the restatement's.  Level 0 spans
    several workgroups of the kernel and ends in a chunk that is not full."""
    cam, trk = _ctx(S320)
    n = 0
    for p in pairs320:
        ref, cur = _pyrs(S320, cam, p)
        npts0 = cur.return3DEdges(0).shape[0]
        assert npts0 > PAIR_INFO_CHUNK and npts0 % PAIR_INFO_CHUNK != 0 and pair_info_groups(320 * 240) >= 2, npts0
        _, Rc, Tc, _ = trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
        for lvl in range(3):
            for R, T in _poses(p, Rc, Tc):
                got = bytes(trk.pairInfo(ref, cur, R, T, lvl))
                want = _spec(S320, cam, ref, cur, R, T, lvl)
                assert got == want, (lvl, np.frombuffer(got, np.float32)[:29] - np.frombuffer(want, np.float32)[:29])
                n += 1
    assert n == 36


def test_spec_640x480_level0():
    cam, trk = _ctx(S640)
    p = synth.make_pair(711, S640)
    ref, cur = _pyrs(S640, cam, p)
    _, Rc, Tc, _ = trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
    assert cur.return3DEdges(0).shape[0] > 8 * PAIR_INFO_CHUNK
    assert bytes(trk.pairInfo(ref, cur, Rc, Tc, 0)) == _spec(S640, cam, ref, cur, Rc, Tc, 0)


def _batch_infos(cam, pairs, exact_eval=False):
    """3 pairs through one batch: (result records, info from the grid's device records, info from the same poses given on the host)"""
    import torch
    from revo_amd import api
    n = len(pairs)
    bt = api.BatchTracker(cam, n)
    bgr, dep = _dev_pairs(pairs)
    d_res = torch.zeros(n * REC, dtype=torch.uint8, device="cuda")
    d_a = torch.zeros(n * INFO, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(n * INFO, dtype=torch.uint8, device="cuda")
    bt.track(bgr.data_ptr(), dep.data_ptr(), d_res.data_ptr())
    assert bt.pair_info(d_results=d_res.data_ptr(), lvl=0, d_info=d_a.data_ptr()) is None
    bt.sync()
    res = api.results_from_buffer(d_res.cpu().numpy().tobytes(), n)
    RT = np.stack([np.concatenate([np.asarray(r["R"], np.float32).T.reshape(9), np.asarray(r["T"], np.float32)]) for r in res])
    bt.pair_info(RT=RT, lvl=0, d_info=d_b.data_ptr())
    bt.sync()
    return res, _split(d_a, INFO), _split(d_b, INFO), bt, (bgr, dep)


def test_batch_equals_single(pairs320):
    """A batch of 3: from the grid's own device records and from host poses, the bytes of the single-pair call; and with
    exact_sums, evalAt's A and b are H / good and -(g / good) bitwise."""
    from revo_amd import api
    cam, trk = _ctx(S320, exact=True)
    pairs = pairs320[:3]
    res, from_dev, from_host, bt, keep = _batch_infos(cam, pairs)
    opt = api.Optimizer(OS, cam)
    iu = np.triu_indices(6)
    for i, p in enumerate(pairs):
        ref, cur = _pyrs(S320, cam, p)
        R, T = res[i]["R"], res[i]["T"]
        single = trk.pairInfo(ref, cur, R, T, 0)
        assert from_dev[i] == bytes(single) and from_host[i] == bytes(single), i
        assert single.flags == 0 and single.good > 1000
        _, info, A, b = opt.evalAt(ref, cur, R, T, 0)
        n = np.float32(single.good)
        assert info.good_pts_edges == single.good and info.bad_pts_edges == single.bad
        assert (np.array(list(single.H), np.float32) / n).tobytes() == np.asarray(A, np.float32)[iu].tobytes()
        assert (-(np.array(list(single.g), np.float32) / n)).tobytes() == np.asarray(b, np.float32).tobytes()
        assert np.float32(info.sum_error_weighted) == np.float32(single.sum_w)


def test_flag_independence(pairs320):
    """Contexts created with exact_sums on and off, at the same poses: identical bytes."""
    p = pairs320[0]
    out = []
    for exact in (False, True):
        cam, trk = _ctx(S320, exact=exact)
        ref, cur = _pyrs(S320, cam, p)
        out.append([bytes(trk.pairInfo(ref, cur, R, T, lvl)) for lvl in range(3) for R, T in _poses(p, np.eye(3), np.zeros(3))[:2]])
    assert out[0] == out[1]


def test_refusals(pairs320):
    import torch
    from revo_amd import api
    cam, trk = _ctx(S320)
    p = pairs320[1]
    ref, cur = _pyrs(S320, cam, p)
    # a current frame without depth: no points, a zero-sum record that is no error, and no covariance
    empty = api.ImgPyramidRGBD(S320, cam, p["curr"][0], np.zeros_like(p["curr"][1]))
    r = trk.pairInfo(ref, empty, np.eye(3), np.zeros(3), 0)
    assert r.good == 0 and r.bad == 0 and r.flags == 0 and not any(list(r.H)) and not any(list(r.g)) and r.sum_w == 0 and r.sum_u == 0
    with pytest.raises(api.RevoError):
        api.pair_covariance(r)
    # a non-orthogonal pose: an error of the single call, bit0 of the batch's record (the other pairs are evaluated)
    bad_R = np.eye(3, dtype=np.float32)
    bad_R[0, 0] = 1.1
    with pytest.raises(api.RevoError) as e:
        trk.pairInfo(ref, cur, bad_R, np.zeros(3), 0)
    assert e.value.code == -4
    with pytest.raises(api.RevoError) as e:
        trk.pairInfo(ref, cur, np.eye(3), np.zeros(3), 3)
    assert e.value.code == -6
    with pytest.raises(api.RevoError) as e:
        trk.pairInfo(cur, ref, np.eye(3), np.zeros(3), 0)
    assert e.value.code == -3
    pairs = pairs320[:3]
    bt = api.BatchTracker(cam, 3)
    bgr, dep = _dev_pairs(pairs)
    bt.build(bgr.data_ptr(), dep.data_ptr())
    RT = np.tile(np.concatenate([np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)]), (3, 1))
    RT[1, :9] = bad_R.T.reshape(9)
    RT[2, 9] = np.nan
    recs = bt.pair_info(RT=RT, lvl=1)
    assert [r.flags for r in recs] == [0, 1, 1] and recs[0].good > 100 and recs[0].level == 1
    for r, rt in zip(recs[1:], RT[1:]):
        b = bytearray(bytes(r))
        assert r.level == 1 and bytes(b[132:180]) == rt.tobytes()
        b[124:180] = bytes(56)
        assert not any(b)
    single = trk.pairInfo(bt.frame(0, S320), bt.frame(1, S320), np.eye(3), np.zeros(3), 1)
    assert bytes(recs[0]) == bytes(single)
    d = torch.zeros(3 * INFO + 16, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(3 * REC, dtype=torch.uint8, device="cuda")
    for kw, code in ((dict(RT=RT, lvl=3), -6), (dict(RT=RT, lvl=-1), -6), (dict(RT=RT, d_results=d_res.data_ptr()), -1), (dict(), -1)):
        with pytest.raises(api.RevoError) as e:
            bt.pair_info(d_info=d.data_ptr(), **kw)
        assert e.value.code == code, kw
    with pytest.raises(api.RevoError) as e:
        bt.pair_info(RT=RT, d_info=d.data_ptr() + 8)
    assert e.value.code == -1


def test_pipeline_after_grid_slot(pairs320):
    """Info enqueued on the after-grid stream of 3 consecutive steps of a depth-4 handle: the batch path's bytes, and the steps'
    result records are those of a run without info."""
    import torch
    from revo_amd import api
    cam, _ = _ctx(S320)
    steps = [pairs320[0:3], pairs320[1:4], [pairs320[3], pairs320[0], pairs320[2]]]
    want = [_batch_infos(cam, st) for st in steps]
    runs = {}
    for with_info in (False, True):
        pipe = api.Pipeline(cam, 3, depth=4)
        try:
            keep, tickets = [], []
            for st in steps:
                bgr, dep = _dev_pairs(st)
                d_res = torch.zeros(3 * REC, dtype=torch.uint8, device="cuda")
                d_info = torch.zeros(3 * INFO, dtype=torch.uint8, device="cuda")
                ticket, stream = pipe.submit(bgr.data_ptr(), dep.data_ptr(), d_res.data_ptr())
                if with_info:
                    pipe.pair_info(ticket, stream, d_info.data_ptr(), d_results=d_res.data_ptr(), lvl=0)
                keep.append((bgr, dep, d_res, d_info))
                tickets.append(ticket)
            for t in tickets:
                pipe.wait(t)
            pipe.drain()
            runs[with_info] = [(_split(k[2], REC), _split(k[3], INFO)) for k in keep]
        finally:
            pipe.close()
    for k in range(3):
        assert runs[True][k][0] == runs[False][k][0], k
        assert runs[True][k][1] == want[k][1], k
        assert all(pr.record(b).good > 1000 for b in runs[True][k][1])


def _seq(seed, n, deg=2.0):
    return [(f[0], f[1], f[2]) for f in synth.make_sequence(seed, S320, n, max_t=0.01, max_rot_deg=0.4,
                                                            bias=[0.004, 0, 0, 0, np.deg2rad(deg), 0])]


def _solo(frames, exact, pair_info):
    from revo_amd import vo
    cam, _ = _ctx(S320, exact=exact)
    g = vo.REVO(S320, cameraPyr=cam, pair_info=pair_info)
    res = [g.push(*f) for f in frames]
    return res, g.pair_infos


def test_revo_vo_records():
    """12 frames with a keyframe change: the option does not move a pose; every frame's record is the single-pair call's on
    hand-built pyramids of the frame and its reported keyframe at the record's own pose; the first frame has bit0."""
    from revo_amd import api
    frames = _seq(21, 12)
    off, none = _solo(frames, False, False)
    on, infos = _solo(frames, False, True)
    assert none == [] and len(infos) == len(frames)
    for (Ma, ka), (Mb, kb) in zip(off, on):
        assert Ma.tobytes() == Mb.tobytes() and ka == kb
    assert any(kf for _, kf in on[1:]), "the sequence needs a keyframe change"
    by_ts = {f[2]: f for f in frames}
    first, kts0 = infos[0]
    assert first.flags == 1 and kts0 == frames[0][2] and first.good == 0 and not any(list(first.H))
    cam, trk = _ctx(S320)
    kf_seen = set()
    for i in range(1, len(frames)):
        info, kts = infos[i]
        kf_seen.add(kts)
        kf = api.ImgPyramidRGBD(S320, cam, by_ts[kts][0], by_ts[kts][1])
        kf.makeKeyframe()
        cur = api.ImgPyramidRGBD(S320, cam, frames[i][0], frames[i][1])
        R, T = _rot(info)
        assert info.flags == 0 and info.level == 0 and info.good > 500, i
        assert bytes(trk.pairInfo(kf, cur, R, T, 0)) == bytes(info), i
        # the record's pose is the reported one: T_w_curr = T_w_kf * T_kf_curr, checked through the keyframe's own reported pose
        if kts == frames[0][2]:
            M = np.eye(4, dtype=np.float32)
            M[:3, :3], M[:3, 3] = R, T
            assert np.allclose(on[i][0], M, atol=1e-6), i
    assert len(kf_seen) >= 2


def test_revo_vo_multi_records():
    """S = 3 with unequal lengths, exact sums (so that the two drivers' poses agree): per stream the records and
    keyframe time stamps of a revo_vo on that sequence alone."""
    from revo_amd import vo
    lens = [12, 9, 14]
    seqs = [_seq(30 + k, n) for k, n in enumerate(lens)]
    m = vo.MultiREVO(S320, 3, exact_sums=True, pair_info=True)
    got = m.run(seqs)
    n_change = 0
    for k, frames in enumerate(seqs):
        res, infos = _solo(frames, True, True)
        assert len(got[k]) == len(frames) and len(got[k].pair_infos) == len(frames)
        for i in range(len(frames)):
            assert got[k][i][0].tobytes() == res[i][0].tobytes() and got[k][i][1] == res[i][1], (k, i)
            assert bytes(got[k].pair_infos[i][0]) == bytes(infos[i][0]) and got[k].pair_infos[i][1] == infos[i][1], (k, i)
        n_change += sum(1 for _, kf in res[1:] if kf)
    assert n_change >= 1


def test_run_tum_covariances(tmp_path, monkeypatch):
    """run_tum --covariances: one line per pose line, the same file with and without --streams 2 under --exact-sums, pose files
    untouched by the option, every finite covariance symmetric positive definite."""
    from revo_amd import run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    names = ["rgbd_synth_a", "rgbd_synth_b"]
    lens = (12, 9)
    for k, (n, ln) in enumerate(zip(names, lens)):
        seq = synth.make_sequence(80 + k, S320, ln, max_t=0.01, max_rot_deg=0.4, bias=[0.004, 0, 0, 0, np.deg2rad(2.0), 0])
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), seq)
    _tum_yaml(tmp_path, S320, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "0", "--exact-sums"]
    for sub, extra in (("plain", []), ("seq", ["--covariances"]), ("multi", ["--covariances", "--streams", "2"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    assert not (tmp_path / "plain" / ("cov_%s.txt" % names[0])).exists()
    iu = np.triu_indices(6)
    for n, ln in zip(names, lens):
        poses = (tmp_path / "plain" / ("poses_%s.txt" % n)).read_bytes()
        assert poses == (tmp_path / "seq" / ("poses_%s.txt" % n)).read_bytes()
        assert poses == (tmp_path / "multi" / ("poses_%s.txt" % n)).read_bytes()
        cov = (tmp_path / "seq" / ("cov_%s.txt" % n)).read_bytes()
        assert cov == (tmp_path / "multi" / ("cov_%s.txt" % n)).read_bytes()
        lines = cov.decode().splitlines()
        assert len(lines) == len(poses.splitlines()) == ln
        n_finite = 0
        for i, (ln_c, ln_p) in enumerate(zip(lines, poses.decode().splitlines())):
            v = ln_c.split()
            assert len(v) == 25 and float(v[0]) == pytest.approx(float(ln_p.split()[0]), abs=1e-6)
            nums = np.array([float(x) for x in v[3:]])
            if i == 0:
                assert np.all(np.isnan(nums))
                continue
            assert np.all(np.isfinite(nums)) and nums[0] > 0
            M = np.zeros((6, 6))
            M[iu] = nums[1:]
            M = M + np.triu(M, 1).T
            assert np.all(np.linalg.eigvalsh(M) > 0), (n, i)
            n_finite += 1
        assert n_finite == ln - 1
