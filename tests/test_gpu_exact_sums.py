"""The tracker's exact-sums mode (revo_ctx_set_exact_sums, api.CameraPyr(exact_sums=True)) on the MI355X.

1. revo_optimizer_eval returns the float nearest the exact sum of the reference's own per-point terms (tests/exact_sums_ref.py),
   bit for bit.
2. The tracker records do not depend on how the work was split: cluster sizes, redundant evaluation, batch size, the
   single-pair call, speculation depth, the pipeline handle.
3. Against the double-accumulating oracle on the 128-pair soak set.
4. revo_vo and revo_vo_multi agree per stream under the shipped defaults; run_tum --exact-sums agrees with and without
   --streams.
5. Exact off is the default path, untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, OptimizerSettings, TrackerSettings  # noqa: E402

import exact_sums_ref as xr  # noqa: E402

S640 = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
KNOBS = ("REVO_TRACK_CLUSTER", "REVO_TRACK_CLUSTER_ONE", "REVO_TRACK_REDUNDANT_BATCH", "REVO_TRACK_REDUNDANT_ONE",
         "REVO_TRACK_KSPEC", "REVO_TRACK_KSPEC_ONE")
REC = 96  # sizeof(revo_pair_result)


def _ctx(s, exact=True):
    from revo_amd import api
    cam = api.CameraPyr(s, exact_sums=exact)
    api.TrackerNew(TrackerSettings(), s, cam)
    return cam


def _dev_pairs(pairs):
    import torch
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")])).cuda()
    return bgr, dep


def _batch_records(cam, pairs, n):
    """the pairs through BatchTracker(n) batch by batch -> raw records (bytes per pair)"""
    import torch
    from revo_amd import api
    bt = api.BatchTracker(cam, n)
    out = []
    for b0 in range(0, len(pairs), n):
        bgr, dep = _dev_pairs(pairs[b0:b0 + n])
        d_res = torch.zeros(n * REC, dtype=torch.uint8, device="cuda")
        bt.track(bgr.data_ptr(), dep.data_ptr(), d_res.data_ptr())
        bt.sync()
        buf = d_res.cpu().numpy().tobytes()
        out += [buf[i * REC:(i + 1) * REC] for i in range(n)]
    return out


def _key(r):
    """what a single-pair call reports as well: pose, error, good / bad, status, evaluations"""
    return (r["R"].tobytes(), r["T"].tobytes(), np.float32(r["err"]).tobytes(), r["good"], r["bad"], r["status"],
            tuple(r["evals"].tolist()))


def _single_keys(cam, s, pairs):
    from revo_amd import api
    trk = api.TrackerNew(TrackerSettings(), s, cam)
    out = []
    for p in pairs:
        ref = api.ImgPyramidRGBD(s, cam, *p["ref"])
        cur = api.ImgPyramidRGBD(s, cam, *p["curr"])
        ref.makeKeyframe()
        status, R, T, err = trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
        info = trk.last_info
        out.append((np.asarray(R, np.float32).tobytes(), np.asarray(T, np.float32).tobytes(), np.float32(err).tobytes(),
                    info.good_pts_edges, info.bad_pts_edges, status, tuple(trk.last_evals.tolist())))
    return out


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def test_eval_equals_the_exact_sums_of_the_reference_terms():
    """The spec test: 16 seeded 640x480 pairs, every level, at the initial, a mid-LM and the converged pose: A, b, the error,
    sum_w / sum_u and the counts are the restatement's, bit for bit."""
    from revo_amd import api
    cam = _ctx(S640)
    assert cam.exact_sums
    opt = api.Optimizer(OptimizerSettings(), cam)
    trk = api.TrackerNew(TrackerSettings(), S640, cam)
    os_ = OptimizerSettings()
    pairs = synth.make_pairs(range(500, 516), S640)
    n_eval = 0
    for p in pairs:
        ref = api.ImgPyramidRGBD(S640, cam, *p["ref"])
        cur = api.ImgPyramidRGBD(S640, cam, *p["curr"])
        ref.makeKeyframe()
        _, Rc, Tc, _ = trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
        gt = p["T_ref_curr"]
        poses = [(np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3]), (Rc, Tc)]
        for lvl in range(S640.nLevels()):
            tab = ref.returnOptimizationStructure(lvl)
            pts = cur.return3DEdges(lvl)
            cam6 = cam.at(lvl)
            c = (cam6.fx, cam6.fy, cam6.cx, cam6.cy, cam6.width, cam6.height)
            for R, T in poses:
                err, info, A, b = opt.evalAt(ref, cur, R, T, lvl)
                e_x, sw, su, good, bad, A_x, b_x = xr.exact_eval(tab, pts, c, R, T, os_.edge_distance_lvl[lvl],
                                                                os_.use_edge_filter, os_.huber_edge)
                where = (p["T_ref_curr"][0, 3], lvl)
                assert (info.good_pts_edges, info.bad_pts_edges) == (good, bad), where
                assert np.float32(info.sum_error_weighted).tobytes() == sw.tobytes(), where
                assert np.float32(info.sum_error_unweighted).tobytes() == su.tobytes(), where
                assert np.float32(err).tobytes() == e_x.tobytes(), where
                assert np.asarray(A, np.float32).tobytes() == A_x.tobytes(), (where, A - A_x)
                assert np.asarray(b, np.float32).tobytes() == b_x.tobytes(), (where, b - b_x)
                n_eval += 1
    assert n_eval == 16 * 4 * 3


PARTITIONS = [  # (label, environment knobs, path)
    ("batch32", {}, ("batch", 32)),
    ("batch32-c1", {"REVO_TRACK_CLUSTER": "1"}, ("batch", 32)),
    ("batch32-c2", {"REVO_TRACK_CLUSTER": "2"}, ("batch", 32)),
    ("batch32-c4-red0", {"REVO_TRACK_CLUSTER": "4", "REVO_TRACK_REDUNDANT_BATCH": "0"}, ("batch", 32)),
    ("batch32-c8", {"REVO_TRACK_CLUSTER": "8"}, ("batch", 32)),
    ("batch32-k1", {"REVO_TRACK_KSPEC": "1"}, ("batch", 32)),
    ("batch32-k3", {"REVO_TRACK_KSPEC": "3"}, ("batch", 32)),
    ("batch32-k4", {"REVO_TRACK_KSPEC": "4"}, ("batch", 32)),
    ("batch8-c16", {"REVO_TRACK_CLUSTER": "16"}, ("batch", 8)),
    ("batch8", {}, ("batch", 8)),
    ("batch1", {}, ("batch", 1)),
    ("pipeline32", {}, ("pipeline", 32)),
    ("single", {}, ("single", 1)),
    ("single-c1-red0", {"REVO_TRACK_CLUSTER_ONE": "1", "REVO_TRACK_REDUNDANT_ONE": "0"}, ("single", 1)),
    ("single-c16-k4", {"REVO_TRACK_CLUSTER_ONE": "16", "REVO_TRACK_KSPEC_ONE": "4"}, ("single", 1)),
    ("single-c2-k1", {"REVO_TRACK_CLUSTER_ONE": "2", "REVO_TRACK_KSPEC": "1"}, ("single", 1)),
]


def _pipeline_records(cam, pairs, n):
    import torch
    from revo_amd import api
    pipe = api.Pipeline(cam, n)
    out = []
    try:
        for b0 in range(0, len(pairs), n):
            bgr, dep = _dev_pairs(pairs[b0:b0 + n])
            d_res = torch.zeros(n * REC, dtype=torch.uint8, device="cuda")
            ticket, _ = pipe.submit(bgr.data_ptr(), dep.data_ptr(), d_res.data_ptr())
            pipe.wait(ticket)
            torch.cuda.synchronize()
            buf = d_res.cpu().numpy().tobytes()
            out += [buf[i * REC:(i + 1) * REC] for i in range(n)]
        pipe.drain()
    finally:
        pipe.close()
    return out


def test_records_do_not_depend_on_the_partition(monkeypatch):
    """64 seeded 640x480 pairs: the same revo_pair_result records (R, T, err, good / bad, evals, flags) whatever the cluster
    size, the redundant threshold, the batch size, the speculation depth or the path; the single-pair call reports the same
    pose, error, counts and evaluations."""
    from revo_amd import api
    pairs = synth.make_pairs(range(2000, 2064), S640)
    base = None
    keys_base = None
    for label, env, (path, n) in PARTITIONS:
        _clear(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cam = _ctx(S640)
        if path == "single":
            keys = _single_keys(cam, S640, pairs)
        else:
            recs = _batch_records(cam, pairs, n) if path == "batch" else _pipeline_records(cam, pairs, n)
            assert len(recs) == 64
            if base is None:
                base = recs
                keys_base = [_key(r) for r in api.results_from_buffer(b"".join(recs), 64)]
                flags = [r["flags"] for r in api.results_from_buffer(b"".join(recs), 64)]
                assert all((f & (2 | 8)) == 0 for f in flags), flags
            diff = [i for i in range(64) if recs[i] != base[i]]
            assert not diff, (label, diff)
            keys = [_key(r) for r in api.results_from_buffer(b"".join(recs), 64)]
        diff = [i for i in range(64) if keys[i] != keys_base[i]]
        assert not diff, (label, diff)
        del cam


def test_against_the_double_accumulating_oracle_128_pairs(capsys):
    """test_tracker_tolerance_distribution_128_pairs' seeds (1000-1127) in bench-sized batches against the oracle with its
    sums in double (ro_set_accum_double).  The normal equations and error sums are the exact ones (test 1); what still
    separates the two LM sequences is upstream of the sums -- the candidate poses (measured 103 of 128 identical
    count sequences, not the 124 aimed at; the default path: 98).  Asserted: more identical sequences than the default path's
    98, poses within 1e-6 wherever the counts agree and on >= 126 of 128 pairs (measured 126; the default path: 127), none above
    5e-4, and >= 24 of the bench's own 32 pairs (measured 25)."""
    from revo_amd import api
    from oracle import ro
    cam = _ctx(S640)
    ot = ro.Tracker(S640, OptimizerSettings(), TrackerSettings())
    L = ro.lib()

    def run(seeds):
        pairs = synth.make_pairs(seeds, S640)
        res = api.results_from_buffer(b"".join(_batch_records(cam, pairs, 32)), len(pairs))
        out = []
        for p, r in zip(pairs, res):
            o_ref, o_cur = ro.Pyramid(S640, *p["ref"]), ro.Pyramid(S640, *p["curr"])
            o_ref.makeKeyframe()
            r_d = ot.trackFrames(o_ref, o_cur, np.eye(3), np.zeros(3))
            same = list(r["evals"][:4]) == list(r_d["evals"][:4])
            dr, dt = synth.rot_angle(r["R"], r_d["R"]), float(np.linalg.norm(r["T"] - r_d["T"]))
            bit = np.asarray(r["R"], np.float32).tobytes() == np.asarray(r_d["R"], np.float32).tobytes() and \
                np.asarray(r["T"], np.float32).tobytes() == np.asarray(r_d["T"], np.float32).tobytes()
            out.append((same, dr, dt, bit))
        return out

    L.ro_set_accum_double(1)
    try:
        soak = run(range(1000, 1128))
        bench = run(range(0, 32))
    finally:
        L.ro_set_accum_double(0)
    same = sum(o[0] for o in soak)
    dr = max(o[1] for o in soak)
    dt = max(o[2] for o in soak)
    bit_same = sum(o[3] for o in soak if o[0])
    worst_same = max([max(o[1], o[2]) for o in soak if o[0]] or [0.0])
    same_bench = sum(o[0] for o in bench)
    with capsys.disabled():
        print("\nexact sums vs double oracle: identical evaluation counts %d/128, poses bit-equal on %d of those (largest "
              "difference there %.3g), max %.3g rad / %.3g m; bench pairs: identical counts %d/32"
              % (same, bit_same, worst_same, dr, dt, same_bench))
    in6 = sum(1 for o in soak if o[1] < 1e-6 and o[2] < 1e-6)
    assert same >= 100
    assert worst_same < 1e-6
    assert in6 >= 126 and dr < 5e-4 and dt < 5e-4
    assert same_bench >= 24


def _seq(seed, n, s=S320):
    bias = [[0.004, 0, 0, 0, np.deg2rad(1.0), 0], [0, 0.003, 0, np.deg2rad(1.0), 0, 0], [0.002, 0, 0.003, 0, np.deg2rad(1.2), 0],
            [0, 0, 0, 0, np.deg2rad(1.5), 0]][seed % 4]
    return [(f[0], f[1], f[2]) for f in synth.make_sequence(seed, s, n, max_t=0.01, max_rot_deg=0.4, bias=bias)]


def _solo(frames, s=S320):
    from revo_amd import vo
    g = vo.REVO(s, cameraPyr=_ctx(s))
    return [g.push(*f) for f in frames]


@pytest.mark.parametrize("S", [1, 8, 32])
def test_multi_stream_equals_solo_under_the_shipped_defaults(monkeypatch, S):
    """revo_vo_multi at S streams (mixed lengths, some streams idle) and revo_vo on each sequence alone, both in exact mode
    and with the shipped tracker knobs (no SAME_PARTITION): the same poses and keyframes, bit for bit."""
    from revo_amd import vo
    from test_gpu_vo_multi import _run_streams
    _clear(monkeypatch)
    if S == 1:
        slots = [0]
    elif S == 8:
        slots = [0, 2, 3, 5, 6, 7]
    else:
        slots = [k for k in range(32) if k % 7 != 3]
    lens = [10 + (7 * k) % 13 for k in range(len(slots))] if S == 32 else [24 + 5 * k for k in range(len(slots))]
    seqs = [_seq(300 + k, n) for k, n in enumerate(lens)]
    m = vo.MultiREVO(S320, S, exact_sums=True)
    assert m.camPyr.exact_sums
    got = _run_streams(m, seqs, slots)
    n_kf = 0
    for k, frames in enumerate(seqs):
        ref = _solo(frames)
        assert len(got[k]) == len(frames)
        for i, ((Mg, kg, _), (Mr, kr)) in enumerate(zip(got[k], ref)):
            assert np.array_equal(Mg, Mr) and kg == kr, (k, i)
        n_kf += sum(1 for r in ref if r[1])
    assert n_kf >= len(seqs)


def test_exact_mode_keeps_the_oracles_keyframes_on_the_metric_sweep():
    """The metric's 640x480 4-level 120-frame sweep (test_gpu_vo.py's, a 0.5 degree pan a frame): exact mode's keyframe
    decisions are the oracle's."""
    from oracle import ro
    from revo_amd import vo
    d = synth.make_sequence(11, S640, 120, max_t=0.01, max_rot_deg=0.4, bias=[0.004, 0, 0, 0, np.deg2rad(0.5), 0], workers=8)
    g = vo.REVO(S640, cameraPyr=_ctx(S640))
    res = g.run([(f[0], f[1], f[2]) for f in d])
    cpu = ro.VO(S640)
    kf_o = [i for i, f in enumerate(d) if cpu.push(f[0], f[1], f[2])[1]]
    kf_g = [i for i, r in enumerate(res) if r[1]]
    print("exact mode, metric sweep: keyframes %s, oracle %s" % (kf_g, kf_o))
    assert kf_g == kf_o and len(kf_g) >= 3, (kf_g, kf_o)


def test_run_tum_exact_sums_sequential_equals_streams(tmp_path, monkeypatch):
    """run_tum --exact-sums sequentially and with --streams 3 (shipped knobs): byte-identical pose files."""
    from revo_amd import run_tum, tum
    from test_gpu_vo_multi import _tum_yaml
    _clear(monkeypatch)
    names = ["rgbd_synth_a", "rgbd_synth_b", "rgbd_synth_c"]
    lens = (14, 22, 9)
    for k, (n, ln) in enumerate(zip(names, lens)):
        seq = synth.make_sequence(60 + k, S320, ln, max_t=0.01, max_rot_deg=0.4,
                                  bias=[0.004, 0, 0, 0, np.deg2rad(1.0), 0])
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), seq)
    _tum_yaml(tmp_path, S320, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--exact-sums"]
    for sub, extra in (("seq", []), ("multi", ["--streams", "3"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    for n, ln in zip(names, lens):
        a = (tmp_path / "seq" / ("poses_%s.txt" % n)).read_bytes()
        b = (tmp_path / "multi" / ("poses_%s.txt" % n)).read_bytes()
        assert a == b and len(a.splitlines()) == ln, n


def test_exact_off_is_the_default_path(monkeypatch):
    """A context whose flag went on and off again gives the records of a fresh default context, and the flag only ever says
    what it was set to; with the flag on, the records are those of a context created in exact mode."""
    from revo_amd import api
    _clear(monkeypatch)
    pairs = synth.make_pairs(range(3000, 3032), S640)
    fresh = _batch_records(_ctx(S640, exact=False), pairs, 32)
    cam = _ctx(S640, exact=False)
    assert cam.exact_sums is False
    cam.setExactSums(True)
    assert cam.exact_sums is True
    on = _batch_records(cam, pairs, 32)
    cam.setExactSums(False)
    assert cam.exact_sums is False
    off = _batch_records(cam, pairs, 32)
    assert off == fresh
    assert on == _batch_records(_ctx(S640, exact=True), pairs, 32)
    # the tracker settings do not reset the flag
    cam.setExactSums(True)
    api.TrackerNew(TrackerSettings(), S640, cam)
    assert cam.exact_sums is True
