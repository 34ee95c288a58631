"""Many sequential-VO streams through one handle (revo_vo_multi_*, vo.MultiREVO): per stream the same bits as a vo.REVO on
that sequence alone, whatever the neighbours do; against the oracle at the metric configuration; argument errors."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, TrackerSettings  # noqa: E402

from test_gpu_configs import SAME_PARTITION  # noqa: E402

INVALID_ARG, CAPACITY = -1, -5  # REVO_ERR_INVALID_ARG, REVO_ERR_CAPACITY
S320 = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
# every motion pans by ~1 degree a frame (what makes the quality vote ask for new keyframes), about different axes
BIASES = [[0.004, 0, 0, 0, np.deg2rad(1.0), 0], [0, 0.003, 0, np.deg2rad(1.0), 0, 0], [0.002, 0, 0.003, 0, np.deg2rad(1.2), 0],
          [0, 0, 0, 0, np.deg2rad(1.5), 0], [0.005, 0.002, 0, 0, np.deg2rad(0.8), np.deg2rad(0.5)],
          [0, 0, 0.004, np.deg2rad(1.0), np.deg2rad(0.6), 0]]


def _seq(seed, n, s=S320, bias_i=None):
    b = BIASES[(seed if bias_i is None else bias_i) % len(BIASES)]
    return [(f[0], f[1], f[2]) for f in synth.make_sequence(seed, s, n, max_t=0.01, max_rot_deg=0.4, bias=b)]


def _solo(frames, s=S320, trk=None, dsf=None):
    from revo_amd import vo
    g = vo.REVO(s, trk, depth_scale_factor=dsf)
    res = [g.push(*f) for f in frames]
    return res, [ts for ts, _ in g.poses], g.nKeyFrames


def _same_partition(monkeypatch):
    for k, v in SAME_PARTITION.items():
        monkeypatch.setenv(k, v)


def _run_streams(m, seqs, slots):
    """lockstep by hand: seqs[k] on stream slots[k]; returns per sequence [(pose, kf, ts)]"""
    out = [[] for _ in seqs]
    pos = [0] * len(seqs)
    by_stream = {s: k for k, s in enumerate(slots)}
    while True:
        frames = []
        for k, s in enumerate(slots):
            if pos[k] < len(seqs[k]) and m.pending(s) == 0:
                f = seqs[k][pos[k]]
                frames.append((s, f[0], f[1], f[2]))
                pos[k] += 1
        if frames:
            m.submit(frames)
        if not any(m.pending(s) for s in slots):
            break
        for s, M, kf, ts in m.step():
            out[by_stream[s]].append((M, kf, ts))
    return out


def test_bit_identical_to_solo_revo_per_stream(monkeypatch):
    _same_partition(monkeypatch)
    from revo_amd import vo
    lens = [30, 45, 36, 40, 33, 42]
    seqs = [_seq(100 + k, n) for k, n in enumerate(lens)]
    m = vo.MultiREVO(S320, 8)
    slots = [0, 2, 3, 4, 6, 7]  # streams 1 and 5 stay idle
    got = _run_streams(m, seqs, slots)
    kf_frames = set()
    for k, frames in enumerate(seqs):
        ref, ts_ref, nkf = _solo(frames)
        assert len(got[k]) == len(frames)
        for i, ((Mg, kg, tg), (Mr, kr)) in enumerate(zip(got[k], ref)):
            assert np.array_equal(Mg, Mr) and kg == kr and tg == ts_ref[i], (k, i)
        assert m.nKeyFrames(slots[k]) == nkf, (k, nkf)
        kf_frames.add(tuple(i for i, r in enumerate(ref) if r[1]))
    # the streams change keyframes at different frames: they fall out of step
    assert len(kf_frames) >= 3 and sum(len(p) >= 2 for p in kf_frames) >= 3, kf_frames
    assert m.nKeyFrames(1) == 0 and m.pending(1) == 0


def test_a_stream_does_not_depend_on_its_neighbours():
    from revo_amd import vo
    target = _seq(7, 36, bias_i=0)
    busy = [_seq(200 + k, 36) for k in range(7)]
    m1 = vo.MultiREVO(S320, 8)
    seqs = busy[:5] + [target] + busy[5:]
    got_busy = _run_streams(m1, seqs, list(range(8)))[5]
    m2 = vo.MultiREVO(S320, 8)
    got_alone = _run_streams(m2, [target], [0])[0]
    assert len(got_busy) == len(got_alone) == len(target)
    for (a, ka, ta), (b, kb, tb) in zip(got_busy, got_alone):
        assert np.array_equal(a, b) and ka == kb and ta == tb


def test_against_the_oracle_at_the_metric_configuration():
    from oracle import ro
    from revo_amd import vo
    s = ImgPyramidSettings.scaled(640, 480, 4, hist_patch=(20, 10, 5, 0, 0, 0))
    n = 60
    # test_gpu_vo.py's metric sweep (a 0.5 degree pan a frame), about different axes
    bias = [[0.004, 0, 0, 0, np.deg2rad(0.5), 0], [0, 0.004, 0, np.deg2rad(0.5), 0, 0], [0.004, 0, 0, 0, -np.deg2rad(0.5), 0],
            [0, 0, 0.004, 0, np.deg2rad(0.5), 0]]
    data = [synth.make_sequence(11 + k, s, n, max_t=0.01, max_rot_deg=0.4, bias=bias[k % 4], workers=8) for k in range(8)]
    m = vo.MultiREVO(s, 8)
    res = m.run([[(f[0], f[1], f[2]) for f in d] for d in data])
    for k, d in enumerate(data):
        cpu = ro.VO(s)
        est_o, kf_o = [], []
        for i, f in enumerate(d):
            po, ko = cpu.push(f[0], f[1], f[2])
            est_o.append(po)
            if ko:
                kf_o.append(i)
        est_g = [r[0] for r in res[k]]
        kf_g = [i for i, r in enumerate(res[k]) if r[1]]
        assert kf_g == kf_o, (k, kf_g, kf_o)
        d_rot = max(synth.rot_angle(a[:3, :3], b[:3, :3]) for a, b in zip(est_g, est_o))
        d_tr = max(float(np.linalg.norm(a[:3, 3] - b[:3, 3])) for a, b in zip(est_g, est_o))
        gt = [f[3] for f in d]
        assert synth.ate_rmse(est_g, est_o) < 1e-3
        assert d_rot < 5e-4 and d_tr < 5e-4
        assert abs(synth.ate_rmse(est_g, gt) - synth.ate_rmse(est_o, gt)) < 1e-3


def test_unequal_lengths_through_two_streams_with_refill(monkeypatch):
    _same_partition(monkeypatch)
    from revo_amd import vo
    lens = [8, 40, 15, 27, 11]
    seqs = [_seq(400 + k, n) for k, n in enumerate(lens)]
    m = vo.MultiREVO(S320, 2)
    res = m.run(seqs)
    assert len(res) == len(seqs)
    for k, frames in enumerate(seqs):
        ref, ts_ref, _ = _solo(frames)
        assert len(res[k]) == len(frames), k
        assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(res[k], ref)), k
        assert [t for t, _ in res[k].poses] == ts_ref
        solo = vo.REVO(S320)
        for f in frames:
            solo.push(*f)
        assert res[k].tum_lines() == solo.tum_lines()


@pytest.mark.parametrize("case", ["hist0", "hist2", "hist3", "hist4", "nocheck", "noedgefilter", "u16"])
def test_tracker_settings_bit_identical(monkeypatch, case):
    _same_partition(monkeypatch)
    from revo_amd import vo
    from revo_amd.settings import OptimizerSettings
    trk = TrackerSettings()
    if case.startswith("hist"):
        trk.n_frames_hist_voting = int(case[4:])
    if case == "nocheck":
        trk.check_tracking_results = 0
    if case == "noedgefilter":
        trk.optimizerSettings = OptimizerSettings(use_edge_filter=0)
    dsf = 5000.0 if case == "u16" else None
    seqs = [_seq(500 + k, 34) for k in range(3)]
    if dsf:
        seqs = [[(b, np.clip(d * dsf, 0, 65535).astype(np.uint16), t) for b, d, t in q] for q in seqs]
    m = vo.MultiREVO(S320, 4, trk, depth_scale_factor=dsf)
    res = m.run(seqs)
    for k, frames in enumerate(seqs):
        ref, _, _ = _solo(frames, trk=trk, dsf=dsf)
        assert len(res[k]) == len(ref)
        assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(res[k], ref)), (case, k)


def test_shared_context_with_a_revo_vo(monkeypatch):
    _same_partition(monkeypatch)
    from revo_amd import vo
    a, b = _seq(600, 30), _seq(601, 30, bias_i=3)
    ref_a, _, _ = _solo(a)
    ref_b, _, _ = _solo(b)
    single = vo.REVO(S320)
    got_a, got_b = [single.push(*a[i]) for i in range(10)], []
    # the handle arrives while the REVO is mid-sequence (its past clouds are on the shared context)
    m = vo.MultiREVO(S320, 4, cameraPyr=single.camPyr)
    with pytest.raises(ValueError):
        vo.MultiREVO(S320, 2, TrackerSettings(), cameraPyr=single.camPyr)  # would reset the shared context's tracker
    for i in range(30):
        if i >= 10:
            got_a.append(single.push(*a[i]))
        while m.pending(1) >= m.max_queue:  # a deferred keyframe change holds its frame one step longer
            got_b += [(M, kf) for _, M, kf, _ in m.step()]
        m.submit([(1, b[i][0], b[i][1], b[i][2])])
        got_b += [(M, kf) for _, M, kf, _ in m.step()]
    while m.pending(1):
        got_b += [(M, kf) for _, M, kf, _ in m.step()]
    assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(got_a, ref_a))
    assert len(got_b) == len(ref_b)
    assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(got_b, ref_b))


def test_keyframe_accessor_matches_the_oracle_pyramid():
    from oracle import ro
    from revo_amd import vo
    frames = _seq(700, 40, bias_i=0)
    m = vo.MultiREVO(S320, 3)
    checked = 0
    got = []
    for i, f in enumerate(frames):
        m.submit([(2, f[0], f[1], f[2])])
        for s, M, kf, ts in m.step():
            got.append((M, kf))
            if kf:
                # keyframe 0 is frame 0, later ones the frame before the one that asked (system.cpp:205-215)
                fi = 0 if len(got) == 1 else len(got) - 2
                pyr, T = m.keyframe(2)
                o = ro.Pyramid(S320, frames[fi][0], frames[fi][1])
                assert np.array_equal(pyr.generateColoredPcl(0, False), o.generateColoredPcl(0, False)), fi
                assert np.array_equal(T, got[fi][0]), fi
                checked += 1
        while m.pending(2):
            for s, M, kf, ts in m.step():
                got.append((M, kf))
                assert kf
                fi = len(got) - 2
                pyr, T = m.keyframe(2)
                o = ro.Pyramid(S320, frames[fi][0], frames[fi][1])
                assert np.array_equal(pyr.generateColoredPcl(0, False), o.generateColoredPcl(0, False)), fi
                assert np.array_equal(T, got[fi][0]), fi
                checked += 1
    assert checked >= 3 and m.nKeyFrames(2) == checked


def test_argument_errors():
    from revo_amd import api, vo
    from revo_amd._lib import RevoError
    from revo_amd.settings import StreamFrame
    from revo_amd import _lib
    f = _seq(800, 2)
    m = vo.MultiREVO(S320, 2, max_queue=1)
    with pytest.raises(RevoError) as e:
        m.submit([(2, f[0][0], f[0][1], 0.0)])  # out-of-range stream
    assert e.value.code == INVALID_ARG
    with pytest.raises(RevoError) as e:
        m.submit([(0, f[0][0], f[0][1], 0.0), (0, f[1][0], f[1][1], 1.0)])  # two frames for one stream
    assert e.value.code == INVALID_ARG
    assert m.pending(0) == 0  # a refused submit queues nothing
    m.submit([(0, f[0][0], f[0][1], 0.0)])
    with pytest.raises(RevoError) as e:
        m.submit([(0, f[1][0], f[1][1], 1.0)])
    assert e.value.code == CAPACITY
    with pytest.raises(RevoError) as e:
        m.reset(0)  # frames pending
    assert e.value.code == INVALID_ARG
    with pytest.raises(RevoError):
        m.reset(-1)
    assert m.pending(5) == -1 and m.nKeyFrames(5) == -1
    with pytest.raises(RevoError):
        m.keyframe(1)  # no keyframe yet
    assert len(m.step()) == 1 and m.pending(0) == 0
    m.reset(0)
    assert m.nKeyFrames(0) == 0
    L = _lib.lib()
    h = C.c_void_p()
    cam = api.CameraPyr(S320)
    assert L.revo_vo_multi_create(cam._h, 0, 2, C.byref(h)) != 0
    assert L.revo_vo_multi_create(cam._h, 2, 0, C.byref(h)) != 0
    # a frame whose rows are shorter than the context's width: refused before anything is uploaded
    arr = (StreamFrame * 1)()
    arr[0].stream, arr[0].bgr, arr[0].bgr_stride = 1, f[0][0].ctypes.data, 10
    arr[0].depth, arr[0].depth_stride = f[0][1].ctypes.data, 320 * 4
    assert L.revo_vo_multi_submit(m._h, 1, arr, 0, 0.0) != 0 and m.pending(1) == 0


def _tum_yaml(tmp_path, s, names):
    (tmp_path / "dataset.yaml").write_text(
        "%%YAML:1.0\nCamera.fx: %r\nCamera.fy: %r\nCamera.cx: %r\nCamera.cy: %r\nCamera.width: %d\nCamera.height: %d\n"
        "width: %d\nheight: %d\nMainFolder: \"%s/\"\nDatasets: [%s]\nASSOCIATE: \"associate.txt\"\n"
        "PYR_MIN_LVL: 2\nPYR_MAX_LVL: 0\nDEPTH_SCALE_FACTOR: 5000.0\n"
        % (float(s.fx), float(s.fy), float(s.cx), float(s.cy), s.width, s.height, s.width, s.height, str(tmp_path / "data"),
           ", ".join('"%s"' % n for n in names)))
    (tmp_path / "settings.yaml").write_text("%YAML:1.0\nCHECK_TRACKING_RESULTS: 1\nCHECK_INIT_VALUES: 1\nUSE_EDGE_FILTER: 1\n"
                                            "N_FRAMES_HIST_VOTING: 3\nDO_OUTPUT_POSES: 1\n")


def test_run_tum_streams_writes_the_sequential_files(tmp_path, monkeypatch):
    """run_tum --streams 2 on a Datasets list of three TUM-layout folders: the poses_<dataset>.txt files are byte-identical to
    the sequential command line's (SAME_PARTITION: the single-pair and the batched tracker partition alike)."""
    _same_partition(monkeypatch)
    from revo_amd import run_tum, tum
    names = ["rgbd_synth_a", "rgbd_synth_b", "rgbd_synth_c"]
    for k, (n, lens) in enumerate(zip(names, (14, 22, 9))):
        seq = synth.make_sequence(40 + k, S320, lens, max_t=0.01, max_rot_deg=0.4, bias=BIASES[k])
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), seq)
    _tum_yaml(tmp_path, S320, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2"]
    for sub, extra in (("seq", []), ("multi", ["--streams", "2"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    for n, lens in zip(names, (14, 22, 9)):
        a = (tmp_path / "seq" / ("poses_%s.txt" % n)).read_bytes()
        b = (tmp_path / "multi" / ("poses_%s.txt" % n)).read_bytes()
        assert a == b and len(a.splitlines()) == lens, n
