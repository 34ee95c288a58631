"""k_track / k_pair_info with the per-point arithmetic laid out in register pairs (revo_amd/csrc/revo_track_px.h): the bits are
those of the scalar form it replaced.

tests/golden/track_pairs.npz was recorded with the library of the commit BEFORE the pair form (REVO_HIP_SO picks a library;
`python tests/test_gpu_track_pairs.py OUT.npz` records, and a second process with the same library reproduced the file before it
was committed).  4 seeded synthetic pairs at 320x240, 3 levels: level 0 has ~6 k points, more than 2 x cluster x 512 for
clusters 1 and 4, so the register-resident points and the streaming loop both run; the coarsest level is evaluated
redundantly (REVO_TRACK_REDUNDANT_BATCH).  Per variant -- the shipped speculation (1 and 3 retries), every level with 2
retries, every level with none, in the default and in the exact-sums mode -- compared byte for byte:
  - the 96-byte pair records of a batch (R, T, err, good, bad, status, evals, flags),
  - the single-pair call on pair 0,
  - the evaluation-only launch (eval_only / EvalOut: error, sums, counts, A, b) at two fixed poses per level,
  - revo_pair_info's record and pair_covariance on pair 0 (k_pair_info)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "track_pairs.npz")
KNOBS = ("REVO_TRACK_CLUSTER", "REVO_TRACK_CLUSTER_ONE", "REVO_TRACK_REDUNDANT_BATCH", "REVO_TRACK_REDUNDANT_ONE",
         "REVO_TRACK_KSPEC", "REVO_TRACK_KSPEC_ONE")
REC = 96  # sizeof(revo_pair_result)
SEEDS = range(7100, 7104)
VARIANTS = [  # (label, knobs)
    ("shipped-c1", {"REVO_TRACK_CLUSTER": "1", "REVO_TRACK_CLUSTER_ONE": "1"}),
    ("shipped-c4", {"REVO_TRACK_CLUSTER": "4", "REVO_TRACK_CLUSTER_ONE": "4"}),
    ("k3-c4", {"REVO_TRACK_CLUSTER": "4", "REVO_TRACK_CLUSTER_ONE": "4", "REVO_TRACK_KSPEC": "3", "REVO_TRACK_KSPEC_ONE": "3"}),
    ("k1-c1", {"REVO_TRACK_CLUSTER": "1", "REVO_TRACK_CLUSTER_ONE": "1", "REVO_TRACK_KSPEC": "1", "REVO_TRACK_KSPEC_ONE": "1"}),
]


def _settings():
    from revo_amd.settings import ImgPyramidSettings
    return ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))


def _pairs():
    from revo_amd import synth
    return synth.make_pairs(SEEDS, _settings())


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def collect(pairs, exact):
    """everything the fixture holds for one variant (the knobs are already in the environment), as uint8 arrays"""
    import torch
    from revo_amd import api
    from revo_amd.settings import OptimizerSettings, TrackerSettings
    S = _settings()
    cam = api.CameraPyr(S, exact_sums=exact)
    trk = api.TrackerNew(TrackerSettings(), S, cam)
    out = {}
    n = len(pairs)
    bt = api.BatchTracker(cam, n)
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")])).cuda()
    d_res = torch.zeros(n * REC, dtype=torch.uint8, device="cuda")
    bt.track(bgr.data_ptr(), dep.data_ptr(), d_res.data_ptr())
    bt.sync()
    out["records"] = d_res.cpu().numpy().copy()
    res = api.results_from_buffer(out["records"].tobytes(), n)
    assert all((r["flags"] & (2 | 8)) == 0 for r in res)
    npts0 = None
    # pair 0 through the single-pair kernels: the tracker, the evaluation-only launch, the information record
    p = pairs[0]
    ref = api.ImgPyramidRGBD(S, cam, *p["ref"])
    cur = api.ImgPyramidRGBD(S, cam, *p["curr"])
    ref.makeKeyframe()
    status, R, T, err = trk.trackFrames(np.eye(3), np.zeros(3), ref, cur)
    info = trk.last_info
    out["single"] = np.concatenate([_u8(np.asarray(R, np.float32)), _u8(np.asarray(T, np.float32)), _u8(np.float32(err)),
                                    _u8(np.asarray([info.good_pts_edges, info.bad_pts_edges, status], np.int32)),
                                    _u8(np.asarray(trk.last_evals, np.int32))])
    opt = api.Optimizer(OptimizerSettings(), cam)
    gt = p["T_ref_curr"]
    ev = []
    for lvl in range(S.nLevels()):
        if lvl == 0:
            npts0 = len(cur.return3DEdges(0))
        for Rp, Tp in ((np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3])):
            e, inf, A, b = opt.evalAt(ref, cur, Rp, Tp, lvl)
            ev += [_u8(np.float32(e)), _u8(np.asarray([inf.good_pts_edges, inf.bad_pts_edges], np.int32)),
                   _u8(np.asarray([inf.sum_error_weighted, inf.sum_error_unweighted], np.float32)),
                   _u8(np.asarray(A, np.float32)), _u8(np.asarray(b, np.float32))]
    out["eval"] = np.concatenate(ev)
    pi = trk.pairInfo(ref, cur, R, T, 0)
    out["pair_info"] = _u8(pi)
    cov, sigma2 = api.pair_covariance(pi)
    out["covariance"] = np.concatenate([_u8(np.ascontiguousarray(cov, np.float64)), _u8(np.float64(sigma2))])
    out["npts0"] = np.asarray([npts0], np.int64)
    return out


def collect_all(setenv, delenv):
    pairs = _pairs()
    got = {}
    for label, knobs in VARIANTS:
        for exact in (False, True):
            for k in KNOBS:
                delenv(k)
            for k, v in knobs.items():
                setenv(k, v)
            for name, arr in collect(pairs, exact).items():
                got["%s/%s/%s" % (label, "exact" if exact else "default", name)] = arr
    return got


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_the_shape_reaches_both_point_paths(golden):
    """level 0 holds more than 2 x cluster x 512 points for the largest cluster used: registers AND the streaming loop"""
    assert int(golden["shipped-c4/default/npts0"][0]) > 2 * 4 * 512


def test_bits_are_those_of_the_scalar_form(golden, monkeypatch):
    got = collect_all(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert sorted(got) == sorted(golden)
    assert len(got) == len(VARIANTS) * 2 * 6
    diff = [k for k in sorted(got) if got[k].tobytes() != golden[k].tobytes()]
    assert not diff, diff


if __name__ == "__main__":  # record: REVO_HIP_SO=<library of the commit before> python tests/test_gpu_track_pairs.py OUT.npz
    sys.path.insert(0, os.path.dirname(HERE))
    data = collect_all(os.environ.__setitem__, lambda k: os.environ.pop(k, None))
    np.savez_compressed(sys.argv[1], **data)
    print("recorded %d arrays, %d bytes, level-0 points %d, library %s"
          % (len(data), sum(a.nbytes for a in data.values()), int(data["shipped-c4/default/npts0"][0]),
             os.environ.get("REVO_HIP_SO", "(the package's)")))
