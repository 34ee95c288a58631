"""revo_pair_info without a GPU: the record's layout, the host-side covariance against a numpy restatement, its refusals, and the
link between the record and exact-sums mode's A and b in the specification (tests/pair_info_ref.py, tests/exact_sums_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from revo_amd import api
from revo_amd.settings import ImgPyramidSettings, OptimizerSettings, PairInfo, PLANE_EDGES3D, PLANE_GRADTABLE

import exact_sums_ref as xr
import pair_info_ref as pr

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_record_layout():
    assert C.sizeof(PairInfo) == 192
    want = dict(H=0, g=84, sum_w=108, sum_u=112, good=116, bad=120, level=124, flags=128, R=132, T=168, reserved=180)
    for name, off in want.items():
        assert getattr(PairInfo, name).offset == off, name


@pytest.fixture(scope="module")
def records():
    """Records of the golden pair at three poses of every level, with what exact_eval says at the same pose."""
    from oracle import ro
    z = np.load(os.path.join(GOLD, "small_pair.npz"))
    s = ImgPyramidSettings.scaled(160, 120, 3, hist_patch=(5, 0, 0, 0, 0, 0))
    ref = ro.Pyramid(s, z["ref_bgr"], z["ref_depth"])
    cur = ro.Pyramid(s, z["cur_bgr"], z["cur_depth"])
    ref.makeKeyframe()
    os_ = OptimizerSettings()
    gt = z["T_ref_curr"]
    poses = [(np.eye(3), np.zeros(3)), (gt[:3, :3], 0.5 * gt[:3, 3]), (z["R"], z["T"])]
    out = []
    for lvl in range(3):
        args = (ref.read(PLANE_GRADTABLE, lvl), cur.read(PLANE_EDGES3D, lvl), ref.camera(lvl))
        for R, T in poses:
            tail = (os_.edge_distance_lvl[lvl], os_.use_edge_filter, os_.huber_edge)
            out.append((pr.pair_info(*args, R, T, *tail, level=lvl), xr.exact_eval(*args, R, T, *tail), lvl, R, T))
    return out


def test_record_of_the_restatement(records):
    for buf, ev, lvl, R, T in records:
        r = pr.record(buf)
        assert len(buf) == 192 and r.level == lvl and r.flags == 0 and list(r.reserved) == [0, 0, 0]
        assert r.good > 50 and (r.good, r.bad) == (ev[3], ev[4])
        assert np.array_equal(np.array(list(r.R), np.float32).reshape(3, 3).T, np.asarray(R, np.float32))
        assert np.array_equal(np.array(list(r.T), np.float32), np.asarray(T, np.float32).reshape(3))


def test_H_and_g_over_good_are_exact_evals_A_and_b(records):
    """In the restatement H / good and -(g / good) are exact_eval's A and b, bit for bit (both divide the same exact sum)."""
    iu = np.triu_indices(6)
    for buf, ev, lvl, _, _ in records:
        r = pr.record(buf)
        n = np.float32(r.good)
        A, b = ev[5], ev[6]
        assert (np.array(list(r.H), np.float32) / n).tobytes() == A[iu].astype(np.float32).tobytes(), lvl
        assert (-(np.array(list(r.g), np.float32) / n)).tobytes() == b.tobytes(), lvl
        assert np.float32(r.sum_w).tobytes() == ev[1].tobytes() and np.float32(r.sum_u).tobytes() == ev[2].tobytes()


def test_covariance_against_numpy(records):
    """Elementwise within 64 * 2^-52 * cond(H) * max|cov|: the backward-error bound of a stable 6x6 factorisation."""
    for buf, _, lvl, _, _ in records:
        r = pr.record(buf)
        cov, s2 = api.pair_covariance(r)
        want, s2w = pr.covariance(r)
        assert s2 == s2w
        bound = 64 * 2.0 ** -52 * np.linalg.cond(pr.H_matrix(r)) * np.abs(want).max()
        worst = np.abs(cov - want).max()
        print("level %d: |cov - numpy| max %.3e, bound %.3e, cond %.3e" % (lvl, worst, bound, np.linalg.cond(pr.H_matrix(r))))
        assert worst <= bound
        assert np.array_equal(cov, cov.T)
        assert np.all(np.linalg.eigvalsh(cov) > 0)


def _refused(rec):
    cov = np.full(36, 7.25, np.float64)
    s2 = C.c_double(-3.5)
    rc = api._lib.lib().revo_pair_info_covariance(C.byref(rec), cov.ctypes.data_as(C.POINTER(C.c_double)), C.byref(s2))
    assert rc == -1, rc  # REVO_ERR_INVALID_ARG
    assert np.all(cov == 7.25) and s2.value == -3.5  # nothing written
    with pytest.raises(api.RevoError):
        api.pair_covariance(rec)


def test_covariance_refusals(records):
    good = pr.record(records[0][0])
    api.pair_covariance(good)  # the unmodified record is accepted
    r = pr.record(records[0][0])
    r.flags = 1
    _refused(r)
    r = pr.record(records[0][0])
    r.good = 6
    _refused(r)
    # rank-deficient: rows (and columns) 0 and 1 of H made equal
    r = pr.record(records[0][0])
    H = pr.H_matrix(r)
    H[1, :] = H[0, :]
    H[:, 1] = H[:, 0]
    H[1, 1] = H[0, 0]
    H[0, 1] = H[1, 0] = H[0, 0]
    assert np.array_equal(H, H.T) and np.array_equal(H[0], H[1])
    for k, v in enumerate(H[np.triu_indices(6)]):
        r.H[k] = v
    _refused(r)
