"""The specification of revo_pair_info (include/revo_hip.h) in numpy: the record k_pair_info writes for one pair at one
pose of one level, built from exact_sums_ref's per-point terms and exact sums, and a float64 restatement of
revo_pair_info_covariance.  Test infrastructure only: nothing under revo_amd/ imports it."""
import ctypes as C

import numpy as np

from revo_amd.settings import PairInfo

import exact_sums_ref as xr


def pair_info(ref_table, pts, cam, R, T, edge_distance, use_edge_filter, huber, level=0):
    """The 192 bytes of the record: ref_table / pts / cam as exact_sums_ref.point_terms takes them, R (3x3, row-major numpy) and
    T the pose curr -> keyframe."""
    terms, sw, su, good, bad = xr.point_terms(ref_table, pts, cam, R, T, edge_distance, use_edge_filter, huber)
    r = PairInfo()
    for k in range(21):
        r.H[k] = xr.round_exact_f32(terms[k])
    for a in range(6):
        r.g[a] = xr.round_exact_f32(terms[21 + a])
    r.sum_w, r.sum_u = xr.round_exact_f32(sw), xr.round_exact_f32(su)
    r.good, r.bad, r.level, r.flags = good, bad, level, 0
    Rc = np.ascontiguousarray(np.asarray(R, np.float32).T).reshape(9)  # column-major, as the C ABI takes it
    for i in range(9):
        r.R[i] = Rc[i]
    for i in range(3):
        r.T[i] = np.asarray(T, np.float32).reshape(3)[i]
    return bytes(r)


def record(buf):
    return PairInfo.from_buffer_copy(buf)


def H_matrix(rec):
    """The symmetric 6x6 float64 matrix of a record's upper triangle."""
    H = np.zeros((6, 6), np.float64)
    H[np.triu_indices(6)] = np.array(list(rec.H), np.float64)
    return H + np.triu(H, 1).T


def covariance(rec):
    """(cov [6, 6] float64, sigma2) of a record: sigma2 = sum_w / (good - 6), cov = sigma2 * inv(H), symmetrised."""
    H = H_matrix(rec)
    s2 = float(rec.sum_w) / float(rec.good - 6)
    X = np.linalg.inv(H)
    return s2 * 0.5 * (X + X.T), s2


assert C.sizeof(PairInfo) == 192
