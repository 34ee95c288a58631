"""Witnesses for tests/track_split_cases.py, from the oracle and the numpy specifications alone (no GPU): the constants of the
table are those of the sources; the restated loops visit every point once; every case has exactly the points per level that
the table states, all of them good at both poses; every case is on the side of each limit that its claims name, under knobs
that a partition of the GPU test sets; every row has a case on each side; the deciders of the init check are decided by the
one point they say.  Only then do the comparisons of tests/test_gpu_track_split.py mean what they claim."""
import numpy as np
import pytest

from revo_amd.settings import OptimizerSettings, TrackerSettings, PLANE_DT, PLANE_EDGES3D, PLANE_GRADTABLE

import exact_sums_ref as xr
import track_split_cases as tc

OS = OptimizerSettings()
T, P = tc.T, tc.P


@pytest.fixture(scope="module")
def ro():
    from oracle import ro as R
    return R


def cam6(s):
    return (s.fx, s.fy, s.cx, s.cy, s.width, s.height)


@pytest.fixture(scope="module")
def facts(ro):
    """name -> the oracle's pyramids of the case and the points per level (finest first)"""
    out = {}
    for name, c in tc.CASES.items():
        s = tc.settings_of(c["size"])
        ref, cur = tc.frames_of(c)
        o_ref, o_cur = ro.Pyramid(s, *ref), ro.Pyramid(s, *cur)
        o_ref.makeKeyframe()
        out[name] = dict(c, name=name, s=s, o_ref=o_ref, o_cur=o_cur,
                         counts=tuple(o_cur.read(PLANE_EDGES3D, l).shape[0] for l in range(s.nLevels())))
    return out


def test_the_constants_are_those_of_the_sources():
    """A changed TRACK_THREADS, TRACK_MAXP, TRACK_MAX_CLUSTER, INFO_CHUNK or shipped threshold moves every limit of the table."""
    have = tc.constants_in_the_sources()
    want = dict(T=tc.T, P=tc.P, MAX_CLUSTER=tc.MAX_CLUSTER, KMAX=tc.KMAX, INFO_THREADS=tc.INFO_THREADS, INFO_CHUNK=tc.INFO_CHUNK,
                INFO_MAX_GROUPS=tc.INFO_MAX_GROUPS, R_BATCH=tc.R_BATCH, R_ONE=tc.R_ONE)
    assert have == want
    assert (T, P, tc.MAX_CLUSTER, tc.R_BATCH, tc.R_ONE, tc.INFO_CHUNK) == (512, 2, 32, 400, 1024, 1024)
    assert tc.R_ONE == P * T  # why rows 4 and 6 coincide for the single pair


def _walk(N, C, r):
    """k_track's loops as written: per member the visits of every index by the register points and by the streaming loop"""
    reg, stream = np.zeros((C, N), np.int32), np.zeros((C, N), np.int32)
    tids = np.arange(T)
    s = tc.stride(N, C, r)
    for m in range(C):
        f = tc.first(N, C, r, m, tids)
        for k in range(P):
            i = f + k * s
            np.add.at(reg[m], i[i < N], 1)
        i = f + P * s
        while (i < N).any():
            np.add.at(stream[m], i[i < N], 1)
            i = i + s
    return reg, stream


@pytest.mark.parametrize("N,C,r", [(0, 4, 0), (1, 32, 0), (513, 2, 0), (513, 16, 0), (1024, 4, 1024), (1025, 4, 1024), (1025, 1, 0), (2049, 2, 0),
                                   (2660, 1, 0), (4097, 4, 0), (5500, 2, 0), (8193, 8, 400), (400, 8, 400), (401, 8, 400)])
def test_the_restated_split_visits_every_point_once(N, C, r):
    """The loops of k_track, walked index by index, against the closed forms of the table (split_facts)."""
    reg, stream = _walk(N, C, r)
    f = tc.split_facts(N, C, r)
    if f["redundant"]:
        assert all(((reg[m] + stream[m]) == 1).all() for m in range(C))  # every member visits all of it
        per_member = stream[0]
    else:
        assert ((reg + stream).sum(axis=0) == 1).all()
        per_member = stream.sum(axis=0)
        assert f["idle"] == sum(1 for m in range(C) if (reg[m] + stream[m]).sum() == 0)
    assert f["streamed"] == int(per_member.sum())
    if f["streamed"]:
        assert int(np.flatnonzero(per_member)[0]) == tc.first_streamed(N, C, r)
    assert f["most"] == tc.points_of_thread(N, C, r, 0, 0) == (0 if N == 0 else int(reg[0][0::tc.stride(N, C, r)].sum() + stream[0][0::tc.stride(N, C, r)].sum()))


def test_info_split():
    assert [tc.info_groups(w * h) for w, h in ((160, 120), (320, 240), (640, 240), (640, 480), (2048, 1024))] == [3, 10, 19, 32, 32]
    for N, G in ((0, 19), (1, 19), (1025, 19), (19 * 1024 + 1, 19), (30480, 19), (2, 3)):
        per = [tc.info_chunks(N, G, g) for g in range(G)]
        assert sum(per) == (N + 1023) // 1024 and max(per) - min(per) <= 1, (N, per)
    assert [tc.info_chunks(19 * 1024 + 1, 19, g) for g in (0, 1)] == [2, 1]


def test_every_case_has_its_counts_and_every_point_is_good(facts):
    """The points per level are the table's; for the single-level cases every point passes the validity test and the edge
    filter at the identity and at the prior (good = N, bad = 0, from the specification), which makes the counts the sharp check."""
    for size, n in (("160", 3521), ("320", 15798), ("640", 30480), ("640t", 36391)):
        assert len(tc.supply(size)[0]) == n, size
    assert tc.CASES["640x240 N=30480"]["N"] == len(tc.supply("640")[0])
    for name, f in facts.items():
        assert f["counts"] == f["levels"], (name, f["counts"])
        if f["size"] == "pyr":
            continue
        s = f["s"]
        table, pts = f["o_ref"].read(PLANE_GRADTABLE, 0), f["o_cur"].read(PLANE_EDGES3D, 0)
        for R, Tr in tc.poses_of(f):
            _, _, _, good, bad = xr.point_terms(table, pts, cam6(s), R, Tr, OS.edge_distance_lvl[0], 1, OS.huber_edge)
            assert (good, bad) == (f["N"], 0), name
    for size, Ns in (("640", tc.BATCH13), ("640t", tc.BATCH4_N)):
        assert max(Ns) <= len(tc.supply(size)[0])


def test_every_claim_holds_under_a_partition_of_the_gpu_test(facts):
    single = {(C, r) for _, _, C, r, _ in tc.SINGLE}
    batch = {(C, r) for _, _, C, r, _ in tc.BATCH + [tc.BATCH4]}
    cost = {(C, r) for _, _, C, r, _ in tc.COST}
    for name, f in facts.items():
        if f["size"] == "pyr":
            for label, env, C, r, k in tc.pyr_partitions(f)[1:]:
                assert tc.level_order(f["counts"], C, r) == f["order"], (name, label)
            assert tc.level_order(f["counts"], 1, 0) == "RRR"
            continue
        for C, r, want in f["claims"]:
            have = tc.split_facts(f["counts"][0], C, r)
            assert {k: have[k] for k in want} == want, (name, C, r, have)
            where = cost if f["special"] else (single | batch if f["N"] in tc.BATCH13 + tc.BATCH4_N else single)
            assert (C, r) in where, (name, C, r)
        assert f["claims"] or f["rows"] == (10,), name
    assert {C for C, _ in single} == {1, 2, 4, 16, 32} and {C for C, _ in batch} == {1, 2, 4, 8, 32}
    assert {k for _, _, _, _, k in tc.SINGLE} == {1, 2, 3, 4}
    assert tc.SINGLE[0][2:] == (1, 0, 1)  # the base: the plain ladder


def _at(f, C, r):
    return tc.split_facts(f["counts"][0], C, r)


def _single(f):
    return f["size"] != "pyr" and not f["special"]


# (row of the table, what must be witnessed, who witnesses it)
REQUIRED = [
    (1, "no point", lambda f: _single(f) and f["counts"] == (0,)),
    (1, "one point", lambda f: _single(f) and f["counts"] == (1,)),
    (2, "63 lanes of one wave", lambda f: _single(f) and f["counts"] == (63,)),
    (2, "one full wave", lambda f: _single(f) and f["counts"] == (64,)),
    (2, "one lane of the second wave", lambda f: _single(f) and f["counts"] == (65,)),
    (3, "T - 1", lambda f: _single(f) and f["counts"] == (T - 1,) and _at(f, 2, 0)["idle"] == 1),
    (3, "T: member 1 without a point", lambda f: _single(f) and f["counts"] == (T,) and _at(f, 2, 0)["member1"] == 0 and _at(f, 1, 0)["most"] == 1),
    (3, "T + 1: a second register point, member 1's first point", lambda f: _single(f) and f["counts"] == (T + 1,) and _at(f, 2, 0)["member1"] == 1 and _at(f, 1, 0)["most"] == 2),
    (4, "P T, nothing streamed", lambda f: _single(f) and f["counts"] == (P * T,) and _at(f, 1, 0)["streamed"] == 0),
    (4, "P T + 1, one point streamed", lambda f: _single(f) and f["counts"] == (P * T + 1,) and _at(f, 1, 0)["streamed"] == 1),
    (4, "redundant: three streamed rounds and more, the last with more than a wave and less than T", lambda f: _single(f) and _at(f, 1, 0)["rounds"] >= 3 and 64 < _at(f, 1, 0)["last_round"] < T and f["counts"][0] < 4096),
    (4, "exchanged: three streamed rounds and more, the last with more than a wave and less than T", lambda f: _single(f) and _at(f, 2, 0)["rounds"] >= 3 and 64 < _at(f, 2, 0)["last_round"] < T),
] + [(4, "P C T at C = %d" % C, lambda f, C=C: _single(f) and f["counts"] == (P * C * T,) and _at(f, C, 0)["streamed"] == 0) for C in (2, 4, 8, 32)
] + [(4, "P C T + 1 at C = %d" % C, lambda f, C=C: _single(f) and f["counts"] == (P * C * T + 1,) and _at(f, C, 0)["streamed"] == 1) for C in (2, 4, 8, 32)
] + [(4, "the init check decided by the streamed point, C = %d" % C,
      lambda f, C=C: f["special"] and f["counts"] == (P * C * T + 1,) and _at(f, C, 0)["streamed"] == 1) for C in (1, 2, 4)
] + [
    (5, "31 of 32 members idle", lambda f: _single(f) and _at(f, 32, 0)["idle"] == 31),
    (5, "14 of 16 members idle", lambda f: _single(f) and _at(f, 16, 0)["idle"] == 14),
    (6, "N = r at 400", lambda f: _single(f) and f["counts"] == (tc.R_BATCH,) and _at(f, 4, tc.R_BATCH)["redundant"]),
    (6, "N = r + 1 at 400", lambda f: _single(f) and f["counts"] == (tc.R_BATCH + 1,) and not _at(f, 4, tc.R_BATCH)["redundant"]),
    (6, "N = r at 1024", lambda f: _single(f) and f["counts"] == (tc.R_ONE,) and _at(f, 4, tc.R_ONE)["redundant"]),
    (6, "N = r + 1 at 1024", lambda f: _single(f) and f["counts"] == (tc.R_ONE + 1,) and not _at(f, 4, tc.R_ONE)["redundant"]),
    (6, "N = r at 0", lambda f: _single(f) and f["counts"] == (0,) and _at(f, 32, 0)["redundant"]),
    (6, "N = r + 1 at 0", lambda f: _single(f) and f["counts"] == (1,) and not _at(f, 32, 0)["redundant"]),
] + [(7, "the order " + o, lambda f, o=o: f["size"] == "pyr" and min(f["counts"]) > 0 and tc.level_order(f["counts"], f["C"], f["r"]) == o)
     for o in ("RRX", "XXR", "RXR", "XRX")
] + [
    (8, "an empty level between levels with points", lambda f: f["size"] == "pyr" and f["counts"][1] == 0 and min(f["counts"][0], f["counts"][2]) > 0),
    (8, "an empty finest level", lambda f: f["size"] == "pyr" and f["counts"][0] == 0 and min(f["counts"][1:]) > 0),
    (10, "k_pair_info without a point", lambda f: _single(f) and f["counts"] == (0,)),
    (10, "k_pair_info with one point", lambda f: _single(f) and f["counts"] == (1,)),
    (10, "a chunk one short", lambda f: _single(f) and f["counts"] == (tc.INFO_CHUNK - 1,)),
    (10, "one chunk", lambda f: _single(f) and f["counts"] == (tc.INFO_CHUNK,) and f["size"] == "640"),
    (10, "one chunk and a point", lambda f: _single(f) and f["counts"] == (tc.INFO_CHUNK + 1,) and f["size"] == "640"),
    (10, "G chunks", lambda f: _single(f) and f["counts"] == (tc.info_groups(f["s"].width * f["s"].height) * tc.INFO_CHUNK,)),
    (10, "G chunks and a point", lambda f: _single(f) and f["counts"] == (tc.info_groups(f["s"].width * f["s"].height) * tc.INFO_CHUNK + 1,)),
    (10, "the whole supply", lambda f: _single(f) and f["counts"] == (len(tc.supply(f["size"])[0]),)),
]


def _witnesses(facts):
    return {(row, label): [n for n, f in facts.items() if row in f["rows"] and pred(f)] for row, label, pred in REQUIRED}


def test_every_row_is_witnessed_on_each_side_of_its_limits(facts):
    wit = _witnesses(facts)
    for row, label, _ in REQUIRED:
        print("row %2d  %-90s %s" % (row, label, wit[(row, label)]))
        assert wit[(row, label)], "row %d: nothing witnesses '%s'" % (row, label)
    assert {r for r, _, _ in REQUIRED} == set(range(1, 11)) - {9}
    assert {r for f in facts.values() for r in f["rows"]} == set(range(1, 11)) - {9}  # 9: BATCH13, below


def test_the_census_bites(facts):
    """Taking any one case away leaves a required witness without a case, or the case names the sibling it stands beside; and no
    two cases give the same reason."""
    wit = _witnesses(facts)
    whys = [f["why"] for f in facts.values()]
    assert len(set(whys)) == len(whys) and all(whys)
    for name, f in facts.items():
        sole = [key for key, names in wit.items() if names == [name]]
        if "sibling" in f["why"]:
            sib = f["why"].split("sibling row of ")[1].split(";")[0].strip()
            assert sib in facts and set(f["rows"]) <= set(facts[sib]["rows"]), (name, sib)
        assert sole, "%s (%s) is the only witness of nothing" % (name, f["why"])


def test_the_batch_of_13_holds_every_row(facts):
    """Row 9: 13 pairs (no multiple of 8: the last three of the second group of eight leave through the XCD mapping), each the
    count of a case of rows 1-6, every one of those rows among them, redundant and exchanged pairs side by side in every batch
    partition with more than one workgroup per pair."""
    assert len(tc.BATCH13) == 13 and len(tc.BATCH13) % 8
    rows = set()
    for N in tc.BATCH13:
        of = [f for f in facts.values() if _single(f) and f["counts"] == (N,)]
        assert of and set(of[0]["rows"]) & set(range(1, 7)), N
        rows |= set(of[0]["rows"])
    assert rows >= set(range(1, 7))
    for label, _, C, r, _ in tc.BATCH:
        kinds = {tc.redundant(N, C, r) for N in tc.BATCH13}
        assert kinds == ({True, False} if C > 1 else {True}), label
    _, _, C, r, _ = tc.BATCH4
    assert [tc.split_facts(N, C, r)["idle"] for N in tc.BATCH4_N] == [31, 30, 0, 0] and tc.split_facts(32769, C, r)["streamed"] == 1


def test_the_deciders_are_decided_by_their_streamed_point(facts):
    """checkInitializationValues from shift_prior: over all N points the identity is cheaper than the prior (flag 1); without
    the special point, which is the last of the tile-ordered list, it is not (the costs tie at 0: flag 0).  So a MODE_COST loop
    that loses the streamed point answers 0 where the specification says 1."""
    n = 0
    for name, f in facts.items():
        if not f["special"]:
            continue
        s = f["s"]
        dt, pts = f["o_ref"].read(PLANE_DT, 0), f["o_cur"].read(PLANE_EDGES3D, 0)
        sp = pts[:, 2] == np.float32(tc.SPECIAL_DEPTH)
        assert sp.sum() == 1 and np.all(pts[~sp, 2] == np.float32(tc.DEPTH))
        sy, sx = tc.decider_supply(f["size"])[2]
        ys, xs = np.nonzero(tc.frames_of(f)[1][1] > 0)
        assert (ys // 32).max() == sy // 32 and ((ys // 32) == sy // 32).sum() == 1, name  # alone in the last row of tiles with points
        prior = tc.shift_prior(f["size"])
        cost = lambda p, pose: xr.eval_cost(dt, p, cam6(s), *pose, OS.edge_distance_lvl[0], 1)  # noqa: E731
        assert cost(pts, tc.IDENTITY) < cost(pts, prior), name
        assert cost(pts[~sp], tc.IDENTITY) == cost(pts[~sp], prior) == 0, name
        n += 1
    assert n == 3


def test_exact_eval_without_points_and_with_one(facts):
    """exact_sums_ref.exact_eval at N = 0 (0 / 0 like the reference: err and every entry NaN, the sums +0) and at N = 1 (every sum
    is its one term)."""
    for name, N in (("160x120 N=0", 0), ("160x120 N=1", 1)):
        f = facts[name]
        table, pts = f["o_ref"].read(PLANE_GRADTABLE, 0), f["o_cur"].read(PLANE_EDGES3D, 0)
        for R, Tr in tc.poses_of(f):
            args = (table, pts, cam6(f["s"]), R, Tr, OS.edge_distance_lvl[0], 1, OS.huber_edge)
            err, sw, su, good, bad, A, b = xr.exact_eval(*args)
            terms, tw, tu, _, _ = xr.point_terms(*args)
            assert (good, bad) == (N, 0)
            if N == 0:
                assert np.isnan(err) and np.isnan(A).all() and np.isnan(b).all()
                assert sw.tobytes() == su.tobytes() == np.float32(0).tobytes()
            else:
                assert sw.tobytes() == tw[0].tobytes() and su.tobytes() == tu[0].tobytes() and err.tobytes() == tw[0].tobytes()
                assert A[np.triu_indices(6)].tobytes() == terms[:21, 0].tobytes() and np.array_equal(b, -terms[21:, 0])  # (the sum of one -0 is +0)
                assert np.abs(terms[:21, 0]).max() > 0


def test_the_oracle_rejects_a_candidate_on_the_way(facts, ro):
    """From the prior the oracle's LM sequence of the cases of rows 1-6 holds rejected candidates (so the retry lanes of
    fused_block see the boundaries), and every case with six points and more takes more than the two evaluations of a level
    that ends at once."""
    L = ro.lib()
    buf = np.zeros(4096, np.uint8)
    rejected = 0
    for name in tc.cases_of(range(1, 7)):
        f = facts[name]
        ot = ro.Tracker(f["s"], OS, TrackerSettings(check_init_values=0))
        L.ro_lm_trace(1)
        try:
            r = ot.trackFrames(f["o_ref"], f["o_cur"], *tc.prior_of(f["size"]))
            n = L.ro_lm_trace_get(buf.ctypes.data_as(ro.u8p), len(buf))
        finally:
            L.ro_lm_trace(0)
        rejected += int(0 in (buf[:n] & 1).tolist())
        if f["N"] >= 63:
            assert r["evals"][0] >= 3, (name, r["evals"])
    assert rejected >= 5, rejected
