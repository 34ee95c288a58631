"""The work split of the tracker, restated, and one case on each side of every limit of it.  Test infrastructure: no GPU is
touched here.

k_track (revo_amd/csrc/revo_track.hip) splits a level of N points by fixed rules.  With T = TRACK_THREADS = 512 threads per
workgroup, P = TRACK_MAXP = 2 register points per thread, C = the cluster (workgroups per pair, up to TRACK_MAX_CLUSTER = 32)
and r = the redundant threshold:  a level is REDUNDANT (every member evaluates all of it, no exchange) when C == 1 or N <= r,
else EXCHANGED (member m starts at m T, the stride is C T, the partial sums meet in the mailbox).  The first P points of a
thread sit in registers, the rest stream from index P * stride on.  The loop pair "register points, streaming loop" exists three
times: full_point (one candidate), fused_block<1..3> (speculation depth 2..4) and the MODE_COST pass of the init check.
k_pair_info (revo_info.hip) deals chunks of INFO_CHUNK = 1024 points round-robin to G = info_groups(pixels) workgroups.

The point count of a level is set by the DEPTH image alone: the edges come from the gray image, the 3-D list of a level is its
edge pixels with a usable depth.  Rows 1-6 and 10 use a single-level noise image (frontend_limit_cases.noise_image, Canny
60 / 20): the keyframe is that image with depth everywhere, the current frame the same image with depth 1.5 at the first N
edge pixels (row-major) that lie at least MARGIN pixels inside the border.  tests/test_track_split_cpu.py proves with the
oracle that every case has the counts and takes the paths stated here; tests/test_gpu_track_split.py runs them.

The table of limits (the `rows` of a case):
   1  N = 0 and N = 1
   2  the wave edge: N = 63, 64, 65
   3  the workgroup edge: N = 511, 512, 513 (thread 0's second register point when redundant, member 1's first point when exchanged)
   4  the last register point and the first streamed one: N = P T, P T + 1 (redundant), P C T, P C T + 1 (exchanged, C = 2, 4, 8,
      32); three and more streamed rounds with a partial last one; the `decider` cases, whose one streamed point alone decides
      checkInitializationValues (decider_depth)
   5  idle members: exchanged levels with N <= (C - 1) T (N = 1 at r = 0 under C = 32; N = 513 under C = 16)
   6  the redundant switch: N = r, r + 1 at r = 400 (batches), 1024 (single pair) and 0
   7  the order of redundant (R) and exchanged (X) levels, coarse to fine: R R X, X X R, R X R, X R X
   8  an empty level between levels with points, an empty finest level
   9  one grid of 13 pairs with one pair of each of rows 1-6 (BATCH13)
  10  k_pair_info: N = 0, 1 (G - 1 idle groups), 1023 / 1024 / 1025, G * 1024 and G * 1024 + 1, the top of the supply
"""
import functools
import os
import re

import numpy as np

from revo_amd import synth
from revo_amd.settings import ImgPyramidSettings, PAIR_INFO_CHUNK, PAIR_INFO_MAX_GROUPS, pair_info_groups

import frontend_limit_cases as fl
import lm_settings_cases as lc

# ---- the constants, as the table was written for them; `constants_in_the_sources` reads them back from the sources ------------
T, P, MAX_CLUSTER, KMAX = 512, 2, 32, 4
INFO_THREADS, INFO_CHUNK, INFO_MAX_GROUPS = 256, 1024, 32
R_BATCH, R_ONE = 400, 1024  # the shipped thresholds: REVO_TRACK_REDUNDANT_BATCH, REVO_TRACK_REDUNDANT_ONE
MARGIN = 4
DEPTH = 1.5

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "revo_amd", "csrc")


def constants_in_the_sources():
    """What revo_dev.h, revo_track.hip and revo_host.hip define today, under the names used here."""
    def text(name):
        with open(os.path.join(_CSRC, name)) as f:
            return f.read()

    def define(src, name):
        return int(re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M).group(1))

    def env_default(src, name):
        return int(re.search(r'env_int\("%s",\s*(\d+),' % name, src).group(1))

    dev, track, host = text("revo_dev.h"), text("revo_track.hip"), text("revo_host.hip")
    return dict(T=define(dev, "TRACK_THREADS"), P=define(track, "TRACK_MAXP"), MAX_CLUSTER=define(dev, "TRACK_MAX_CLUSTER"),
                KMAX=define(dev, "TRACK_KMAX"), INFO_THREADS=define(dev, "INFO_THREADS"), INFO_CHUNK=define(dev, "INFO_CHUNK"),
                INFO_MAX_GROUPS=define(dev, "INFO_MAX_GROUPS"), R_BATCH=env_default(host, "REVO_TRACK_REDUNDANT_BATCH"),
                R_ONE=env_default(host, "REVO_TRACK_REDUNDANT_ONE"))


# ---- the rules of the split -------------------------------------------------------------------------------------------------

def redundant(N, C, r):
    return C == 1 or N <= r  # revo_track.hip: `cluster == 1 || N <= prm.redundant_n`


def stride(N, C, r):
    return T if redundant(N, C, r) else C * T


def first(N, C, r, member, tid):
    return tid if redundant(N, C, r) else member * T + tid


def points_of_thread(N, C, r, member, tid):
    f, s = first(N, C, r, member, tid), stride(N, C, r)
    return 0 if f >= N else (N - f + s - 1) // s


def first_streamed(N, C, r):
    """index of the first point that the streaming loops read: `first + TRACK_MAXP * stride` of thread 0 of member 0"""
    return P * stride(N, C, r)


def streamed(N, C, r):
    """(points read by the streaming loops, rounds of the longest thread's loop, points of the last round)"""
    s = stride(N, C, r)
    n = max(0, N - P * s)
    rounds = (n + s - 1) // s
    return n, rounds, (n - (rounds - 1) * s if rounds else 0)


def idle_members(N, C, r):
    """members of an exchanged level without a point (`first >= N` for all their threads): they publish zeros"""
    return 0 if redundant(N, C, r) else C - min(C, (N + T - 1) // T)


def info_groups(npix):
    return max(1, min(INFO_MAX_GROUPS, (npix + 8 * INFO_CHUNK - 1) // (8 * INFO_CHUNK)))  # revo_dev.h


def info_chunks(N, G, g):
    """chunks of k_pair_info's workgroup g: g, g + G, ... below ceil(N / INFO_CHUNK)"""
    return len(range(g, (N + INFO_CHUNK - 1) // INFO_CHUNK, G))


def split_facts(N, C, r):
    n, rounds, last = streamed(N, C, r)
    return dict(redundant=redundant(N, C, r), streamed=n, rounds=rounds, last_round=last, idle=idle_members(N, C, r),
                most=points_of_thread(N, C, r, 0, 0), member1=0 if redundant(N, C, r) or C < 2 else points_of_thread(N, C, r, 1, 0))


# ---- the partitions of the GPU test: (label, knobs, C, r, speculation depth) ---------------------------------------------------

def _one(C, r, k):
    return ("single-c%d-r%d-k%d" % (C, r, k),
            {"REVO_TRACK_CLUSTER_ONE": str(C), "REVO_TRACK_REDUNDANT_ONE": str(r), "REVO_TRACK_KSPEC": str(k)}, C, r, k)


def _batch(C, r, k):
    return ("batch-c%d-r%d-k%d" % (C, r, k),
            {"REVO_TRACK_CLUSTER": str(C), "REVO_TRACK_CLUSTER_ONE": str(C), "REVO_TRACK_REDUNDANT_BATCH": str(r), "REVO_TRACK_KSPEC": str(k)}, C, r, k)


# the first is the base: the plain ladder (one workgroup, nothing redundant to switch, one candidate per pass)
SINGLE = [_one(1, 0, 1), _one(1, R_ONE, 4), _one(2, 0, 2), _one(2, R_ONE, 3), _one(4, 0, 3), _one(4, R_ONE, 1), _one(4, R_BATCH, 2),
          _one(16, 0, 4), _one(16, R_ONE, 2), _one(32, 0, 1), _one(32, R_ONE, 4)]
BATCH = [_batch(1, R_BATCH, 2), _batch(2, R_BATCH, 1), _batch(4, R_BATCH, 4), _batch(8, R_BATCH, 3), _batch(8, 0, 2)]
BATCH4 = _batch(32, 0, 2)
# batches of ONE pair (their records carry the flags that the single-pair call does not return): REVO_TRACK_CLUSTER_ONE picks
# their cluster, REVO_TRACK_REDUNDANT_BATCH their threshold
COST = [_batch(1, 0, 1), _batch(2, 0, 1), _batch(2, R_ONE, 1), _batch(4, 0, 1), _batch(4, R_BATCH, 1), _batch(16, 0, 1), _batch(32, 0, 1),
        _batch(32, R_ONE, 1)]


# ---- images and masks ---------------------------------------------------------------------------------------------------------

SIZES = {"160": (160, 120), "320": (320, 240), "640": (640, 240), "640t": (640, 288)}


def settings_of(size):
    if size == "pyr":
        return lc.S320
    w, h = SIZES[size]
    return ImgPyramidSettings.scaled(w, h, 1, canny_threshold1=60, canny_threshold2=20)


@functools.lru_cache(maxsize=None)
def noise_frame(size):
    """(bgr, full depth) of the size's noise image: the keyframe of every single-level case.  Do not modify."""
    w, h = SIZES[size]
    bgr, _ = fl.noise_image(w, h)
    return bgr, np.full((h, w), DEPTH, np.float32)


@functools.lru_cache(maxsize=None)
def supply(size):
    """(ys, xs) of the noise image's edge pixels at least MARGIN pixels inside the border, row-major (from the oracle)."""
    from oracle import ro
    from revo_amd.settings import PLANE_EDGES
    w, h = SIZES[size]
    e = ro.Pyramid(settings_of(size), *noise_frame(size)).read(PLANE_EDGES, 0) > 0
    e[:MARGIN] = e[h - MARGIN:] = False
    e[:, :MARGIN] = e[:, w - MARGIN:] = False
    ys, xs = np.nonzero(e)
    return ys, xs


def masked_depth(size, N):
    """Depth DEPTH at the first N pixels of the supply, 0 elsewhere."""
    w, h = SIZES[size]
    ys, xs = supply(size)
    assert N <= len(ys), (size, N, len(ys))
    d = np.zeros((h, w), np.float32)
    d[ys[:N], xs[:N]] = DEPTH
    return d


SPECIAL_DEPTH = 0.15  # the decider's one near point: shift_prior moves it by 4 pixels, the others by 0.4


@functools.lru_cache(maxsize=None)
def decider_supply(size):
    """For the init check (TrackerNew::evalCostFunction reads the keyframe's DT at the FLOOR of a projection): the pixels of the
    supply whose point at depth DEPTH costs 0 at the identity and 0 under shift_prior (`ties`, row-major), and the last pixel of
    the supply's last row whose point at depth SPECIAL_DEPTH costs 0 at the identity and more than 0 under shift_prior.
    -> (ys, xs of the ties, (y, x) of the special pixel)"""
    from oracle import ro
    from revo_amd.settings import PLANE_DT, PLANE_EDGES3D
    import exact_sums_ref as xr
    w, h = SIZES[size]
    s = settings_of(size)
    bgr, full = noise_frame(size)
    ys, xs = supply(size)
    order = np.lexsort((ys, xs))  # the oracle lists a level's points column by column
    ref = ro.Pyramid(s, bgr, full)
    ref.makeKeyframe()
    dt = ref.read(PLANE_DT, 0)
    cam = (s.fx, s.fy, s.cx, s.cy, w, h)
    cost = {}
    for z in (DEPTH, SPECIAL_DEPTH):
        d = np.zeros((h, w), np.float32)
        d[ys, xs] = z
        pts = ro.Pyramid(s, bgr, d).read(PLANE_EDGES3D, 0)
        assert len(pts) == len(ys)
        for name, (R, T) in (("eye", IDENTITY), ("init", shift_prior(size))):
            c = np.zeros(len(ys), np.float32)
            c[order] = xr.cost_terms(dt, pts, cam, R, T, 1e9, 0)
            cost[(z, name)] = c
    tie = (cost[(DEPTH, "eye")] == 0) & (cost[(DEPTH, "init")] == 0)
    cand = np.flatnonzero((ys == ys[-1]) & (cost[(SPECIAL_DEPTH, "eye")] == 0) & (cost[(SPECIAL_DEPTH, "init")] > 0))
    assert len(cand), size
    return ys[tie], xs[tie], (int(ys[cand[-1]]), int(xs[cand[-1]]))


def decider_depth(size, N):
    """N - 1 ties at depth DEPTH from the top of the image and the special pixel in its last row: the special point is the last of
    the tile-ordered list (the one point a level of N = P * stride + 1 streams) and alone makes the identity cheaper than the prior."""
    w, h = SIZES[size]
    ys, xs, (sy, sx) = decider_supply(size)
    assert N - 1 <= len(ys) and ys[N - 2] < (sy // 32) * 32, (size, N)  # the others end above the special pixel's row of tiles
    d = np.zeros((h, w), np.float32)
    d[ys[:N - 1], xs[:N - 1]] = DEPTH
    d[sy, sx] = SPECIAL_DEPTH
    return d


def prior_of(size):
    """A fixed prior of a fraction of a pixel: about 0.4 pixel of translation at depth DEPTH and 0.3 mrad about every axis."""
    s = settings_of(size)
    t = 0.4 * DEPTH / s.fx
    M = synth.se3_exp(np.array([t, -0.7 * t, 0.5 * t, 3e-4, -3e-4, 3e-4]))
    return M[:3, :3].astype(np.float32), M[:3, 3].astype(np.float32)


def shift_prior(size):
    """The prior of the `decider` cases: no rotation, +0.4 pixel in x and y at depth DEPTH (so every point of that depth keeps
    the pixel it came from under TrackerNew::evalCostFunction's floor), more for a nearer point."""
    s = settings_of(size)
    return np.eye(3, dtype=np.float32), np.array([0.4 * DEPTH / s.fx, 0.4 * DEPTH / s.fy, 0.0], np.float32)


IDENTITY = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))


def poses_of(case):
    return [IDENTITY, prior_of(case["size"])]


# masks of the three-level pair (synth.make_pair(3, S320)): name -> depth of the current frame from (its depth, its level edges)
def _every(k):
    def f(depth, edges):
        d = np.zeros_like(depth)
        d[::k, ::k] = depth[::k, ::k]
        return d
    return f


def _without_level(l, below_row=0):
    """No depth in the 2^l x 2^l source block of every level-l edge pixel at or below level-l row `below_row`."""
    def f(depth, edges):
        d = depth.copy()
        k = 1 << l
        el = edges[l] > 0
        el[:below_row] = False
        d[np.kron(el, np.ones((k, k), bool))] = 0.0
        return d
    return f


PYR_MASKS = {"all": lambda depth, edges: depth.copy(), "every 2nd": _every(2), "every 4th": _every(4),
             "no level 0": _without_level(0), "no level 1": _without_level(1),
             "few level 1": _without_level(1, 24)}


@functools.lru_cache(maxsize=None)
def pyr_pair():
    """The three-level pair at 320 x 240 and the level edges of its current frame (oracle).  Do not modify."""
    from oracle import ro
    from revo_amd.settings import PLANE_EDGES
    p = synth.make_pair(3, lc.S320)
    o = ro.Pyramid(lc.S320, *p["curr"])
    return p, tuple(o.read(PLANE_EDGES, l) for l in range(3))


def frames_of(case):
    """((bgr, depth) of the keyframe, (bgr, depth) of the current frame)"""
    if case["size"] == "pyr":
        p, edges = pyr_pair()
        return p["ref"], (p["curr"][0], PYR_MASKS[case["mask"]](p["curr"][1], edges))
    bgr, full = noise_frame(case["size"])
    return (bgr, full), (bgr, decider_depth(case["size"], case["N"]) if case["special"] else masked_depth(case["size"], case["N"]))


# ---- the cases ----------------------------------------------------------------------------------------------------------------

CASES = {}


def _case(size, N, rows, claims=(), why="", special=False):
    """claims: (C, r, facts) -- what split_facts(N, C, r) must say for this case to be on the side of the limit it is here for;
    every (C, r) named is one of the GPU test's partitions."""
    name = "%s N=%d%s" % ("x".join(map(str, SIZES[size])), N, " decider" if special else "")
    assert name not in CASES, name
    CASES[name] = dict(size=size, N=N, rows=tuple(rows), claims=tuple(claims), why=why, special=special, levels=(N,))


def _pyr(mask, r, C, levels, order, rows, why):
    name = "pyr %s r=%d" % (mask, r)
    assert name not in CASES, name
    CASES[name] = dict(size="pyr", mask=mask, N=None, rows=tuple(rows), levels=tuple(levels), r=r, C=C, order=order, why=why,
                       claims=(), special=False)


RED, EXC = dict(redundant=True), dict(redundant=False)
# row 1
_case("160", 0, (1, 6, 10), [(32, 0, dict(RED, most=0)), (1, 0, dict(most=0))], "no point at all: redundant even at r = 0, every sum empty")
_case("160", 1, (1, 5, 6, 10), [(32, 0, dict(EXC, idle=31)), (16, 0, dict(EXC, idle=15)), (2, 0, dict(EXC, idle=1)), (1, 0, dict(most=1))],
      "one point: exchanged at r = 0 with every member but one idle (31 of 32); G - 1 idle groups of k_pair_info")
# row 2
_case("160", 63, (2,), [(1, 0, dict(most=1))], "one lane short of a wave")
_case("160", 64, (2,), [(1, 0, dict(most=1))], "one full wave")
_case("160", 65, (2,), [(1, 0, dict(most=1))], "the first lane of the second wave")
# row 3
_case("160", 511, (3,), [(1, 0, dict(most=1)), (2, 0, dict(EXC, idle=1))], "one thread short of a workgroup: member 1 idle")
_case("160", 512, (3,), [(1, 0, dict(most=1)), (2, 0, dict(EXC, idle=1, member1=0))], "one point per thread, member 1 still idle")
_case("160", 513, (3, 5), [(1, 0, dict(most=2)), (2, 0, dict(EXC, idle=0, member1=1)), (16, 0, dict(EXC, idle=14)), (16, R_ONE, RED)],
      "thread 0's second register point when redundant, member 1's first point when exchanged; 14 of 16 members idle")
# row 4, redundant / C = 1 (and row 6 at the single pair's shipped threshold, where r = P T: the two rows coincide)
_case("160", 1024, (4, 6), [(1, 0, dict(most=2, streamed=0)), (4, R_ONE, dict(RED, streamed=0)), (32, R_ONE, RED), (2, 0, dict(EXC, streamed=0))],
      "the last register point (P T) and N = r at REVO_TRACK_REDUNDANT_ONE = 1024 = P T: rows 4 and 6 coincide for the single pair")
_case("160", 1025, (4, 6), [(1, 0, dict(most=3, streamed=1)), (4, R_ONE, dict(EXC, streamed=0)), (32, R_ONE, dict(EXC, idle=29))],
      "the first streamed point (P T + 1) and N = r + 1 at REVO_TRACK_REDUNDANT_ONE: sibling row of 160x120 N=1024")
_case("160", 2660, (4,), [(1, 0, dict(rounds=4, last_round=100)), (1, R_ONE, dict(rounds=4))], "four streamed rounds, the last with 100 points, in one workgroup")
# row 4, exchanged
_case("160", 2048, (4,), [(2, 0, dict(EXC, streamed=0, most=2)), (2, R_ONE, dict(EXC, streamed=0))], "P C T at C = 2: the last register point of the last thread of member 1")
_case("160", 2049, (4,), [(2, 0, dict(EXC, streamed=1, most=3)), (2, R_ONE, dict(EXC, streamed=1))], "P C T + 1 at C = 2: one streamed point")
_case("320", 4096, (4,), [(4, 0, dict(EXC, streamed=0)), (4, R_ONE, dict(EXC, streamed=0))], "P C T at C = 4")
_case("320", 4097, (4,), [(4, 0, dict(EXC, streamed=1)), (4, R_ONE, dict(EXC, streamed=1))], "P C T + 1 at C = 4")
_case("320", 5500, (4,), [(2, 0, dict(EXC, rounds=4, last_round=380)), (4, 0, dict(EXC, rounds=1, last_round=1404)), (1, 0, dict(rounds=9))],
      "exchanged with four streamed rounds and a partial last one (C = 2); nine rounds in one workgroup")
_case("640", 8192, (4,), [(8, R_BATCH, dict(EXC, streamed=0)), (8, 0, dict(EXC, streamed=0))], "P C T at C = 8 (the batch partitions)")
_case("640", 8193, (4,), [(8, R_BATCH, dict(EXC, streamed=1)), (8, 0, dict(EXC, streamed=1))], "P C T + 1 at C = 8 (the batch partitions)")
_case("640t", 32768, (4,), [(32, 0, dict(EXC, streamed=0, idle=0)), (32, R_ONE, dict(EXC, streamed=0))], "P C T at the largest cluster, 32")
_case("640t", 32769, (4,), [(32, 0, dict(EXC, streamed=1, idle=0)), (32, R_ONE, dict(EXC, streamed=1))], "P C T + 1 at the largest cluster")
# row 6 at the batches' shipped threshold (r = 0: the cases of row 1)
_case("160", 400, (6,), [(4, R_BATCH, RED), (8, R_BATCH, RED), (4, 0, EXC)], "N = r at REVO_TRACK_REDUNDANT_BATCH = 400")
_case("160", 401, (6,), [(4, R_BATCH, EXC), (8, R_BATCH, dict(EXC, idle=7)), (4, R_ONE, RED)], "N = r + 1 at REVO_TRACK_REDUNDANT_BATCH")
# the MODE_COST loop: the one point that decides the init check is the one a wrong loop bound would lose (the last in tile order)
_case("160", 1025, (4,), [(1, 0, dict(streamed=1)), (2, R_ONE, dict(EXC, streamed=0))], "the init check decided by the one streamed point of one workgroup",
      special=True)
_case("160", 2049, (4,), [(2, 0, dict(EXC, streamed=1)), (2, R_ONE, dict(EXC, streamed=1))], "the init check decided by the one streamed point of a pair of workgroups",
      special=True)
_case("320", 4097, (4,), [(4, 0, dict(EXC, streamed=1)), (4, R_BATCH, dict(EXC, streamed=1))], "the init check decided by the one streamed point of four workgroups",
      special=True)
# row 10 (those of row 1 are above)
_case("640", 1023, (10,), why="k_pair_info: a chunk one point short")
_case("640", 1024, (10,), why="k_pair_info: one full chunk, 18 idle groups")
_case("640", 1025, (10,), why="k_pair_info: the first point of group 1")
_case("640", 19 * 1024, (10,), why="k_pair_info: G chunks, one per group (G = 19 at 640 x 240)")
_case("640", 19 * 1024 + 1, (10,), why="k_pair_info: the first chunk of group 0's second round")
_case("640", 30480, (10,), why="k_pair_info: the top of the image's supply, 30 chunks over 19 groups, the last one partial")

# rows 7 and 8: three levels at 320 x 240; (mask, r, C, points per level finest first, the order coarse to fine)
_pyr("all", 2200, 4, (7433, 2200, 692), "RRX", (7,), "the natural order; level 1 sits on N = r")
_pyr("every 4th", 462, 4, (462, 552, 642), "XXR", (7,), "coarse levels exchanged, the finest redundant and on N = r: the epoch rests at the end")
_pyr("every 2nd", 1829, 4, (1829, 2044, 691), "RXR", (7,), "an exchanged level between two redundant ones")
_pyr("few level 1", 396, 4, (5079, 396, 690), "XRX", (7,), "a redundant level with points between two exchanged ones: the epoch rests in the middle")
_pyr("no level 1", 0, 4, (4562, 0, 690), "XRX", (8,), "an empty level between two exchanged ones (empty: redundant even at r = 0)")
_pyr("no level 0", 2000, 4, (0, 2166, 692), "RXR", (8,), "an empty finest level behind an exchanged one")


def pyr_partitions(case):
    """The single-pair partitions of a three-level case: the base, then its own threshold under its cluster and under 16."""
    return [SINGLE[0], _one(case["C"], case["r"], 1), _one(case["C"], case["r"], 3), _one(16, case["r"], 2)]


def level_order(levels, C, r):
    """'R' / 'X' per level, coarse to fine"""
    return "".join("R" if redundant(n, C, r) else "X" for n in reversed(levels))


# row 9: the 13 pairs of the one batch (640 x 240), one and more of each of rows 1-6
BATCH13 = (0, 1, 64, 65, 400, 401, 512, 513, 1024, 1025, 2049, 8192, 8193)
BATCH4_N = (1, 513, 32768, 32769)  # the batch of four under C = 32 (640 x 288)


def batch_case(size, N):
    """A pair of a batch: the size's noise image with N points, as a case of its own (not in CASES)."""
    return dict(size=size, N=N, special=False, levels=(N,))


def cases_of(rows, decider=False):
    """names of the single-level cases of CASES that stand for one of `rows`"""
    return [n for n, c in CASES.items() if c["size"] != "pyr" and set(c["rows"]) & set(rows) and c["special"] == decider]


def pyr_cases():
    return [n for n, c in CASES.items() if c["size"] == "pyr"]


assert PAIR_INFO_CHUNK == INFO_CHUNK and PAIR_INFO_MAX_GROUPS == INFO_MAX_GROUPS and pair_info_groups(640 * 240) == info_groups(640 * 240)
