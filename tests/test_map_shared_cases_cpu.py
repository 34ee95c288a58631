"""The schedules of the map's shared-state tests (map_shared_cases.py) checked without a GPU: scripted() names every feature and
every mutation and keeps its three coverage rules, each computed from SHARES and FORMS; the random schedules are reproducible;
and every DevBuf, HostRows and EventTimer member of struct revo_map is entered in SHARES or NOT_SHARED, so that the next feature
added to the handle fails here until it is."""
import os

import map_shared_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "revo_amd", "csrc", "revo_map_impl.h")


def _adjacent(steps):
    """The ordered pairs of features that two consecutive steps call (a mutation between two calls parts them)."""
    return {(a[1], b[1]) for a, b in zip(steps, steps[1:]) if a[0] == b[0] == "call"}


def _missing_pairs(steps):
    return sorted(set(sc.sharing_pairs()) - _adjacent(steps))


def _calls(steps):
    return [s[1:] for s in steps if s[0] == "call"]


def test_the_tables_name_features():
    names = set(sc.FEATURES)
    assert all(callable(f) and f.__name__ == n for n, f in sc.FEATURES.items())
    for member, users in sc.SHARES.items():
        assert len(users) >= 2 and len(set(users)) == len(users) and set(users) <= names, member
    assert set(sc.FORMS) | set(sc.FORMS.values()) <= names and not set(sc.FORMS) & set(sc.FORMS.values())
    assert set(sc.NO_WAIT) <= set(sc.FORMS.values()) and all(hasattr(sc.FEATURES[n], "args") for n in sc.NO_WAIT)
    assert set(sc.AFTER_MUTATION) <= names and list(sc.MUTATIONS) == ["merge_grow", "subtract_part", "carve_view", "clear_merge"]
    assert all(reason for reason in sc.NOT_SHARED.values()) and not set(sc.NOT_SHARED) & set(sc.SHARES)
    for size in ("small", "large"):  # large is larger along every axis, in views and in pixels; no z length is a multiple of 32
        assert sc.BOX[size][1][2] % 32
    assert all(a < b for a, b in zip(sc.BOX["small"][1], sc.BOX["large"][1])) and sc.NV["small"] < sc.NV["large"]
    assert all(a < b for cam in (sc.MAP_CAM, sc.BOX_CAM) for a, b in zip(cam["small"][1], cam["large"][1]))


def test_scripted_names_every_feature_and_mutation():
    steps = sc.scripted()
    assert {s[1] for s in steps if s[0] == "call"} == set(sc.FEATURES)
    assert [s[1] for s in steps if s[0] == "mutate"] == list(sc.MUTATIONS)
    assert all(s[0] in ("call", "mutate") and (s[0] == "mutate" or s[2] in sc.SIZES) for s in steps)


def test_scripted_takes_every_sharing_pair_in_both_orders():
    pairs = sc.sharing_pairs()
    assert pairs and all((b, a) in pairs for a, b in pairs)
    assert ("raycast", "view_gain") in pairs and ("known_field", "observe") in pairs and ("plan_paths", "plan") in pairs
    assert ("mesh", "surface_raycast") in pairs and ("frontiers", "distance_field") in pairs
    assert _missing_pairs(sc.scripted()) == []
    # the check bites: a schedule without one of its calls misses pairs
    steps = list(sc.scripted())
    first = next(i for i, s in enumerate(steps) if s[0] == "call" and s[1] == "view_gain")
    assert _missing_pairs([s for s in steps if s[:2] != ("call", "view_gain")]) and _missing_pairs(steps[:first])


def test_scripted_runs_every_feature_large_small_large():
    calls = _calls(sc.scripted())
    triples = set(zip(calls, calls[1:], calls[2:]))
    for name in sc.FEATURES:
        assert ((name, "large"), (name, "small"), (name, "large")) in triples, name


def test_scripted_follows_each_form_by_the_other():
    adjacent = _adjacent(sc.scripted())
    for host, device in sc.FORMS.items():
        assert (host, device) in adjacent and (device, host) in adjacent, host


def test_scripted_follows_every_mutation_by_the_readers_of_the_table():
    steps = sc.scripted()
    for name in sc.MUTATIONS:
        i = steps.index(("mutate", name))
        assert [s[:2] for s in steps[i + 1:i + 1 + len(sc.AFTER_MUTATION)]] == [("call", f) for f in sc.AFTER_MUTATION], name


def test_random_schedules_are_reproducible_and_leave_nothing_out():
    seen = {s[1] for s in sc.scripted() if s[0] == "call"}
    for seed in sc.RANDOM_SEEDS:
        a = sc.random_schedule(seed, sc.RANDOM_LENGTH)
        assert a == sc.random_schedule(seed, sc.RANDOM_LENGTH) and len(a) == sc.RANDOM_LENGTH
        assert all((s[0] == "call" and s[1] in sc.FEATURES and s[2] in sc.SIZES) or (s[0] == "mutate" and s[1] in sc.MUTATIONS) for s in a)
        muts = [s[1] for s in a if s[0] == "mutate"]
        assert muts and muts == (list(sc.MUTATIONS) * 3)[:len(muts)]  # each valid after the one before
        seen |= {s[1] for s in a if s[0] == "call"}
    assert len({sc.random_schedule(seed, sc.RANDOM_LENGTH) for seed in sc.RANDOM_SEEDS}) == len(sc.RANDOM_SEEDS)
    assert seen == set(sc.FEATURES)


def test_every_member_of_the_handle_is_entered():
    text = open(HEADER).read()
    members = sc.handle_members(text)
    assert len(members) >= 37 and {"zbuf", "views", "ray_time", "tsdf_bgr", "tsdfray_views", "cov"} <= set(members)
    missing = [m for m in members if m not in sc.SHARES and m not in sc.NOT_SHARED]
    assert not missing, "members of struct revo_map without an entry in map_shared_cases.SHARES / NOT_SHARED: %s" % missing
    stale = [m for m in sc.NOT_SHARED if m not in members]
    assert not stale, "NOT_SHARED names what struct revo_map no longer has: %s" % stale
    # the check bites: a member added to the struct is found
    grown = text.replace("  DevBuf tsdfraywork, tsdfrayout;", "  DevBuf tsdfraywork, tsdfrayout, newscratch;\n  EventTimer new_time;")
    assert grown != text and [m for m in sc.handle_members(grown) if m not in sc.SHARES and m not in sc.NOT_SHARED] == ["newscratch", "new_time"]


def test_the_inputs_have_something_to_show():
    import numpy as np
    from revo_amd import mapfile
    rec = sc.base_records()
    assert 2 * (len(rec) + len(sc.grid_records())) > 1024 >= 2 * len(rec)  # the first merge_grow is a rehash of the 1 024-slot table
    for size in sc.SIZES:
        lo, n = sc.BOX[size]
        ax = mapfile.key_axes(rec["key"])
        assert np.all((ax >= lo) & (ax < np.add(lo, n)), 1).sum() >= 20
        cells, col = sc.tsdf_volume(size)
        assert (cells["weight"] > 0).any() and (cells["sum"] < 0).any() and (cells["sum"] > 0).any() and (col["weight"] > 0).any()
        assert len(mapfile.mesh_records(cells, lo, sc.VOXEL).triangles) > 0
        assert sc.seen_volume(size).any() and (sc.cost_field(size) != mapfile.PLAN_NONE).any()
        assert len(mapfile.frontier_records(rec, lo, n, sc.seen_volume(size))) > 0
