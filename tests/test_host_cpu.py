"""CPU-side tests of the host logic: the C-ABI library loads and exports every symbol the
header declares (no compute calls without a GPU), struct layouts match the header, the
product fails loudly without a device, and the N>1 path (shard + gather + max-time) works
with world_size 2 on gloo."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from revo_amd import _lib
    L = _lib.lib()
    syms = _lib.declared_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(L, s), "librevo_hip.so does not export %s" % s
    assert b"gfx950" in L.revo_version()
    # exactly the header: every defined dynamic symbol, of any type, is one of its functions
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    leaked = sorted(s for s in exported if s.startswith(("_Z", "__device_stub__", "__hip_cuid_")))
    assert not leaked, "librevo_hip.so exports internals: %s" % leaked[:10]
    assert exported == set(syms), ("exported but not declared: %s; declared but not exported: %s"
                                   % (sorted(exported - set(syms)), sorted(set(syms) - exported)))


def test_struct_layouts_and_defaults_match_the_header():
    from revo_amd import _lib
    from revo_amd.settings import ImgPyramidSettings, OptimizerSettings, TrackerSettings, PairResult, ResidualInfo
    L = _lib.lib()
    ps, os_, ts = ImgPyramidSettings(width=1, height=1), OptimizerSettings(), TrackerSettings(0, 0, 0, 0)
    L.revo_pyr_settings_default(C.byref(ps))
    ref = ImgPyramidSettings()
    for f, _ in ImgPyramidSettings._fields_:
        a, b = getattr(ps, f), getattr(ref, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), f
    z = OptimizerSettings()
    C.memset(C.byref(z), 0, C.sizeof(z))
    L.revo_opt_settings_default(C.byref(z))
    assert bytes(z) == bytes(os_)
    L.revo_tracker_settings_default(C.byref(ts))
    assert bytes(ts) == bytes(TrackerSettings())
    assert C.sizeof(PairResult) == 96 and C.sizeof(ResidualInfo) == 16
    assert ref.nLevels() == 3 and ref.level_size(2) == (160, 120)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from revo_amd import api
    from revo_amd.settings import ImgPyramidSettings
    with pytest.raises(api.RevoError) as e:
        api.CameraPyr(ImgPyramidSettings())
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "revo_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("# oracle", ""), "%s mentions the oracle" % f


WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as dist
from revo_amd import parallel
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
mine = parallel.shard_pairs(8, rank, world)
assert mine == list(range(rank * 4, rank * 4 + 4))
rec = np.zeros((4, 24), np.float32)
for i, p in enumerate(mine):
    rec[i, :9] = np.eye(3).T.reshape(9) * (p + 1)
    rec[i, 9:12] = [p, 2 * p, 3 * p]
    rec[i, 12] = 0.5 * p
local = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())
allrec = parallel.gather_records(local, world)
pre = torch.zeros(world * local.numel(), dtype=torch.uint8)
assert parallel.gather_records(local, world, out=pre) is pre and torch.equal(pre, allrec)
assert allrec.numel() == world * 4 * 96
R, T, err = parallel.records_to_poses(allrec.numpy().tobytes(), 8)
for p in range(8):
    assert np.allclose(R[p], np.eye(3) * (p + 1)) and np.allclose(T[p], [p, 2 * p, 3 * p]) and err[p] == 0.5 * p
t = parallel.max_over_ranks(1.0 + rank, world)
assert t == float(world)
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_shard_and_gather_world2_gloo(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "worker.py"
    script.write_text(WORKER % ROOT)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=120)
        assert p.returncode == 0, out.decode()


def test_shard_validation():
    from revo_amd import parallel
    with pytest.raises(ValueError):
        parallel.shard_pairs(10, 0, 4)
    assert parallel.shard_pairs(256, 7, 8) == list(range(224, 256))


SPAWNED = r"""
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from revo_amd import parallel
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert int(os.environ["LOCAL_RANK"]) == rank and os.environ["MASTER_ADDR"] == "127.0.0.1"
dist.init_process_group("gloo", rank=rank, world_size=world)
local = torch.full((2 * 96,), rank + 1, dtype=torch.uint8)
allrec = parallel.gather_records(local, world)
assert allrec.numel() == world * 2 * 96 and int(allrec[-1]) == world
assert parallel.max_over_ranks(float(rank), world) == float(world - 1)
dist.destroy_process_group()
if rank == 0:
    print("spawned world", world, sys.argv[1:])
if len(sys.argv) > 1 and sys.argv[1] == "fail" and rank == 1:
    sys.exit(3)
"""


def test_spawn_ranks_is_what_bench_uses_for_gpus_n(tmp_path, capfd):
    """`python bench.py --gpus N` without a launcher starts N ranks through parallel.spawn_ranks."""
    from revo_amd import parallel
    script = tmp_path / "spawned.py"
    script.write_text(SPAWNED % ROOT)
    assert parallel.spawn_ranks(str(script), ["--x", "1"], 2, timeout=120) == [0, 0]
    assert "spawned world 2 ['--x', '1']" in capfd.readouterr().out
    codes = parallel.spawn_ranks(str(script), ["fail"], 2, timeout=120)
    assert codes[1] == 3  # a failing rank is reported, the job does not hang
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "parallel.spawn_ranks(" in src and '"WORLD_SIZE" not in os.environ and a.gpus > 1' in src


def test_world1_group_goes_through_the_backend():
    """With a live process group of size 1 the gather and the max-time are real collectives (gloo here, RCCL
    on the GPU box: tests/test_gpu_multi.py)."""
    script = r"""
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from unittest import mock
from revo_amd import parallel
dist.init_process_group("gloo", rank=0, world_size=1)
local = torch.arange(192, dtype=torch.int64).to(torch.uint8)
with mock.patch.object(dist, "all_gather_into_tensor", wraps=dist.all_gather_into_tensor) as ag, \
     mock.patch.object(dist, "all_reduce", wraps=dist.all_reduce) as ar:
    out = parallel.gather_records(local, 1)
    t = parallel.max_over_ranks(2.5, 1)
assert ag.call_count == 1 and ar.call_count == 1 and out is not local and torch.equal(out, local) and t == 2.5
dist.destroy_process_group()
assert parallel.gather_records(local, 1) is local  # no group: a single rank's records are their own gather
""" % ROOT
    from revo_amd import parallel
    env = parallel.rendezvous_env(0, 1)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()


def test_cpp_adapters_compile_against_reference_shaped_types():
    """tests/cpp/adapter_refshape.cpp static_asserts the reference's signatures (imgpyramidrgbd.h:45-117,
    tracker.h:69-80) on the adapters, against Eigen / cv shaped stand-ins; both hosts must compile."""
    for src in ("adapter_refshape.cpp", "adapter_track.cpp"):
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", os.path.join(ROOT, "tests", "cpp", src)],
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-3000:]


def _one_json_line(stdout):
    lines = [ln for ln in stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # stdout carries exactly one line, the record
    return json.loads(lines[0])


def _check_dry_run_line(rec, world, pairs, steps):
    assert rec["dry_run"] is True and rec["value"] is None  # never mistaken for a measurement
    assert rec["n_gpus"] == world and rec["steps"] == steps and rec["scaling"] == "weak"
    assert rec["config"]["global_pairs"] == world * pairs and rec["config"]["pairs_per_gpu"] == pairs
    assert rec["collective"]["ranks_seen"] == list(range(world)) and rec["collective"]["world_size"] == world
    # every rank's own step time travels in the line (a straggler GPU must be visible in the first real N > 1 run)
    assert len(rec["ms_per_step_per_rank"]) == world and max(rec["ms_per_step_per_rank"]) <= rec["ms_per_step"] * 1.0001
    every = rec["collective"]["steps_per_collective"]
    assert every == 2  # the records of two steps per collective at every world size (parallel.gather_every_default)
    assert rec["collective"]["bytes_per_rank"] == pairs * 96 * every
    # every step of the warm-up and of the timed loop was gathered and checked (record by record, rank order, step index)
    assert rec["collective"]["steps_gathered_and_checked"] == steps + rec["warmup"]


def test_bench_rank_plumbing_world2_self_spawned():
    """`python bench.py --gpus 2` (no launcher): spawn -> rendezvous on 127.0.0.1 -> static shard -> one 96-byte record per
    pair -> all_gather -> max-over-ranks -> ONE JSON line from rank 0, on gloo with a stubbed step: the
    first real 8-GPU run cannot fail on orchestration."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-cpu", "--steps", "3",
                        "--warmup", "1", "--pairs", "4"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    _check_dry_run_line(_one_json_line(r.stdout), 2, 4, 3)


def test_bench_rank_plumbing_world2_under_torchrun():
    """The driver's own launch line (python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...): RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the launcher."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-cpu",
                        "--steps", "2", "--warmup", "1", "--pairs", "3"], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    rec = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(rec) == 1  # rank 0 only
    _check_dry_run_line(rec[0], 2, 3, 2)


def test_gather_schedule_windows_cover_every_step_once():
    """parallel.gather_window / gather_tail: every step of a phase travels in exactly one collective, whatever the phase
    start and the window size."""
    from revo_amd import parallel
    for every in (1, 2, 3, 4):
        for start, end in ((0, 7), (5, 25), (3, 4), (6, 6)):
            seen = []
            for t in range(start, end):
                w = parallel.gather_window(t, every, start)
                if w:
                    assert w[1] == every and w[0] + every - 1 == t
                    seen += list(range(w[0], w[0] + w[1]))
            tail = parallel.gather_tail(end, every, start)
            if tail:
                assert 0 < tail[1] < every and tail[0] + tail[1] == end
                seen += list(range(tail[0], tail[0] + tail[1]))
            assert seen == list(range(start, end)), (every, start, end, seen)
    assert parallel.gather_every_default(1) == 2 and parallel.gather_every_default(8) == 2


def test_bench_world8_a_late_rank_does_not_serialise_the_others():
    """VERDICT r04 #12 / SURVEY 8(e): the step's only collective sits in the after-grid slot of a tracker stream, i.e. in front
    of that stream's NEXT grid two steps later -- it is never waited for by the host in the step loop.  World size 8 on gloo,
    a stubbed 30 ms step, rank 3 late in ONE step.  The dry run keeps a LOGICAL clock next to the wall clock (a step costs its
    nominal time, a collective completes at the maximum of the ranks' issue times, waiting moves the waiter's clock there), so
    the schedule property is asserted EXACTLY (the sleep-based inequality alone depended on the host):
      * a collective is first waited for two steps after it was issued, on every rank;
      * a delay shorter than that slack (24 ms < one 30 ms step) costs the other ranks nothing, the late rank its delay;
      * a delay longer than the slack (50 ms) costs the others exactly the excess (20 ms).
    The wall-clock loops are reported too and must not contradict it grossly."""
    steps, step_ms = 10, 30.0
    for delay_ms, others_extra in ((24.0, 0.0), (50.0, 20.0)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run-cpu", "--steps", str(steps),
                            "--warmup", "2", "--pairs", "2", "--dry-run-step-ms", str(step_ms), "--dry-run-delay-rank", "3",
                            "--dry-run-delay-ms", str(delay_ms)], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        rec = _one_json_line(r.stdout)
        _check_dry_run_line(rec, 8, 2, steps)
        assert rec["collective"]["steps_gathered_and_checked"] == steps + 2
        assert rec["min_steps_between_issue_and_first_wait_per_rank"] == [2] * 8
        logical = rec["logical_ms_loop_per_rank"]
        assert logical[3] == steps * step_ms + delay_ms, logical
        assert [x for i, x in enumerate(logical) if i != 3] == [steps * step_ms + others_extra] * 7, logical
        loops = rec["ms_loop_per_rank"]  # wall clock (sleep-based): only a sanity bound
        assert min(loops) >= steps * step_ms * 0.98 and loops[3] >= steps * step_ms + 0.9 * delay_ms, loops


def test_ab_bench_variant_specs():
    """profiles/ab_bench.py: NAME=SPEC[@bench args] -> (name, environment, extra arguments)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ab_bench", os.path.join(ROOT, "profiles", "ab_bench.py"))
    ab = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ab)
    assert ab.parse_variant("base=") == ("base", {}, [])
    name, env, extra = ab.parse_variant("d3=REVO_TRACK_DEPTH=3,profiles/build/x.so@--buffers 4 --gather-every 1")
    assert name == "d3" and env["REVO_TRACK_DEPTH"] == "3" and env["REVO_HIP_SO"].endswith("profiles/build/x.so")
    assert os.path.isabs(env["REVO_HIP_SO"]) and extra == ["--buffers", "4", "--gather-every", "1"]
    assert ab.parse_variant("b2=@--build-streams 2") == ("b2", {}, ["--build-streams", "2"])
