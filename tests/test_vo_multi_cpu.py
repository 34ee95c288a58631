"""revo_vo_multi without a GPU: the ctypes structs against the C header, and MultiREVO.run's scheduling (refill order,
per-sequence output order, build submitted ahead of the step) against a fake handle."""
import os
import subprocess

import ctypes as C
import numpy as np

from revo_amd import vo
from revo_amd.settings import StreamFrame, StreamResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_structs_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "revo_hip.h"\n'
                   '#define F(T, m) printf(#T "." #m " %zu\\n", offsetof(T, m));\n'
                   'int main(void) {\n'
                   '  printf("revo_stream_frame %zu\\nrevo_stream_result %zu\\n", sizeof(revo_stream_frame), sizeof(revo_stream_result));\n'
                   '  F(revo_stream_frame, stream) F(revo_stream_frame, bgr) F(revo_stream_frame, bgr_stride) F(revo_stream_frame, depth)\n'
                   '  F(revo_stream_frame, depth_stride) F(revo_stream_frame, timestamp)\n'
                   '  F(revo_stream_result, stream) F(revo_stream_result, new_keyframe) F(revo_stream_result, timestamp)\n'
                   '  F(revo_stream_result, pose)\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, check=True).stdout.decode().splitlines())
    assert int(got["revo_stream_frame"]) == C.sizeof(StreamFrame)
    assert int(got["revo_stream_result"]) == C.sizeof(StreamResult)
    for T, name in ((StreamFrame, "revo_stream_frame"), (StreamResult, "revo_stream_result")):
        for f, _ in T._fields_:
            assert int(got[name + "." + f]) == getattr(T, f).offset, (name, f)


class FakeMulti(vo.MultiREVO):
    """The handle's contract without a device: one frame per stream per submit, queue bound, one frame reported per stream
    per step; a frame whose index is in `defer` is reported one step late (a keyframe change) with new_keyframe set."""

    def __init__(self, n_streams, max_queue=2, defer=()):
        self.n_streams, self.max_queue = n_streams, max_queue
        self.q = [[] for _ in range(n_streams)]
        self.owed = [None] * n_streams
        self.defer = set(defer)
        self.log = []

    def submit(self, frames):
        seen = set()
        for s, bgr, depth, ts in frames:
            assert s not in seen and self.pending(s) < self.max_queue
            seen.add(s)
            self.q[s].append(ts)
        self.log.append(("submit", sorted(seen)))

    def pending(self, s):
        return len(self.q[s]) + (self.owed[s] is not None)

    def reset(self, s):
        assert self.pending(s) == 0
        self.log.append(("reset", s))

    def step(self):
        out = []
        for s in range(self.n_streams):
            if self.owed[s] is not None:
                ts, self.owed[s] = self.owed[s], None
                out.append((s, np.eye(4) * ts, True, ts))
            elif self.q[s]:
                ts = self.q[s].pop(0)
                if ts in self.defer:
                    self.owed[s] = ts
                    continue
                out.append((s, np.eye(4) * ts, False, ts))
        self.log.append(("step", [r[0] for r in out]))
        return out


def _seqs(lens):
    # frame j of sequence k has time stamp 1000 k + j (unique: it identifies the frame in the fake's records)
    return [[(None, None, 1000.0 * k + j) for j in range(n)] for k, n in enumerate(lens)]


def test_run_returns_every_sequence_in_frame_order_and_refills_freed_streams():
    lens = [3, 7, 0, 2, 5, 4]
    m = FakeMulti(2, defer={1002.0, 4001.0})
    res = m.run(_seqs(lens))
    assert len(res) == len(lens)
    for k, n in enumerate(lens):
        assert [ts for ts, _ in res[k].poses] == [1000.0 * k + j for j in range(n)]
        assert [kf for _, kf in res[k]] == [1000.0 * k + j in (1002.0, 4001.0) for j in range(n)]
    # sequence 0 (3 frames) ends first on stream 0, which is reset and takes sequence 2 (empty), then 3; stream 1 keeps 1
    resets = [e[1] for e in m.log if e[0] == "reset"]
    assert resets[0] == 0 and len(resets) == len(lens)
    # the first two submits come before the first step: step t+1's frames are built while step t runs
    assert [e[0] for e in m.log[:3]] == ["submit", "submit", "step"]


def test_run_tum_lines_are_the_sequential_format():
    m = FakeMulti(3)
    res = m.run(_seqs([2, 3]))
    lines = res[1].tum_lines()
    assert len(lines) == 3 and lines[0].split()[0] == "1000.000000" and lines[1].split()[0] == "1001.000000000"
    assert lines == vo.tum_lines(res[1].poses)


def test_run_tum_refuses_save_model_with_streams(capsys):
    from revo_amd import run_tum
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--streams", "2", "--save-model", "model"]) == 2
    assert "--save-model is not supported together with --streams" in capsys.readouterr().out
    assert run_tum.main(["settings.yaml", "dataset.yaml", "--streams", "0"]) == 2
