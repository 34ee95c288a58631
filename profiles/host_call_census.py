"""A fixed small workload over the host core's four paths, for counting HIP API calls per library build:

    rocprofv3 --hip-trace --stats -- python profiles/host_call_census.py        (REVO_HIP_SO picks the library)

160x120, 3 levels: 8 sequential frames through vo.REVO, 2 pipelined steps of a 2-pair batch (api.Pipeline), one host-buffer
job of 2 pairs, 4 steps of a 2-stream vo.MultiREVO.  Every per-frame and per-step call of the library (launches, asynchronous
copies, event records, stream waits, event and stream synchronisations) is issued a fixed number of times by this script, so
two builds that sequence their work the same way give the same counts (profiles/host_refactor_calls.txt)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from revo_amd import api, synth, vo
    from revo_amd.settings import ImgPyramidSettings
    s = ImgPyramidSettings.scaled(160, 120, 3, hist_patch=(5, 0, 0, 0, 0, 0))
    seq = synth.make_sequence(5, s, 8, max_t=0.01, max_rot_deg=0.4)
    pairs = [synth.make_pair(40 + i, s) for i in range(2)]

    g = vo.REVO(s)
    for f in seq:
        g.push(f[0], f[1], f[2])
    del g

    cam = api.CameraPyr(s)
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).cuda()
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")]).astype(np.float32)).cuda()
    rec = torch.zeros(2 * 96, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pipe = api.Pipeline(cam, 2)
    for _ in range(2):
        ticket, _stream = pipe.submit(bgr.data_ptr(), dep.data_ptr(), rec.data_ptr())
        pipe.wait(ticket)
    pipe.drain()
    pipe.close()

    hb = api.HostBatchTracker(cam)
    hb.track([((p["ref"][0], p["ref"][1].astype(np.float32)), (p["curr"][0], p["curr"][1].astype(np.float32))) for p in pairs])

    m = vo.MultiREVO(s, 2, cameraPyr=cam)
    seq2 = synth.make_sequence(6, s, 4, max_t=0.01, max_rot_deg=0.4)
    for k in range(4):
        m.submit([(0, *seq[k][:3]), (1, *seq2[k][:3])])
        m.step()
    del m
    cam.close()
    print("census workload done")


if __name__ == "__main__":
    main()
