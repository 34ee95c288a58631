"""k_edt_rows searches four pixels per lane from aligned 16-byte LDS windows (revo_amd/csrc/revo_edt_px.h).  Here: the GPU's DT
plane of every level against the oracle's exact EDT of the GPU's own edge plane, bit for bit.

Geometries: 160 x 120 with 2 levels (the 80-wide level has 20 groups per row, a wave spans several rows, the last block of both
levels has fewer rows than the others); 36 x 16, one level (the smallest accepted width that is 4 mod 8: a row is no whole
number of half-waves); 640 x 480 with 4 levels (the shipped workgroup shape: one group per lane at every level).
Images: flat (no edge: every pixel is the no-edge value), a small bright square in the top-left and in the bottom-right corner
(the far pixels search almost the whole width), vertical bars at the columns 0, 3, 4 and w-1 (quad borders), one synthetic frame.
And one two-pair step through the pipeline handle (the EDT deferred to the auxiliary stream) against the same step through a
batch alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd import synth  # noqa: E402
from revo_amd.settings import ImgPyramidSettings, TrackerSettings  # noqa: E402

GEOMETRIES = [(160, 120, 2), (36, 16, 1), (640, 480, 4)]
NO_EDGE = np.sqrt(np.float32(1e15))


@pytest.fixture(scope="module")
def api():
    from revo_amd import api as A
    return A


@pytest.fixture(scope="module")
def ro():
    from oracle import ro as R
    return R


def _images(w, h, s):
    """(name, bgr, depth, must_have_edges)"""
    depth = np.full((h, w), 1.5, np.float32)
    gray3 = lambda g: np.repeat(g[..., None], 3, 2)
    k = max(3, min(w, h) // 5)  # side of the bright square
    flat = np.full((h, w), 60, np.uint8)
    tl, br, bars = flat.copy(), flat.copy(), flat.copy()
    tl[1:1 + k, 1:1 + k] = 255
    br[h - 1 - k:h - 1, w - 1 - k:w - 1] = 255
    for c in (0, 3, 4, w - 1):
        bars[:, c] = 255
    pair = synth.make_pair(11, s)
    return [("flat", gray3(flat), depth, False), ("square top-left", gray3(tl), depth, True),
            ("square bottom-right", gray3(br), depth, True), ("bars", gray3(bars), depth, True),
            ("synthetic frame", pair["ref"][0], pair["ref"][1], w >= 160)]


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["%dx%dx%d" % g for g in GEOMETRIES])
def test_dt_planes_equal_the_exact_edt_of_the_gpus_edges(api, ro, geom):
    w, h, levels = geom
    s = ImgPyramidSettings.scaled(w, h, levels, hist_patch=(10, 5, 0, 0, 0, 0) if w >= 160 else (0, 0, 0, 0, 0, 0),
                                  use_edge_hist=1 if w >= 160 else 0)
    cam = api.CameraPyr(s)
    for name, bgr, depth, must_have_edges in _images(w, h, s):
        gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
        gp.makeKeyframe()
        for lvl in range(levels):
            edges = gp.returnEdges(lvl)
            assert edges.shape == (h >> lvl, w >> lvl)
            got = gp.returnDistTransform(lvl)
            want = ro.edt(edges)
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s %dx%d level %d: %d pixels differ" % (
                name, w, h, lvl, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            if name == "flat":
                assert not edges.any() and (got == NO_EDGE).all()
            elif must_have_edges and lvl == 0:
                assert edges.any() and got.min() == 0.0 and got.max() < NO_EDGE
                if name.startswith("square"):
                    assert got.max() > 0.5 * (w >> lvl)  # a pixel that searched more than half the row


def test_pipelined_step_equals_the_batch_alone(api):
    """The keyframes' EDT of a pipelined step runs deferred, on the auxiliary stream: same records as the batch alone."""
    import torch
    dev = torch.device("cuda", 0)
    s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
    cam = api.CameraPyr(s)
    api.TrackerNew(TrackerSettings(), s, cam)
    n = 2
    pairs = [synth.make_pair(300 + i, s) for i in range(n)]
    bgr = torch.from_numpy(np.stack([p[k][0] for p in pairs for k in ("ref", "curr")])).to(dev)
    dep = torch.from_numpy(np.stack([p[k][1] for p in pairs for k in ("ref", "curr")])).to(dev)
    bt = api.BatchTracker(cam, n)
    res = torch.zeros(n * 96, dtype=torch.uint8, device=dev)
    bt.track(bgr.data_ptr(), dep.data_ptr(), res.data_ptr())
    bt.sync()
    want = res.cpu().numpy().tobytes()
    assert all(r["flags"] & (2 | 4 | 8) == 0 for r in api.results_from_buffer(want, n))
    pipe = api.Pipeline(cam, n)
    out = torch.zeros(n * 96, dtype=torch.uint8, device=dev)
    ticket, _ = pipe.submit(bgr.data_ptr(), dep.data_ptr(), out.data_ptr())
    pipe.wait(ticket)
    pipe.drain()
    assert out.cpu().numpy().tobytes() == want
    pipe.close()
