"""k_canny_nms4 decides every pixel by one comparison against the largest value its magnitude must exceed (threshold form,
revo_amd/csrc/revo_nms_px.h).  Here: the edge planes of all levels against the oracle's cv::Canny, bit for bit, at the smallest
shapes at which the kernel's indexing can go wrong, on images made of ties and of saturated magnitudes.

Shapes: 40 x 34, one level (a partial last bitmap word; a height that is no multiple of the 6 rows a thread walks);
32 x 6 (one word, one row group); 64 x 50 with two levels (the second level 32 x 25 comes out of pyrDown)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd.settings import ImgPyramidSettings, PLANE_EDGES, PLANE_GRAY  # noqa: E402

SHAPES = [(40, 34, 1), (32, 6, 1), (64, 50, 2)]
# canny_threshold1 / canny_threshold2: the shipped pair, equal, first above second and second above first
THRESHOLDS = [(150, 100), (60, 60), (100, 20), (20, 100)]


def _images(w, h):
    """(name, gray) -- B = G = R, so the gray plane is the image itself."""
    y, x = np.mgrid[0:h, 0:w]
    saw = lambda t: (((t // 3) % 5) * 50).astype(np.uint8)  # plateaus of 3 pixels, steps of 50, a drop of 200: ties along t
    rng = np.random.default_rng(20250)
    return [("constant", np.full((h, w), 128, np.uint8)),
            ("checker4", (((x // 4 + y // 4) % 2) * 255).astype(np.uint8)),   # |grad|^2 up to 2 * 1020^2 at the corners
            ("checker3", (((x // 3 + y // 3) % 2) * 255).astype(np.uint8)),   # cells that straddle the threads' 4 columns
            ("ramp_h", saw(x)), ("ramp_v", saw(y)), ("ramp_d1", saw(x + y)), ("ramp_d2", saw(x - y + h)),
            ("noise", rng.integers(0, 256, (h, w), dtype=np.uint8))]


@pytest.fixture(scope="module")
def api():
    from revo_amd import api as A
    return A


@pytest.fixture(scope="module")
def ro():
    from oracle import ro as R
    return R


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_edges_equal_the_oracles_canny(api, ro, shape):
    w, h, levels = shape
    depth = np.full((h, w), 1.5, np.float32)
    images = _images(w, h)
    edge_pixels = 0
    for thr in THRESHOLDS:
        # no edge histogram: fillInEdges leaves every level's edge plane as Canny made it
        s = ImgPyramidSettings.scaled(w, h, levels, canny_threshold1=thr[0], canny_threshold2=thr[1], use_edge_hist=0,
                                      hist_patch=(0, 0, 0, 0, 0, 0))
        cam = api.CameraPyr(s)
        for name, gray in images:
            gp = api.ImgPyramidRGBD(s, cam, np.repeat(gray[..., None], 3, 2), depth)
            assert np.array_equal(gp._read(PLANE_GRAY, 0), gray), (name, "gray plane is not the image")
            for lvl in range(levels):
                g = gp._read(PLANE_GRAY, lvl)
                assert g.shape == (h >> lvl, w >> lvl)
                want = ro.canny(g, thr[0], thr[1])
                got = gp._read(PLANE_EDGES, lvl)
                assert np.array_equal(got, want), "%s %dx%d level %d thresholds %s: %d pixels differ" % (
                    name, w, h, lvl, thr, int((got != want).sum()))
                edge_pixels += int((want > 0).sum())
                if name == "constant":
                    assert not want.any()
    assert edge_pixels > 0  # the comparison saw edges
