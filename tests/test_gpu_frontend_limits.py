"""The pyramid build at every limit of the geometry build_geom accepts (tests/frontend_limit_cases.py: the table, the cases and
what each one witnesses; tests/test_frontend_limits_cpu.py: the proof, from the oracle, that each case lands where the table
says).  Here every case runs on the GPU and every plane of its pyramid -- gray, depth, both edge maps, histogram, both edge
lists, distance transform, gradient table -- equals the oracle's bit for bit; the small cases run again as the frames of one
batch; the refused geometries are refused with the rule's own words.  There is no tolerance anywhere in this file.

Findings: one case failed and was fixed in the kernels -- 640 x 140 with a histogram patch of 70 pixels: a tile that spans four
bitmap words was counted over three (k_hyst's and k_hyst_out's histogram loops; hist_wide_tile now).  No geometry had to be
refused, and the batch handle accepts every geometry the context accepts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from revo_amd.settings import ImgPyramidSettings  # noqa: E402

import frontend_limit_cases as fl  # noqa: E402
from test_gpu_parity import assert_same, compare_pyramid  # noqa: E402

INVALID_ARG = -1


@pytest.fixture(scope="module")
def api():
    from revo_amd import api as A
    return A


@pytest.fixture(scope="module")
def ro():
    from oracle import ro as R
    return R


def _tag(prefix, name):
    return prefix + "_" + name.replace(" ", "_")


@pytest.mark.parametrize("name", list(fl.CASES))
def test_case_bit_exact(api, ro, monkeypatch, name):
    c = fl.CASES[name]
    for k, v in c["env"].items():  # read when the context is created (build_geom)
        monkeypatch.setenv(k, v)
    s = fl.settings_of(c)
    bgr, depth = fl.image_of(c)
    cam = api.CameraPyr(s)
    gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
    op = ro.Pyramid(s, bgr, depth)
    gp.makeKeyframe()
    op.makeKeyframe()
    compare_pyramid(_tag("limit", name), gp, op, s, True)
    assert gp.return3DEdges(0).shape[0] > 0
    if set(c["rows"]) & {6, 7}:
        top = c["levels"] - 1
        for dense in (False, True):
            assert_same(_tag("limit_pcl%d" % dense, name), gp.generateColoredPcl(top, dense), op.generateColoredPcl(top, dense))


@pytest.mark.parametrize("name", fl.BATCH_CASES)
def test_case_as_batch_frames(api, ro, name):
    """Four frames through one batch of two pairs: the case's image, the flat image, the image flipped left-right, the image
    again.  Frame f of the batch starts f * npix into every plane: at 16 pixels per level that is 16 bytes of gray, 2 bytes of
    validity bits, one 16-byte quad of the EDT's rows."""
    import torch
    c = fl.CASES[name]
    s = fl.settings_of(c)
    bgr, depth = fl.image_of(c)
    frames = [(bgr, depth), fl.flat_image(c["w"], c["h"]),
              (np.ascontiguousarray(bgr[:, ::-1]), np.ascontiguousarray(depth[:, ::-1])), (bgr, depth)]
    cam = api.CameraPyr(s)
    bt = api.BatchTracker(cam, 2)  # (refusing a geometry the context accepted would raise here, with INVALID_ARG and a reason)
    d_bgr = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    d_dep = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    bt.build(d_bgr.data_ptr(), d_dep.data_ptr())
    bt.sync()
    for f, (b, d) in enumerate(frames):
        compare_pyramid(_tag("limit_batch%d" % f, name), bt.frame(f, s), ro.Pyramid(s, b, d), s, False)


def test_refused_geometries(api, ro):
    for what, (geom, rule) in fl.REFUSED.items():
        with pytest.raises(api.RevoError) as e:
            api.CameraPyr(fl.refused_settings(geom))
        assert e.value.code == INVALID_ARG, (what, e.value)
        assert rule in str(e.value), (what, str(e.value))
    # ... and a refusal leaves nothing behind: the next context builds what the oracle builds
    from revo_amd import synth
    s = ImgPyramidSettings.scaled(160, 120, 3, hist_patch=(5, 0, 0, 0, 0, 0))
    bgr, depth = synth.make_pair(1, s)["ref"]
    cam = api.CameraPyr(s)
    gp = api.ImgPyramidRGBD(s, cam, bgr, depth)
    op = ro.Pyramid(s, bgr, depth)
    gp.makeKeyframe()
    op.makeKeyframe()
    compare_pyramid("limit_after_refusals", gp, op, s, True)
