"""PNG decoding on the GPU (revo_png_*, png.GpuPngDecoder): bit-exact against the writer's pixels over the corpus, in both
output formats and many sizes, mixed batches, bad files isolated from their neighbours, capacity; device frames into
vo.MultiREVO (submit_device == submit); run_tum --gpu-decode writes the same pose files as the CPU decoders."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngcorpus as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, CAPACITY, UNSUPPORTED, CORRUPT = 0, -1, -5, -7, -8


def _dec(n=64, comp=512 << 20, raw=1920 * 4 * 1081 + 1081):
    from revo_amd import png
    return png.GpuPngDecoder(n, comp, raw)


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def _cases(h, w, rng):
    """(png bytes, format, expected) for one size: every colour type, filters, levels, strategies and IDAT splits."""
    from revo_amd import png
    rgb = pc.noisy_rgb(rng, h, w)
    rgba = np.concatenate([rgb, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
    gray = rgb[..., 1].copy()
    ga = np.stack([gray, rgb[..., 0]], axis=2)
    d16 = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    d16[: h // 2] = 5000  # a smooth part too
    out = []
    k = 0
    for pix, ct in ((rgb, 2), (rgba, 6), (gray, 0), (ga, 4)):
        for filt in (0, 1, 2, 3, 4, "random"):
            level, strat = [(0, "default"), (1, "fixed"), (6, "filtered"), (9, "huffman"), (6, "rle"), (9, "default")][k % 6]
            split = [None, 1, 8192, "random"][k % 4] if h * w < 100000 or k % 4 != 1 else None
            data = pc.write_png(pix, ct, filters=filt, level=level, strategy=strat, split=split, seed=k)
            k += 1
            exp = pc.as_bgr8(pix)
            if ct in (2, 6):
                assert np.array_equal(_pil(data)[..., :3], pix[..., :3])
            out.append((data, png.BGR8, exp))
    for filt in (0, 1, 2, 3, 4, "random"):
        data = pc.write_png(d16, 0, bit_depth=16, filters=filt, level=[1, 6, 9][k % 3], seed=k)
        k += 1
        assert np.array_equal(_pil(data).astype(np.uint16), d16)
        out.append((data, png.U16, d16))
    out.append((pc.write_png(gray, 0, filters="random"), png.U16, gray.astype(np.uint16)))
    return out


def _run(dec, cases):
    import torch
    from revo_amd import png
    outs = []
    for data, fmt, exp in cases:
        outs.append(torch.full(exp.shape, 77, dtype=torch.uint8 if fmt == png.BGR8 else torch.uint16, device="cuda"))
    codes = dec.wait(dec.submit([c[0] for c in cases], [c[1] for c in cases], outs))
    return outs, codes


@pytest.mark.parametrize("hw", [(480, 640), (1, 1), (3, 17), (7, 33), (1080, 1920)])
def test_decode_is_bit_exact(hw):
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    cases = _cases(hw[0], hw[1], rng)
    dec = _dec()
    outs, codes = _run(dec, cases)
    for i, ((data, fmt, exp), o) in enumerate(zip(cases, outs)):
        assert codes[i] == OK, "case %d: %d" % (i, codes[i])
        assert np.array_equal(o.cpu().numpy(), exp), "case %d differs" % i


def test_mixed_batch_and_512_images():
    rng = np.random.default_rng(5)
    cases = []
    for hw in ((480, 640), (1, 1), (3, 17), (12, 30)):
        cases += _cases(hw[0], hw[1], rng)
    rng.shuffle(cases)
    dec = _dec(n=512, comp=256 << 20)
    outs, codes = _run(dec, cases)
    assert (codes == OK).all()
    for (data, fmt, exp), o in zip(cases, outs):
        assert np.array_equal(o.cpu().numpy(), exp)
    small = _cases(9, 21, rng)
    big = [small[i % len(small)] for i in range(512)]
    outs, codes = _run(dec, big)
    assert (codes == OK).all()
    for (data, fmt, exp), o in zip(big, outs):
        assert np.array_equal(o.cpu().numpy(), exp)


def test_bad_files_get_their_own_codes():
    from revo_amd import png
    rng = np.random.default_rng(9)
    good = _cases(16, 24, rng)
    rgb = pc.noisy_rgb(rng, 16, 24)
    raw = pc.filter_rows(rgb.reshape(16, 72), 3, [1] * 16)
    z = bytearray(pc.compress(raw, 6))
    z[-2] ^= 0x40  # Adler mismatch (CRCs still right: only the decode finds it)
    adler = pc.write_png(rgb, 2, zdata=bytes(z))
    z2 = pc.compress(raw[:-30], 6)  # too few rows: underrun
    short = pc.write_png(rgb, 2, zdata=z2)
    bad_filter = pc.write_png(rgb, 2, zdata=pc.compress(b"\x07" + raw[1:], 6))
    trunc = pc.write_png(rgb, 2, zdata=pc.compress(raw, 6)[:-40])
    pal = pc.write_png(rgb[..., 0], 3, palette=bytes(range(256)) * 3)
    crc = bytearray(pc.write_png(rgb, 2))
    crc[40] ^= 1
    bad = [(adler, png.BGR8, CORRUPT), (short, png.BGR8, CORRUPT), (bad_filter, png.BGR8, CORRUPT), (trunc, png.BGR8, CORRUPT),
           (pal, png.BGR8, UNSUPPORTED), (bytes(crc), png.BGR8, CORRUPT),
           (pc.write_png(rgb, 2), png.U16, UNSUPPORTED), (pc.write_png(rgb, 2, interlace=1), png.BGR8, UNSUPPORTED)]
    mixed, want = [], []
    for i, g in enumerate(good):
        mixed.append(g)
        want.append(OK)
        if i < len(bad):
            mixed.append((bad[i][0], bad[i][1], np.zeros((16, 24, 3) if bad[i][1] == png.BGR8 else (16, 24), np.uint8)))
            want.append(bad[i][2])
    outs, codes = _run(_dec(), mixed)
    assert codes.tolist() == want
    for (data, fmt, exp), o, c in zip(mixed, outs, codes):
        if c == OK:
            assert np.array_equal(o.cpu().numpy(), exp)
    # a size mismatch is that image's INVALID_ARG
    import torch
    d = _dec()
    o = torch.empty((16, 25, 3), dtype=torch.uint8, device="cuda")
    assert d.wait(d.submit([pc.write_png(rgb, 2)], png.BGR8, [o])).tolist() == [INVALID_ARG]


def test_capacity():
    import torch
    from revo_amd import _lib, png
    d = _dec(n=4, comp=4096)
    pix = np.zeros((4, 4, 3), np.uint8)
    outs = [torch.empty((4, 4, 3), dtype=torch.uint8, device="cuda") for _ in range(5)]
    with pytest.raises(_lib.RevoError) as e:
        d.submit([pc.write_png(pix, 2)] * 5, png.BGR8, outs)
    assert e.value.code == CAPACITY
    noise = np.random.default_rng(1).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    big = [torch.empty((64, 64, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    with pytest.raises(_lib.RevoError) as e:
        d.submit([pc.write_png(noise, 2)] * 2, png.BGR8, big)
    assert e.value.code == CAPACITY
    assert d.wait(d.submit([pc.write_png(pix, 2)] * 4, png.BGR8, outs[:4])).tolist() == [OK] * 4


def test_synthetic_dataset_files_decode_like_load_frame(tmp_path):
    from revo_amd import png, synth, tum
    from revo_amd.settings import ImgPyramidSettings
    s = ImgPyramidSettings.scaled(320, 240, 3, hist_patch=(10, 5, 0, 0, 0, 0))
    tum.write_synthetic_dataset(str(tmp_path), synth.make_sequence(3, s, 4))
    rows = tum.read_associate(str(tmp_path / "associate.txt"))
    files, fmts, exp = [], [], []
    for rts, rf, dts, df in rows:
        bgr, depth = tum.load_frame(str(tmp_path), rf, df)
        files += [open(os.path.join(tmp_path, rf), "rb").read(), open(os.path.join(tmp_path, df), "rb").read()]
        fmts += [png.BGR8, png.U16]
        exp += [bgr, depth]
    outs, codes = _run(_dec(), list(zip(files, fmts, exp)))
    assert (codes == OK).all()
    for o, e in zip(outs, exp):
        assert np.array_equal(o.cpu().numpy(), e)


@pytest.mark.parametrize("u16", [False, True])
def test_submit_device_matches_submit(u16):
    import torch
    from revo_amd import vo
    from test_gpu_vo_multi import S320, _seq
    seqs = [_seq(seed, 10) for seed in (1, 2)]
    dsf = 5000.0 if u16 else None

    def frames(seq):
        out = []
        for bgr, depth, ts in seq:
            d = np.clip(np.rint(depth.astype(np.float64) * 5000), 0, 65535).astype(np.uint16) if u16 else depth
            out.append((bgr, d, ts))
        return out

    host = [frames(s) for s in seqs]
    dev = [[(torch.from_numpy(np.ascontiguousarray(b)).cuda(),
             (torch.from_numpy(d.view(np.int16)).cuda().view(torch.uint16) if u16 else torch.from_numpy(d).cuda()), ts)
            for b, d, ts in seq] for seq in host]
    runs = []
    for src, dev_path in ((host, False), (dev, True)):
        m = vo.MultiREVO(S320, 2, depth_scale_factor=dsf)
        res, kfs = [], []
        for t in range(len(src[0])):
            fr = [(s, src[s][t][0], src[s][t][1], src[s][t][2]) for s in range(2)]
            (m.submit_device if dev_path else m.submit)(fr)
            res += [(s, M, kf, ts) for s, M, kf, ts in m.step()]
        while any(m.pending(s) for s in range(2)):
            res += [(s, M, kf, ts) for s, M, kf, ts in m.step()]
        for s in range(2):
            pyr, T = m.keyframe(s)
            kfs.append(([pyr._read(k, 0) for k in range(5)] + [pyr.generateColoredPcl(0)], T, m.nKeyFrames(s)))
        runs.append((res, kfs))
    (ra, ka), (rb, kb) = runs
    assert len(ra) == 2 * len(seqs[0]) == len(rb)
    for (sa, Ma, kfa, tsa), (sb, Mb, kfb, tsb) in zip(ra, rb):
        assert (sa, kfa, tsa) == (sb, kfb, tsb) and np.array_equal(Ma, Mb)
    assert any(kf for _, _, kf, _ in ra)
    for (pa, Ta, na), (pb, Tb, nb) in zip(ka, kb):
        assert na == nb and np.array_equal(Ta, Tb)
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))


def test_submit_device_argument_checks():
    import torch
    from revo_amd import _lib, vo
    from test_gpu_vo_multi import S320
    m = vo.MultiREVO(S320, 2, depth_scale_factor=5000.0)
    bgr = torch.zeros((240, 320, 3), dtype=torch.uint8, device="cuda")
    dep = torch.zeros((240, 320), dtype=torch.uint16, device="cuda")
    with pytest.raises(_lib.RevoError):
        m.submit_device([(0, bgr, dep, 0.0), (0, bgr, dep, 1.0)])  # two frames for one stream
    with pytest.raises(_lib.RevoError):
        m.submit_device([(5, bgr, dep, 0.0)])                      # stream out of range
    h = torch.zeros((240, 320), dtype=torch.uint16).pin_memory()
    with pytest.raises(_lib.RevoError):
        m.submit_device([(0, bgr, h, 0.0)])                        # not device memory
    m.submit_device([(0, bgr, dep, 0.0)])
    m.submit_device([(0, bgr, dep, 1.0)])
    with pytest.raises(_lib.RevoError) as e:
        m.submit_device([(0, bgr, dep, 2.0)])                      # queue full (max_queue 2)
    assert e.value.code == CAPACITY


def test_run_tum_gpu_decode_writes_the_same_poses(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from revo_amd import run_tum, synth, tum
    from test_gpu_vo_multi import BIASES, S320, _tum_yaml
    names = ["rgbd_synth_a", "rgbd_synth_b", "rgbd_synth_c"]
    for k, (n, lens) in enumerate(zip(names, (14, 22, 9))):
        seq = synth.make_sequence(40 + k, S320, lens, max_t=0.01, max_rot_deg=0.4, bias=BIASES[k])
        tum.write_synthetic_dataset(str(tmp_path / "data" / n), seq)
    # one colour frame of one folder as a palette PNG, which the device decoder leaves to the CPU fallback
    rows = tum.read_associate(str(tmp_path / "data" / names[1] / "associate.txt"))
    f = str(tmp_path / "data" / names[1] / rows[3][1])
    Image.open(f).convert("P", palette=Image.ADAPTIVE).save(f)
    assert Image.open(f).mode == "P"
    _tum_yaml(tmp_path, S320, names)
    args = [str(tmp_path / "settings.yaml"), str(tmp_path / "dataset.yaml"), "--decoders", "2", "--streams", "2"]
    for sub, extra in (("cpu", []), ("gpu", ["--gpu-decode"])):
        (tmp_path / sub).mkdir()
        monkeypatch.chdir(tmp_path / sub)
        assert run_tum.main(args + extra) == 0
    txt = capsys.readouterr().out
    assert "decoded on the GPU, 1 frames on the CPU fallback" in txt
    assert "--decoders has no effect with --gpu-decode" in txt
    for n, lens in zip(names, (14, 22, 9)):
        a = (tmp_path / "cpu" / ("poses_%s.txt" % n)).read_bytes()
        b = (tmp_path / "gpu" / ("poses_%s.txt" % n)).read_bytes()
        assert a == b and len(a.splitlines()) == lens, n
