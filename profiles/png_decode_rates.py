"""GPU PNG decode rates (revo_png_*): images/s and input GB/s for batches of 64, 256 and 1024 640x480 files, RGB8 (noisy render,
sensor-like) and Gray16 depth, timed end to end (submit -> wait) and for the device part alone (events around the launch).
Usage: python profiles/png_decode_rates.py [--quick]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    import torch
    import pngcorpus as pc
    from revo_amd import png
    quick = "--quick" in sys.argv
    rng = np.random.default_rng(0)
    h, w = 480, 640
    kinds = {}
    rgb = [pc.write_png(pc.noisy_rgb(rng, h, w, 6.0), 2, filters=4, level=6) for _ in range(8)]
    kinds["rgb8_noisy"] = (rgb, png.BGR8, h * w * 3)
    rgbc = [pc.write_png(pc.noisy_rgb(rng, h, w, 0.0), 2, filters=4, level=6) for _ in range(8)]
    kinds["rgb8_clean"] = (rgbc, png.BGR8, h * w * 3)
    y, x = np.mgrid[0:h, 0:w]
    d16 = [pc.write_png(np.clip(5000 + 3000 * np.sin(x / 50.0 + k) + rng.normal(0, 8, (h, w)), 0, 65535).astype(np.uint16), 0,
                        bit_depth=16, filters=4, level=6) for k in range(8)]
    kinds["gray16"] = (d16, png.U16, h * w * 2)
    batches = (64,) if quick else (64, 256, 1024)
    dec = png.GpuPngDecoder(max(batches), max(batches) * max(len(f) for v in kinds.values() for f in v[0]) + (1 << 20),
                            png.raw_bytes(w, h, png.BGR8))
    s = torch.cuda.Stream()
    for name, (files, fmt, rawb) in kinds.items():
        ratio = np.mean([len(f) for f in files]) / (h * w * (3 if fmt == png.BGR8 else 2))
        print("%s: compressed/raw %.3f" % (name, ratio))
        for n in batches:
            fl = [files[i % len(files)] for i in range(n)]
            shape = (n, h, w, 3) if fmt == png.BGR8 else (n, h, w)
            out = torch.empty(shape, dtype=torch.uint8 if fmt == png.BGR8 else torch.uint16, device="cuda")
            outs = list(out.unbind(0))
            codes = dec.wait(dec.submit(fl, fmt, outs, s))  # warm-up
            assert (codes == 0).all(), codes
            reps = 2 if n >= 256 else 3
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t_e2e, t_dev = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                e0.record(s)
                t = dec.submit(fl, fmt, outs, s)
                e1.record(s)
                dec.wait(t)
                t_e2e.append(time.perf_counter() - t0)
                t_dev.append(e0.elapsed_time(e1) / 1e3)
            te, td = min(t_e2e), min(t_dev)
            nb = sum(len(f) for f in fl)
            print("  batch %5d: end-to-end %8.1f ms = %7.0f images/s %6.3f GB/s in | device %8.1f ms = %7.0f images/s"
                  % (n, te * 1e3, n / te, nb / te / 1e9, td * 1e3, n / td))


if __name__ == "__main__":
    main()
