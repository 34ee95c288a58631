"""CPU tests of the PNG decoder's host half: revo_png_probe (chunk list, CRCs, IHDR, unsupported layouts) and the host build of
the inflate core the device kernel runs (revo_amd/csrc/revo_inflate.h), byte-exact against zlib and safe on bad input."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pngcorpus as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, CORRUPT = 0, -7, -8


def _probe(data):
    from revo_amd import png
    return png.probe(data)


def test_probe_reports_the_layout_across_split_idat():
    rng = np.random.default_rng(1)
    pix = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    for split in (None, 1, 8192, "random"):
        data = pc.write_png(pix, 2, filters="random", split=split)
        rc, info = _probe(data)
        z = pc.compress(pc.filter_rows(pix.reshape(13, 51), 3, [0] * 13))
        assert rc == OK
        assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace) == (17, 13, 8, 2, 0)
        assert info.raw_bytes == 13 * (1 + 51)
        assert info.idat_bytes > 0 and (split is not None or info.idat_bytes == len(z))
    d16 = pc.write_png(rng.integers(0, 65536, (5, 9), dtype=np.uint16), 0, bit_depth=16)
    rc, info = _probe(d16)
    assert rc == OK and (info.bit_depth, info.color_type, info.raw_bytes) == (16, 0, 5 * 19)


def test_probe_rejects_malformed_files():
    pix = np.zeros((4, 4, 3), np.uint8)
    good = pc.write_png(pix, 2)
    assert _probe(good)[0] == OK
    assert _probe(b"\x88" + good[1:])[0] == CORRUPT                       # signature
    bad = bytearray(good)
    bad[8 + 8 + 3] ^= 1                                                   # a byte of the IHDR data: CRC mismatch
    assert _probe(bytes(bad))[0] == CORRUPT
    no_ihdr = pc.SIG + pc.chunk(b"IDAT", zlib.compress(b"\x00" * 52)) + pc.chunk(b"IEND", b"")
    assert _probe(no_ihdr)[0] == CORRUPT
    assert _probe(good[:-12])[0] == CORRUPT                               # no IEND
    zero = pc.SIG + pc.chunk(b"IHDR", struct.pack(">IIBBBBB", 0, 4, 8, 2, 0, 0, 0)) + good[33:]
    assert _probe(zero)[0] == CORRUPT
    assert _probe(b"")[0] == CORRUPT
    assert _probe(good[:40])[0] == CORRUPT                                # truncated chunk


def test_probe_reports_adam7_and_palette_as_unsupported():
    pix = np.zeros((4, 4, 3), np.uint8)
    rc, info = _probe(pc.write_png(pix, 2, interlace=1))
    assert rc == UNSUPPORTED and info.interlace == 1
    pal = pc.write_png(np.zeros((4, 4), np.uint8), 3, palette=b"\x00\x00\x00\xff\xff\xff")
    rc, info = _probe(pal)
    assert rc == UNSUPPORTED and info.color_type == 3
    rgb16 = pc.write_png(np.zeros((4, 4, 3), np.uint16), 2, bit_depth=16)
    assert _probe(rgb16)[0] == UNSUPPORTED


def _harness(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "inflate_harness")
    src = os.path.join(ROOT, "tests", "cpp", "inflate_harness.cpp")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", exe]
    # a sanitizer build where the toolchain has one (host code only): any read or write out of range aborts the run
    if subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + base[1:],
                      capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return exe


def _inflate(exe, tmp_path, cases):
    rec, res = str(tmp_path / "rec.bin"), str(tmp_path / "res.bin")
    with open(rec, "wb") as f:
        for z, n in cases:
            f.write(struct.pack("<QQ", len(z), n))
            f.write(z)
    subprocess.run([exe, rec, res], check=True, timeout=300)
    d = open(res, "rb").read()
    out, i = [], 0
    for _, n in cases:
        st = struct.unpack_from("<i", d, i)[0]
        out.append((st, d[i + 4:i + 4 + n]))
        i += 4 + n
    assert i == len(d)
    return out


def _png_idat_cases():
    """The IDAT streams of PNG files of every filter, level and strategy."""
    rng = np.random.default_rng(3)
    pix = pc.noisy_rgb(rng, 24, 37)
    out = []
    for f in (0, 1, 2, 3, 4, "random"):
        for level in (0, 1, 6, 9):
            for strat in pc.STRATEGIES:
                rows = pc.filter_rows(pix.reshape(24, 37 * 3), 3, [f] * 24 if f != "random" else
                                      [int(x) for x in rng.integers(0, 5, 24)])
                out.append(("png_f%s_l%d_%s" % (f, level, strat), rows, pc.compress(rows, level, strat)))
    return out


def test_host_inflate_is_byte_exact_against_zlib(tmp_path):
    exe = _harness(tmp_path)
    cases = pc.zlib_corpus() + _png_idat_cases()
    names = [c[0] for c in cases]
    assert {"huffman_only_geometric", "dist_32768_len_258", "distance_1_runs", "empty_stored_blocks"} <= set(names)
    res = _inflate(exe, tmp_path, [(z, len(raw)) for _, raw, z in cases])
    for (name, raw, z), (st, out) in zip(cases, res):
        assert zlib.decompress(z) == raw
        assert st == 0, "%s: status %d" % (name, st)
        assert out == raw, name


def test_corpus_forces_long_codes_and_far_matches():
    # the Huffman-only stream of geometric bytes uses 15-bit codes: a code of length L means a symbol of probability ~2^-L
    geo = [c for c in pc.zlib_corpus() if c[0] == "huffman_only_geometric"][0][1]
    counts = np.bincount(np.frombuffer(geo, np.uint8), minlength=256)
    rare = counts[counts > 0].min() / counts.sum()
    assert rare < 2.0 ** -15
    name, raw, z = [c for c in pc.zlib_corpus() if c[0] == "dist_32768_len_258"][0]
    assert zlib.decompress(z) == raw and len(raw) == 32768 + 258 * 40


def test_host_inflate_rejects_bad_streams(tmp_path):
    exe = _harness(tmp_path)
    bad = pc.bad_streams()
    res = _inflate(exe, tmp_path, [(z, n) for _, z, n in bad])
    for (name, z, n), (st, _) in zip(bad, res):
        assert st != 0, name
    codes = {name: st for (name, _, _), (st, _) in zip(bad, res)}
    assert codes["distance_before_start"] == 7   # rinf::E_DIST
    assert codes["adler_mismatch"] == 11         # rinf::E_ADLER
    assert codes["fdict"] == 2 and codes["overrun"] == 8 and codes["underrun"] == 9
    assert all(codes[k] == 10 for k in codes if k.startswith("truncated"))


def test_gpu_decode_without_streams_is_refused(tmp_path):
    r = subprocess.run([sys.executable, "-m", "revo_amd.run_tum", "s.yaml", "d.yaml", "--gpu-decode"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "--streams 1" in r.stdout
