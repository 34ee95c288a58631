"""The voxel map's contract restated in numpy (tests/voxel_map_ref.py) at its edges, and the binary PLY it is saved as.
No GPU: the device map is checked against this restatement in tests/test_gpu_voxel_map.py."""
from fractions import Fraction

import numpy as np

import voxel_map_ref as ref

F = np.float32
I4 = np.eye(4, dtype=np.float32)


def _pts(*xs):
    """points on the x axis (identity pose: pw = ((1 x + 0 y) + 0 z) + 0 = x)."""
    xs = np.asarray(xs, np.float32)
    return np.stack([xs, np.zeros_like(xs), np.ones_like(xs)], 1)


def test_keys_on_voxel_boundaries_both_sides_of_zero():
    v = F(0.25)
    x = np.array([0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 0.2499999, -0.2500001, -1e-30, 1e-30], np.float32)
    pw = ref.world_points(_pts(*x), I4)
    assert np.array_equal(pw[:, 0], x)
    ok, k, q = ref.keys_and_fixed(pw, v)
    assert ok.all()
    assert k[:, 0].tolist() == [0, 0, 1, -1, 2, -2, 0, -2, -1, 0]
    # floor of negative quotients: a point just below zero is in voxel -1, exactly on -v it is voxel -1 too
    assert k[:, 2].tolist() == [4] * len(x)
    assert q[2, 0] == 1 << 18 and q[3, 0] == -(1 << 18)


def test_world_point_rounds_every_operation():
    T = np.array([[0.1, 0.7, 0.3, 0.01], [0.2, -0.5, 0.9, 1.3], [-0.3, 0.2, 0.4, -2.2], [0, 0, 0, 1]], np.float32)
    xyz = np.array([[1.1, -0.7, 2.3], [0.3, 0.123, 4.9]], np.float32)
    pw = ref.world_points(xyz, T)
    for n in range(2):
        for i in range(3):
            a = F(T[i, 0] * xyz[n, 0])
            b = F(T[i, 1] * xyz[n, 1])
            c = F(T[i, 2] * xyz[n, 2])
            assert pw[n, i] == F(F(F(a + b) + c) + T[i, 3])


def test_range_and_key_limits_drop_points():
    v = F(2.0 ** -9)  # |k| = 2^20 at 2048 m: both limits meet
    x = np.array([2047.998046875, -2047.9990234375, -2048.0, 2048.0, 4096.0, np.inf, -np.inf, np.nan], np.float32)
    ok, k, _ = ref.keys_and_fixed(ref.world_points(_pts(*x), I4), v)
    assert ok.tolist() == [True, True, False, False, False, False, False, False]
    assert k[0, 0] == ref.KEY_MAX and k[1, 0] == ref.KEY_MIN
    v = F(2.0 ** -10)  # |k| reaches 2^20 at 1024 m, inside the 2048 m range: the key limit drops on its own
    x = np.array([1023.9990234375, 1024.0, -1024.0, -1024.0009765625], np.float32)
    ok, k, _ = ref.keys_and_fixed(ref.world_points(_pts(*x), I4), v)
    assert ok.tolist() == [True, False, True, False]
    assert k[0, 0] == ref.KEY_MAX and k[2, 0] == ref.KEY_MIN
    # a pose that overflows float32: pw = inf, dropped and counted
    T = I4.copy()
    T[0, 0] = 3e38
    m = ref.VoxelMapRef(0.1)
    m.integrate(np.array([[2.0, 0, 0], [0, 0.5, 0]], np.float32), np.zeros((2, 3), np.uint8), T)
    assert m.points_dropped == 1 and m.points_integrated == 1


def test_nan_and_inf_depth_are_not_input_points():
    depth = np.array([[1.0, np.nan, np.inf], [-np.inf, 0.05, 6.0], [2.0, 3.0, 5.19]], np.float32)
    edges = np.full((3, 3), 255, np.uint8)
    bgr = np.arange(27, dtype=np.uint8).reshape(3, 3, 3)
    xyz, rgb = ref.select_points(depth, edges, bgr, 500.0, 500.0, 1.0, 1.0, 0.1, 5.2, dense=True)
    assert xyz[:, 2].tolist() == [1.0, 2.0, 3.0, F(5.19)]
    assert rgb[0].tolist() == [2, 1, 0] and rgb[1].tolist() == [20, 19, 18]  # BGR bytes -> R, G, B
    edges[2, 1] = 0
    xyz, _ = ref.select_points(depth, edges, bgr, 500.0, 500.0, 1.0, 1.0, 0.1, 5.2, dense=False)
    assert xyz[:, 2].tolist() == [1.0, 2.0, F(5.19)]


def test_colour_rounds_half_up():
    sc = np.array([[1, 3, 2], [0, 510, 255]], np.int64)
    cnt = np.array([2, 2], np.int64)
    assert ref.mean_colour(sc, cnt).tolist() == [[1, 2, 1], [0, 255, 128]]
    assert ref.mean_colour(np.array([[2, 6, 5]]), np.array([4])).tolist() == [[1, 2, 1]]  # .5 -> up, 1.5 -> 2, 1.25 -> 1
    m = ref.VoxelMapRef(1.0)
    m.integrate(_pts(0.1, 0.2), np.array([[0, 10, 255], [1, 11, 254]], np.uint8), I4)
    xyz, rgb, cnt = m.points()
    assert cnt.tolist() == [2] and rgb.tolist() == [[1, 11, 255]]


def test_colour_bytes_come_back_from_the_cloud():
    c = np.arange(256, dtype=np.float32)
    cloud = np.zeros((256, 8), np.float32)
    cloud[:, 4] = c / F(255)
    cloud[:, 5] = (255 - c) / F(255)
    cloud[:, 6] = c / F(255)
    _, rgb = ref.points_from_pcl(cloud)
    assert rgb[:, 0].tolist() == list(range(256)) and rgb[:, 1].tolist() == list(range(255, -1, -1))


def test_key_order_across_sign_changes():
    k = np.array([[0, 0, 0], [0, 0, -1], [0, -1, 0], [-1, 0, 0], [-1, 5, 5], [1, -5, -5], [0, 0, 1],
                  [ref.KEY_MIN, ref.KEY_MAX, 0], [ref.KEY_MAX, ref.KEY_MIN, ref.KEY_MIN]], np.int64)
    packed = ref.pack_keys(k)
    order = np.argsort(packed, kind="stable")
    assert [tuple(r) for r in k[order]] == sorted(tuple(r) for r in k)  # ascending packed key = lexicographic (x, y, z)
    assert packed.max() < np.uint64(1 << 63)  # bit 63 is never set: the device's empty marker is all ones
    # the map extracts in that order
    m = ref.VoxelMapRef(0.5)
    xs = np.array([0.1, -0.1, 0.6, -0.6, 1e-3], np.float32)
    m.integrate(np.stack([xs, -xs, xs], 1), np.zeros((5, 3), np.uint8), I4)
    xyz, _, cnt = m.points()
    q = [int(np.rint(F(x) * ref.FIX)) for x in (-0.6, -0.1, 0.1, 1e-3, 0.6)]
    assert xyz[:, 0].tolist() == [F(q[0] / 2 ** 20), F(q[1] / 2 ** 20), F((q[2] + q[3]) / 2 / 2 ** 20), F(q[4] / 2 ** 20)]
    assert cnt.tolist() == [1, 1, 2, 1]


def test_fixed_point_sums_stay_exact_in_float64():
    # the documented limit: |q| < 2^31 (|pw| < 2048 m at 2^-20 m) and up to 2^22 points per voxel keep |sum q| < 2^53
    qmax = (1 << 31) - 1
    for cnt in (1, 3, 1 << 10, 1 << 22):
        for q in (qmax, -qmax, qmax - 12345, 1):
            s = q * cnt
            assert abs(s) < 1 << 53 and int(np.float64(s)) == s
            got = ref.mean_position(np.array([[s, -s, 0]], np.int64), np.array([cnt]))[0]
            exact = Fraction(s, cnt) / (1 << 20)
            assert got[0] == F(float(exact)) and got[1] == -got[0] and got[2] == 0
    # a voxel fed the same point n times lands on that point's fixed-point value
    x = np.array([1.2345678, -0.0001, 2047.9], np.float32)
    for xi in x:
        q = np.int64(np.rint(xi * ref.FIX))
        assert ref.mean_position(np.array([[q * 1000, 0, 0]]), np.array([1000]))[0, 0] == F(float(q) / (1 << 20))
    # the multiplication by 2^20 is exact for every float32 below 2048 m
    rng = np.random.default_rng(0)
    v = rng.uniform(-2048, 2048, 100000).astype(np.float32)
    assert np.array_equal((v * ref.FIX).astype(np.float64), v.astype(np.float64) * 2.0 ** 20)


def test_voxel_ply_header_and_layout(tmp_path):
    from revo_amd import ply
    xyz = np.array([[1.5, -2.25, 3.0], [0.1, 0.2, 0.3]], np.float32)
    rgb = np.array([[255, 0, 7], [1, 2, 3]], np.uint8)
    cnt = np.array([1, 0x01020304], np.uint32)
    p = ply.write_voxel_ply(str(tmp_path / "m.ply"), xyz, rgb, cnt)
    data = open(p, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\n"
              b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uint count\nend_header\n")
    assert data.startswith(header) and len(data) == len(header) + 2 * 19
    rec = data[len(header):]
    assert rec[:12] == np.array([1.5, -2.25, 3.0], "<f4").tobytes() and rec[12:15] == bytes([255, 0, 7])
    assert rec[15:19] == b"\x01\x00\x00\x00" and rec[19 + 15:19 + 19] == b"\x04\x03\x02\x01"
    a, b, c = ply.read_voxel_ply(p)
    assert np.array_equal(a, xyz) and np.array_equal(b, rgb) and np.array_equal(c, cnt)
    p0 = ply.write_voxel_ply(str(tmp_path / "e.ply"), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))
    assert open(p0, "rb").read() == header.replace(b"vertex 2", b"vertex 0")


def test_run_tum_rejects_a_bad_voxel(capsys):
    from revo_amd import run_tum
    for v in ("0", "-0.01", "nan", "inf"):
        assert run_tum.main(["settings.yaml", "dataset.yaml", "--map", v]) == 2
        assert "--map needs a positive voxel" in capsys.readouterr().out
