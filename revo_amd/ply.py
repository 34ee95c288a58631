"""Keyframe model export: the non-GL half of gui/MapDrawer.h.

MapDrawer::addPclAndKfPoseToQueue (MapDrawer.h:81-95) collects one coloured cloud
(ImgPyramidRGBD::generateColoredPcl, imgpyramidrgbd.cpp:279-327) and one pose per keyframe;
MapDrawer::saveModel (MapDrawer.h:97-170) writes them as two ASCII PLY files.  The file layout
below is the reference's, including its quirks: outputPcl.ply holds the points in their own
keyframe's coordinates (the viewer applies the pose when drawing), colours are written as
float*255 in "%g" form, and the edge count in outputKf.ply's header is 9*K-1.
`world=True` is an addition (points moved into the world frame) and is off by default.
"""
import os

import numpy as np


def _g(v):
    return "%g" % float(v)  # operator<<(float), 6 significant digits


class ModelExporter:
    def __init__(self):
        self.pclKfHost = []  # N x 8 float32 per keyframe
        self.vpKfsF = []     # 4x4 float32 T_w_kf per keyframe

    @property
    def nPts(self):
        return int(sum(len(p) for p in self.pclKfHost))

    def addPclAndKfPoseToQueue(self, kfPcl, T_Wkf):
        kfPcl = np.asarray(kfPcl, np.float32)
        if kfPcl.ndim != 2 or kfPcl.shape[1] != 8:
            raise ValueError("kfPcl must be N x 8 (X,Y,Z,1,r,g,b,1)")
        self.pclKfHost.append(kfPcl)
        self.vpKfsF.append(np.asarray(T_Wkf, np.float32).reshape(4, 4))

    def pcl_lines(self, world=False):
        for pcl, T in zip(self.pclKfHost, self.vpKfsF):
            xyz = pcl[:, :3]
            if world:
                xyz = (xyz @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
            rgb = pcl[:, 4:7] * np.float32(255.0)
            for p, c in zip(xyz, rgb):
                yield "%s %s %s %s %s %s" % (_g(p[0]), _g(p[1]), _g(p[2]), _g(c[0]), _g(c[1]), _g(c[2]))

    def kf_lines(self):
        w = np.float32(0.1)
        h = np.float32(w * np.float32(0.75))
        z = np.float32(w * np.float32(0.6))
        corners = np.array([[w, h, z], [w, -h, z], [-w, -h, z], [-w, h, z]], np.float32)
        for T in self.vpKfsF:
            R, t = T[:3, :3], T[:3, 3]
            for p in [t] + [R @ c + t for c in corners]:
                yield "%s %s %s 0 0 255" % (_g(p[0]), _g(p[1]), _g(p[2]))
        for k in range(len(self.vpKfsF)):
            cc, p1, p2, p3, p4 = (5 * k + i for i in range(5))
            for a, b in ((cc, p1), (cc, p2), (cc, p3), (cc, p4), (p1, p4), (p1, p2), (p2, p3), (p3, p4)):
                yield "%d %d 0 0 255" % (a, b)
            if k > 0:
                yield "%d %d 0 255 0" % ((k - 1) * 5, cc)

    def saveModel(self, directory=".", world=False):
        """Writes outputPcl.ply and outputKf.ply (MapDrawer.h:101,118) into `directory`."""
        os.makedirs(directory, exist_ok=True)
        pcl_path = os.path.join(directory, "outputPcl.ply")
        with open(pcl_path, "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex %d\n" % self.nPts)
            f.write("property float32 x\nproperty float32 y\nproperty float32 z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
            for line in self.pcl_lines(world):
                f.write(line + "\n")
        kf_path = os.path.join(directory, "outputKf.ply")
        K = len(self.vpKfsF)
        with open(kf_path, "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex %d\n" % (K * 5))
            f.write("property float32 x\nproperty float32 y\nproperty float32 z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\n")
            f.write("element edge %d\nproperty int vertex1\nproperty int vertex2\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % (K * 9 - 1))
            for line in self.kf_lines():
                f.write(line + "\n")
        return pcl_path, kf_path


VOXEL_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                            ("count", "<u4")])  # 19 bytes per vertex, packed


def voxel_ply_header(n):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property uint count\nend_header\n" % n).encode("ascii")


def write_voxel_ply(path, xyz, rgb, count):
    """The voxel map (api.VoxelMap) as binary little-endian PLY: one vertex per voxel in the order given (key order),
    xyz float32, rgb uchar, and the number of points fused into the voxel as `count` (uint32)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    count = np.asarray(count, np.uint32).reshape(-1)
    if not (len(xyz) == len(rgb) == len(count)):
        raise ValueError("xyz, rgb and count must have one row per voxel")
    v = np.empty(len(xyz), VOXEL_PLY_DTYPE)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    v["count"] = count
    with open(path, "wb") as f:
        f.write(voxel_ply_header(len(v)))
        f.write(v.tobytes())
    return path


VOXEL_PLY_NORMALS_DTYPE = np.dtype(VOXEL_PLY_DTYPE.descr + [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")])  # 31 bytes per vertex


def voxel_ply_normals_header(n):
    return voxel_ply_header(n).replace(b"end_header\n", b"property float nx\nproperty float ny\nproperty float nz\nend_header\n")


def write_voxel_ply_normals(path, xyz, rgb, count, normal):
    """write_voxel_ply's file with the voxel's normal (api.VoxelMap.normals) as nx ny nz behind `count`."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    count = np.asarray(count, np.uint32).reshape(-1)
    normal = np.asarray(normal, np.float32).reshape(-1, 3)
    if not (len(xyz) == len(rgb) == len(count) == len(normal)):
        raise ValueError("xyz, rgb, count and normal must have one row per voxel")
    v = np.empty(len(xyz), VOXEL_PLY_NORMALS_DTYPE)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    v["count"] = count
    v["nx"], v["ny"], v["nz"] = normal[:, 0], normal[:, 1], normal[:, 2]
    with open(path, "wb") as f:
        f.write(voxel_ply_normals_header(len(v)))
        f.write(v.tobytes())
    return path


def read_voxel_ply_normals(path):
    """Reader for write_voxel_ply_normals' files -> (xyz, rgb, count as read_voxel_ply's, normal N x 3 float32)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int([l for l in data[:end].decode("ascii").split("\n") if l.startswith("element vertex")][0].split()[2])
    if data[:end] != voxel_ply_normals_header(n):
        raise ValueError("not a voxel map PLY with normals")
    v = np.frombuffer(data, VOXEL_PLY_NORMALS_DTYPE, count=n, offset=end)
    return (np.stack([v["x"], v["y"], v["z"]], 1), np.stack([v["red"], v["green"], v["blue"]], 1), v["count"].copy(),
            np.stack([v["nx"], v["ny"], v["nz"]], 1))


def read_voxel_ply(path):
    """Reader for write_voxel_ply's files -> (xyz N x 3 float32, rgb N x 3 uint8, count N uint32)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int([l for l in data[:end].decode("ascii").split("\n") if l.startswith("element vertex")][0].split()[2])
    if data[:end] != voxel_ply_header(n):
        raise ValueError("not a voxel map PLY")
    v = np.frombuffer(data, VOXEL_PLY_DTYPE, count=n, offset=end)
    return (np.stack([v["x"], v["y"], v["z"]], 1), np.stack([v["red"], v["green"], v["blue"]], 1), v["count"].copy())


MESH_PLY_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<u4", (3,))])  # 13 bytes per face, packed


def mesh_ply_header(nv, nf, normals=False, colors=False):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\n%s%s"
            "element face %d\nproperty list uchar uint vertex_indices\nend_header\n"
            % (nv, "property float nx\nproperty float ny\nproperty float nz\n" if normals else "",
               "property uchar red\nproperty uchar green\nproperty uchar blue\n" if colors else "", nf)).encode("ascii")


def mesh_ply_vertex_dtype(normals=False, colors=False):
    return np.dtype([("p", "<f4", (3,))] + ([("n", "<f4", (3,))] if normals else []) + ([("rgb", "u1", (3,))] if colors else []))


def write_mesh_ply(path, vertices, triangles, normals=None, colors=None):
    """A triangle mesh (mapfile.Mesh) as binary little-endian PLY: `vertex` elements x y z float32 and `face` elements, each a
    list of three uint32 vertex indices, both in the order given.  normals ([V, 3] float32): nx ny nz behind the position;
    colors ([V, 4] uint8 B, G, R, k): red green blue behind those (k is not written).  Without them the file is what it was."""
    v = np.ascontiguousarray(np.asarray(vertices, "<f4").reshape(-1, 3))
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    if len(t) and int(t.max()) >= len(v):
        raise ValueError("a triangle names a vertex the mesh does not have")
    rows = np.zeros(len(v), mesh_ply_vertex_dtype(normals is not None, colors is not None))
    rows["p"] = v
    if normals is not None:
        rows["n"] = np.asarray(normals, "<f4").reshape(len(v), 3)
    if colors is not None:
        rows["rgb"] = np.asarray(colors, np.uint8).reshape(len(v), 4)[:, 2::-1]
    f = np.empty(len(t), MESH_PLY_FACE_DTYPE)
    f["n"], f["v"] = 3, t
    with open(path, "wb") as out:
        out.write(mesh_ply_header(len(v), len(t), normals is not None, colors is not None))
        out.write(rows.tobytes())
        out.write(f.tobytes())
    return path


def read_mesh_ply(path, attributes=False):
    """Reader for write_mesh_ply's files -> (vertices V x 3 float32, triangles T x 3 uint32).  attributes: -> (vertices,
    triangles, normals or None, colors or None); colors [V, 4] uint8 B, G, R and 255 (the file does not hold k)."""
    data = open(path, "rb").read()
    if b"end_header\n" not in data:
        raise ValueError("not a mesh PLY")
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii", "replace").split("\n")
    count = {l.split()[1]: int(l.split()[2]) for l in lines if l.startswith("element ")}
    nv, nf = count.get("vertex", 0), count.get("face", 0)
    has_n, has_c = "property float nx" in lines, "property uchar red" in lines
    dt = mesh_ply_vertex_dtype(has_n, has_c)
    if data[:end] != mesh_ply_header(nv, nf, has_n, has_c) or len(data) != end + dt.itemsize * nv + 13 * nf:
        raise ValueError("not a mesh PLY")
    rows = np.frombuffer(data, dt, count=nv, offset=end)
    v = rows["p"].reshape(nv, 3).copy()
    f = np.frombuffer(data, MESH_PLY_FACE_DTYPE, count=nf, offset=end + dt.itemsize * nv)
    if nf and not np.all(f["n"] == 3):
        raise ValueError("not a triangle mesh")
    t = f["v"].astype(np.uint32).reshape(nf, 3)
    if not attributes:
        return v, t
    colors = None
    if has_c:
        colors = np.full((nv, 4), 255, np.uint8)
        colors[:, :3] = rows["rgb"].reshape(nv, 3)[:, ::-1]
    return v, t, rows["n"].reshape(nv, 3).copy() if has_n else None, colors


def read_ply_vertices(path):
    """Minimal reader for the files above (tests): -> (V x 6 float array, list of edge tuples)."""
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    nv = ne = 0
    i = 2
    while lines[i] != "end_header":
        t = lines[i].split()
        if t[:2] == ["element", "vertex"]:
            nv = int(t[2])
        if t[:2] == ["element", "edge"]:
            ne = int(t[2])
        i += 1
    body = [l for l in lines[i + 1:] if l]
    verts = np.array([[float(x) for x in l.split()] for l in body[:nv]], np.float64).reshape(nv, 6)
    edges = [tuple(int(x) for x in l.split()) for l in body[nv:]]
    return verts, edges, ne
