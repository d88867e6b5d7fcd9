"""Triangle-mesh readers for the mesh bake (partmanip_amd/mesh2sdf.py: TSDFfromMesh.mesh2sdf) and the surface sampler of the posed
point cloud (partmanip_amd/mesh2pc.py: PCfromMesh), standard library + numpy only (the sampler draws its uniforms from a torch
generator).

    vertices (V, 3) float32, faces (F, 3) int64 = load_mesh(path)
    points (count, 3) float32, face_index (count,) int64 = sample_surface(vertices, faces, count, generator)

Wavefront OBJ: `v x y z` and `f` records; a face corner is `i`, `i/j`, `i/j/k` or `i//k` (only the position index is used), indices
are 1-based or negative (relative to the vertices read so far), a polygon is fan-triangulated around its first corner; every
other record is ignored.  Vertices are kept as the file lists them.
STL: binary when the file is exactly 84 + 50 n bytes long with n the count at offset 80 (a binary STL may begin with the word
`solid`, so the first bytes decide nothing), ASCII otherwise.  STL stores three corners per triangle; corners at exactly the same
position become one vertex (numbered in order of first appearance), which is what makes a closed STL surface closed again.
"""
import os
import struct

import numpy as np

# The Franka scene's rigid parts in the reference's order (mesh2pc.py:20-24, 44-51; mesh2sdf.py:142-145): eight links, the hand, two
# fingers (one file twice), then the object.
FRANKA_MESH_DIR = os.path.join("assets", "franka_description", "meshes", "visual")
FRANKA_MESHES = [f"link{i}.obj" for i in range(8)] + ["hand.obj", "finger.stl", "finger.stl"]
OBJ_MESH_PATH = os.path.join("assets", "objs", "cube", "cube.obj")


def scene_mesh_paths(asset_root):
    """The mesh files of the scene's parts under `asset_root`, in part order."""
    return [os.path.join(asset_root, FRANKA_MESH_DIR, name) for name in FRANKA_MESHES] + [os.path.join(asset_root, OBJ_MESH_PATH)]


def load_obj(path):
    verts, faces = [], []
    with open(path, "r", errors="replace") as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v" and len(tok) >= 4:
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "f" and len(tok) >= 4:
                idx = []
                for c in tok[1:]:
                    i = int(c.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for a in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[a], idx[a + 1]))
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    fa = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if fa.size and (fa.min() < 0 or fa.max() >= len(v)):
        raise ValueError(f"{path}: a face refers to a vertex that does not exist")
    return v, fa


def _merge_corners(corners):
    """(n, 3, 3) float32 corner positions -> (vertices, faces): one vertex per distinct position, in order of first appearance."""
    flat = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 3) + np.float32(0.0)     # -0.0 -> +0.0: one position
    _, first, inv = np.unique(flat.view(np.dtype((np.void, 12))).reshape(-1), return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # unique's (byte-sorted) numbering -> order of first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return flat[first[order]], rank[inv.reshape(-1)].reshape(-1, 3).astype(np.int64)


def load_stl(path):
    with open(path, "rb") as f:
        data = f.read()
    if len(data) >= 84:
        n = struct.unpack_from("<I", data, 80)[0]
        if len(data) == 84 + 50 * n:
            rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n, offset=84)
            return _merge_corners(rec["v"])
    corners = []
    for line in data.decode("ascii", errors="replace").splitlines():
        tok = line.split()
        if len(tok) >= 4 and tok[0] == "vertex":
            corners.append((float(tok[1]), float(tok[2]), float(tok[3])))
    if not corners or len(corners) % 3:
        raise ValueError(f"{path}: neither a binary STL (84 + 50 n bytes) nor an ASCII STL with whole triangles")
    return _merge_corners(np.asarray(corners, dtype=np.float32).reshape(-1, 3, 3))


def load_mesh(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        return load_obj(path)
    if ext == ".stl":
        return load_stl(path)
    raise ValueError(f"{path}: only .obj and .stl meshes are read")


def drop_double_corner_faces(vertices, faces):
    """Faces with two corners at the same position are dropped (the reference's `faces[x1]`, mesh2sdf.py:209-210, which follows
    trimesh's merge of equal vertices: so positions are compared, not only indices)."""
    p = np.asarray(vertices, dtype=np.float32)[np.asarray(faces, dtype=np.int64)]              # (F, 3, 3)
    same = (p[:, 0] == p[:, 1]).all(axis=1) | (p[:, 0] == p[:, 2]).all(axis=1) | (p[:, 1] == p[:, 2]).all(axis=1)
    return np.asarray(faces, dtype=np.int64)[~same]


def sample_surface(vertices, faces, count, generator):
    """Area-proportional surface sample (stands in for trimesh.sample.sample_surface, the reference's mesh2pc.py:37): `count` points
    -> (points float32 (count, 3), face_index int64 (count,) into the faces that drop_double_corner_faces keeps).  u = torch.rand(count, 3, generator,
    float64); triangle areas and their inclusive cumulative sum in fp64 in face order; the face is the first i with
    cdf[i] > u0 * cdf[-1] (a zero-area face is never picked); (a, b) = (u1, u2), reflected to (1 - a, 1 - b) where a + b > 1; the
    point is v0 + a (v1 - v0) + b (v2 - v0) in fp64, rounded once to float32."""
    import torch
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = drop_double_corner_faces(v32, np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    if len(faces) == 0:
        raise ValueError("sample_surface: no triangle is left to sample")
    tri = v32.astype(np.float64)[faces]                                                         # (F, 3, 3)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    cdf = np.cumsum(area)
    if not (cdf[-1] > 0.0) or not np.isfinite(cdf[-1]):
        raise ValueError("sample_surface: the mesh has no surface area")
    u = torch.rand(int(count), 3, generator=generator, dtype=torch.float64).numpy()
    i = np.searchsorted(cdf, u[:, 0] * cdf[-1], side="right")                                   # first i with cdf[i] > u0 * total
    i = np.minimum(i, np.flatnonzero(area > 0.0)[-1])                                           # u0 * total rounded up to total
    a, b = u[:, 1].copy(), u[:, 2].copy()
    flip = a + b > 1.0
    a[flip], b[flip] = 1.0 - a[flip], 1.0 - b[flip]
    pts = tri[i, 0] + a[:, None] * e1[i] + b[:, None] * e2[i]
    return pts.astype(np.float32), i.astype(np.int64)


def save_obj(path, vertices, faces):
    """Minimal writer (tools and tests): `v` with 9 significant digits (float32 round-trips), 1-based `f`."""
    with open(path, "w") as f:
        for v in np.asarray(vertices, dtype=np.float32):
            f.write("v %.9g %.9g %.9g\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in np.asarray(faces, dtype=np.int64):
            f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))
