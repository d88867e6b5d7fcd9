"""Yardstick of the mesh bake (partmanip_amd/mesh2sdf.py: TSDFfromMesh.mesh2sdf, csrc/mesh_bake.hip): a brute-force numpy
restatement of the contract, written from its description and sharing no text with the kernel, plus seeded meshes.

* grid layout: the reference's fp32 expressions (center = (vmax + vmin) / 2, range = vmax - vmin + 2 trunc, shape = ceil(range /
  voxel), voxel idx at (idx - shape // 2) * voxel + center, every operation rounded to fp32), here with numpy float32 scalars;
* magnitude: for every (point, triangle) pair the closest point of the triangle by the Voronoi region the point falls in (a
  corner, an edge, the face), sqrt of the smallest squared distance; a triangle without area is its longest edge;
* sign by the generalised winding number w = sum of solid angles / 4 pi (van Oosterom-Strackee, atan2), inside iff |w| >= 0.5;
* an independent sign: the parity of the crossings of a ray in a fixed irrational direction (closed meshes only).

`dtype` selects the arithmetic: float64 is the yardstick, float32 is "what a plain fp32 evaluation of the same formulas loses"
(e_ref of the GPU tests).  The fp32 voxel positions and fp32 vertices are exact inputs of both."""
import atexit
import functools
import gzip
import os
import shutil
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

TRUNC = 4 * 0.5 / 50                    # sdf_trunc of the shipped configuration (size 0.5, resolution 50)
VOXEL = 0.002                           # pre_store_sdf_voxel_size
RAY = np.array([1.0, np.sqrt(2.0), np.sqrt(3.0)]) / np.sqrt(6.0)


# ------------------------------------------------------------------------------------------------------------ grid layout
def grid_layout(vertices, trunc=TRUNC, voxel=VOXEL):
    """((X, Y, Z), [xs, ys, zs] float32 coordinate tables, bbox_min float32 (3,)) in numpy float32 arithmetic."""
    v = np.asarray(vertices, dtype=np.float32)
    f = np.float32
    vmax, vmin = v.max(axis=0), v.min(axis=0)
    center = (vmax + vmin) / f(2)
    rng = vmax - vmin + f(2 * trunc)
    shape_f = np.ceil(rng / f(voxel))
    assert center.dtype == rng.dtype == shape_f.dtype == np.float32
    shape = tuple(int(s) for s in shape_f)
    half = np.floor(shape_f / f(2))
    tables = [(np.arange(shape[a]).astype(np.float32) - half[a]) * f(voxel) + center[a] for a in range(3)]
    assert all(t.dtype == np.float32 for t in tables)
    return shape, tables, np.array([t[0] for t in tables], dtype=np.float32)


def range_over_voxel(vertices, trunc=TRUNC, voxel=VOXEL):
    """range / voxel in fp64: the tests assert that it is not within 1e-3 of an integer, so the fp32 ceil cannot fall either way."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    return (v.max(axis=0) - v.min(axis=0) + 2 * trunc) / voxel


def grid_points(tables, index=None):
    """(n, 3) float32 positions of the whole grid (k fastest) or of the flat voxel indices `index`."""
    X, Y, Z = (len(t) for t in tables)
    idx = np.arange(X * Y * Z) if index is None else np.asarray(index)
    return np.stack([tables[0][idx // (Y * Z)], tables[1][(idx // Z) % Y], tables[2][idx % Z]], axis=1)


# ------------------------------------------------------------------------------------------------------------ faces
def clean_faces(vertices, faces):
    """Faces with two corners at the same position are dropped."""
    p = np.asarray(vertices, dtype=np.float32)[np.asarray(faces)]
    keep = ~((p[:, 0] == p[:, 1]).all(1) | (p[:, 0] == p[:, 2]).all(1) | (p[:, 1] == p[:, 2]).all(1))
    return np.asarray(faces)[keep]


def _split_degenerate(tri64):
    """(triangles with an area, (n, 2, 3) longest edges of those without): collinear means a zero cross product in fp64."""
    cr = np.cross(tri64[:, 1] - tri64[:, 0], tri64[:, 2] - tri64[:, 0])
    flat = (cr == 0).all(axis=1)
    segs = []
    for t in tri64[flat]:
        pairs = [(t[0], t[1]), (t[1], t[2]), (t[2], t[0])]
        segs.append(max(pairs, key=lambda ab: float(np.sum((ab[1] - ab[0]) ** 2))))
    return tri64[~flat], np.asarray(segs, dtype=np.float64).reshape(-1, 2, 3)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _tri_d2(p, tri):
    """(n, F) squared distances point -> triangle: the closest point by Voronoi region (corners A, B, C; edges AB, AC, BC; face)."""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    ab, ac = b - a, c - a
    ap, bp, cp = p[:, None] - a, p[:, None] - b, p[:, None] - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = va + vb + vc
        v, w = vb / den, vc / den
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    s = np.select(conds, [zero, one, t_ab, zero, zero, one - t_bc], default=v)      # closest = A + s AB + t AC
    t = np.select(conds, [zero, zero, zero, one, t_ac, t_bc], default=w)
    diff = ap - ab * s[..., None] - ac * t[..., None]
    return _dot(diff, diff)


def _seg_d2(p, seg):
    a, b = seg[None, :, 0], seg[None, :, 1]
    ab, ap = b - a, p[:, None] - a
    t = np.clip(_dot(ap, ab) / _dot(ab, ab), 0, 1)
    diff = ap - ab * t[..., None]
    return _dot(diff, diff)


def _turns(p, tri):
    """(n,) sum over triangles of atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) = (sum of solid angles) / 2."""
    a, b, c = tri[None, :, 0] - p[:, None], tri[None, :, 1] - p[:, None], tri[None, :, 2] - p[:, None]
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    num = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return np.arctan2(num, den).sum(axis=1)


def _crossings(p, tri):
    """(n,) number of triangles the ray p + t RAY, t > 0, crosses (Moller-Trumbore, fp64)."""
    a = tri[None, :, 0]
    e1, e2 = tri[None, :, 1] - a, tri[None, :, 2] - a
    h = np.cross(RAY[None, None], e2)
    det = _dot(e1, h)
    s = p[:, None] - a
    with np.errstate(divide="ignore", invalid="ignore"):
        u = _dot(s, h) / det
        q = np.cross(s, e1)
        v = _dot(q, RAY[None, None]) / det
        t = _dot(q, e2) / det
    hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    return hit.sum(axis=1)


def evaluate(points, vertices, faces, trunc=TRUNC, dtype=np.float64, parity=False, pairs_per_chunk=1 << 20, threads=8):
    """points (n, 3) float32, vertices (V, 3) float32, faces (F, 3) -> dict of (n,) arrays: 'd' the unsigned distance, 'w' the
    winding number, 'sdf' = clamp(-d if |w| >= 0.5 else d, -trunc, trunc), all in `dtype` arithmetic, and with parity=True
    'inside_parity' (bool, fp64 ray crossings odd)."""
    faces = clean_faces(vertices, faces)
    tri64 = np.asarray(vertices, dtype=np.float32).astype(np.float64)[faces]
    full64, seg64 = _split_degenerate(tri64)
    full, seg = full64.astype(dtype), seg64.astype(dtype)
    pts = np.asarray(points, dtype=np.float32)
    n = len(pts)
    step = max(1, pairs_per_chunk // max(1, len(faces)))

    def work(lo):
        p = pts[lo:lo + step].astype(dtype)
        d2 = np.full(len(p), np.inf, dtype=dtype)
        turn = np.zeros(len(p), dtype=dtype)
        if len(full):
            d2 = np.minimum(d2, _tri_d2(p, full).min(axis=1))
            turn = _turns(p, full)
        if len(seg):
            d2 = np.minimum(d2, _seg_d2(p, seg).min(axis=1))
        par = (_crossings(p.astype(np.float64), full64) % 2 == 1) if parity else None
        assert d2.dtype == dtype and turn.dtype == dtype
        return lo, d2, turn, par

    out_d2, out_turn = np.empty(n, dtype=dtype), np.empty(n, dtype=dtype)
    out_par = np.zeros(n, dtype=bool)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        for lo, d2, turn, par in ex.map(work, range(0, n, step)):
            out_d2[lo:lo + len(d2)] = d2
            out_turn[lo:lo + len(d2)] = turn
            if parity:
                out_par[lo:lo + len(d2)] = par
    d = np.sqrt(out_d2)
    w = out_turn / dtype(2 * np.pi)
    res = dict(d=d, w=w, sdf=np.clip(np.where(np.abs(w) >= dtype(0.5), -d, d), dtype(-trunc), dtype(trunc)))
    if parity:
        res["inside_parity"] = out_par
    return res


def bake64(vertices, faces, trunc=TRUNC, voxel=VOXEL):
    """The whole contract in fp64 on the fp32 grid: the reference's dict with a float64 'sdf'."""
    shape, tables, bbox_min = grid_layout(vertices, trunc, voxel)
    r = evaluate(grid_points(tables), vertices, faces, trunc)
    return {'sdf': r["sdf"].reshape(shape), 'bbox_min': bbox_min, 'voxel_size': voxel}


# ------------------------------------------------------------------------------------------------------------ meshes
HAND_BYTES = 483975


@functools.lru_cache(maxsize=None)
def hand_obj():
    """Path of the open real mesh hand.obj.  The fixture is kept gzip-compressed (tests/golden/hand.obj.gz, the file's 483 975 bytes
    unchanged inside); it is unpacked once per process into a temporary folder that is removed at exit."""
    folder = tempfile.mkdtemp(prefix="mesh_bake_")
    atexit.register(shutil.rmtree, folder, ignore_errors=True)
    path = os.path.join(folder, "hand.obj")
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand.obj.gz"), "rb") as src:
        data = src.read()
    assert len(data) == HAND_BYTES
    with open(path, "wb") as dst:
        dst.write(data)
    return path


BOX_HALF = (0.0313, 0.0227, 0.0171)                         # non-round half-extents
BOX_CENTRE = (0.0112, -0.0071, 0.0043)
TORUS_R, TORUS_r = 0.0811, 0.0294


def box_mesh(half=BOX_HALF, centre=BOX_CENTRE):
    """12 outward-facing triangles of an axis-aligned box."""
    h, c = np.asarray(half, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * h + c
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v.astype(np.float32), np.asarray(faces, dtype=np.int64)


def torus_mesh(R=TORUS_R, r=TORUS_r, nu=100, nv=100):
    """Torus around the z axis, nu x nv quads split along one diagonal: 2 nu nv triangles, closed."""
    u = 2 * np.pi * np.arange(nu) / nu
    v = 2 * np.pi * np.arange(nv) / nv
    uu, vv = np.meshgrid(u, v, indexing="ij")
    pts = np.stack([(R + r * np.cos(vv)) * np.cos(uu), (R + r * np.cos(vv)) * np.sin(uu), r * np.sin(vv)], axis=-1).reshape(-1, 3)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            faces += [(a, b, c), (a, c, d)]
    return pts.astype(np.float32), np.asarray(faces, dtype=np.int64)


def torus_sdf(p, R=TORUS_R, r=TORUS_r):
    p = np.asarray(p, dtype=np.float64)
    return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R) ** 2 + p[:, 2] ** 2) - r


def torus_chord_bound(R=TORUS_R, r=TORUS_r, n=100):
    """H = 2 [(R + r)(1 - cos(pi / n)) + r (1 - cos(pi / n))]: the two chord sags of an inscribed facet, doubled for the quad's diagonal."""
    return 2 * ((R + r) * (1 - np.cos(np.pi / n)) + r * (1 - np.cos(np.pi / n)))


DYADIC_HALF = (0.03125, 0.0234375, 0.015625)                # exact in fp32, and so are the halves and quarters of its edges


def degenerate_mesh():
    """A box with dyadic corners plus (a) a face with two corners at the same position (a repeated vertex under another index) and
    (b) a collinear sliver lying strictly inside one box edge (corners at -1/2, 0, +1/2 of the edge's half-length, all exact in
    fp32).  Every point of the sliver is a point of the box's surface, so the distance field is that of the box, and no closest
    point of the sliver can beat the edge it lies in.  Returns (vertices, faces with both, faces without them)."""
    v, f = box_mesh(DYADIC_HALF, (0.0, 0.0, 0.0))
    assert np.all(v[0] == -np.asarray(DYADIC_HALF, dtype=np.float32)) and np.all(v[1][:2] == v[0][:2])   # edge 0-1 runs along z
    q = DYADIC_HALF[2] / 2
    sl = np.array([[v[0][0], v[0][1], -q], [v[0][0], v[0][1], 0.0], [v[0][0], v[0][1], q]], dtype=np.float32)
    v2 = np.concatenate([v, v[3:4], sl], axis=0)             # vertex 8 repeats vertex 3; 9, 10, 11 are the sliver
    extra = np.array([[2, 3, 8], [9, 10, 11]], dtype=np.int64)
    return v2, np.concatenate([f, extra], axis=0), f


def edge_use_counts(faces):
    """{undirected edge: number of faces using it}."""
    f = np.asarray(faces)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return counts
