"""Seeded scenes for the tests of the grouped mesh observers (TSDFfromMesh(groups=), PCfromMesh(groups=),
pm_mesh_tsdf_query_groups_f32): a grid library with a shared range and groups, one group per environment, and what an environment
owns by the definition.  numpy only; not product code.

small_scene(): the six 'cut' parts of mesh_tsdf_parts.make_parts(3101, ..., size = 0.5, res = 10) -- res = 10 is not a multiple of
the 4-voxel brick, so the last work-group of an environment is part-filled -- with two shared rows, the groups [[2], [3, 4, 5], []]
and six environments [0, 1, 2, -1, 1, 0] over M = 2 + 3 pose slots.

boundary_scene(): 63 shared rows and groups of 3, 2 and 1 rows of tiny grids (8^3 cells of a sphere's distance), so that the group
of environment 0 straddles the 64-lane boundary of the kernel's ballot (ordinals 63 | 64, 65) and M = 66 slots need two passes of
the pose test."""
import numpy as np

from tests import mesh_tsdf_parts as P

F32 = np.float32
SIZE, RES = 0.5, 10


def library(parts, n_shared, groups):
    """parts: one dict per library row; groups: lists of rows (each past the shared range, consecutive overall).  A group's i-th row
    takes slot n_shared + i, as TSDFfromMesh(groups=) lays a cabinet's bodies out."""
    rows = [r for g in groups for r in g]
    assert rows == list(range(n_shared, len(parts)))
    slot = list(range(n_shared)) + [n_shared + i for g in groups for i in range(len(g))]
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    return dict(parts=parts, NG_shared=n_shared, grid_slot=np.asarray(slot, dtype=np.int32), group_off=off,
                M=n_shared + max(len(g) for g in groups))


def small_scene():
    sc = library(P.make_parts(3101, 'cut', n_parts=6, size=SIZE, res=RES), 2, [[2], [3, 4, 5], []])
    R, T = P.random_poses(3102, 6, M=5)
    sc.update(R=R, T=T, env_group=np.array([0, 1, 2, -1, 1, 0], dtype=np.int32))
    return sc


def sphere_grid(radius, cells=8, voxel_size=0.05, trunc=4 * SIZE / RES):
    """cells^3 samples of the distance to a sphere about the grid's centre, clamped to +-trunc: valid for u in [1, cells - 2]."""
    idx = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), axis=-1)
    pts = (idx - (cells - 1) / 2.0) * voxel_size
    d = np.linalg.norm(pts, axis=-1) - radius
    return {'sdf': np.clip(d, -trunc, trunc).astype(F32), 'bbox_min': pts.reshape(-1, 3).min(axis=0).astype(F32),
            'voxel_size': float(F32(voxel_size))}


def boundary_scene(seed=3103):
    rng = np.random.RandomState(seed)
    parts = [sphere_grid(r) for r in rng.uniform(0.05, 0.09, size=63 + 6)]
    sc = library(parts, 63, [[63, 64, 65], [66, 67], [68]])
    B, M = 4, sc["M"]
    R, T = P.random_poses(seed + 1, B, M=M)
    # the shared spheres keep to x < 0.05; the group's rows sit apart from them and from each other, high above the ground
    T[:, :63, 0] = rng.uniform(-0.2, 0.05, size=(B, 63)).astype(F32)
    for i in range(3):
        T[:, 63 + i] = np.asarray([0.17, -0.15 + 0.15 * i, 0.1 + 0.1 * i], dtype=F32) + rng.uniform(-0.01, 0.01, size=(B, 3)).astype(F32)
    sc.update(R=R, T=T, env_group=np.array([0, 1, 2, -1], dtype=np.int32))
    return sc


def own_rows(sc, b, env_group=None, max_group_grids=None, t0=0, t1=None):
    """The library rows environment b samples, in ordinal order, by the definition; [t0, t1) cuts the ordinals."""
    g = int((sc["env_group"] if env_group is None else env_group)[b])
    rows = list(range(sc["NG_shared"]))
    if 0 <= g < len(sc["group_off"]) - 1:
        lo, hi = (sc["NG_shared"] + int(sc["group_off"][g + i]) for i in (0, 1))
        rows += list(range(lo, hi if max_group_grids is None else min(hi, lo + max_group_grids)))
    return rows[t0:t1]


def restate_own(sc, b, rows=None, base=None):
    """The fp64 restatement of environment b's volume over `rows` (default: its own), (res^3,)."""
    rows = own_rows(sc, b) if rows is None else rows
    slots = sc["grid_slot"][rows]
    vol, _ = P.restate([sc["parts"][r] for r in rows], sc["R"][b:b + 1, slots], sc["T"][b:b + 1, slots], res=RES, size=SIZE, base=base)
    return vol.reshape(-1)
