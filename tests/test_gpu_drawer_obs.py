"""The closed open_drawer loop with the two mesh observers: make_open_drawer_env(scene_meshes=groups, observers={"pc": ...,
"mesh_tsdf": ...}) over the three cabinets of tests/drawer_scene_fixtures, the grids baked by mesh2sdf.bake_groups at a coarse voxel
size.  The rows an environment returns are the direct queries on env.compute_scene_pose(), bit for bit; they are finite although
the pose table carries NaN past a cabinet's body count; environments holding different cabinets see different volumes."""
import json
import os

import numpy as np
import pytest
import torch

from tests import depth_render_ref as D
from tests import drawer_scene_fixtures as DS
from tests import kinematic_episode as E
from tests import mesh_bake_ref as MB
from tests.helpers import GOLDEN, npy, same_bits, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MOBILE_URDF = os.path.join(GOLDEN, "franka_panda_sdf_mobile.urdf")
N, K = 5, 64
SIZE, RES, ORIGIN = 2.0, 20, (-1.5, -1.0, 0.0)               # the workspace of tests/test_gpu_drawer_scene.py's depth_tsdf loop
BAKE_VOXEL = 0.05


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    from partmanip_amd.envs import make_open_drawer_env, pc_observer, tsdf_observer
    from partmanip_amd.mesh2pc import PCfromMesh
    from partmanip_amd.mesh2sdf import TSDFfromMesh, bake_groups, bake_mesh
    from partmanip_amd.urdf import load_urdf
    assets, meshes = DS.load_groups(tmp_path_factory.mktemp("cabinets"))
    with open(os.path.join(GOLDEN, "kinematics_default_dof.json")) as f:
        cfg = {"robot": {"driveMode": "ik", "dof": json.load(f)["mobile"]}, "explore_step": 40, "maxEpisodeLength": 200, "random_reset": False}
    nr = len(load_urdf(MOBILE_URDF).robot_kwargs()["mesh_bodies"])
    robot = [D.finger_mesh()] + [MB.box_mesh((0.04, 0.03, 0.05), (0.0, 0.0, 0.0))] * (nr - 1)
    trunc = 4 * SIZE / RES
    cache = str(tmp_path_factory.mktemp("grids"))
    grids = bake_groups(DEV, meshes, trunc, BAKE_VOXEL, cache_dir=cache)
    files = sorted(os.listdir(cache))
    again = bake_groups(DEV, meshes, trunc, BAKE_VOXEL, cache_dir=cache)                  # the second call reads the files
    finger, box = (bake_mesh(DEV, trunc, BAKE_VOXEL, vertices=m[0], faces=m[1]) for m in robot[:2])
    obj_id = np.arange(N) % 3
    tsdf = TSDFfromMesh(N, SIZE, RES, DEV, vox_origin=ORIGIN, sdf_dicts=[finger] + [box] * (nr - 1), groups=grids, group_of=obj_id)
    pc = PCfromMesh(N, DEV, num_points=K, meshes=robot, groups=meshes, group_of=obj_id)
    torch.manual_seed(3301)
    ob_pc = pc_observer(pc)
    env = make_open_drawer_env(cfg, N, DEV, MOBILE_URDF, assets, E.DT, hold="always", scene_meshes=meshes,
                               observers={"pc": ob_pc, "mesh_tsdf": tsdf_observer(tsdf)})
    snap = lambda obs: dict(pc=obs["pc"].clone(), tsdf=obs["mesh_tsdf"].clone(), R=env.compute_scene_pose()[0].clone(),   # noqa: E731
                            T=env.compute_scene_pose()[1].clone())
    first = snap(env.reset())
    bb = npy(env.task.part_bbox).astype(np.float64)
    pull = bb[:, 0] - bb[:, 4]
    a = np.zeros((N, 10), dtype=np.float32)
    a[:, 3:6] = pull / np.linalg.norm(pull, axis=1, keepdims=True)
    for _ in range(3):
        obs, _, reset, _ = env.step(t(a, device=DEV))
        assert not bool(reset.any())
    return dict(env=env, tsdf=tsdf, pc=pc, sel=ob_pc.sel, nr=nr, first=first, last=snap(obs), meshes=meshes, grids=grids, again=again,
                files=files, cache=cache, obj_id=obj_id)


def test_bake_groups_one_grid_per_body_and_the_cache(loop):
    meshes, grids, again = loop["meshes"], loop["grids"], loop["again"]
    assert [len(g) for g in grids] == [len(m) for m in meshes] == [2, 7, 2]
    n = 0
    for bodies, gb, ga in zip(meshes, grids, again):
        for mesh, d, d2 in zip(bodies, gb, ga):
            assert (mesh is None) == (d is None) == (d2 is None)
            if d is None:
                continue
            n += 1
            assert d['sdf'].dtype == np.float32 and d['sdf'].ndim == 3 and float(d['voxel_size']) == BAKE_VOXEL
            assert d['sdf'].min() < 0.5 * BAKE_VOXEL * 3 ** 0.5 + 1e-6 and (d['sdf'] > 0).any()   # a cell within half a diagonal of the surface
            assert same_bits(d['sdf'], d2['sdf']) and same_bits(np.asarray(d['bbox_min']), np.asarray(d2['bbox_min']))
    assert n == 2 + 7 + 1 and len(loop["files"]) == len(set(loop["files"])) <= n and sorted(os.listdir(loop["cache"])) == loop["files"]
    assert all(f.endswith(".npy") and len(f) == 64 + 4 for f in loop["files"])


@pytest.mark.parametrize("when", ["first", "last"])
def test_rows_are_the_direct_queries_on_the_scene_pose(loop, when):
    s, tsdf, pc, nr = loop[when], loop["tsdf"], loop["pc"], loop["nr"]
    assert tuple(s["R"].shape) == (N, nr + 7, 3, 3) == (N, tsdf.part_num, 3, 3) and pc.part_num == nr + 7
    assert bool(torch.isnan(s["R"][0, nr + 2:]).all()) and bool(torch.isfinite(s["R"][1]).all())     # cabinet A has two bodies, B seven
    assert tuple(s["tsdf"].shape) == (N, RES ** 3) and tuple(s["pc"].shape) == (N, 3 * K)
    assert bool(torch.isfinite(s["tsdf"]).all()) and bool(torch.isfinite(s["pc"]).all())
    assert torch.equal(tsdf.query_tsdf(s["R"], s["T"]).reshape(N, -1), s["tsdf"])
    assert torch.equal(pc.query_pc(s["R"], s["T"], sel=loop["sel"]).reshape(N, -1), s["pc"])
    vol = npy(s["tsdf"])
    for b in range(N):
        scene_only = npy(tsdf.query_tsdf(s["R"][b:b + 1], s["T"][b:b + 1], group_of=[-1])).reshape(-1)
        print(f"{when}: environment {b} (object {loop['obj_id'][b]}): its cabinet changes {(vol[b] != scene_only).sum()} voxels")
        assert (vol[b] != scene_only).sum() >= 4, b                                       # the cabinet is in the volume
    assert same_bits(vol[0], vol[3])                                                      # the same cabinet in the same state
    assert not same_bits(vol[0], vol[1]) and not same_bits(vol[1], vol[2]) and not same_bits(vol[0], vol[2])
    # every environment's points come from the robot and from its own cabinet
    rows = npy(loop["sel"])
    for b in range(N):
        own = pc.own_rows(int(loop["obj_id"][b]))
        assert np.isin(rows[b], own).all() and (rows[b] >= pc.pts_shared).any(), b


def test_the_held_drawer_moves_in_both_observations(loop):
    first, last = loop["first"], loop["last"]
    for b in range(N):
        assert not torch.equal(first["tsdf"][b], last["tsdf"][b]), b
        assert not torch.equal(first["pc"][b], last["pc"][b]), b
