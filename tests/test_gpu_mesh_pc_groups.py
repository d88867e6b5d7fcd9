"""The grouped mesh cloud on the GPU: PCfromMesh(groups=) keeps one point library (the shared parts' points, then every object's
bodies) and hands pm_mesh_pc_query_f32 one selection per environment, drawn from that environment's own cloud.  The kernel is the
existing one, so every check is an equality of bit patterns against an ungrouped PCfromMesh(part_pcs = the environment's own
parts) queried with the same points."""
import numpy as np
import pytest
import torch

from tests import drawer_scene_fixtures as DS
from tests import mesh_bake_ref as MB
from tests.helpers import npy, same_bits, t
from tests.mesh_tsdf_parts import random_poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 48
GROUP_OF = np.array([0, 1, 2, -1, 1, 0], dtype=np.int32)


def meshes():
    shared = [MB.box_mesh((0.04, 0.03, 0.05), (0.0, 0.0, 0.01)), DS.ellipsoid_mesh((0.05, 0.03, 0.04))]
    groups = [[MB.box_mesh((0.02, 0.05, 0.03), (0.0, 0.0, 0.0)), None, DS.ellipsoid_mesh((0.03, 0.03, 0.06))],
              [MB.box_mesh((0.06, 0.02, 0.02), (0.01, 0.0, 0.0))],
              [None, None]]
    return shared, groups


@pytest.fixture(scope="module")
def scene():
    from partmanip_amd.mesh2pc import PCfromMesh
    shared, groups = meshes()
    pc = PCfromMesh(6, DEV, num_points=K, meshes=shared, groups=groups, group_of=GROUP_OF, seed=7)
    R, T = random_poses(3201, 6, M=pc.part_num)
    return dict(pc=pc, R=t(R, device=DEV), T=t(T, device=DEV))


def own_cloud(sc, b, sel_rows):
    """The ungrouped PCfromMesh over environment b's own parts, queried with the same points (sel_rows: rows of the library, -1 kept)."""
    from partmanip_amd.mesh2pc import PCfromMesh
    pc = sc["pc"]
    rows = pc.own_rows(int(GROUP_OF[b]))
    pts, part = npy(pc.pts), npy(pc.part_of)
    slots = part[rows][::K]
    assert (part[rows].reshape(-1, K) == slots[:, None]).all()
    own = PCfromMesh(1, DEV, num_points=K, part_pcs=pts[rows].reshape(-1, K, 3))
    where = np.searchsorted(rows, sel_rows)
    assert (rows[np.minimum(where, len(rows) - 1)] == sel_rows)[sel_rows >= 0].all()     # every selected row is one of its own
    sel = np.where(sel_rows >= 0, where, -1).astype(np.int32)
    idx = torch.as_tensor(slots, dtype=torch.long, device=DEV)
    return npy(own.query_pc(sc["R"][b:b + 1, idx].contiguous(), sc["T"][b:b + 1, idx].contiguous(), sel=t(sel, device=DEV)))[0]


def test_library_layout(scene):
    pc = scene["pc"]
    assert pc.part_num == 2 + 3 and pc.num_shared == 2 and pc.pts_shared == 2 * K
    assert pc.group_off.tolist() == [0, 2 * K, 3 * K, 3 * K] and pc.max_group_points == 2 * K
    assert tuple(pc.pts.shape) == (5 * K, 3)
    assert npy(pc.part_of).reshape(-1, K)[:, 0].tolist() == [0, 1, 2, 4, 2]               # a point names its slot


def test_group_sel_cloud_equals_the_ungrouped_cloud_of_the_own_parts(scene):
    pc = scene["pc"]
    sel = pc.group_sel(generator=torch.Generator().manual_seed(11))
    assert tuple(sel.shape) == (6, K) and sel.dtype == torch.int32 and sel.is_cuda
    got = npy(pc.query_pc(scene["R"], scene["T"], sel=sel))
    assert got.shape == (6, K, 3) and np.isfinite(got).all()
    rows = npy(sel)
    for b in range(6):
        assert same_bits(got[b], own_cloud(scene, b, rows[b])), b
    assert np.array_equal(rows[0], rows[5]) and np.array_equal(rows[1], rows[4])          # one selection per object
    assert (rows[3] < pc.pts_shared).all() and (rows[2] < pc.pts_shared).all()            # nothing to draw but the shared parts
    assert (rows[0] >= pc.pts_shared).any() and (rows[1] >= pc.pts_shared).any()
    # select='random' draws such a table per call from the CPU global generator
    torch.manual_seed(5)
    a = npy(pc.query_pc(scene["R"], scene["T"]))
    used = npy(pc.last_sel)
    torch.manual_seed(5)
    assert np.array_equal(npy(pc.group_sel()), used) and same_bits(a, npy(pc.query_pc(scene["R"], scene["T"], sel=pc.last_sel)))
    assert not np.array_equal(npy(pc.group_sel()), used)                                  # the next draw differs
    # into the head of a wider row, and a slice of the environments with its own group_of
    out = torch.full((6, 3 * K + 4), -7.0, device=DEV)
    pc.query_pc(scene["R"], scene["T"], sel=sel, out=out)
    assert same_bits(npy(out[:, :3 * K]).reshape(6, K, 3), got) and bool((out[:, 3 * K:] == -7.0).all())
    torch.manual_seed(5)
    one = npy(pc.query_pc(scene["R"][4:6], scene["T"][4:6], group_of=[1, 0]))
    assert same_bits(one, a[4:6])
    # ... or with the table on the device, where an id outside [-1, G) counts as 'no object'
    torch.manual_seed(5)
    one = npy(pc.query_pc(scene["R"][4:6], scene["T"][4:6], group_of=t(np.array([1, 9], dtype=np.int32), device=DEV)))
    assert same_bits(one[0], a[4]) and same_bits(npy(pc.last_sel)[1], used[3]) and np.isfinite(one).all()


def test_all_has_nan_exactly_past_each_environments_own_points(scene):
    pc = scene["pc"]
    got = npy(pc.query_pc(scene["R"], scene["T"], select='all'))
    width = pc.pts_shared + pc.max_group_points
    assert got.shape == (6, width, 3) and pc.last_sel is not None
    for b in range(6):
        rows = pc.own_rows(int(GROUP_OF[b]))
        n = len(rows)
        assert n == [4 * K, 3 * K, 2 * K, 2 * K, 3 * K, 4 * K][b]
        assert np.isfinite(got[b, :n]).all() and np.isnan(got[b, n:]).all(), b
        sel_rows = np.concatenate([rows, np.full(width - n, -1)])
        assert same_bits(got[b], own_cloud(scene, b, sel_rows)), b
