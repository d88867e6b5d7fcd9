"""Part-mask channel of the depth and mesh clouds, everything that needs no GPU: the numpy statement of the masked depth cloud
(tests/masked_cloud_ref.py) against the reference's own data, the argument checks of the new wrappers (raised before any launch: the
tensors here live on the CPU, so a check that came late would surface as the 'no CPU fallback' error instead), the observers' widths
and the three entry points in the header and the ctypes table."""
import ctypes

import numpy as np
import pytest
import torch

from tests import masked_cloud_ref as MC
from tests.golden import cases
from tests.helpers import load
from tests.test_capi_symbols import header_functions

NEW = ("pm_depth_cloud_f32", "pm_cloud_gather_labeled_f32", "pm_mesh_pc_query_labeled_f32")


# ------------------------------------------------------------------------------------------- 1. the numpy statement
def test_numpy_statement_reproduces_the_reference_cloud():
    """Compact (non-zero rows + the first zero row), sample, gather: the xyz columns are the reference's final cloud, bit for bit."""
    fx = load("depth2pc_small")
    world = fx["world"]
    assert world.shape == (2, 2304, 3) and world.dtype == np.float32
    seg = np.random.RandomState(1).randint(-1, 12, size=(2, 2304)).astype(np.int32)
    rows, clouds, srcs, lengths = MC.masked_cloud(world, seg, 64, zero_label=-2.5)
    assert lengths.tolist() == [925, 922] and srcs[0][0] == 0 and srcs[1][0] == 0
    assert np.array_equal(rows[..., :3].view(np.uint32), fx["final_pc_1024"][:, :64].view(np.uint32))
    for b in range(2):
        assert (np.diff(srcs[b]) > 0).all() and np.array_equal(clouds[b], world[b][srcs[b]])
        zero = (rows[b, :, :3] == 0).all(axis=1)
        assert zero[0] and (rows[b, zero, 3] == np.float32(-2.5)).all()                  # FPS starts at index 0: the zero point
        # every other label is seg at a pixel whose world point is the row's
        for k in np.flatnonzero(~zero)[:8]:
            hits = np.flatnonzero((world[b] == rows[b, k, :3]).all(axis=1))
            assert rows[b, k, 3] in seg[b][hits].astype(np.float32)
    # K beyond the kept count: the lowest index repeats
    idx = MC.sample(clouds[1][:5], 9)
    assert sorted(idx[:5].tolist()) == [0, 1, 2, 3, 4] and idx[5:].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------- 2. argument checks before the device
def test_depth_cloud_rejects_bad_arguments_before_any_launch():
    from partmanip_amd import ops
    depth, pose = torch.ones(2, 3, 4, 5), torch.eye(4).repeat(3, 1, 1)
    args = (30.0, 28.0, 2.0, 1.5, [-1, -1, -1], [1, 1, 1])
    for bad_depth in (depth[0], depth.double(), depth[:, :, :, ::2], torch.ones(2, 3, 0, 5)):
        with pytest.raises(ValueError, match="depth"):
            ops.depth_cloud(bad_depth, pose, *args)
    for bad_pose in (pose[:2], pose[:, :3], pose.double()):
        with pytest.raises(ValueError, match="cam_pose"):
            ops.depth_cloud(depth, bad_pose, *args)
    for cap in (0, -3):
        with pytest.raises(ValueError, match="cap"):
            ops.depth_cloud(depth, pose, *args, cap=cap)
    with pytest.raises(ValueError, match="lo, hi"):
        ops.depth_cloud(depth, pose, 30.0, 28.0, 2.0, 1.5, [-1, -1], [1, 1, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_cloud(depth, pose, *args)


def test_cloud_gather_labeled_rejects_bad_arguments_before_any_launch():
    from partmanip_amd import ops
    B, ld, K, P = 2, 10, 4, 60
    xyz, src = torch.zeros(B, ld, 3), torch.zeros(B, ld, dtype=torch.int32)
    idx, seg = torch.zeros(B, K, dtype=torch.int32), torch.zeros(B, 3, 4, 5, dtype=torch.int32)
    for bad in (xyz[0], torch.zeros(B, ld, 4), xyz.double()):
        with pytest.raises(ValueError, match="xyz"):
            ops.cloud_gather_labeled(bad, src, idx, seg)
    for bad in (src.long(), src[:, :9], src[:1]):
        with pytest.raises(ValueError, match="src"):
            ops.cloud_gather_labeled(xyz, bad, idx, seg)
    for bad in (idx.long(), idx[:1], idx[0], idx[:, :0]):
        with pytest.raises(ValueError, match="idx"):
            ops.cloud_gather_labeled(xyz, src, bad, seg)
    for bad in (seg.float(), seg[:1], seg.view(B, P)[:, ::2], seg[:, :, :, :3]):
        with pytest.raises(ValueError, match="seg"):
            ops.cloud_gather_labeled(xyz, src, idx, bad)
    for bad in (torch.empty(B, 4 * K - 1), torch.empty(B * 4 * K), torch.empty(B + 1, 4 * K), torch.empty(B, 4 * K, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out"):
            ops.cloud_gather_labeled(xyz, src, idx, seg, out=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cloud_gather_labeled(xyz, src, idx, seg, out=torch.empty(B, 4 * K + 7))


def test_entry_points_reject_bad_arguments_before_any_launch():
    from partmanip_amd._lib import lib
    p = ctypes.c_void_p(64)                                  # never dereferenced: every call below fails validation first
    box = (ctypes.c_float * 3)(0, 0, 0)

    def cloud(depth=p, B=2, M=3, H=4, W=5, pose=p, lo=box, hi=box, cap=60, xyz=p, src=p, lengths=p):
        return lib.pm_depth_cloud_f32(depth, B, M, H, W, pose, 1.0, 1.0, 0.0, 0.0, ctypes.cast(lo, ctypes.c_void_p) if lo else None,
                                      ctypes.cast(hi, ctypes.c_void_p) if hi else None, cap, xyz, src, lengths, None)
    for kw in (dict(depth=None), dict(pose=None), dict(lo=None), dict(hi=None), dict(xyz=None), dict(lengths=None), dict(B=0), dict(M=0),
               dict(H=0), dict(W=-1), dict(cap=0), dict(M=4, H=1 << 15, W=1 << 14)):
        assert cloud(**kw) == -1, kw

    def gather(xyz=p, src=p, B=2, ld=10, idx=p, K=4, seg=p, seg_stride=60, P=60, out=p, out_stride=16):
        return lib.pm_cloud_gather_labeled_f32(xyz, src, B, ld, idx, K, seg, seg_stride, P, 0.0, out, out_stride, None)
    for kw in (dict(xyz=None), dict(src=None), dict(idx=None), dict(seg=None), dict(out=None), dict(B=0), dict(ld=0), dict(K=0), dict(P=0),
               dict(out_stride=15), dict(seg_stride=59)):
        assert gather(**kw) == -1, kw

    def mesh(labels=p, out_stride=64, K=16, sel=p):
        return lib.pm_mesh_pc_query_labeled_f32(p, p, 128, p, p, 2, 3, sel, 0, K, p, out_stride, labels, None)
    assert mesh(labels=None) == -1 and mesh(out_stride=63) == -1 and mesh(K=0) == -1 and mesh(sel=None) == -1


def test_labels_mask_and_out_checks_of_the_mesh_cloud():
    from partmanip_amd.mesh2pc import PCfromMesh, random_poses
    pcs = load("mesh_pc_ref_small")["part_pcs"]                                          # (12, 64, 3)
    pc = PCfromMesh(3, "cpu", num_points=64, part_pcs=pcs)
    assert pc.labels.dtype == torch.float32 and pc.labels.tolist() == [float(i) for i in range(12)]      # None: the slot index
    robot = PCfromMesh(3, "cpu", num_points=64, part_pcs=pcs, labels=[1] * 11 + [0])
    assert robot.labels.tolist() == [1.0] * 11 + [0.0]
    assert PCfromMesh(3, "cpu", num_points=64, part_pcs=pcs, labels=np.linspace(0, 1, 12)).labels.dtype == torch.float32
    for bad in ([1] * 11, np.zeros((12, 1)), ["a"] * 12, [True] * 12):
        with pytest.raises(ValueError, match="labels"):
            PCfromMesh(3, "cpu", num_points=64, part_pcs=pcs, labels=bad)
    R, T = random_poses(3, 12, torch.Generator().manual_seed(1), "cpu")
    sel = torch.arange(64, dtype=torch.int32)
    for bad_out in (torch.empty(3, 3 * 64), torch.empty(3, 4 * 64 - 1), torch.empty(2, 4 * 64), torch.empty(3 * 4 * 64)):
        with pytest.raises(ValueError, match="out"):
            pc.query_pc(R, T, sel=sel, out=bad_out, mask=True)                           # 3K columns do for mask=False only
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.query_pc(R, T, sel=sel, out=torch.empty(3, 3 * 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.query_pc(R, T, sel=sel, out=torch.empty(3, 4 * 64 + 25), mask=True)


def test_depth2pc_masked_checks_before_the_device():
    from partmanip_amd.depth2tsdf import TSDFVolume
    c = cases.DEPTH2PC_CASES["depth2pc_small"]
    inp = cases.depth2pc_inputs(c)
    vol = TSDFVolume("cpu", size=c["size"], resolution=10, _vol_origin=c["vol_origin"])
    vol.register_camera(inp["cam_pose"], np.asarray(c["intr"], dtype=np.float32), c["h"], c["w"], c["b"])
    depth = torch.from_numpy(inp["depth"])
    seg = torch.zeros(depth.shape, dtype=torch.int32)
    with pytest.raises(ValueError, match="depth_im"):
        vol.depth2pc_masked(depth[:1], seg[:1])
    for bad in (seg.long(), seg[:, :2], seg.transpose(2, 3).contiguous().transpose(2, 3), None):
        with pytest.raises(ValueError, match="seg"):
            vol.depth2pc_masked(depth, bad)
    with pytest.raises(ValueError, match="K"):
        vol.depth2pc_masked(depth, seg, K=0)
    for bad_out in (torch.empty(2, 4 * 64 - 1), torch.empty(3, 4 * 64), torch.empty(2, 64, 4)):
        with pytest.raises(ValueError, match="out"):
            vol.depth2pc_masked(depth, seg, K=64, out=bad_out)
    with pytest.raises(ValueError, match="cap"):
        vol.depth2pc_masked(depth, seg, K=64, cap=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.depth2pc_masked(depth, seg, K=64, out=torch.empty(2, 4 * 64 + 25))


# ------------------------------------------------------------------------------------------- 3. the observers
def test_observer_widths():
    from partmanip_amd.envs import depth_pc_observer, pc_observer
    from partmanip_amd.mesh2pc import PCfromMesh
    pc = PCfromMesh(3, "cpu", num_points=64, part_pcs=load("mesh_pc_ref_small")["part_pcs"])
    assert pc_observer(pc).width == 3 * 64 and pc_observer(pc, mask=True).width == 4 * 64
    sel = torch.arange(40, dtype=torch.int32)
    ob = pc_observer(pc, sel=sel, mask=True)
    assert ob.width == 160 and ob.sel is sel
    cam = vol = object()                                     # only the write touches them
    assert depth_pc_observer(cam, vol).width == 3 * 1024 and depth_pc_observer(cam, vol, num_points=64).width == 192
    assert depth_pc_observer(cam, vol, mask=True).width == 4 * 1024
    assert depth_pc_observer(cam, vol, num_points=64, mask=True, zero_label=-1.0).width == 256


# ------------------------------------------------------------------------------------------- 4. the ABI
def test_abi_version_stays_and_the_three_entry_points_are_declared():
    from partmanip_amd import _lib
    fns = header_functions()
    assert _lib.ABI_VERSION == 163 and _lib.lib.pm_version() == 163
    for name, nargs in zip(NEW, (17, 13, 14)):
        assert fns[name] == ("int", nargs) and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(_lib.lib, name), name
