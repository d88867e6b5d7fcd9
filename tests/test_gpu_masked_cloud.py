"""Part-mask channel of the depth and mesh clouds on the GPU: pm_depth_cloud_f32 (depth images -> compact cloud + source pixels),
pm_cloud_gather_labeled_f32 (sampled rows (x, y, z, label)), pm_mesh_pc_query_labeled_f32 (the posed mesh cloud with its part's
label) and what is built on them: TSDFVolume.depth2pc_masked, PCfromMesh.query_pc(mask=True), pc_observer / depth_pc_observer(mask=True).

Every comparison is an equality of bit patterns: the contracts fix every rounding.  Expected values come from the reference's own
world cloud (tests/golden/depth2pc_small.npz) or oracle.ref_cpu.depth2pc's, plus the plain indexing of tests/masked_cloud_ref.py; the
one step in between is masked_cloud_ref.plus_zero_rows (the reference's cropped rows carry -0.0, the kernels write +0.0).
Every cloud stays at <= 8192 points per environment, so the sampler runs on one work-group per cloud."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from tests import helpers
from tests import kinematic_episode as E
from tests import masked_cloud_ref as MC
from tests.golden import cases
from tests.helpers import GOLDEN, bits, load, npy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
t = functools.partial(helpers.t, device=DEV)
SENTINEL = -777.25
SRC_SENTINEL = -12345


# ------------------------------------------------------------------------------------------- the cases of the front end
def fixture_case():
    c = cases.DEPTH2PC_CASES["depth2pc_small"]
    inp = cases.depth2pc_inputs(c)
    return dict(depth=inp["depth"], pose=inp["cam_pose"], intr=c["intr"], size=c["size"], origin=c["vol_origin"],
                world=MC.plus_zero_rows(load("depth2pc_small")["world"]))


def seeded_case(depth, pose, intr, size, origin):
    depth, pose = np.ascontiguousarray(depth, dtype=np.float32), np.ascontiguousarray(pose, dtype=np.float32)
    world = ref_cpu.depth2pc(depth, pose, intr, size, origin, K=1, return_world=True)[1]
    return dict(depth=depth, pose=pose, intr=intr, size=size, origin=origin, world=MC.plus_zero_rows(world))


def eye_poses(m, shift=0.01):
    pose = np.tile(np.eye(4, dtype=np.float32), (m, 1, 1))
    pose[:, :3, 3] = shift * np.arange(m, dtype=np.float32)[:, None]                      # view 0: zero translation
    return pose


INTR = [[30.0, 0.0, 15.5], [0.0, 28.0, 11.5], [0.0, 0.0, 1.0]]
IN_BOX, OUT_OF_BOX = 0.5, 5.0                                 # depths inside / beyond the box (-1, -1, 0.1) .. (1, 1, 2.1)


def mixed_batch():
    """B = 5 over 2 x 24 x 32 pixels (P = 1536: a full chunk of 1024 and half of one): every pixel cropped / none cropped / the first
    cropped pixel in the second chunk / a seeded mix of the two depths / seeded depths around the far face."""
    rng = np.random.RandomState(41)
    d = np.full((5, 1536), IN_BOX, dtype=np.float32)
    d[0] = OUT_OF_BOX
    d[2, 1100:1300:3] = OUT_OF_BOX
    d[3] = np.where(rng.rand(1536) < 0.6, OUT_OF_BOX, IN_BOX)
    d[4] = rng.uniform(1.5, 2.6, size=1536)
    return seeded_case(d.reshape(5, 2, 24, 32), eye_poses(2), INTR, 2.0, [-1.0, -1.0, 0.1])


def tiny_case():
    rng = np.random.RandomState(42)
    d = np.where(rng.rand(1, 1, 5, 7) < 0.5, OUT_OF_BOX, IN_BOX)
    return seeded_case(d, eye_poses(1), [[6.0, 0.0, 3.0], [0.0, 5.0, 2.0], [0.0, 0.0, 1.0]], 2.0, [-1.0, -1.0, 0.1])


def origin_case():
    """depth = 0 under a pose without translation, in a box around the origin: those pixels are inside the box and equal to zero."""
    rng = np.random.RandomState(43)
    d = np.where(rng.rand(2, 1, 24, 32) < 0.3, 0.0, IN_BOX)
    d[1, 0, 0, :5] = IN_BOX                                   # environment 1: the first zero is not pixel 0
    return seeded_case(d, eye_poses(1), INTR, 2.0, [-1.0, -1.0, -1.0])


def two_rounds_case():
    """P = 70 x 71 = 4970 pixels: more than the 4096 the kernel takes per pair of barriers, the second round part-filled; environment
    1 meets its first cropped pixel in that second round."""
    rng = np.random.RandomState(44)
    d = np.where(rng.rand(2, 4970) < 0.5, OUT_OF_BOX, IN_BOX)
    d[1, :4500] = IN_BOX
    d[1, 4500] = OUT_OF_BOX
    return seeded_case(d.reshape(2, 1, 70, 71), eye_poses(1), [[90.0, 0.0, 35.0], [0.0, 90.0, 34.5], [0.0, 0.0, 1.0]], 2.0, [-1.0, -1.0, 0.1])


CASES = {"fixture": fixture_case, "tiny": tiny_case, "mixed": mixed_batch, "origin": origin_case, "two_rounds": two_rounds_case}
_BUILT = {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def box(c):
    lo = np.asarray(c["origin"], dtype=np.float32)
    return lo, (np.float32(c["size"]) + lo).astype(np.float32)


def cam_args(c):
    i = c["intr"]
    return (i[0][0], i[1][1], i[0][2], i[1][2]) + box(c)


def raw_depth_cloud(c, cap=None, want_src=True):
    """pm_depth_cloud_f32 into buffers filled with sentinels (ops.depth_cloud hands out fresh memory)."""
    from partmanip_amd._lib import check, lib
    depth, pose = t(c["depth"]), t(c["pose"])
    B, M, H, W = depth.shape
    cap = M * H * W if cap is None else cap
    xyz = torch.full((B, cap, 3), SENTINEL, device=DEV)
    src = torch.full((B, cap), SRC_SENTINEL, dtype=torch.int32, device=DEV) if want_src else None
    lengths = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    fx, fy, cx, cy, lo, hi = cam_args(c)
    lo3, hi3 = (ctypes.c_float * 3)(*lo.tolist()), (ctypes.c_float * 3)(*hi.tolist())
    check(lib.pm_depth_cloud_f32(depth.data_ptr(), B, M, H, W, pose.data_ptr(), fx, fy, cx, cy, ctypes.cast(lo3, ctypes.c_void_p),
                                 ctypes.cast(hi3, ctypes.c_void_p), cap, xyz.data_ptr(), 0 if src is None else src.data_ptr(),
                                 lengths.data_ptr(), torch.cuda.current_stream().cuda_stream), "pm_depth_cloud_f32")
    return npy(xyz), None if src is None else npy(src), npy(lengths)


# ------------------------------------------------------------------------------------------- 1. front end = composition
@pytest.mark.parametrize("name", list(CASES))
def test_front_end_equals_the_composition_and_the_numpy_statement(name):
    from partmanip_amd import ops
    c = case(name)
    world = c["world"]
    B, P = world.shape[:2]
    depth, pose = t(c["depth"]), t(c["pose"])
    full = ops.depth_backproject(depth, pose, *cam_args(c))
    assert np.array_equal(bits(full), bits(world))                                       # the shared arithmetic kept its bits
    comp, comp_len = (npy(a) for a in ops.depth_compact(full))
    xyz, src, lengths = raw_depth_cloud(c)
    _, clouds, srcs, want_len = MC.masked_cloud(world, np.zeros((B, P), dtype=np.int32), 1)
    assert np.array_equal(lengths, comp_len) and np.array_equal(lengths, want_len)
    for b in range(B):
        n = int(lengths[b])
        assert np.array_equal(bits(xyz[b, :n]), bits(comp[b, :n])) and np.array_equal(bits(xyz[b, :n]), bits(clouds[b])), b
        assert np.array_equal(src[b, :n], srcs[b]) and (np.diff(src[b, :n]) > 0).all(), b
        assert np.array_equal(bits(xyz[b, :n]), bits(world[b][src[b, :n]])), b
        assert (xyz[b, n:] == SENTINEL).all() and (src[b, n:] == SRC_SENTINEL).all(), b  # rows past lengths[b] are not written
    # the wrapper: the same bits in fresh buffers
    oxyz, osrc, olen = ops.depth_cloud(depth, pose, *cam_args(c))
    assert tuple(oxyz.shape) == (B, P, 3) and tuple(osrc.shape) == (B, P) and osrc.dtype == torch.int32 and np.array_equal(npy(olen), lengths)
    for b in range(B):
        n = int(lengths[b])
        assert np.array_equal(bits(oxyz[b, :n]), bits(xyz[b, :n])) and np.array_equal(npy(osrc[b, :n]), src[b, :n])
    if name == "fixture":
        assert P == 2304 and lengths.tolist() == [925, 922] and src[0, 0] == 0 and src[1, 0] == 0
    if name == "tiny":
        assert P == 35 and 1 < lengths[0] < 35
    if name == "mixed":
        zero = (world == 0).all(axis=2)
        assert lengths[0] == 1 and src[0, 0] == 0 and lengths[1] == P and not zero[1].any()
        assert int(np.argmax(zero[2])) == 1100 and 1 < lengths[3] < P and 1 < lengths[4] < P
    if name == "two_rounds":
        zero = (world == 0).all(axis=2)
        assert P == 4970 and int(np.argmax(zero[1])) == 4500 and src[1, 4500] == 4500 and 4500 < lengths[1] < P and 1 < lengths[0] < P
    if name == "origin":
        zero = (world == 0).all(axis=2)
        inside = (c["depth"].reshape(B, P) == 0)
        assert np.array_equal(zero, inside) and inside[0, 0:40].any() and int(np.argmax(zero[1])) >= 5
        assert lengths.tolist() == ((~zero).sum(axis=1) + 1).tolist()


# ------------------------------------------------------------------------------------------- 2. cap
@pytest.mark.parametrize("cap", [512, 922, 925, 2304])
def test_cap_keeps_the_first_points(cap):
    c = case("fixture")
    full_xyz, full_src, full_len = raw_depth_cloud(c)
    xyz, src, lengths = raw_depth_cloud(c, cap=cap)
    assert lengths.tolist() == [min(925, cap), min(922, cap)]
    for b in range(2):
        n = int(lengths[b])
        assert np.array_equal(bits(xyz[b, :n]), bits(full_xyz[b, :n])) and np.array_equal(src[b, :n], full_src[b, :n])
        assert (xyz[b, n:] == SENTINEL).all() and (src[b, n:] == SRC_SENTINEL).all()
    # src = NULL: the same cloud, nothing else
    xyz2, none, len2 = raw_depth_cloud(c, cap=cap, want_src=False)
    assert none is None and np.array_equal(len2, lengths) and np.array_equal(bits(xyz2), bits(xyz))
    from partmanip_amd import ops
    oxyz, osrc, olen = ops.depth_cloud(t(c["depth"]), t(c["pose"]), *cam_args(c), cap=cap, want_src=False)
    assert osrc is None and tuple(oxyz.shape) == (2, cap, 3) and np.array_equal(npy(olen), lengths)


# ------------------------------------------------------------------------------------------- 3. the labelled gather
@pytest.mark.parametrize("zero_label", [0.0, -2.5])
def test_labelled_gather_against_numpy(zero_label):
    from partmanip_amd import ops
    B, ld, K, P = 3, 50, 67, 300                              # 4 K = 268 floats: two blocks, the second part-filled
    rng = np.random.RandomState(51)
    xyz = rng.uniform(-1, 1, size=(B, ld, 3)).astype(np.float32)
    xyz[:, 7] = 0.0                                           # the zero point
    xyz[1, 9] = (0.0, 0.0, 1e-30)                             # not the zero point
    src = rng.randint(0, P, size=(B, ld)).astype(np.int32)
    src[0, 3], src[2, 11], src[1, 7] = P, -1, -1              # outside [0, P): a NaN label; the zero point's src is never read
    seg = rng.randint(-1, 12, size=(B, P)).astype(np.int32)
    seg[0, :4] = (-1, 2 ** 31 - 1, 16777217, 123456789)       # the miss label and large positives (rounded as a cast rounds)
    src[0, 20:24] = (0, 1, 2, 3)
    idx = rng.randint(0, ld, size=(B, K)).astype(np.int32)
    idx[0, :6] = (20, 21, 22, 23, 3, 7)
    idx[1, :4] = (7, 9, -1, ld)
    idx[2, :3] = (11, ld, -1)
    width = 4 * K + 7
    buf = torch.full((B, width), SENTINEL, device=DEV)
    got = ops.cloud_gather_labeled(t(xyz), t(src), t(idx), t(seg), zero_label=zero_label, out=buf)
    assert got.data_ptr() == buf.data_ptr() and bool((buf[:, 4 * K:] == SENTINEL).all())
    want = np.full((B, K, 4), np.nan, dtype=np.float32)
    for b in range(B):
        for k in range(K):
            i = idx[b, k]
            if not 0 <= i < ld:
                continue
            want[b, k, :3] = xyz[b, i]
            if (xyz[b, i] == 0).all():
                want[b, k, 3] = zero_label
            elif 0 <= src[b, i] < P:
                want[b, k, 3] = np.float32(seg[b, src[b, i]])
    g = npy(buf[:, :4 * K]).reshape(B, K, 4)
    assert np.array_equal(np.isnan(g), np.isnan(want))
    assert np.array_equal(bits(g)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    assert np.isnan(g[1, 2]).all() and np.isnan(g[1, 3]).all() and np.isnan(g[2, 1]).all()         # idx = -1 and ld: four NaN
    assert np.isnan(g[0, 4, 3]) and not np.isnan(g[0, 4, :3]).any() and np.isnan(g[2, 0, 3])       # src outside [0, P)
    assert g[0, 5, 3] == np.float32(zero_label) and g[1, 0, 3] == np.float32(zero_label) and g[1, 1, 3] == np.float32(seg[1, src[1, 9]])
    assert g[0, 0, 3] == -1.0 and g[0, 1, 3] == np.float32(2 ** 31) and g[0, 2, 3] == 16777216.0
    # seg as the images' own 4-D tensor, and a fresh result
    fresh = ops.cloud_gather_labeled(t(xyz), t(src), t(idx), t(seg.reshape(B, 3, 10, 10)), zero_label=zero_label)
    assert tuple(fresh.shape) == (B, 4 * K) and np.array_equal(bits(fresh), bits(buf[:, :4 * K]))


# ------------------------------------------------------------------------------------------- 4. end to end
@pytest.fixture(scope="module")
def fixture_volume():
    from partmanip_amd.depth2tsdf import TSDFVolume
    c = cases.DEPTH2PC_CASES["depth2pc_small"]
    inp = cases.depth2pc_inputs(c)
    vol = TSDFVolume(DEV, size=c["size"], resolution=10, _vol_origin=c["vol_origin"])
    vol.register_camera(inp["cam_pose"], np.asarray(c["intr"], dtype=np.float32), c["h"], c["w"], c["b"])
    seg = np.random.RandomState(61).randint(-1, 12, size=inp["depth"].shape).astype(np.int32)
    return vol, t(inp["depth"]), seg


@pytest.mark.parametrize("K", [64, 1024])                    # 1024: more than the 925 / 922 kept points, the lowest index repeats
def test_depth2pc_masked_end_to_end(fixture_volume, K):
    vol, depth, seg = fixture_volume
    fx = load("depth2pc_small")
    final = MC.plus_zero_rows(fx["final_pc_1024"][:, :K])
    want, _, _, _ = MC.masked_cloud(MC.plus_zero_rows(fx["world"]), seg.reshape(2, -1), K, zero_label=-1.0)
    assert np.array_equal(bits(want[..., :3]), bits(final))
    got = vol.depth2pc_masked(depth, t(seg), K=K, zero_label=-1.0)
    assert tuple(got.shape) == (2, K, 4) and got.dtype == torch.float32
    assert np.array_equal(bits(got[..., :3]), bits(vol.depth2pc(depth, K=K))) and np.array_equal(bits(got[..., :3]), bits(final))
    assert np.array_equal(bits(got), bits(want))
    assert (want[:, 0, 3] == -1.0).all() and len(np.unique(want[..., 3])) > 5
    # out = a view into a wider buffer; a cap that does not truncate
    buf = torch.full((2, 4 * K + 25), SENTINEL, device=DEV)
    res = vol.depth2pc_masked(depth, t(seg), K=K, out=buf, cap=1000, zero_label=-1.0)
    assert res.data_ptr() == buf.data_ptr() and tuple(res.shape) == (2, K, 4)
    assert np.array_equal(bits(buf[:, :4 * K]), bits(want.reshape(2, -1))) and bool((buf[:, 4 * K:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------- 5. the mesh cloud
def ref32(pts, part_of, R, T, sel):
    """numpy float32, one rounding per operation, in the contract's association; sel (K,), (B, K) or None -> (B, K, 3) and the
    parts (B, K), -1 where q is outside [0, Q) or the part outside [0, M): those points are NaN."""
    B, M = R.shape[:2]
    Q = len(pts)
    q = np.arange(Q) if sel is None else np.asarray(sel, dtype=np.int64)
    q = np.broadcast_to(q, (B, q.shape[-1]))
    okq = (q >= 0) & (q < Q)
    qc = np.where(okq, q, 0)
    p = part_of.astype(np.int64)[qc]
    ok = okq & (p >= 0) & (p < M)
    pc = np.where(ok, p, 0)
    x = pts.astype(np.float32)[qc]
    Rs = R.astype(np.float32)[np.arange(B)[:, None], pc]
    Ts = T.astype(np.float32)[np.arange(B)[:, None], pc]
    v = ((x[..., None, 0] * Rs[..., 0] + x[..., None, 1] * Rs[..., 1]) + x[..., None, 2] * Rs[..., 2]) + Ts
    assert v.dtype == np.float32
    return np.where(ok[..., None], v, np.float32(np.nan)), np.where(ok, p, -1)


def labelled(pts, part_of, R, T, sel, labels):
    v, p = ref32(pts, part_of, R, T, sel)
    lab = np.where(p >= 0, np.asarray(labels, dtype=np.float32)[np.maximum(p, 0)], np.float32(np.nan))
    return np.concatenate([v, lab[..., None].astype(np.float32)], axis=-1)


def mesh_scene(B, M, p, seed, labels):
    from partmanip_amd.mesh2pc import PCfromMesh
    from tests.mesh_tsdf_parts import random_poses
    pcs = np.random.RandomState(seed).uniform(-0.07, 0.07, size=(M, p, 3)).astype(np.float32)
    R, T = random_poses(seed + 1, B, M)
    return PCfromMesh(B, DEV, num_points=p, part_pcs=pcs, labels=labels), pcs, R, T


@pytest.mark.parametrize("M", [5, 70])                       # 70 parts: the poses are not staged in LDS
def test_masked_mesh_cloud_over_every_selection(M):
    B, p = 3, 40
    labels = np.random.RandomState(71).randint(-3, 9, size=M).astype(np.float32) + 0.5
    pc, pcs, R, T = mesh_scene(B, M, p, 170 + M, labels)
    pts, part_of = pcs.reshape(-1, 3), np.arange(M * p, dtype=np.int32) // p
    Rd, Td = t(R), t(T)
    rng = np.random.RandomState(72)
    for sel in (rng.randint(0, M * p, size=61).astype(np.int32), rng.randint(0, M * p, size=(B, 61)).astype(np.int32)):
        got = pc.query_pc(Rd, Td, sel=t(sel), mask=True)
        assert tuple(got.shape) == (B, 61, 4)
        assert np.array_equal(bits(got), bits(labelled(pts, part_of, R, T, sel, labels))), sel.shape
        assert np.array_equal(bits(got[..., :3]), bits(pc.query_pc(Rd, Td, sel=t(sel))))
    got = pc.query_pc(Rd, Td, select='all', mask=True)
    assert tuple(got.shape) == (B, M * p, 4) and np.array_equal(bits(got), bits(labelled(pts, part_of, R, T, None, labels)))
    fps_pc, _, _, _ = mesh_scene(B, M, p, 170 + M, labels)
    fps_pc.num_points = 16
    got = fps_pc.query_pc(Rd, Td, select='fps', mask=True)
    idx = npy(fps_pc.last_sel)
    full = npy(pc.query_pc(Rd, Td, select='all'))
    assert np.array_equal(idx, ref_cpu.fps(full, 16)) and np.array_equal(bits(got), bits(labelled(pts, part_of, R, T, idx, labels)))
    # into the head of a wider row at an odd stride
    buf = torch.full((B, 4 * 61 + 7), SENTINEL, device=DEV)
    sel = rng.randint(0, M * p, size=61).astype(np.int32)
    res = pc.query_pc(Rd, Td, sel=t(sel), out=buf, mask=True)
    assert res.data_ptr() == buf.data_ptr() and bool((buf[:, 4 * 61:] == SENTINEL).all())
    assert np.array_equal(bits(buf[:, :4 * 61]), bits(labelled(pts, part_of, R, T, sel, labels).reshape(B, -1)))


def test_masked_mesh_cloud_bad_indices_give_four_nan():
    from partmanip_amd import ops
    B, M, p, K = 3, 5, 40, 61
    labels = np.arange(M, dtype=np.float32) * 2 - 1
    pc, pcs, R, T = mesh_scene(B, M, p, 180, labels)
    Q = M * p
    pts, part_of = pcs.reshape(-1, 3), np.arange(Q, dtype=np.int32) // p
    sel = np.random.RandomState(73).randint(0, Q, size=(B, K)).astype(np.int32)
    bad = sel.copy()
    bad[0, 3], bad[2, 0], bad[1, K - 1] = -1, Q, Q           # one step outside, never farther
    victim = int(sel[1, 5])
    bad_part = part_of.copy()
    bad_part[victim] = M
    got = npy(ops.mesh_pc_query(pc.pts, t(bad_part), t(R), t(T), t(bad), labels=pc.labels)).reshape(B, K, 4)
    want = labelled(pts, bad_part, R, T, bad, labels)
    nan = np.isnan(want).any(axis=-1)
    assert nan[0, 3] and nan[2, 0] and nan[1, K - 1] and nan[1, 5] and np.isnan(want[nan]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])


def test_masked_mesh_cloud_of_a_grouped_scene():
    """The layout of tests/mesh_groups_scene.small_scene(): two shared parts, groups of 1, 3 and 0 bodies, six environments holding
    [0, 1, 2, -1, 1, 0] over M = 5 pose slots.  A body's label is its SLOT's: body j of whichever object sits in slot 2 + j."""
    from partmanip_amd.mesh2pc import PCfromMesh
    from tests import mesh_groups_scene as GS
    sc = GS.small_scene()
    K = 24
    rng = np.random.RandomState(74)
    cloud = lambda: rng.uniform(-0.07, 0.07, size=(K, 3)).astype(np.float32)            # noqa: E731
    shared = np.stack([cloud(), cloud()])
    groups = [[cloud()], [cloud(), cloud(), cloud()], []]
    labels = [1, 1, 7, 8, 9]
    pc = PCfromMesh(6, DEV, num_points=K, part_pcs=shared, groups=groups, group_of=sc["env_group"], labels=labels)
    assert pc.part_num == sc["M"] == 5
    pts, part_of = npy(pc.pts), npy(pc.part_of)
    sel = pc.group_sel(generator=torch.Generator().manual_seed(12))
    got = pc.query_pc(t(sc["R"]), t(sc["T"]), sel=sel, mask=True)
    assert tuple(got.shape) == (6, K, 4)
    assert np.array_equal(bits(got), bits(labelled(pts, part_of, sc["R"], sc["T"], npy(sel), labels)))
    assert np.array_equal(bits(got[..., :3]), bits(pc.query_pc(t(sc["R"]), t(sc["T"]), sel=sel)))
    lab = npy(got)[..., 3]
    assert set(lab[3].tolist()) <= {1.0} and set(lab[0].tolist()) <= {1.0, 7.0} and 7.0 in lab[0] and set(lab[1].tolist()) <= {1.0, 7.0, 8.0, 9.0}
    full = npy(pc.query_pc(t(sc["R"]), t(sc["T"]), select='all', mask=True))             # NaN rows past an environment's own points
    own = [len(pc.own_rows(int(g))) for g in sc["env_group"]]
    for b in range(6):
        assert not np.isnan(full[b, :own[b]]).any() and np.isnan(full[b, own[b]:]).all()


# ------------------------------------------------------------------------------------------- 6. the observers
def grasp_env(N, **kw):
    from partmanip_amd.envs import make_grasp_cube_env
    tree, bp, dof = E.scene()
    kw.setdefault("free_body_pose", E.CUBE_POSE)
    return make_grasp_cube_env(dict(E.CFG), N, DEV, tree, E.DT, base_pose=bp, dof=dof, **kw)


def finger():
    from partmanip_amd import meshio
    return meshio.load_mesh(os.path.join(GOLDEN, "finger.stl"))


ROBOT_MASK = [1] * 11 + [0]                                   # the reference's robot mask (hand_base.py:222-227)


def test_mesh_cloud_observer_row_is_cloud_labels_and_proprio():
    from partmanip_amd.envs import pc_observer
    from partmanip_amd.mesh2pc import PCfromMesh
    N, K = 8, 256
    pc = PCfromMesh(N, DEV, num_points=K, meshes=[finger()] * 12, labels=ROBOT_MASK)
    ob = pc_observer(pc, mask=True)
    assert ob.width == 4 * K
    env = grasp_env(N, observers={"mesh_pc": ob}, add_proprio_obs=True)
    assert env.num_obs == {"normal_state": 37, "proprio_state": 25, "mesh_pc": 4 * K + 25}
    obs = env.reset()
    rng = np.random.default_rng(0)
    want_label = pc.labels[pc.part_of[ob.sel.long()].long()]
    assert set(npy(want_label).tolist()) == {0.0, 1.0}
    for _ in range(3):
        obs, _, _, _ = env.step(t(rng.uniform(-1, 1, (N, 7)).astype(np.float32)))
        row = obs["mesh_pc"]
        assert tuple(row.shape) == (N, 4 * K + 25) and bool(torch.isfinite(row).all())
        assert torch.equal(row[:, 4 * K:], obs["proprio_state"]) and torch.equal(obs["proprio_state"][:, :7], obs["normal_state"][:, :7])
        cloud = row[:, :4 * K].view(N, K, 4)
        assert np.array_equal(bits(cloud), bits(pc.query_pc(*env.task.compute_scene_pose(), sel=ob.sel, mask=True)))
        assert np.array_equal(bits(cloud[..., :3]), bits(pc.query_pc(*env.task.compute_scene_pose(), sel=ob.sel)))
        assert torch.equal(cloud[..., 3], want_label.expand(N, K))


def test_depth_cloud_observer_row_and_a_pointnet_policy_over_it():
    from partmanip_amd import camera
    from partmanip_amd.algo_utils.actor_critic import ActorCritic
    from partmanip_amd.depth2tsdf import TSDFVolume
    from partmanip_amd.envs import depth_pc_observer
    from partmanip_amd.mesh2depth import DepthFromMesh
    N, K, im_h, im_w = 8, 64, 18, 32
    cam_pose, intr, _, _ = camera.shipped_rig({"look_at": [0.0, 0.0, 0.1], "radius": 0.6}, image_mode=True)
    intr = np.array([[intr[0][0] / 4, 0, im_w // 2], [0, intr[1][1] / 4, im_h // 2], [0, 0, 1]])      # the 128 x 72 view at a quarter
    cam = DepthFromMesh(N, DEV, cam_pose, intr, im_h, im_w, meshes=[finger()] * 12, labels=ROBOT_MASK)
    vol = TSDFVolume(DEV, 2, 50, (-1, -1, 0.0))
    vol.register_camera(cam_pose, intr, im_h, im_w, N)
    env = grasp_env(N, observers={"depth_pc": depth_pc_observer(cam, vol, num_points=K, mask=True, zero_label=-1.0)})
    assert env.num_obs["depth_pc"] == 4 * K
    env.reset()
    obs, _, _, _ = env.step(torch.zeros(N, 7, device=DEV))
    frame = cam.render_frame(*env.task.compute_scene_pose(), depth=True, seg=True, rgb=False)
    want = vol.depth2pc_masked(frame.depth, frame.seg, K=K, zero_label=-1.0)
    assert np.array_equal(bits(obs["depth_pc"]), bits(want.reshape(N, -1)))
    assert np.array_equal(bits(want[..., :3]), bits(vol.depth2pc(frame.depth, K=K)))
    assert set(npy(want[..., 3]).reshape(-1).tolist()) <= {-1.0, 0.0, 1.0}               # the zero point, the cube, the robot
    model = dict(action_std=0.5, action_activate="tanh", clipAction=1.0,
                 network=dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=True, point_num=K))
    policy = ActorCritic(env.num_obs["depth_pc"], env.num_actions, model).to(DEV)
    act = policy.act(obs["depth_pc"])
    assert tuple(act.shape) == (N, env.num_actions) and bool(torch.isfinite(act).all())
