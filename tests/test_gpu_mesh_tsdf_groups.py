"""The grouped mesh-TSDF on the GPU: every environment samples the shared grids and its own cabinet's (pm_mesh_tsdf_query_groups_f32,
ops.mesh_tsdf_query_groups, TSDFfromMesh(groups=)).  Every check is an equality of bit patterns: the grouped volume of an
environment is DEFINED as what pm_mesh_tsdf_query_f32 gives for that environment's own rows (B = 1), and that entry is pinned
against the reference by tests/test_gpu_mesh_tsdf.py.  The fp64 restatement (tests/mesh_tsdf_parts.restate, on the CPU) only shows
that the scenes exercise what they claim to: own rows change 21 to 43 % of the voxels of the small scene's environments that have
any, and every row at an ordinal >= 64 of the boundary scene changes at least 29 voxels."""
import numpy as np
import pytest
import torch

from tests import mesh_groups_scene as S
from tests import mesh_tsdf_parts as P
from tests.helpers import npy, same_bits, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES, SIZE = S.RES, S.SIZE
N3 = RES ** 3
VOX = SIZE / RES
TRUNC = 4 * VOX
i32 = lambda a: t(np.asarray(a, dtype=np.int32), device=DEV)                             # noqa: E731


class Lib:
    """A scene's grid library on the device, through TSDFfromMesh's own merge (un-padded grids, one flat buffer)."""

    def __init__(self, sc):
        from partmanip_amd.mesh2sdf import TSDFfromMesh
        self.sc = sc
        self.obj = TSDFfromMesh(1, SIZE, RES, DEV, sdf_dicts=sc["parts"])
        o = self.obj
        self.tables = (o.sdf_field, o.sdf_field_off, o.sdf_field_res, o.sdf_bbox_min, o.sdf_voxel_size)
        self.ground = o._ground
        self.origin = o._origin3
        self.R, self.T = t(sc["R"], device=DEV), t(sc["T"], device=DEV)

    def grouped(self, R=None, T=None, base=None, grid_slot=None, group_off=None, env_group=None, NG_shared=None, **kw):
        from partmanip_amd import ops
        sc = self.sc
        return ops.mesh_tsdf_query_groups(*self.tables, sc["grid_slot"] if grid_slot is None else grid_slot,
                                          sc["NG_shared"] if NG_shared is None else NG_shared,
                                          sc["group_off"] if group_off is None else group_off,
                                          sc["env_group"] if env_group is None else env_group, self.R if R is None else R,
                                          self.T if T is None else T, RES, VOX, self.origin, TRUNC, self.ground if base is None else base, **kw)

    def subset(self, b, rows, base=None, R=None, T=None, brick_skip=True):
        """pm_mesh_tsdf_query_f32 with B = 1 on the rows `rows` of the library as its parts (the flat buffer is shared: a row keeps
        its offset), each with the pose of the slot it names; an empty row list is clamp(base / trunc)."""
        from partmanip_amd import ops
        base = self.ground if base is None else base
        if len(rows) == 0:
            return torch.clamp((base if base.dim() == 1 else base[0]) / TRUNC, -1, 1).reshape(1, N3)
        rows_t = torch.as_tensor(rows, dtype=torch.long, device=DEV)
        slots = torch.as_tensor(self.sc["grid_slot"][rows], dtype=torch.long, device=DEV)
        R, T = self.R if R is None else R, self.T if T is None else T
        f, off, shp, mn, vs = self.tables
        return ops.mesh_tsdf_query(f, off[rows_t].contiguous(), shp[rows_t].contiguous(), mn[rows_t].contiguous(), vs[rows_t].contiguous(),
                                   R[b:b + 1, slots].contiguous(), T[b:b + 1, slots].contiguous(), RES, VOX, self.origin, TRUNC, base,
                                   brick_skip=brick_skip)

    def want(self, env_group=None, brick_skip=True, **kw):
        B = len(self.sc["R"])
        return np.concatenate([npy(self.subset(b, S.own_rows(self.sc, b, env_group, **kw), brick_skip=brick_skip)) for b in range(B)])


@pytest.fixture(scope="module")
def small():
    lib = Lib(S.small_scene())
    lib.ref = lib.want()
    lib.ref.setflags(write=False)
    return lib


@pytest.fixture(scope="module")
def boundary():
    return Lib(S.boundary_scene())


# ------------------------------------------------------------------------------------------- 1. equality on own subsets
@pytest.mark.parametrize("brick_skip", [True, False])
def test_every_environment_equals_the_ungrouped_entry_on_its_own_rows(small, brick_skip):
    got = npy(small.grouped(brick_skip=brick_skip))
    assert got.shape == (6, N3)
    assert same_bits(got, small.want(brick_skip=brick_skip)) and same_bits(got, small.ref)
    shared_only = small.want(env_group=np.full(6, -1))
    for b, g in enumerate(small.sc["env_group"]):
        changed = (got[b] != shared_only[b]).mean()
        print(f"environment {b} (group {g}): own rows change {100 * changed:.1f} % of the voxels")
        if g in (0, 1):
            assert changed >= 0.05, b                         # otherwise the equality above shows nothing
        else:
            assert same_bits(got[b], shared_only[b]), b       # the empty group and 'no group'
    assert same_bits(npy(small.grouped(brick_skip=brick_skip)), got)                      # the bits repeat


# ------------------------------------------------------------------------------------------- 2. the 64-ordinal boundary
@pytest.mark.parametrize("brick_skip", [True, False])
def test_a_group_that_straddles_the_ballots_64_lanes(boundary, brick_skip):
    sc = boundary.sc
    assert sc["NG_shared"] == 63 and sc["M"] == 66 and S.own_rows(sc, 0)[63:] == [63, 64, 65]
    got = npy(boundary.grouped(brick_skip=brick_skip))
    assert same_bits(got, boundary.want(brick_skip=brick_skip))
    assert same_bits(got[3], npy(boundary.subset(3, list(range(63))))[0])
    for b in range(3):
        rows = S.own_rows(sc, b)
        full = S.restate_own(sc, b)
        for tt in range(63, len(rows)):
            without = [r for r in rows if r != rows[tt]]
            n64 = int((np.abs(S.restate_own(sc, b, rows=without) - full) > 1e-3).sum())
            n_gpu = int((npy(boundary.subset(b, without))[0] != got[b]).sum())
            print(f"environment {b}: ordinal {tt} (row {rows[tt]}) changes {n64} voxels in fp64, {n_gpu} on the device")
            assert n64 >= 1 and n_gpu >= 1, (b, tt)
    # ordinal ranges on both sides of the boundary
    for t0, t1 in ((0, 64), (64, 66), (63, 65), (65, 66)):
        want = np.concatenate([npy(boundary.subset(b, S.own_rows(sc, b, t0=t0, t1=t1))) for b in range(4)])
        assert same_bits(npy(boundary.grouped(t0=t0, t1=t1, brick_skip=brick_skip)), want), (t0, t1)


# ------------------------------------------------------------------------------------------- 3. NaN poses
def test_a_nan_pose_counts_only_in_a_slot_an_own_row_names(small):
    R, T = small.R.clone(), small.T.clone()
    R[0, 3:] = float("nan")                                   # environment 0 holds group 0: slots 0, 1, 2
    T[5, 4, 1] = float("inf")
    R[3, 2:] = float("nan")                                   # environment 3 holds nothing: slots 0, 1
    T[3, 2:] = float("nan")
    R[2, 2:] = float("nan")                                   # environment 2 holds the empty group
    assert same_bits(npy(small.grouped(R=R, T=T)), small.ref)
    assert same_bits(npy(small.grouped(R=R, T=T, brick_skip=False)), small.ref)
    for slot, where in ((2, "R"), (0, "T")):
        R, T = small.R.clone(), small.T.clone()
        (R if where == "R" else T)[0, slot].view(-1)[1] = float("nan")
        for kw in ({}, {"t0": 1, "t1": 2}, {"brick_skip": False}):     # whatever the ordinal range is
            got = npy(small.grouped(R=R, T=T, **kw))
            assert np.isnan(got[0]).all() and not np.isnan(got[1:]).any(), (slot, kw)
            if not kw:
                assert same_bits(got[1:], small.ref[1:])


# ------------------------------------------------------------------------------------------- 4. the class
@pytest.fixture(scope="module")
def tsdf(small):
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    p = small.sc["parts"]
    return TSDFfromMesh(6, SIZE, RES, DEV, sdf_dicts=p[:2], groups=[[p[2]], [p[3], p[4], p[5]], []], group_of=small.sc["env_group"])


def test_class_is_one_launch_of_the_grouped_entry(small, tsdf):
    from partmanip_amd import ops
    assert tsdf.part_num == 5 and tsdf.num_shared == 2 and tsdf.max_group_grids == 3
    assert tsdf.grid_slot.tolist() == small.sc["grid_slot"].tolist() and tsdf.group_off.tolist() == small.sc["group_off"].tolist()
    ops.TIMER.enable("mesh_tsdf_query_groups", "mesh_tsdf_query")
    try:
        vol = tsdf.query_tsdf(small.R, small.T)
        torch.cuda.synchronize()
        assert len(ops.TIMER.events.get("mesh_tsdf_query_groups", ())) == 1 and not ops.TIMER.events.get("mesh_tsdf_query")
    finally:
        ops.TIMER.disable()
    assert tuple(vol.shape) == (6, RES, RES, RES) and same_bits(npy(vol).reshape(6, -1), small.ref)
    # a slice of the environments with its own group_of, on the host and on the device
    one = tsdf.query_tsdf(small.R[4:6], small.T[4:6], group_of=[1, 0])
    assert same_bits(npy(one).reshape(2, -1), small.ref[4:6])
    one = tsdf.query_tsdf(small.R[1:2], small.T[1:2], group_of=tsdf._group_of[1:2])
    assert same_bits(npy(one).reshape(1, -1), small.ref[1:2])


def test_separate_volumes_min_is_the_whole(small, tsdf):
    scene, obj = tsdf.query_tsdf_seperately(small.R, small.T)
    whole = tsdf.query_tsdf(small.R, small.T)
    assert torch.equal(torch.minimum(scene, obj), whole) and same_bits(npy(whole).reshape(6, -1), small.ref)
    shared_only = small.want(env_group=np.full(6, -1))
    assert same_bits(npy(scene).reshape(6, -1), shared_only)
    ground = npy(torch.clamp(small.ground / TRUNC, -1, 1))
    assert same_bits(npy(obj[3]).reshape(-1), ground) and same_bits(npy(obj[2]).reshape(-1), ground)
    assert not same_bits(npy(obj[1]).reshape(-1), ground)


# ------------------------------------------------------------------------------------------- 5. other inputs
def test_a_base_per_environment_after_initialize_sdf(small, tsdf):
    pred = P.seeded_pred(3104, B=6, res=RES, size=SIZE)
    try:
        tsdf.initialize_sdf(t(pred, device=DEV))
        base = tsdf._init_base
        assert tuple(base.shape) == (6, N3)
        got = npy(tsdf.query_tsdf(small.R, small.T)).reshape(6, -1)
        want = np.concatenate([npy(small.subset(b, S.own_rows(small.sc, b), base=base[b:b + 1].contiguous())) for b in range(6)])
        assert same_bits(got, want) and not same_bits(got, small.ref)
        # the separate volumes: the shared rows against that base, the own rows against the ground plane as before
        scene, obj = tsdf.query_tsdf_seperately(small.R, small.T)
        want = np.concatenate([npy(small.subset(b, [0, 1], base=base[b:b + 1].contiguous())) for b in range(6)])
        assert same_bits(npy(scene).reshape(6, -1), want)
        want = np.concatenate([npy(small.subset(b, S.own_rows(small.sc, b)[2:])) for b in range(6)])
        assert same_bits(npy(obj).reshape(6, -1), want)
    finally:
        tsdf._init_base = tsdf._ground


def test_out_into_a_wider_row_leaves_the_tail_alone(small, tsdf):
    rows = torch.full((6, N3 + 5), -7.0, device=DEV)
    vol = tsdf.query_tsdf(small.R, small.T, out=rows[:, :N3 + 2])
    assert vol.data_ptr() == rows.data_ptr()
    assert same_bits(npy(rows[:, :N3]), small.ref) and bool((rows[:, N3:] == -7.0).all())
    rows.fill_(-7.0)
    small.grouped(out=rows)
    assert same_bits(npy(rows[:, :N3]), small.ref) and bool((rows[:, N3:] == -7.0).all())


def test_tables_on_the_device_with_a_larger_bound(small):
    sc = small.sc
    for most in (3, 40):
        got = small.grouped(grid_slot=i32(sc["grid_slot"]), group_off=i32(sc["group_off"]), env_group=i32(sc["env_group"]), max_group_grids=most)
        assert same_bits(npy(got), small.ref), most
    with pytest.raises(ValueError, match="max_group_grids"):
        small.grouped(group_off=i32(sc["group_off"]), env_group=i32(sc["env_group"]))
    # a bound below the largest group: the first rows of the group
    got = small.grouped(group_off=i32(sc["group_off"]), env_group=i32(sc["env_group"]), max_group_grids=2)
    assert same_bits(npy(got), small.want(max_group_grids=2)) and not same_bits(npy(got)[1], small.ref[1])


def test_bad_tables_on_the_device_are_handled_as_stated(small):
    """Host tables are validated by the wrapper; device tables are not read there, so the kernel cuts them: a group id outside
    [-1, G) owns the shared rows only, offsets are cut to [0, NG - NG_shared], a row whose grid_slot lies outside [0, M) is not
    sampled (and its pose neither read nor examined).  Each case against the equivalent valid tables."""
    sc = small.sc
    ids = np.array([7, 1, -5, 2 ** 31 - 1, 1, 0], dtype=np.int32)
    got = small.grouped(group_off=i32(sc["group_off"]), env_group=i32(ids), max_group_grids=3)
    assert same_bits(npy(got), small.want(env_group=np.array([-1, 1, -1, -1, 1, 0])))
    # offsets below 0 and past the library: group 0 becomes rows [2, 3), group 1 rows [3, 6)
    got = small.grouped(group_off=i32([-9, 1, 10 ** 6]), env_group=i32([0, 1, 1, -1, 1, 0]), max_group_grids=9)
    clamped = dict(sc, group_off=np.array([0, 1, 4], dtype=np.int32))
    want = np.concatenate([npy(small.subset(b, S.own_rows(clamped, b, np.array([0, 1, 1, -1, 1, 0])))) for b in range(6)])
    assert same_bits(npy(got), want)
    # row 4 (ordinal 3 of group 1) names a slot that does not exist: the scene without that row; a NaN pose where it pointed is not seen
    for bad in (5, -1, 2 ** 31 - 1):
        slot = sc["grid_slot"].copy()
        slot[4] = bad
        want = np.concatenate([npy(small.subset(b, [r for r in S.own_rows(sc, b) if r != 4])) for b in range(6)])
        for skip in (True, False):
            got = small.grouped(grid_slot=i32(slot), brick_skip=skip)
            assert same_bits(npy(got), want), (bad, skip)
    assert not same_bits(want[1], small.ref[1])
    # G = 0: a one-entry offset table, every id out of range
    got = small.grouped(group_off=i32([0]), env_group=i32(sc["env_group"]), max_group_grids=0, NG_shared=6,
                        grid_slot=i32([0, 1, 2, 2, 3, 4]))
    want = np.concatenate([npy(small.subset(b, list(range(6)))) for b in range(6)])
    assert same_bits(npy(got), want)


def test_timing_tool_tiny_run_asserts_grouped_equals_all_in_one():
    """tools/time_drawer_tsdf.py at its smallest size, in this process: the grouped volume equals the all-in-one scene of the
    ungrouped entry (absent cabinets parked far away by finite poses), which the tool itself asserts before it reports a ratio."""
    from tools import time_drawer_tsdf as tool
    row, = tool.scene_rows([4], True)
    assert row["same_bits"] and row["finite"] and row["cloud_finite"] and row["voxels_changed_by_the_cabinets"] > 0.01
    assert row["grouped_ms"] > 0 and row["all_in_one_ms"] > 0 and row["parts_per_env_all_in_one"] == 3 + 6


def test_wrapper_refuses_bad_host_tables(small):
    sc = small.sc
    with pytest.raises(ValueError, match="group_off"):
        small.grouped(group_off=[0, 1, 3, 5])
    with pytest.raises(ValueError, match="env_group"):
        small.grouped(env_group=[0, 1, 3, -1, 1, 0])
    with pytest.raises(ValueError, match="grid_slot"):
        small.grouped(grid_slot=[0, 1, 2, 2, 5, 4])
    with pytest.raises(ValueError, match="NG_shared"):
        small.grouped(NG_shared=7)
    with pytest.raises(ValueError, match="t0, t1"):
        small.grouped(t0=2, t1=6)
    with pytest.raises(ValueError, match="t0, t1"):
        small.grouped(t0=3, t1=3)


def test_every_einval_condition_is_refused_before_a_launch():
    """Any non-NULL pointer will do: a call that is refused launches and reads nothing."""
    from partmanip_amd._lib import lib
    one = 1
    good = dict(fields=one, part_off=one, part_shape=one, part_bbox_min=one, part_voxel_size=one, grid_slot=one, NG=6, NG_shared=2,
                group_off=one, G=3, env_group=one, max_group_grids=3, pose_R=one, pose_T=one, B=6, M=5, t0=0, t1=5, res=10,
                vox_size=0.05, ox=0.0, oy=0.0, oz=0.0, sdf_trunc=0.2, base=one, base_per_env=0, out=one, out_stride=1000,
                brick_skip=1, stream=None)
    call = lambda **kw: lib.pm_mesh_tsdf_query_groups_f32(*dict(good, **kw).values())    # noqa: E731
    for name in ("fields", "part_off", "part_shape", "part_bbox_min", "part_voxel_size", "grid_slot", "pose_R", "pose_T", "base", "out",
                 "group_off", "env_group"):
        assert call(**{name: None}) == -1, name
    for kw in (dict(B=0), dict(B=65536), dict(M=0), dict(NG=0), dict(NG_shared=-1), dict(NG_shared=7), dict(G=-1), dict(max_group_grids=-1),
               dict(t0=-1), dict(t0=5), dict(t0=3, t1=3), dict(t1=6), dict(t1=2 ** 31 - 1), dict(res=0), dict(res=1025), dict(out_stride=999),
               dict(sdf_trunc=0.0), dict(sdf_trunc=-1.0)):
        assert call(**kw) == -1, kw
    assert call(group_off=None, env_group=None, G=1) == -1                                # NULL group tables pass with G = 0 only
