"""The swept contact test on the GPU (pm_articulation_sweep_f32 / pm_articulation_sweep_groups_f32, ops.articulation_sweep,
Articulation.sweep).  The entry is DEFINED as a composition of existing entries, so every check is an equality of bit patterns:
sweep_dist[:, k] against Articulation.forward at the numpy float32 candidate q_k, then ops.body_pose_gather, then the sensor's body
distances; steps against the numpy rule on the kernel's own distances; targets_out against the numpy candidates.

Shapes: N = 3, the golden Franka (13 bodies, 9 DOFs), three sensing bodies of 128 points (a 64-point chunk boundary inside every
segment), the 5 cm cube's grid at pose slot 11 of the task's twelve; S in {1, 4, 8}.  The grouped scene is
tests/test_gpu_mesh_sdf_points.py's: 5 pose slots, groups of 1 and 3 rows and an environment that holds none; S in {1, 4, 8} too."""
import numpy as np
import pytest
import torch

from tests import contact_episode as CE
from tests import guarded_step_ref as GS
from tests import kinematic_episode as E
from tests import kinematics_ref as K
from tests import mesh_tsdf_parts as P
from tests.helpers import npy, same_bits, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3
DT = np.float32(E.DT)
MARGIN = 0.004


def dev(a, dtype=None):
    return t(a, dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def fx():
    """The Franka, the contact episode's sensor and seeded states: every environment's target configuration brings the right finger
    to within a centimetre of a cube of its own, from a joint state a few centimetres away (joint steps of up to 0.08 rad)."""
    from partmanip_amd.contact import ContactSensor
    from partmanip_amd.envs import guard_slot_body
    from partmanip_amd.kinematics import Articulation
    from partmanip_amd.mesh2pc import PCfromMesh
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    tree, bp, dof0 = E.scene()
    nb, nd = tree.num_bodies, tree.num_dofs
    art = Articulation(tree, N, DEV)
    tsdf = TSDFfromMesh(N, 0.5, 10, DEV, sdf_dicts=CE.grids())
    pc = PCfromMesh(N, DEV, num_points=CE.POINTS, part_pcs=CE.part_clouds())
    sensor = ContactSensor.from_cloud(tsdf, pc, CE.SLOTS, targets=(CE.CUBE_SLOT, CE.CUBE_SLOT + 1), names=CE.NAMES)
    part_body, part_C = CE.part_tables(nb + 1)
    slot_body = guard_slot_body(nb, part_body=part_body)
    assert slot_body.tolist() == list(range(10)) + [11, -1]
    rng = np.random.RandomState(7301)
    lo, hi = np.float32(tree.lower), np.float32(tree.upper)
    q = np.clip(np.float32(dof0)[None] + rng.uniform(-0.1, 0.1, size=(N, nd)), lo, hi).astype(np.float32)
    tg = (q + rng.uniform(-0.08, 0.08, size=(N, nd))).astype(np.float32)
    tg[:, -2:] = q[:, -2:] + rng.uniform(-0.01, 0.01, size=(N, 2)).astype(np.float32)          # the two finger joints are prismatic
    tg[0, 1] = hi[1] + 0.5                                     # one target beyond a joint limit
    kw = tree.robot_kwargs()
    end = K.fk(tree, K.clamp(tg, lo, hi).astype(np.float64), np.zeros((N, nd)), np.float32(bp).astype(np.float64))
    R = P.random_poses(7302, N, 12)[0]
    T = rng.uniform(-1, 1, size=(N, 12, 3)).astype(np.float32)
    R[:, :11], T[:, :11] = np.nan, np.nan                      # the robot's slots of the table are never read
    T[:, 11] = (end["pos"][:, kw["rtip_rb_index"]] + rng.uniform(-0.012, 0.012, size=(N, 3))).astype(np.float32)
    vmax = np.full(nd, 2.5, dtype=np.float32)                  # 2.5 rad/s * dt = 0.042: it binds for some joints and not for others
    return dict(tree=tree, art=art, sensor=sensor, tsdf=tsdf, base=dev(np.float32(bp)), lo=lo, hi=hi, q=q, tg=tg, R=R, T=T, vmax=vmax,
                slot_body=slot_body, slot_C=dev(part_C), nb=nb, nd=nd)


def state(q):
    s = np.zeros(q.shape + (2,), dtype=np.float32)
    s[..., 0] = q
    s[..., 1] = 0.25                                           # a velocity the sweep must not look at
    return dev(s)


def sweep(fx, S, q=None, tg=None, R=None, T=None, reset=None, free=None, vmax=None, cull=True, rows=slice(None), sensor=None, slot_body=None,
          margin=MARGIN, **kw):
    s = fx["sensor"] if sensor is None else sensor
    pick = lambda a, d: (d if a is None else a)[rows]         # noqa: E731
    flag = lambda a: None if a is None else dev(np.asarray(a, dtype=bool)[rows])        # noqa: E731
    tables, Rd, Td, groups = s.tsdf._point_tables(dev(pick(R, fx["R"])), dev(pick(T, fx["T"])), kw.pop("group_of", None))
    d, st, to = fx["art"].sweep(state(pick(q, fx["q"])), fx["base"], dev(pick(tg, fx["tg"])), float(DT), *tables, Rd, Td, s._pts, s._carrier,
                                s._seg_off, fx["slot_body"] if slot_body is None else slot_body, S, margin=margin, reset=flag(reset),
                                free=flag(free), vmax=None if vmax is None else dev(vmax), slot_C=fx["slot_C"], p0=s.targets[0],
                                p1=s.targets[1], pt_id=s._pt_id, chunk_sphere=s.chunk_sphere, cull=cull, **groups, **kw)
    return npy(d), npy(st), npy(to)


def compose(fx, qk, R, T, sensor=None, slot_body=None, slot_C="fx", group_of=None):
    """The definition, from existing launches: forward kinematics at qk (N, nd), the gathered poses of the slots the robot places,
    the caller's table elsewhere, the sensor's body distances, their minimum (torch.min: a NaN wins)."""
    from partmanip_amd import ops
    s = fx["sensor"] if sensor is None else sensor
    sb = np.asarray(fx["slot_body"] if slot_body is None else slot_body)
    n = len(qk)
    rb, _ = fx["art"].forward(state(qk), fx["base"], rigid_body=torch.zeros(n, fx["nb"], 13, device=DEV),
                              jacobian=torch.zeros(n, fx["nb"] - 1, 6, fx["nd"], device=DEV))
    rows = np.where(sb[None] >= 0, np.arange(n)[:, None] * fx["nb"] + sb[None], -1).astype(np.int32)
    Rg, Tg = ops.body_pose_gather(rb, dev(rows), fx["slot_C"] if isinstance(slot_C, str) else slot_C)
    placed = dev(sb >= 0)
    Rk = torch.where(placed[None, :, None, None], Rg, dev(R))
    Tk = torch.where(placed[None, :, None], Tg, dev(T))
    return npy(s.sense(Rk, Tk, group_of=group_of, per_point=False).body_dist.min(dim=1)[0])


def check(fx, S, got, q, tg, R, T, reset, free, vmax, margin=MARGIN, **kw):
    d, st, to = got
    cand = GS.candidates(q, tg, fx["lo"], fx["hi"], vmax, DT, reset, S, dtype=np.float32)
    assert cand.dtype == np.float32 and d.shape == (len(q), S + 1) and st.dtype == np.int32
    for k in range(S + 1):
        assert same_bits(d[:, k], compose(fx, cand[k], R, T, **kw)), (S, k)
    forced = np.zeros(len(q), dtype=bool) | (False if reset is None else np.asarray(reset)) | (False if free is None else np.asarray(free))
    want = GS.select(d, np.float32(margin), forced)
    assert same_bits(st, want), (st, want)
    assert same_bits(to, cand[want, np.arange(len(q))])
    return want


# ------------------------------------------------------------------------------------------- 1. the composition, ungrouped
@pytest.mark.parametrize("S", [1, 4, 8])
@pytest.mark.parametrize("limited", [False, True])
def test_equals_the_composition_of_the_existing_entries(fx, S, limited):
    vmax = fx["vmax"] if limited else None
    cuts = []
    for reset, free in ((None, None), ([False, True, False], [False, False, True])):
        got = sweep(fx, S, reset=reset, free=free, vmax=vmax)
        cuts.append(check(fx, S, got, fx["q"], fx["tg"], fx["R"], fx["T"], reset, free, vmax))
        off, again = sweep(fx, S, reset=reset, free=free, vmax=vmax, cull=False), sweep(fx, S, reset=reset, free=free, vmax=vmax)
        assert all(same_bits(a, b) and same_bits(a, c) for a, b, c in zip(got, off, again))
        for b in range(N):                                    # a batch of 3 equals its environments run alone
            one = sweep(fx, S, reset=reset, free=free, vmax=vmax, rows=slice(b, b + 1))
            assert all(same_bits(a[b:b + 1], o) for a, o in zip(got, one)), b
        d = got[0]
        assert (d < 1).any() and not np.isnan(d).any()
    print(f"S = {S}, vmax {'on' if limited else 'off'}: steps {cuts[0].tolist()} unforced, {cuts[1].tolist()} with reset / free; "
          f"distances: {np.round(got[0], 5).tolist()}")
    assert cuts[1][1] == S and cuts[1][2] == S
    if S == 8 and not limited:
        assert (cuts[0] < S).any() and (got[0].min(axis=1) <= MARGIN).any()      # the scene does make the rule cut a step


def test_the_velocity_limit_is_the_articulation_steps(fx):
    """What the sweep calls q' is what pm_articulation_step_f32 writes: executing targets_out with vmax=None leaves the bits of
    q_steps in dof_state, and a free sweep's targets_out is the plain step's joint state."""
    S = 8
    d, st, to = sweep(fx, S, vmax=fx["vmax"], free=[True] * N)
    ds = state(fx["q"])
    fx["art"].step(ds, fx["base"], targets=dev(fx["tg"]), vmax=dev(fx["vmax"]), dt=float(DT))
    assert same_bits(npy(ds[..., 0]), to) and (st == S).all()
    d, st, to = sweep(fx, S, vmax=fx["vmax"])
    ds = state(fx["q"])
    fx["art"].step(ds, fx["base"], targets=dev(to), vmax=None, dt=float(DT))
    assert same_bits(npy(ds[..., 0]), to)


# ------------------------------------------------------------------------------------------- 2. the composition, grouped
@pytest.fixture(scope="module")
def grouped(fx):
    """Pose slots 0, 1 are placed by robot bodies 9 and 11 (the fingers; they carry the points and own the two shared rows, which
    lie outside the target range), slots 2, 3, 4 are the table's: groups of 1 row (slot 2) and 3 rows (slots 2, 3, 4), environment
    2 holds none.  The target grids sit round the right finger's end position."""
    from partmanip_amd.contact import ContactSensor
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    parts = P.make_parts(4207, "cont", n_parts=6)
    env_group = np.array([0, 1, -1])
    tsdf = TSDFfromMesh(N, P.SIZE, 10, DEV, sdf_dicts=parts[:2], groups=[[parts[2]], [parts[3], parts[4], parts[5]]], group_of=env_group)
    rng = np.random.RandomState(7311)
    pts = rng.uniform(-0.04, 0.04, size=(200, 3)).astype(np.float32)
    carrier = np.where(np.arange(200) < 130, 0, 1)
    sensor = ContactSensor(tsdf, pts, carrier, [130, 70], targets=(2, 5))
    slot_body = np.array([9, 11, -1, -1, -1], dtype=np.int32)
    kw = fx["tree"].robot_kwargs()
    end = K.fk(fx["tree"], K.clamp(fx["tg"], fx["lo"], fx["hi"]).astype(np.float64), np.zeros((N, fx["nd"])), npy(fx["base"]).astype(np.float64))
    R, T = P.random_poses(7312, N, 5)
    T[:, 2:] = (end["pos"][:, kw["rtip_rb_index"]][:, None] + rng.uniform(-0.05, 0.05, size=(N, 3, 3))).astype(np.float32)
    R[:, :2], T[:, :2] = np.nan, np.nan                        # placed by the robot: never read
    R[0, 3] = np.nan                                           # environment 0 owns slot 2 only, no carrier names slot 3
    T[2, 2:5] = np.nan                                         # environment 2 owns nothing
    C = dev(P.random_poses(7313, 1, 1)[0][0])                  # slot 0 has a mesh-frame matrix, slot 1 none
    return dict(sensor=sensor, slot_body=slot_body, R=R, T=T, C=C, env_group=env_group, parts=parts, tsdf=tsdf)


def sweep_grouped(fx, g, S, R=None, T=None, reset=None, free=None, vmax=None, rows=slice(None), **kw):
    s = g["sensor"]
    flag = lambda a: None if a is None else dev(np.asarray(a, dtype=bool)[rows])        # noqa: E731
    tables, Rd, Td, groups = s.tsdf._point_tables(dev((g["R"] if R is None else R)[rows]), dev((g["T"] if T is None else T)[rows]),
                                                  g["env_group"][rows])
    d, st, to = fx["art"].sweep(state(fx["q"][rows]), fx["base"], dev(fx["tg"][rows]), float(DT), *tables, Rd, Td, s._pts, s._carrier,
                                s._seg_off, g["slot_body"], S, margin=MARGIN, reset=flag(reset), free=flag(free),
                                vmax=None if vmax is None else dev(vmax), slot_C=g["C"], p0=s.targets[0], p1=s.targets[1], pt_id=s._pt_id,
                                chunk_sphere=s.chunk_sphere, **groups, **kw)
    return npy(d), npy(st), npy(to)


@pytest.mark.parametrize("S", [1, 4, 8])
def test_grouped_equals_the_composition_and_the_ungrouped_entry_on_own_rows(fx, grouped, S):
    g = grouped
    for reset, free, vmax in ((None, None, None), ([False, True, False], [True, False, False], fx["vmax"])):
        flags = dict(reset=reset, free=free, vmax=vmax)
        got = sweep_grouped(fx, g, S, **flags)
        want = check(fx, S, got, fx["q"], fx["tg"], g["R"], g["T"], reset, free, vmax, sensor=g["sensor"], slot_body=g["slot_body"],
                     slot_C=g["C"])
        assert all(same_bits(a, b) for a, b in zip(got, sweep_grouped(fx, g, S, cull=False, **flags)))
        assert all(same_bits(a, b) for a, b in zip(got, sweep_grouped(fx, g, S, **flags)))
        for b in range(N):                                    # a batch of 3 equals its environments run alone
            one = sweep_grouped(fx, g, S, rows=slice(b, b + 1), **flags)
            assert all(same_bits(a[b:b + 1], o) for a, o in zip(got, one)), b
        if reset is not None:
            assert want[0] == S and want[1] == S              # forced: free and reset
    got = sweep_grouped(fx, g, S)
    d = got[0]
    assert not np.isnan(d).any() and (d[:2] < 1).any() and (d[2] == 1).all()       # environment 2 has nothing to touch
    # the ungrouped entry on environment b's own rows: part tables gathered by row, pose table = the rows' slots then the five slots
    o = g["tsdf"]
    own = [[(0, 0), (1, 1), (2, 2)], [(0, 0), (1, 1), (3, 2), (4, 3), (5, 4)]]
    s = g["sensor"]
    for b in range(2):
        rows, slots = [r for r, _ in own[b]], [sl for _, sl in own[b]]
        n = len(rows)
        ix = torch.as_tensor(rows + [0] * 5, dtype=torch.long, device=DEV)
        sl = slots + list(range(5))
        R1 = np.where(np.isnan(g["R"][b:b + 1, sl]), 0, g["R"][b:b + 1, sl])       # a NaN slot no own row names is not part of the call
        T1 = np.where(np.isnan(g["T"][b:b + 1, sl]), 0, g["T"][b:b + 1, sl])
        sb = np.concatenate([g["slot_body"][slots], g["slot_body"]]).astype(np.int32)
        Cw = torch.zeros(n + 1, 3, 3, device=DEV)             # slot 0's matrix sits at own ordinal 0 and at carrier slot n + 0
        Cw[:] = torch.eye(3, device=DEV)
        Cw[0], Cw[n] = g["C"][0], g["C"][0]
        one = fx["art"].sweep(state(fx["q"][b:b + 1]), fx["base"], dev(fx["tg"][b:b + 1]), float(DT), o.sdf_field,
                              o.sdf_field_off[ix].contiguous(), o.sdf_field_res[ix].contiguous(), o.sdf_bbox_min[ix].contiguous(),
                              o.sdf_voxel_size[ix].contiguous(), dev(R1), dev(T1), s._pts, (s._carrier + n).contiguous(), s._seg_off, sb, S,
                              margin=MARGIN, slot_C=Cw, p0=2, p1=min(5, n), pt_id=s._pt_id, chunk_sphere=s.chunk_sphere)
        assert all(same_bits(a[b:b + 1], npy(x)) for a, x in zip(got, one)), b


# ------------------------------------------------------------------------------------------- 3. edge cases
def test_a_nan_target_or_pose_stays_in_its_environment(fx):
    S = 4
    ref = sweep(fx, S)
    tg = fx["tg"].copy()
    tg[1, 3] = np.nan
    d, st, to = sweep(fx, S, tg=tg)
    assert not np.isnan(d[1, 0]) and np.isnan(d[1, 1:]).all() and st[1] == 0
    assert same_bits(to[1], GS.candidates(fx["q"], tg, fx["lo"], fx["hi"], None, DT, None, S, dtype=np.float32)[0, 1])
    assert all(same_bits(a[[0, 2]], r[[0, 2]]) for a, r in zip((d, st, to), ref))
    check(fx, S, (d, st, to), fx["q"], tg, fx["R"], fx["T"], None, None, None)
    T = fx["T"].copy()
    T[2, 11, 1] = np.inf                                      # the cube's slot: the table's pose counts
    d, st, to = sweep(fx, S, T=T)
    assert np.isnan(d[2]).all() and st[2] == 0 and all(same_bits(a[:2], r[:2]) for a, r in zip((d, st, to), ref))
    d, st, to = sweep(fx, S, T=T, free=[False, False, True])
    assert np.isnan(d[2]).all() and st[2] == S                # forced, and the distances are written all the same


def test_carriers_off_the_robot_world_points_and_an_empty_segment(fx):
    """A sensor whose middle segment is empty, whose first rides on the cube's own slot (a slot the robot does not place) and on no
    slot at all (carrier -1: world points), and whose last rides on the right finger."""
    from partmanip_amd.contact import ContactSensor
    S = 4
    rng = np.random.RandomState(7321)
    near = fx["T"][0, 11]
    pts = np.concatenate([rng.uniform(-0.03, 0.03, size=(40, 3)), near + rng.uniform(-0.04, 0.04, size=(30, 3)),
                          CE.part_clouds()[10][:70]]).astype(np.float32)
    carrier = np.concatenate([np.full(40, 11), np.full(30, -1), np.full(70, 10)])
    sensor = ContactSensor(fx["tsdf"], pts, carrier, [70, 0, 70], targets=(11, 12))
    got = sweep(fx, S, sensor=sensor)
    check(fx, S, got, fx["q"], fx["tg"], fx["R"], fx["T"], None, None, None, sensor=sensor)
    assert (got[0][0] < 0).all()                              # environment 0's world points sit inside its cube at every candidate
    assert all(same_bits(a, b) for a, b in zip(got, sweep(fx, S, sensor=sensor, cull=False)))


def test_refusals(fx):
    from partmanip_amd import _lib
    bad = fx["slot_body"].copy()
    bad[3] = fx["nb"]
    with pytest.raises(ValueError, match="slot_body"):
        sweep(fx, 4, slot_body=bad)
    bad[3] = -2
    with pytest.raises(ValueError, match="slot_body"):
        sweep(fx, 4, slot_body=bad)
    for S in (0, 64):
        with pytest.raises(ValueError, match="substeps"):
            sweep(fx, S)
    with pytest.raises(ValueError, match="margin"):
        sweep(fx, 4, margin=float("nan"))
    with pytest.raises(ValueError, match="free"):
        sweep(fx, 4, free=[True])
    # the C entry itself: a device slot_body is not read on the host, so the range check is the kernel's -- a body outside [-1, nb)
    # gives the slot a NaN pose, and no address is formed from it
    dbad = dev(np.where(np.arange(12) == 3, 2 ** 30, fx["slot_body"]).astype(np.int32))
    d, st, to = sweep(fx, 4, slot_body=dbad)
    assert np.isnan(d).all() and (st == 0).all()
    assert _lib.lib.pm_articulation_sweep_f32 is not None
