"""The posed-point distance query, everything that needs no GPU: the restatement of tests/mesh_sdf_points_ref.py against the
mesh-TSDF restatement at the workspace lattice, the C entries' refusals, every argument check of ops.mesh_sdf_points,
TSDFfromMesh.query_points and ContactSensor (all raise before anything touches a device), the carrier sort and the chunk table, and
the condition under which the contact-grasp episode's onset step can be asserted as an equality on the GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import contact_episode as CE
from tests import kinematic_episode as E
from tests import mesh_sdf_points_ref as RF
from tests import mesh_tsdf_parts as P
from tests.test_capi_symbols import header_functions


# ------------------------------------------------------------------------------------------- the restatement
def test_restatement_at_the_lattice_is_the_mesh_tsdf_restatement():
    """carrier = -1 at the res = 10 voxel centres, then clamp(min(dist, base) / trunc): in float64 it is mesh_tsdf_parts.restate's
    volume (the same operations, so to round-off of the last few of them), and the float32 run rounds to the same volume wherever no
    sample lies within float32 round-off of a validity border."""
    parts = P.fixture_parts("cont")
    R, T = P.random_poses(3301, 2)
    vol, margin = P.restate(parts, R, T, res=10)
    trunc = 4 * P.SIZE / 10
    c64 = RF.lattice(10, dtype=np.float64)
    d64 = RF.restate(parts, R, T, c64, dtype=np.float64)["dist"]
    mine = np.clip(np.minimum(d64, c64[None, :, 2]) / trunc, -1, 1)
    assert np.abs(mine - vol.reshape(2, -1)).max() < 1e-12 and (d64 < 1).mean() > 0.05
    c32 = RF.lattice(10)
    d32 = RF.restate(parts, R, T, c32)["dist"]
    assert d32.dtype == np.float32
    v32 = np.clip(np.minimum(d32, c32[None, :, 2]) / np.float32(trunc), -1, 1)
    clear = margin > 1e-3
    assert clear.mean() > 0.99 and np.abs(v32 - vol.reshape(2, -1))[clear].max() < 2e-6


# ------------------------------------------------------------------------------------------- the C ABI
def test_header_ctypes_table_and_library_agree_on_the_new_entries():
    from partmanip_amd import _lib
    P_, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert header_functions()["pm_mesh_sdf_points_f32"] == ("int", 26) and header_functions()["pm_mesh_sdf_points_groups_f32"] == ("int", 33)
    res, args = _lib.SIGNATURES["pm_mesh_sdf_points_f32"]
    old = _lib.SIGNATURES["pm_mesh_tsdf_query_f32"][1]
    assert res is I and args == old[:11] + [P_, L, P_, P_, P_, I, P_, I, P_, L, P_, P_, P_, I, P_]
    gargs = _lib.SIGNATURES["pm_mesh_sdf_points_groups_f32"][1]
    assert gargs == args[:5] + [P_, I, I, P_, I, P_, I] + args[5:]
    assert hasattr(_lib.lib, "pm_mesh_sdf_points_f32") and hasattr(_lib.lib, "pm_mesh_sdf_points_groups_f32")
    assert _lib.ABI_VERSION == 163 == _lib.lib.pm_version()


def test_every_einval_condition_is_refused_before_a_launch():
    """Any non-NULL pointer will do: a call that is refused launches and reads nothing."""
    from partmanip_amd._lib import lib
    one = 1
    good = dict(fields=one, part_off=one, part_shape=one, part_bbox_min=one, part_voxel_size=one, pose_R=one, pose_T=one, B=3, M=5, p0=0, p1=5,
                pts=one, pts_env_stride=0, carrier=one, pt_id=None, chunk_sphere=None, NP=131, seg_off=one, NS=3, dist=one, ld_dist=131,
                arg=None, seg_min=one, seg_arg=one, cull=1, stream=None)
    call = lambda **kw: lib.pm_mesh_sdf_points_f32(*dict(good, **kw).values())           # noqa: E731
    ggood = dict(list(good.items())[:5] + [("grid_slot", one), ("NG", 6), ("NG_shared", 2), ("group_off", one), ("G", 2), ("env_group", one),
                                           ("max_group_grids", 3)] + list(good.items())[5:])
    gcall = lambda **kw: lib.pm_mesh_sdf_points_groups_f32(*dict(ggood, **kw).values())   # noqa: E731
    bad = [dict(B=0), dict(B=65536), dict(M=0), dict(p0=-1), dict(p0=5), dict(p0=2, p1=2), dict(NP=0), dict(NP=2 ** 30 + 1), dict(NS=-1),
           dict(seg_off=None), dict(pts_env_stride=392), dict(pts_env_stride=-1), dict(seg_min=None), dict(seg_arg=None),
           dict(NS=0, seg_off=None), dict(dist=None, seg_min=None, seg_arg=None), dict(ld_dist=130), dict(dist=None, arg=one, ld_dist=130)]
    for name in ("fields", "part_off", "part_shape", "part_bbox_min", "part_voxel_size", "pose_R", "pose_T", "pts", "carrier"):
        assert call(**{name: None}) == -1 and gcall(**{name: None}) == -1, name
    for kw in bad:
        assert call(**kw) == -1, kw
        assert gcall(**kw) == -1, kw
    assert call(p1=6) == -1
    for kw in (dict(grid_slot=None), dict(group_off=None), dict(env_group=None), dict(NG=0), dict(NG_shared=-1), dict(NG_shared=7), dict(G=-1),
               dict(max_group_grids=-1), dict(p1=6), dict(M=32769)):
        assert gcall(**kw) == -1, kw


# ------------------------------------------------------------------------------------------- the wrappers' checks
@pytest.fixture(scope="module")
def cpu():
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    sc = RF.scene(4101, 3)
    parts = list(sc["parts"]) + [sc["parts"][0]] * 3
    sc["tsdf"] = TSDFfromMesh(3, P.SIZE, 10, "cpu", sdf_dicts=parts)
    sc["tensors"] = {k: torch.from_numpy(sc[k]) for k in ("R", "T", "pts", "world")}
    return sc


def op(sc, **kw):
    from partmanip_amd import ops
    o, x = sc["tsdf"], sc["tensors"]
    a = dict(pts=x["pts"], carrier=sc["carrier"], pose_R=x["R"], pose_T=x["T"])
    a.update({k: kw.pop(k) for k in list(kw) if k in a})
    return ops.mesh_sdf_points(o.sdf_field, o.sdf_field_off, o.sdf_field_res, o.sdf_bbox_min, o.sdf_voxel_size, a["pose_R"], a["pose_T"],
                               a["pts"], a["carrier"], **kw)


def test_ops_wrapper_checks_come_before_the_device(cpu):
    x = cpu["tensors"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):                            # good arguments reach the device check
        op(cpu, seg_off=[0, 1, 65, 131], want_arg=True)
    for kw, what in ((dict(pts=x["pts"][:, :2]), "pts"), (dict(pts=x["pts"].double()), "pts"), (dict(pts=x["world"][:2]), "pts"),
                     (dict(pts=torch.zeros(0, 3)), "pts"), (dict(carrier=cpu["carrier"][:5]), "carrier"),
                     (dict(carrier=np.full(131, 7)), "carrier"), (dict(carrier=np.full(131, -2)), "carrier"),
                     (dict(carrier=np.zeros(131)), "carrier"), (dict(pt_id=np.zeros(5, dtype=np.int64)), "pt_id"),
                     (dict(seg_off=[0, 70, 65, 131]), "seg_off"), (dict(seg_off=[1, 65, 131]), "seg_off"), (dict(seg_off=[0, 65, 130]), "seg_off"),
                     (dict(seg_off=[0]), "seg_off"), (dict(chunk_sphere=torch.zeros(2, 4)), "chunk_sphere"),
                     (dict(chunk_sphere=torch.zeros(3, 4).double()), "chunk_sphere"), (dict(p0=3, p1=3), "p0, p1"), (dict(p1=8), "p0, p1"),
                     (dict(want_dist=False), "want_dist"), (dict(dist=torch.zeros(3, 100)), "dist"), (dict(dist=torch.zeros(2, 131)), "dist"),
                     (dict(NG_shared=2), "grid_slot="), (dict(pose_R=x["R"][:, :5]), "pose_R"), (dict(pose_T=x["T"][:2]), "pose_T"),
                     (dict(grid_slot=[0] * 6, NG_shared=2, group_off=[0, 5], env_group=[0, 0, 0]), "grid_slot"),
                     (dict(grid_slot=list(range(7)), NG_shared=2, group_off=[0, 4], env_group=[0, 0, 0]), "group_off"),
                     (dict(grid_slot=list(range(7)), NG_shared=2, group_off=[0, 5], env_group=[0, 1, 0]), "env_group"),
                     (dict(grid_slot=list(range(7)), NG_shared=2, group_off=[0, 5], env_group=[0, 0, 0], p1=8), "p0, p1")):
        with pytest.raises(ValueError, match=what):
            op(cpu, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(cpu, grid_slot=list(range(7)), NG_shared=2, group_off=[0, 5], env_group=[0, -1, 0], p1=7)


def test_query_points_checks_come_before_the_device(cpu):
    o, x = cpu["tsdf"], cpu["tensors"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.query_points(x["pts"], x["R"], x["T"], carrier=cpu["carrier"], segments=[1, 64, 66], return_arg=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.query_points(x["world"], x["R"], x["T"])
    for kw, what in ((dict(points=x["pts"][:, :2]), "points"), (dict(points=torch.zeros(0, 3)), "points"), (dict(parts=(2, 2)), "parts"),
                     (dict(parts=(0, 8)), "parts"), (dict(carrier=np.full(131, 7)), "carrier"), (dict(carrier=np.zeros(4, dtype=np.int64)), "carrier"),
                     (dict(segments=[1, 64, 65]), "segments"), (dict(segments=[132, -1]), "segments"), (dict(group_of=[0, 0, 0]), "group_of")):
        a = dict(points=x["pts"], carrier=cpu["carrier"])
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            o.query_points(a.pop("points"), x["R"], x["T"], **a)
    assert len(o._point_layouts) <= 8


def test_contact_sensor_refusals(cpu):
    from partmanip_amd.contact import ContactSensor
    from partmanip_amd.mesh2pc import PCfromMesh
    o = cpu["tsdf"]
    make = lambda **kw: ContactSensor(**dict(dict(tsdf=o, points=cpu["pts"], carrier=cpu["carrier"], segments=[1, 64, 66], targets=(0, 4)), **kw))   # noqa: E731
    s = make(names=("a", "b", "c"))
    assert (s.num_points, s.num_bodies, s.targets, s.body("b")) == (131, 3, (0, 4), 1)
    for kw, what in ((dict(carrier=np.full(131, 7)), "carrier"), (dict(carrier=np.full(131, -2)), "carrier"), (dict(carrier=cpu["carrier"][:9]), "carrier"),
                     (dict(targets=(2, 2)), "targets"), (dict(targets=(3, 1)), "targets"), (dict(targets=(0, 8)), "targets"),
                     (dict(points=cpu["pts"][:, :2]), "points"), (dict(segments=[1, 64]), "segments"), (dict(names=("a", "b")), "names"),
                     (dict(names=("a", "a", "b")), "names")):
        with pytest.raises(ValueError, match=what):
            make(**kw)
    with pytest.raises(ValueError, match="names"):
        make().body("lfinger")
    pc = PCfromMesh(3, "cpu", num_points=8, part_pcs=np.zeros((5, 8, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="pc: its part_num 5 differs from tsdf's 7"):
        ContactSensor.from_cloud(o, pc, (1, 2), targets=(0, 4))
    pc = PCfromMesh(3, "cpu", num_points=8, part_pcs=np.random.RandomState(0).rand(7, 8, 3).astype(np.float32))
    s = ContactSensor.from_cloud(o, pc, (4, 6), targets=(0, 4), points_per_body=5, names=("x", "y"))
    assert s.num_points == 10 and s.layout.carrier[s.layout.pt_id >= 0].tolist() == [4] * 5 + [6] * 5
    with pytest.raises(ValueError, match="slots"):
        ContactSensor.from_cloud(o, pc, (4, 9), targets=(0, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.sense(cpu["tensors"]["R"], cpu["tensors"]["T"])


# ------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("segments", [[1, 64, 66], [40, 0, 91], None])
def test_carrier_sort_padding_and_chunk_spheres(segments):
    from partmanip_amd.contact import CHUNK, PointLayout, chunk_spheres
    rng = np.random.RandomState(17)
    NP = 131
    pts = rng.uniform(-0.1, 0.1, size=(NP, 3)).astype(np.float32)
    carrier = rng.randint(-1, 4, size=NP)                      # shuffled: nothing is sorted on the way in
    L = PointLayout(NP, carrier, segments)
    real = L.pt_id >= 0
    assert real.sum() == NP and np.array_equal(np.sort(L.pt_id[real]), np.arange(NP))       # every point once
    assert np.array_equal(L.src[L.pos], np.arange(NP)) and np.array_equal(L.pt_id[L.pos], np.arange(NP))
    assert np.array_equal(L.carrier, carrier[L.src]) and not L.identity
    n = len(L.src)
    # a chunk holds one carrier, and padding repeats a point of its own chunk (the run's last)
    for c0 in range(0, n, CHUNK):
        sl = slice(c0, min(c0 + CHUNK, n))
        assert len(set(L.carrier[sl])) == 1
        pad = np.flatnonzero(~real[sl])
        if len(pad):
            assert pad[0] > 0 and np.array_equal(pad, np.arange(pad[0], sl.stop - c0)) and (L.src[sl][pad] == L.src[sl][pad[0] - 1]).all()
    bounds = [0, NP] if segments is None else np.concatenate([[0], np.cumsum(segments)])
    if segments is None:
        assert L.seg_off is None
    else:
        assert L.seg_off[0] == 0 and L.seg_off[-1] == n and (np.diff(L.seg_off) >= 0).all() and (L.seg_off[:-1] % CHUNK == 0).all()
    off = [0, n] if segments is None else L.seg_off
    for s in range(len(bounds) - 1):
        mine = L.pt_id[off[s]:off[s + 1]]
        mine = mine[mine >= 0]
        assert np.array_equal(np.sort(mine), np.arange(bounds[s], bounds[s + 1]))           # a segment keeps its own points
        car = carrier[mine]
        assert (np.diff(car) >= 0).all()                                                    # sorted by carrier ...
        assert all((np.diff(mine[car == c]) > 0).all() for c in np.unique(car))              # ... stably
    sph = chunk_spheres(torch.from_numpy(pts[L.src])).numpy().astype(np.float64)
    assert sph.shape == ((n + CHUNK - 1) // CHUNK, 4)
    d = np.linalg.norm(pts[L.src].astype(np.float64) - sph[np.arange(n) // CHUNK, :3], axis=1)
    assert (d[real] <= sph[np.arange(n) // CHUNK, 3][real]).all() and (sph[:, 3] < 0.2).all()


def test_layout_of_sorted_world_points_is_the_identity():
    from partmanip_amd.contact import PointLayout
    L = PointLayout(200)
    assert L.identity and len(L.src) == 200 and L.seg_off is None
    L = PointLayout(128, np.repeat([2, 5], 64), [64, 64])
    assert L.identity and L.seg_off.tolist() == [0, 64, 128]
    with pytest.raises(ValueError, match="segments"):
        PointLayout(10, None, [4, 5])
    with pytest.raises(ValueError, match="carrier"):
        PointLayout(10, np.zeros(10))


# ------------------------------------------------------------------------------------------- the contact grasp
def test_contact_grasp_episode_reaches_hold_clear_of_round_off():
    """In float64 the scripted episode does reach `hold` under the contact predicate, and at the observation that sets it and the
    one before it both fingers' |body_dist - contact_margin| exceed 100 x the float32 composition's error: the onset step is safe to
    assert as an equality on the GPU.  contact_margin = 0.002, KinematicEnv's default, satisfies this for the fixture."""
    r64, r32 = CE.run_reference(E.MAX_EPISODE_LENGTH), CE.run_reference(E.MAX_EPISODE_LENGTH, dtype=np.float32)
    on = CE.hold_onset(r64)
    assert on is not None and on >= 2 and CE.hold_onset(r32) == on
    assert r64[on - 1]["reached"] and not r64[on - 1]["hold"]
    for at in (on - 1, on - 2):
        for body in (1, 2):
            d64, d32 = float(r64[at]["body_dist"][body]), float(r32[at]["body_dist"][body])
            e32 = abs(d32 - d64)
            print(f"observation after step {at + 1}, {CE.NAMES[body]}: {d64:.6f}, |d - margin| = {abs(d64 - CE.MARGIN):.3e}, fp32 error {e32:.3e}")
            assert abs(d64 - CE.MARGIN) > 100 * e32 and e32 < 1e-6
    assert (r64[on - 1]["body_dist"][1:] <= CE.MARGIN).all() and not (r64[on - 2]["body_dist"][1:] <= CE.MARGIN).any()
    gap = E.run_reference(E.MAX_EPISODE_LENGTH)
    print(f"hold onset: step {on + 1} under the contact predicate, step {next(i for i, s in enumerate(gap) if s['hold']) + 1} under the gap rule")
