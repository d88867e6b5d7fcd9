"""The posed-point distance query on the GPU (pm_mesh_sdf_points_f32 / pm_mesh_sdf_points_groups_f32, ops.mesh_sdf_points,
TSDFfromMesh.query_points).  The kernel is specified op by op, so every check but one is an equality of bit patterns with the
float32 restatement of tests/mesh_sdf_points_ref.py (written from the contract), with the existing TSDF kernel at the workspace
lattice, or between two ways of asking.  The one tolerance is the project's standing rule against the float64 restatement.
Shapes: B in {1, 3}, 4 synthetic parts of differing grid shapes and voxel sizes, 131 points in segments (1, 64, 66) -- one point, one
whole chunk, a chunk and two points; the carriers are unsorted, so every call goes through the sort, the padding and the way back."""
import numpy as np
import pytest
import torch

from tests import mesh_sdf_points_ref as RF
from tests import mesh_tsdf_parts as P
from tests.helpers import npy, record_margin, same_bits, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG = list(RF.SEGMENTS)
NP_ = RF.NP_
i32 = lambda a: t(np.asarray(a, dtype=np.int32), device=DEV)                             # noqa: E731


def make_tsdf(parts, B=1, **kw):
    from partmanip_amd.mesh2sdf import TSDFfromMesh
    return TSDFfromMesh(B, P.SIZE, 10, DEV, sdf_dicts=parts, **kw)


def pad_parts(sc):
    """The scene's grids plus one copy of grid 0 per carrier slot, so that the part tables have a row per pose slot; the copies sit
    at ordinals >= n_parts, outside every `parts` range the tests ask for."""
    return list(sc["parts"]) + [sc["parts"][0]] * (sc["M"] - sc["n_parts"])


@pytest.fixture(scope="module", params=[1, 3])
def sc(request):
    s = RF.scene(4101, request.param)
    s["tsdf"] = make_tsdf(pad_parts(s))
    s["dev"] = {k: t(s[k], device=DEV) for k in ("R", "T", "pts", "world")}
    s["mixed"] = np.where((np.arange(NP_) % 3 == 0)[None, :, None], s["world"], s["pts"][None]).astype(np.float32)
    s["mixed_carrier"] = np.where(np.arange(NP_) % 3 == 0, -1, s["carrier"])
    s["cases"] = {"shared_carried": (s["pts"], s["carrier"]), "world_per_env": (s["world"], None),
                  "mixed_per_env": (s["mixed"], s["mixed_carrier"])}
    s["ref"] = {}
    for name, (pts, car) in s["cases"].items():
        kw = dict(pts=pts, carrier=car, p1=s["n_parts"], segments=SEG)
        s["ref"][name] = (RF.restate(pad_parts(s), s["R"], s["T"], **kw), RF.restate(pad_parts(s), s["R"], s["T"], dtype=np.float64, **kw))
    return s


def ask(s, name, cull=True, **kw):
    pts, car = s["cases"][name]
    d, a, (sm, sa) = s["tsdf"].query_points(t(pts, device=DEV), s["dev"]["R"], s["dev"]["T"], carrier=car, parts=(0, s["n_parts"]),
                                            segments=SEG, return_arg=True, cull=cull, **kw)
    return dict(dist=npy(d), arg=npy(a), seg_min=npy(sm), seg_arg=npy(sa))


def equal(got, want):
    return all(same_bits(got[k], want[k]) for k in ("dist", "arg", "seg_min", "seg_arg"))


# ------------------------------------------------------------------------------------------- 1. the float32 restatement, bit for bit
@pytest.mark.parametrize("name", ["shared_carried", "world_per_env", "mixed_per_env"])
def test_equals_the_float32_restatement_with_cull_on_and_off(sc, name):
    want = sc["ref"][name][0]
    on, off = ask(sc, name, cull=True), ask(sc, name, cull=False)
    near = float((want["dist"] < 1).mean())
    print(f"{name}: {100 * near:.0f} % of the points inside a valid box; arg histogram {np.bincount(want['arg'].ravel() + 1).tolist()}")
    assert 0.3 < near and (want["arg"] == -1).any() and len(np.unique(want["arg"])) >= 4       # near, far, and several parts win
    assert on["dist"].shape == (len(sc["R"]), NP_) and on["arg"].dtype == np.int32 and on["seg_arg"].dtype == np.int32
    for k in ("dist", "arg", "seg_min", "seg_arg"):
        assert same_bits(on[k], want[k]), (name, k, "cull on")
        assert same_bits(off[k], want[k]), (name, k, "cull off")
    assert equal(on, off)


# ------------------------------------------------------------------------------------------- 2. the lattice identity
def test_at_the_lattice_it_is_the_tsdf_kernels_volume(sc):
    """Points = the res = 10 voxel centres float32(i) * float32(vox) + float32(origin), carried by a slot whose pose is the
    identity: clamp(min(dist, base) / trunc) is query_tsdf's volume bit for bit."""
    tsdf = sc["tsdf"]
    R, T = sc["dev"]["R"].clone(), sc["dev"]["T"].clone()
    slot = sc["M"] - 1
    R[:, slot], T[:, slot] = torch.eye(3, device=DEV), 0.0
    c = RF.lattice(10)
    for cull in (True, False):
        dist = tsdf.query_points(t(c, device=DEV), R, T, carrier=np.full(len(c), slot), cull=cull)
        vol = tsdf.query_tsdf(R, T).reshape(len(sc["R"]), -1)
        # on the host: numpy's float32 division is a true division (the tensor library multiplies by a scalar's reciprocal)
        mine = np.clip(np.minimum(npy(dist), npy(tsdf._ground)[None]) / np.float32(tsdf.sdf_trunc), -1, 1)
        assert mine.dtype == np.float32 and same_bits(mine, npy(vol)), cull
        assert float((dist < 1).float().mean()) > 0.02                                    # the parts are in the workspace


# ------------------------------------------------------------------------------------------- 3. against float64
@pytest.mark.parametrize("name", ["shared_carried", "world_per_env", "mixed_per_env"])
def test_within_four_times_the_float32_restatements_own_error(sc, name):
    want32, want64 = sc["ref"][name]
    got = ask(sc, name)
    for k in ("dist", "seg_min"):
        e_ref = float(np.abs(want32[k].astype(np.float64) - want64[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - want64[k]).max())
        print(f"{name} {k}: e_ref = {e_ref:.3e}, max |hip - fp64| = {err:.3e} = {err / e_ref:.2f} e_ref; "
              f"{int((want64['margin'] < 1e-3).sum())} points within 1e-3 cells of a validity border")
        record_margin(f"contact: query_points {name} B={len(sc['R'])} {k} max |hip - fp64| / e_ref", err / e_ref, 4.0, e_ref=e_ref)
        assert e_ref > 0 and err <= 4 * e_ref, (name, k, err, e_ref)


# ------------------------------------------------------------------------------------------- 4. groups
@pytest.fixture(scope="module")
def grouped():
    """2 shared rows (slots 0, 1: the sensing bodies' own grids), groups of 1 and 3 rows (slots 2, and 2, 3, 4), environment 2
    holds nothing.  The points ride on slots 0, 1 and 4 -- slot 4 is named by a row only in environment 1."""
    B = 3
    parts = P.make_parts(4207, "cont", n_parts=6)
    rng = np.random.RandomState(4208)
    R, T = P.random_poses(4209, B, 5)
    T[:, 1:] = T[:, :1] + rng.uniform(-0.05, 0.05, size=(B, 4, 3)).astype(np.float32)
    pts = rng.uniform(-0.07, 0.07, size=(NP_, 3)).astype(np.float32)
    carrier = rng.choice([0, 1, 4], size=NP_)
    g = dict(parts=parts, R=R, T=T, pts=pts, carrier=carrier, env_group=np.array([0, 1, -1]),
             own=[[(0, 0), (1, 1), (2, 2)], [(0, 0), (1, 1), (3, 2), (4, 3), (5, 4)], [(0, 0), (1, 1)]])
    g["tsdf"] = make_tsdf(parts[:2], B, groups=[[parts[2]], [parts[3], parts[4], parts[5]]], group_of=g["env_group"])
    assert g["tsdf"].part_num == 5 and g["tsdf"].grid_slot.tolist() == [0, 1, 2, 2, 3, 4]
    return g


def ask_grouped(g, R=None, T=None, parts=None, cull=True):
    R, T = g["R"] if R is None else R, g["T"] if T is None else T
    d, a, (sm, sa) = g["tsdf"].query_points(t(g["pts"], device=DEV), t(R, device=DEV), t(T, device=DEV), carrier=g["carrier"], parts=parts,
                                            segments=SEG, return_arg=True, cull=cull)
    return dict(dist=npy(d), arg=npy(a), seg_min=npy(sm), seg_arg=npy(sa))


def own_rows_ungrouped(g, b, lo, hi):
    """The ungrouped entry (B = 1) on environment b's own rows: the part tables gathered by row, the pose table = the poses of the
    rows' slots followed by the scene's five slots, which the carriers then name (their rows of the part tables repeat row 0 and lie
    outside [p0, p1))."""
    from partmanip_amd import ops
    o = g["tsdf"]
    rows = [r for r, _ in g["own"][b]]
    slots = [s for _, s in g["own"][b]]
    n = len(rows)
    ix = torch.as_tensor(rows + [0] * 5, dtype=torch.long, device=DEV)
    sl = torch.as_tensor(slots + list(range(5)), dtype=torch.long, device=DEV)
    R, T = t(g["R"], device=DEV)[b:b + 1, sl].contiguous(), t(g["T"], device=DEV)[b:b + 1, sl].contiguous()
    lay_car = i32(g["carrier"] + n)
    d, a, sm, sa = ops.mesh_sdf_points(o.sdf_field, o.sdf_field_off[ix].contiguous(), o.sdf_field_res[ix].contiguous(),
                                       o.sdf_bbox_min[ix].contiguous(), o.sdf_voxel_size[ix].contiguous(), R, T, t(g["pts"], device=DEV),
                                       lay_car, lo, min(hi, n), seg_off=np.concatenate([[0], np.cumsum(SEG)]), want_arg=True)
    return dict(dist=npy(d), arg=npy(a), seg_min=npy(sm), seg_arg=npy(sa))


@pytest.mark.parametrize("parts", [None, (2, 5), (1, 3)])
def test_grouped_equals_the_ungrouped_entry_on_own_rows(grouped, parts):
    g = grouped
    lo, hi = parts or (0, 5)
    got, off = ask_grouped(g, parts=parts), ask_grouped(g, parts=parts, cull=False)
    assert equal(got, off)
    want32 = RF.restate(g["parts"], g["R"], g["T"], g["pts"], g["carrier"], own=g["own"], p0=lo, p1=hi, segments=SEG)
    assert equal(got, want32)
    for b in range(3):
        if lo >= len(g["own"][b]):                            # no own ordinal in the range: every point is far
            assert (got["dist"][b] == 1).all() and (got["arg"][b] == -1).all()
            continue
        one = own_rows_ungrouped(g, b, lo, hi)
        for k in one:
            assert same_bits(got[k][b:b + 1], one[k]), (b, k)
    assert (got["dist"][:2] < 1).mean() > 0.2


def test_grouped_nan_poses(grouped):
    g = grouped
    ref = ask_grouped(g)
    R, T = g["R"].copy(), g["T"].copy()
    R[0, 3] = np.nan                                          # environment 0 holds group 0 (slot 2); no carrier names slot 3
    T[2, 2:4] = np.nan                                        # environment 2 holds nothing; carriers name 0, 1, 4
    assert equal(ask_grouped(g, R=R, T=T), ref) and equal(ask_grouped(g, R=R, T=T, cull=False), ref)
    for b, slot, why in ((1, 3, "an own row's slot"), (2, 4, "a carrier's slot"), (0, 4, "a carrier's slot"), (0, 0, "both")):
        R, T = g["R"].copy(), g["T"].copy()
        (R if slot != 3 else T)[b, slot].reshape(-1)[1] = np.inf if slot == 0 else np.nan
        for kw in ({}, {"parts": (0, 1)}, {"cull": False}):
            got = ask_grouped(g, R=R, T=T, **kw)
            assert np.isnan(got["dist"][b]).all() and np.isnan(got["seg_min"][b]).all(), (why, kw)
            assert (got["arg"][b] == -1).all() and (got["seg_arg"][b] == -1).all(), (why, kw)
            others = [e for e in range(3) if e != b]
            assert not np.isnan(got["dist"][others]).any()
            if not kw:
                assert all(same_bits(got[k][others], ref[k][others]) for k in ref), why


# ------------------------------------------------------------------------------------------- 5. edge cases
def test_far_points_ties_and_a_duplicated_point(sc):
    tsdf, R, T = sc["tsdf"], sc["dev"]["R"], sc["dev"]["T"]
    B = len(sc["R"])
    far = t(np.full((5, 3), 10.0, dtype=np.float32), device=DEV)
    d, a = tsdf.query_points(far, R, T, return_arg=True)
    assert bool((d == 1).all()) and bool((a == -1).all()) and tuple(d.shape) == (B, 5)
    # two identical grids under one pose: the smaller ordinal
    twin = make_tsdf([sc["parts"][1], sc["parts"][1], sc["parts"][0]])
    R3, T3 = R[:, [1, 1, 4]].contiguous(), T[:, [1, 1, 4]].contiguous()
    w = t(sc["world"], device=DEV)
    d, a = twin.query_points(w, R3, T3, parts=(0, 2), return_arg=True)
    d1 = twin.query_points(w, R3, T3, parts=(1, 2))
    assert same_bits(npy(d), npy(d1)) and set(np.unique(npy(a))) <= {-1, 0} and float((d < 1).float().mean()) > 0.05
    # every point far: the whole segment ties at 1, and the smallest index of the caller's order wins although the sorted layout
    # starts each segment with another point
    d, (sm, sa) = tsdf.query_points(t(sc["pts"] + np.float32(10), device=DEV), R, T, carrier=sc["carrier"], parts=(0, sc["n_parts"]),
                                    segments=SEG)
    assert bool((d == 1).all()) and bool((sm == 1).all()) and npy(sa).tolist() == [[0, 1, 65]] * B
    assert sc["carrier"][65] != sc["carrier"][65:].min()                       # the layout does move point 65 back
    # a duplicated point: the nearest point i of the last segment and a second index j hold the same body-frame point under two
    # carrier slots with one pose, the LARGER index under the SMALLER slot, so that the sorted layout turns their order round
    want = sc["ref"]["shared_carried"][0]
    Rd, Td = R.clone(), T.clone()
    pts, car = sc["pts"].copy(), sc["carrier"].copy()
    i = int(want["seg_arg"][0, 2])
    j = 65 if i != 65 else 66
    first, second = min(i, j), max(i, j)
    low, high = sc["n_parts"], sc["n_parts"] + 1
    src = int(car[i]) if car[i] >= 0 else low
    Rd[:, low], Td[:, low] = R[:, src], T[:, src]
    Rd[:, high], Td[:, high] = R[:, src], T[:, src]
    pts[j] = pts[i]
    car[first], car[second] = high, low
    ref = RF.restate(pad_parts(sc), npy(Rd), npy(Td), pts, car, p1=sc["n_parts"], segments=SEG)
    assert same_bits(ref["dist"][:, first], ref["dist"][:, second])
    print("the duplicated point is its segment's nearest in environments", np.flatnonzero(ref["seg_arg"][:, 2] == first).tolist())
    d, (sm, sa) = tsdf.query_points(t(pts, device=DEV), Rd, Td, carrier=car, parts=(0, sc["n_parts"]), segments=SEG)
    assert same_bits(npy(d), ref["dist"]) and same_bits(npy(sa), ref["seg_arg"]) and same_bits(npy(sm), ref["seg_min"])
    assert not (npy(sa)[:, 2] == second).any()


def test_a_carrier_outside_the_pose_table_reads_nothing(sc):
    from partmanip_amd import ops
    o, M = sc["tsdf"], sc["M"]
    car = sc["carrier"].copy()
    bad = np.arange(NP_) % 4 == 1
    car[bad] = np.resize([M, -2, 2 ** 31 - 1, -2 ** 31], bad.sum())
    tables = (o.sdf_field, o.sdf_field_off, o.sdf_field_res, o.sdf_bbox_min, o.sdf_voxel_size)
    d, a, _, _ = ops.mesh_sdf_points(*tables, sc["dev"]["R"], sc["dev"]["T"], sc["dev"]["pts"], i32(car), 0, sc["n_parts"], want_arg=True)
    ok = np.where(bad, -1, car)
    want = RF.restate(pad_parts(sc), sc["R"], sc["T"], sc["pts"], ok, p1=sc["n_parts"])
    want["dist"][:, bad], want["arg"][:, bad] = 1, -1
    assert same_bits(npy(d), want["dist"]) and same_bits(npy(a), want["arg"]) and (want["dist"][:, ~bad] < 1).any()


def test_wide_rows_segment_outputs_alone_streams_and_repeats(sc):
    from partmanip_amd import ops
    o, B = sc["tsdf"], len(sc["R"])
    want = sc["ref"]["world_per_env"][0]
    tables = (o.sdf_field, o.sdf_field_off, o.sdf_field_res, o.sdf_bbox_min, o.sdf_voxel_size)
    seg_off = np.concatenate([[0], np.cumsum(SEG)])
    call = lambda **kw: ops.mesh_sdf_points(*tables, sc["dev"]["R"], sc["dev"]["T"], sc["dev"]["world"], None, 0, sc["n_parts"],   # noqa: E731
                                            seg_off=seg_off, **kw)
    rows = torch.full((B, NP_ + 9), -7.0, device=DEV)
    d, a, sm, sa = call(dist=rows[:, :NP_ + 4], want_arg=True)
    assert d.data_ptr() == rows.data_ptr() and bool((rows[:, NP_:] == -7.0).all())
    assert same_bits(npy(rows[:, :NP_]), want["dist"]) and same_bits(npy(a), want["arg"]) and tuple(a.shape) == (B, NP_)
    d2, a2, sm2, sa2 = call(want_dist=False)
    assert d2 is None and a2 is None and same_bits(npy(sm2), want["seg_min"]) and same_bits(npy(sa2), want["seg_arg"])
    assert same_bits(npy(sm), want["seg_min"]) and same_bits(npy(sa), want["seg_arg"])
    outs = []
    for _ in range(2):
        for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                outs.append(call(want_arg=True))
            torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for d3, a3, sm3, sa3 in outs:
        assert same_bits(npy(d3), want["dist"]) and same_bits(npy(a3), want["arg"]) and same_bits(npy(sm3), want["seg_min"])
        assert same_bits(npy(sa3), want["seg_arg"])


def test_an_empty_segment_in_the_middle(sc):
    seg = [3, 0, NP_ - 3]
    want = RF.restate(pad_parts(sc), sc["R"], sc["T"], sc["pts"], sc["carrier"], p1=sc["n_parts"], segments=seg)
    d, (sm, sa) = sc["tsdf"].query_points(sc["dev"]["pts"], sc["dev"]["R"], sc["dev"]["T"], carrier=sc["carrier"], parts=(0, sc["n_parts"]),
                                          segments=seg)
    assert same_bits(npy(d), want["dist"]) and same_bits(npy(sm), want["seg_min"]) and same_bits(npy(sa), want["seg_arg"])
    assert bool((sm[:, 1] == 1).all()) and bool((sa[:, 1] == -1).all())


# ------------------------------------------------------------------------------------------- 6. the sensor and the timing tool
def test_contact_sensor_is_the_same_query(sc):
    from partmanip_amd.contact import ContactSensor
    want = sc["ref"]["shared_carried"][0]
    sensor = ContactSensor(sc["tsdf"], sc["pts"], sc["carrier"], SEG, targets=(0, sc["n_parts"]), names=("a", "b", "c"))
    r = sensor.sense(sc["dev"]["R"], sc["dev"]["T"])
    assert same_bits(npy(r.dist), want["dist"]) and same_bits(npy(r.arg), want["arg"])
    assert same_bits(npy(r.body_dist), want["seg_min"]) and same_bits(npy(r.body_point), want["seg_arg"])
    r = sensor.sense(sc["dev"]["R"], sc["dev"]["T"], per_point=False)
    assert r.dist is None and r.arg is None and same_bits(npy(r.body_dist), want["seg_min"]) and sensor.body("c") == 2


def test_timing_tool_tiny_run():
    """tools/time_contact.py at its smallest size, in this process: it asserts that the kernel and its tensor-library baseline agree
    before it reports a time."""
    from tools import time_contact as tool
    rows = tool.sense_rows([4], tiny=True)
    assert {r["scene"] for r in rows} == {"cube", "cabinets"}
    for r in rows:
        assert r["hip_ms"] > 0 and r["torch_ms"] > 0 and r["max_abs_diff"] <= 1e-5 and r["in_range"] > 0.1 and r["cull_on_equals_off"]
    step, = tool.step_rows([4], steps=3)
    assert step["plain_step_ms"] > 0 and step["contact_step_ms"] > 0 and step["contact_grasp_step_ms"] > 0
