"""The open_drawer task step (partmanip_amd.tasks.OpenDrawerTensors, pm_open_drawer_post_f32, pm_open_drawer_reset_f32), everything
that needs no GPU: the numpy restatement of the contract (tests/open_drawer_ref.py) against the REFERENCE's outputs in the fixtures,
the fixtures' own conditions, argument validation of the C entry points, of the wrappers and of the constructor.

Tolerance rule (the one of tests/test_gpu_open_drawer.py): e_ref = max |out32 - out64| of a fixture's output group is what the
reference's own float32 run loses against its float64 run; the float32 restatement must stay within 4 e_ref of out64, the float64
restatement within 1e-12 (it is the same arithmetic in another association)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import yaml

from tests import grasp_cube_ref as G
from tests import open_drawer_ref as OD
from tests.helpers import GOLDEN, ROOT, load

FIXTURES = ["open_drawer_ref_small", "open_drawer_ref_70"]
GROUPS = ("normal_state", "part_bbox", "rew", "extras", "pose_R", "pose_T")
RUNS = (("ik_train", "ik", True, False), ("ik_test_rand", "ik", False, True), ("pos_train_rand", "pos", True, True),
        ("pos_test", "pos", False, False))


def generator():
    spec = importlib.util.spec_from_file_location("make_open_drawer_golden", os.path.join(GOLDEN, "make_open_drawer_golden.py"))
    m = importlib.util.module_from_spec(spec)
    keep = os.environ.get("PYTORCH_JIT")
    try:
        spec.loader.exec_module(m)                            # sets PYTORCH_JIT for its own run; irrelevant once torch is imported
    finally:
        if keep is None:
            os.environ.pop("PYTORCH_JIT", None)
        else:
            os.environ["PYTORCH_JIT"] = keep
    return m


def ref_post(fx, dtype=np.float64):
    return OD.post(fx["rigid_body_all"], fx["dof_state_all"], fx["root"], fx["rigid_body_mask"], fx["dof_state_mask"], int(fx["obj_actor"]),
                   int(fx["ltip"]), int(fx["rtip"]), fx["part_bbox_init"], fx["part_axis_dir_init"], fx["joint_lo"], fx["joint_hi"],
                   fx["dof_lo"], fx["dof_hi"], fx["obj_id"], fx["before_succ_objid"], fx["part_slot"], fx["part_C"], dtype=dtype)


def ref_pre(fx, post, drive, train, rnd, dtype=np.float64):
    """Restated begin_step on the fixture: (bookkeeping dict, root, dof_state_all, pos_act_all)."""
    nd = fx["dof_state_mask"].shape[1] - 1
    jl, jr = int(fx["ltip"]) - 1, int(fx["rtip"]) - 1
    tgt = G.control(fx["actions" if drive == "ik" else "actions_pos"], post["robot_dof_state"], fx["jac"], jl, jr, fx["dof_lo"],
                    fx["dof_hi"], float(fx["dt"]), drive, dtype=dtype)
    before = dict(rew=post["rew"], success=post["success"], progress=fx["before_progress"],
                  epis_max_rew=fx["before_epis_max_rew"].astype(dtype), epis_max_step=fx["before_epis_max_step"])
    s = G.bookkeeping(before, tgt, fx["default_dof_pos"].astype(dtype), int(fx["explore_step"]),
                      200 if train else int(fx["max_episode_length_test"]), train)
    root, dof, pa = OD.reset(s["reset"], s["pos_act"], fx["dof_state_mask"], fx["root"], fx["dof_state_all"], fx["pos_act_all_before"], 0,
                             int(fx["obj_actor"]), fx["robot_default_root"], fx["obj_default_root"], fx["default_dof_pos"],
                             fx["joint_lo"], fx["u"] if rnd else None, dtype=dtype)
    assert tgt.shape[1] == nd
    return s, root, dof, pa


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_restatement_reproduces_the_reference_float64(name):
    fx = load(name)
    got = ref_post(fx)
    for k in GROUPS:
        np.testing.assert_allclose(got[k], fx["out64_" + k], rtol=0, atol=1e-12, err_msg=k)
    for k in ("success", "is_reached", "succ_objid"):
        assert np.array_equal(got[k], fx["out64_" + k]), k
    # the bonus is 0.1 for any number of reach sub-flags: a counted bonus would differ here
    rf = got["reach_flags"]
    assert (rf.sum(axis=1) >= 2).any()
    np.testing.assert_allclose(got["extras"][:, 2] + G.norm(got["normal_state"][:, :3] - got["normal_state"][:, 13:16]), 0.1 * rf.any(axis=1),
                               rtol=0, atol=1e-12)
    for run, drive, train, rnd in RUNS:
        s, root, dof, pa = ref_pre(fx, got, drive, train, rnd)
        o = lambda k: fx[f"out64_{run}_{k}"]                    # noqa: E731
        assert np.array_equal(s["reset"], o("reset")) and np.array_equal(s["progress"], o("after_progress")), run
        assert np.array_equal(s["success"], o("after_success")) and np.array_equal(s["epis_max_step"], o("after_epis_max_step")), run
        np.testing.assert_allclose(s["epis_max_rew"], o("after_epis_max_rew"), rtol=0, atol=1e-12)
        np.testing.assert_allclose(pa, o("pos_act_all"), rtol=0, atol=1e-11, err_msg=run)
        np.testing.assert_allclose(root, o("root"), rtol=0, atol=1e-12, err_msg=run)
        np.testing.assert_allclose(dof, o("dof_state_all"), rtol=0, atol=1e-12, err_msg=run)
        if train:
            assert np.array_equal(s["reset_succ"], o("reset_succ"))
            assert np.float32(s["succ_rate"]) == o("succ_rate").reshape(-1)[0]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_generators_conditions_hold_on_the_committed_fixtures(name):
    fx = load(name)
    generator().check_conditions(fx)
    assert fx["root"].shape[0] == (5 if name.endswith("small") else 70)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= os.path.getsize(os.path.join(GOLDEN, "grasp_cube_ref_64.npz"))


def test_float32_restatement_is_within_the_reference_margin():
    """The association the kernels use (this restatement in float32) against the float64 reference: within 4 e_ref per group."""
    for name in FIXTURES:
        fx = load(name)
        got = ref_post(fx, np.float32)
        for k in GROUPS:
            assert got[k].dtype == np.float32, k
            e_ref = np.abs(fx["out32_" + k].astype(np.float64) - fx["out64_" + k]).max()
            err = np.abs(got[k].astype(np.float64) - fx["out64_" + k]).max()
            assert err <= 4 * e_ref, (k, err, e_ref)
        assert np.array_equal(got["success"], fx["out64_success"]) and np.array_equal(got["is_reached"], fx["out64_is_reached"])


def test_build_masks_follows_the_reference_layout():
    from partmanip_amd.tasks.open_drawer import build_masks, default_part_slot
    fx = load("open_drawer_ref_70")
    g = generator()
    N = 70
    types = [g.TYPES[i % 3] for i in range(N)]
    rb, dm, B, D = build_masks(13, 9, [t[0] for t in types], [t[1] for t in types], [t[2] for t in types], [t[3] for t in types],
                               [t[4] for t in types])
    assert rb.dtype == np.int32 and np.array_equal(rb, fx["rigid_body_mask"]) and np.array_equal(dm, fx["dof_state_mask"])
    assert (B, D) == (fx["rigid_body_all"].shape[0], fx["dof_state_all"].shape[0])
    assert default_part_slot(13) == fx["part_slot"].tolist() == list(range(10)) + [11, 13, 14]


def make_task(fx, device="cpu", **kw):
    from partmanip_amd.tasks import OpenDrawerTensors
    N = fx["root"].shape[0]
    cfg = {"robot": {"driveMode": "ik", "dof": fx["default_dof_pos"].tolist(), "root": fx["robot_default_root"].tolist()},
           "explore_step": int(fx["explore_step"]), "maxEpisodeLength": 200}
    args = dict(rigid_body_mask=fx["rigid_body_mask"], dof_state_mask=fx["dof_state_mask"], obj_id=fx["obj_id"],
                part_bbox_init=fx["part_bbox_init"], part_axis_dir_init=fx["part_axis_dir_init"],
                part_joint_lower_limits=fx["joint_lo"], part_joint_upper_limits=fx["joint_hi"], num_objs=int(fx["num_objs"]),
                num_rigid_bodies=fx["rigid_body_all"].shape[0], num_dof_states=fx["dof_state_all"].shape[0])
    args.update(kw)
    return OpenDrawerTensors(N, device, cfg, float(fx["dt"]), **args)


def test_constructor_checks_the_masks_and_constants_once_on_the_host():
    fx = load("open_drawer_ref_small")
    task = make_task(fx)
    assert task.rigid_body_mask.dtype == torch.int32 and task.dof_state_mask.dtype == torch.int32 and task.obj_id.dtype == torch.int32
    assert task.num_actions == 7 and task.num_obs == {"normal_state": 47}
    assert np.array_equal(task.part_C.numpy(), fx["part_C"]) and np.array_equal(task.part_slot.numpy(), fx["part_slot"])
    assert np.array_equal(task.obj_default_root.numpy(), fx["obj_default_root"])
    assert task.extras["success_objnum"] is task.succ_objid_lst and tuple(task.succ_objid_lst.shape) == (3,)
    assert task.num_rigid_bodies == fx["rigid_body_all"].shape[0]
    assert make_task(fx, num_rigid_bodies=None, num_dof_states=None).num_dof_states == int(fx["dof_state_mask"].max()) + 1
    B, D = fx["rigid_body_all"].shape[0], fx["dof_state_all"].shape[0]
    bad = fx["rigid_body_mask"].copy()
    bad[2, 14] = B
    with pytest.raises(ValueError, match="rigid_body_mask"):
        make_task(fx, rigid_body_mask=bad)
    bad[2, 14] = -1
    with pytest.raises(ValueError, match="rigid_body_mask"):
        make_task(fx, rigid_body_mask=bad, num_rigid_bodies=None)
    bad = fx["dof_state_mask"].copy()
    bad[4, 9] = D
    with pytest.raises(ValueError, match="dof_state_mask"):
        make_task(fx, dof_state_mask=bad)
    bad = fx["dof_state_mask"].copy()
    bad[1, 9] = bad[0, 3]                                      # two environments would write one row
    with pytest.raises(ValueError, match="twice"):
        make_task(fx, dof_state_mask=bad)
    with pytest.raises(ValueError, match="dof_state_mask"):
        make_task(fx, dof_state_mask=fx["dof_state_mask"][:, :9])
    with pytest.raises(ValueError, match="rigid_body_mask"):
        make_task(fx, rigid_body_mask=fx["rigid_body_mask"].astype(np.float32))
    with pytest.raises(ValueError, match="obj_id"):
        make_task(fx, obj_id=np.array([0, 1, 3, 0, 1]))
    with pytest.raises(ValueError, match="obj_id"):
        make_task(fx, num_objs=2)
    with pytest.raises(ValueError, match="part_bbox_init"):
        make_task(fx, part_bbox_init=fx["part_bbox_init"][:, :7])
    with pytest.raises(ValueError, match="part_joint_upper_limits"):
        make_task(fx, part_joint_upper_limits=fx["joint_hi"][:4])
    with pytest.raises(ValueError, match="actors"):
        make_task(fx, obj_actor=0)
    # state tensors shorter than the masks reach are refused before any launch
    t = lambda k: torch.from_numpy(fx[k])                     # noqa: E731
    with pytest.raises(ValueError, match="rigid_body_all"):
        task.end_step(t("rigid_body_all")[:-1], t("dof_state_all"), t("root"))
    with pytest.raises(ValueError, match="dof_state_all"):
        task.begin_step(t("actions"), t("jac"), t("dof_state_all")[:-1], t("root"), torch.zeros(D - 1))
    with pytest.raises(ValueError, match="pos_act_all"):
        task.begin_step(t("actions"), t("jac"), t("dof_state_all"), t("root"), torch.zeros(D + 1))


def test_shipped_yaml_asks_for_the_mobile_base_and_is_refused():
    import tasks
    from partmanip_amd.tasks import OpenDrawerTensors
    assert tasks.OpenDrawerTensors is OpenDrawerTensors
    fx = load("open_drawer_ref_small")
    with open(os.path.join(ROOT, "cfg", "tasks", "open_drawer.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["obs_mode"]["normal_state"] == 29 + 2 * 12       # the mobile Franka's 12 DOFs
    with pytest.raises(NotImplementedError, match="mobile"):
        OpenDrawerTensors(5, "cpu", cfg, 1 / 60, fx["rigid_body_mask"], fx["dof_state_mask"], fx["obj_id"], fx["part_bbox_init"],
                          fx["part_axis_dir_init"], fx["joint_lo"], fx["joint_hi"], 3)
    for mode in ("ik_abs", "heuristic"):
        with pytest.raises(NotImplementedError, match=mode):
            OpenDrawerTensors(5, "cpu", {"robot": {"driveMode": mode}}, 1 / 60, fx["rigid_body_mask"], fx["dof_state_mask"], fx["obj_id"],
                              fx["part_bbox_init"], fx["part_axis_dir_init"], fx["joint_lo"], fx["joint_hi"], 3)
    assert "mobile" in OpenDrawerTensors.__doc__ and "NotImplementedError" in OpenDrawerTensors.__doc__


def post_args(fx):
    t = lambda k, d=None: torch.from_numpy(fx[k] if d is None else fx[k].astype(d))   # noqa: E731
    return dict(rigid_body_all=t("rigid_body_all"), dof_state_all=t("dof_state_all"), root=t("root"), rigid_body_mask=t("rigid_body_mask"),
                dof_state_mask=t("dof_state_mask"), obj_actor=1, ltip=10, rtip=12, part_bbox_init=t("part_bbox_init"),
                part_axis_dir_init=t("part_axis_dir_init"), joint_lo=t("joint_lo"), joint_hi=t("joint_hi"), dof_lo=t("dof_lo"),
                dof_hi=t("dof_hi"))


def test_ops_reject_bad_arguments_and_cpu_tensors():
    from partmanip_amd import ops
    fx = load("open_drawer_ref_small")
    N, D = 5, fx["dof_state_all"].shape[0]
    a = post_args(fx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.open_drawer_post(**a)
    bad = [("rigid_body_all", a["rigid_body_all"][:, :12]), ("rigid_body_all", a["rigid_body_all"].double()),
           ("dof_state_all", a["dof_state_all"].reshape(-1)), ("root", a["root"][:, :, :12]),
           ("rigid_body_mask", a["rigid_body_mask"].long()), ("dof_state_mask", a["dof_state_mask"][:4]),
           ("dof_state_mask", a["dof_state_mask"].t()), ("part_bbox_init", a["part_bbox_init"][:, :4]),
           ("part_axis_dir_init", a["part_axis_dir_init"].double()), ("joint_lo", a["joint_lo"][:3]), ("dof_hi", a["dof_hi"][:8]),
           ("obj_actor", 2), ("ltip", 13), ("rtip", -1)]
    for k, v in bad:
        with pytest.raises(ValueError):
            ops.open_drawer_post(**{**a, k: v})
    outs = [dict(normal_state=torch.zeros(N, 46)), dict(extras=torch.zeros(N, 7)), dict(rew=torch.zeros(N + 1)),
            dict(success=torch.zeros(N)), dict(part_bbox=torch.zeros(N, 24)), dict(robot_dof_state=torch.zeros(N, 10, 2)),
            dict(part_dof_state=torch.zeros(N, 1)), dict(succ_objid=torch.zeros(3, dtype=torch.bool)),
            dict(succ_objid=torch.zeros(3), obj_id=torch.zeros(N, dtype=torch.int32)),
            dict(succ_objid=torch.zeros(3, dtype=torch.bool), obj_id=torch.zeros(N, dtype=torch.int64)),
            dict(pose_R=torch.zeros(N, 13, 3, 3)), dict(pose_R=torch.zeros(N, 12, 3, 3), part_slot=torch.zeros(13, dtype=torch.int32)),
            dict(pose_T=torch.zeros(N, 13, 3), part_slot=torch.zeros(13, dtype=torch.int32), part_C=torch.zeros(12, 3, 3))]
    for kw in outs:
        with pytest.raises(ValueError):
            ops.open_drawer_post(**a, **kw)
    r = dict(reset=torch.zeros(N, dtype=torch.bool), pos_act=torch.zeros(N, 9), dof_state_mask=a["dof_state_mask"], root=a["root"].clone(),
             dof_state_all=a["dof_state_all"].clone(), pos_act_all=torch.zeros(D), robot_actor=0, obj_actor=1,
             robot_default_root=torch.zeros(7), obj_default_root=torch.zeros(7), default_dof_pos=torch.zeros(9), joint_lo=a["joint_lo"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.open_drawer_reset(**r)
    for k, v in (("reset", torch.zeros(N)), ("pos_act", torch.zeros(N, 8)), ("pos_act_all", torch.zeros(D - 1)), ("obj_actor", 0),
                 ("robot_actor", 2), ("robot_default_root", torch.zeros(13)), ("default_dof_pos", torch.zeros(10)),
                 ("u", torch.zeros(N, 3)), ("dof_state_mask", a["dof_state_mask"].long()), ("robot_dof_state", torch.zeros(N, 9)),
                 ("part_dof_state", torch.zeros(N, 2).double())):
        with pytest.raises(ValueError):
            ops.open_drawer_reset(**{**r, k: v})


def test_c_entry_points_reject_null_pointers_and_bad_sizes():
    from partmanip_amd._lib import lib
    one = ctypes.c_void_p(16)                                 # a non-null address that is never dereferenced on these paths

    def post(rb=one, B=100, D=60, N=4, nrb=13, nd=9, na=2, obj=1, lt=10, rt=12, obj_id=one, num_objs=3, ns_stride=47, ex_stride=8,
             part_slot=one, M=13, pose_R=one, succ_objid=one):
        return lib.pm_open_drawer_post_f32(rb, B, one, D, one, N, nrb, nd, na, obj, lt, rt, one, one, obj_id, num_objs, one, one, one,
                                           one, one, one, 0.5, part_slot, None, M, one, ns_stride, one, one, one, one, one, ex_stride,
                                           succ_objid, one, one, pose_R, one, None)

    assert post(rb=None) == -1 and post(N=0) == -1 and post(nrb=0) == -1 and post(nd=0) == -1 and post(B=0) == -1 and post(D=0) == -1
    assert post(B=2 ** 31) == -1 and post(obj=2) == -1 and post(lt=13) == -1 and post(rt=-1) == -1
    assert post(ns_stride=46) == -1 and post(ex_stride=7) == -1 and post(obj_id=None) == -1 and post(num_objs=0) == -1
    assert post(part_slot=None) == -1 and post(M=0) == -1 and post(nrb=1000, lt=0, rt=0) == -1

    def rst(reset=one, N=4, nd=9, na=2, ra=0, oa=1, rnd=0, u=None, D=60, root=one):
        return lib.pm_open_drawer_reset_f32(reset, one, one, N, nd, na, ra, oa, one, one, rnd, u, 0.05, 0.26, one, one, root, one, D, one,
                                            None, None, None)

    assert rst(reset=None) == -1 and rst(N=0) == -1 and rst(nd=0) == -1 and rst(na=0) == -1 and rst(D=0) == -1 and rst(root=None) == -1
    assert rst(ra=2) == -1 and rst(oa=-1) == -1 and rst(ra=1) == -1 and rst(rnd=1) == -1 and rst(D=2 ** 31) == -1


def test_abi_version():
    from partmanip_amd import _lib
    assert _lib.ABI_VERSION >= 157 and _lib.lib.pm_version() == _lib.ABI_VERSION
