"""The mobile Franka (partmanip_amd.tasks.MobileFranka, pm_franka_control_mobile_f32), everything that needs no GPU: the fixtures' own
conditions on the committed files, the numpy restatement of the contract (tests/mobile_franka_ref.py) against the REFERENCE's float64
outputs, the robot description, the task classes around it, argument validation of the C entry point and of the wrapper.

Tolerance: the float64 restatement is the reference's arithmetic in another association (a solve for its inverse): within 1e-12."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import yaml

from tests import mobile_franka_ref as MF
from tests.helpers import GOLDEN, ROOT, load

FIXTURES = ["mobile_franka_ref_small", "mobile_franka_ref_70"]
GROUPS = ("normal_state", "part_bbox", "rew", "extras", "pose_R", "pose_T")
RUNS = (("ik_train", "ik", True, False), ("ik_test_rand", "ik", False, True), ("pos_train_rand", "pos", True, True),
        ("pos_test", "pos", False, False))
MESH = [3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15]
SHIPPED_ROOT = [0.4, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
SHIPPED_DOF = [0, 0, 0, -0.2724, -0.1511, 0.2898, -2.3792, -2.8973, 2.4690, 2.3973, 0.04, 0.04]


def generator():
    spec = importlib.util.spec_from_file_location("make_mobile_franka_golden", os.path.join(GOLDEN, "make_mobile_franka_golden.py"))
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


@pytest.mark.parametrize("name", FIXTURES)
def test_the_generators_conditions_hold_on_the_committed_fixtures(name):
    fx = load(name)
    keep = os.environ.get("PYTORCH_JIT")
    try:
        generator().check_conditions(fx)
    finally:
        if keep is None:
            os.environ.pop("PYTORCH_JIT", None)
        else:
            os.environ["PYTORCH_JIT"] = keep
    N = 5 if name.endswith("small") else 70
    assert fx["root"].shape[0] == N and fx["dof_state_mask"].shape == (N, 13) and fx["rigid_body_mask"].shape == (N, 19)
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= os.path.getsize(os.path.join(GOLDEN, "grasp_cube_ref_64.npz"))
    if N == 5:                                                # the reference's shipped robot
        assert np.array_equal(fx["robot_default_root"], np.float32(SHIPPED_ROOT)) and np.array_equal(fx["default_dof_pos"], np.float32(SHIPPED_DOF))


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_restatement_reproduces_the_reference_float64(name):
    fx = load(name)
    after = MF.post(fx)
    assert after["normal_state"].shape[1] == 53
    for k in GROUPS:
        np.testing.assert_allclose(after[k], fx["out64_" + k], rtol=0, atol=1e-12, err_msg=k)
    for k in ("success", "is_reached", "succ_objid"):
        assert np.array_equal(after[k], fx["out64_" + k]), k
    for run, drive, train, rnd in RUNS:
        s, _, root, dof, pa = MF.begin_step(fx, after, drive, train, rnd)
        o = lambda k: fx[f"out64_{run}_{k}"]                    # noqa: E731
        assert np.array_equal(s["reset"], o("reset")) and np.array_equal(s["progress"], o("after_progress")), run
        assert np.array_equal(s["success"], o("after_success")) and np.array_equal(s["epis_max_step"], o("after_epis_max_step")), run
        np.testing.assert_allclose(s["epis_max_rew"], o("after_epis_max_rew"), rtol=0, atol=1e-12)
        np.testing.assert_allclose(pa, o("pos_act_all"), rtol=0, atol=1e-12, err_msg=run)
        np.testing.assert_allclose(root, o("root"), rtol=0, atol=1e-12, err_msg=run)
        np.testing.assert_allclose(dof, o("dof_state_all"), rtol=0, atol=1e-12, err_msg=run)
        if train:
            assert np.array_equal(s["reset_succ"], o("reset_succ"))
            assert np.float32(s["succ_rate"]) == o("succ_rate").reshape(-1)[0]


def test_float32_restatement_is_within_the_reference_margin():
    """The restated drive in float32 against the float64 reference: within 4 e_ref of the targets, the rule of the GPU tests."""
    for name in FIXTURES:
        fx = load(name)
        after = MF.post(fx)
        for run, drive, train, rnd in RUNS:
            pa = MF.begin_step(fx, after, drive, train, rnd, dtype=np.float32)[4]
            assert pa.dtype == np.float32
            want = fx[f"out64_{run}_pos_act_all"]
            e_ref = np.abs(fx[f"out32_{run}_pos_act_all"].astype(np.float64) - want).max()
            assert np.abs(pa.astype(np.float64) - want).max() <= 4 * e_ref, (name, run)


def test_mobile_franka_defaults_action_counts_and_refusals():
    import tasks
    from partmanip_amd.tasks import Franka, MobileFranka
    from partmanip_amd.tasks.franka import PANDA_DOF_LOWER, PANDA_DOF_UPPER
    assert tasks.MobileFranka is MobileFranka
    for cfg in ({}, {"mobile": True}, {"assetFile": "franka_panda_sdf_mobile"}, {"mobile": True, "assetFile": "franka_panda_sdf_mobile"}):
        r = MobileFranka({"driveMode": "ik", **cfg}, 1 / 60, 4, "cpu")
        assert r.mobile is True and r.num_base_dofs == 3 and r.num_actions == 10 and r.num_dofs == 12 and r.num_rigid_body == 17
        assert (r.ltip_rb_index, r.rtip_rb_index) == (14, 16) and list(r.mesh_bodies) == MESH and r.driveMode == "ik"
    assert MobileFranka({"driveMode": "pos"}, 1 / 60, 4, "cpu").num_actions == 11
    assert MobileFranka({}, 1 / 60, 4, "cpu").num_actions == 10                        # 'ik' is the default drive, as in Franka
    lo, hi = r.dof_lower_limits_tensor.numpy(), r.dof_upper_limits_tensor.numpy()
    assert np.array_equal(lo, np.float32((-0.2, -0.2, -0.1) + PANDA_DOF_LOWER)) and np.array_equal(hi, np.float32((0.2, 0.2, 0.1) + PANDA_DOF_UPPER))
    want = (lo + hi) / 2
    want[:3], want[-2:] = 0, hi[-2:]
    assert np.array_equal(r.default_dof_pos.numpy(), want)                            # base 0, arm mid-range, gripper open
    assert np.array_equal(r.default_root.numpy(), np.float32([0, 0, 0, 0, 0, 0, 1])) and np.array_equal(r.base_R.numpy(), np.eye(3, dtype=np.float32))
    assert tuple(r.coordinate_transform_matrix.shape) == (11, 3, 3)
    for k in ("device", "num_envs", "dt", "driveMode", "num_actions", "dof_lower_limits_tensor", "dof_upper_limits_tensor",
              "default_dof_pos", "default_root", "coordinate_transform_matrix", "ltip_rb_index", "rtip_rb_index"):
        assert hasattr(r, k) and hasattr(Franka({}, 1 / 60, 4, "cpu"), k), k
    # robot.root / robot.dof; base_R is the reference's quat_to_mat of the root quaternion, float32, contiguous
    for name in FIXTURES:
        fx = load(name)
        r = MobileFranka({"root": fx["robot_default_root"].tolist(), "dof": fx["default_dof_pos"].tolist()}, 1 / 60, 4, "cpu")
        assert np.array_equal(r.default_dof_pos.numpy(), fx["default_dof_pos"]) and np.array_equal(r.default_root.numpy(), fx["robot_default_root"])
        assert r.base_R.dtype == torch.float32 and tuple(r.base_R.shape) == (3, 3) and r.base_R.is_contiguous()
        np.testing.assert_allclose(r.base_R.numpy(), MF.base_matrix(fx["robot_default_root"]), rtol=0, atol=4 * np.finfo(np.float32).eps)
    assert np.abs(r.base_R.numpy() - r.base_R.numpy().T).max() >= 0.3
    # a simulator's own layout overrides the defaults
    r = MobileFranka({}, 1 / 60, 4, "cpu", num_dofs=10, num_rigid_body=15, dof_lower=[-1] * 10, dof_upper=[1] * 10, ltip_rb_index=12,
                     rtip_rb_index=14, mesh_bodies=range(3, 14))
    assert r.num_actions == 10 and r.mesh_bodies == tuple(range(3, 14)) and r.default_dof_pos.tolist() == [0] * 8 + [1, 1]
    assert MobileFranka({"driveMode": "pos"}, 1 / 60, 4, "cpu", num_dofs=10, dof_lower=[-1] * 10, dof_upper=[1] * 10).num_actions == 9
    for mode in ("ik_abs", "heuristic"):
        with pytest.raises(NotImplementedError, match=mode):
            MobileFranka({"driveMode": mode}, 1 / 60, 4, "cpu")
    with pytest.raises(NotImplementedError, match="torque"):
        MobileFranka({"driveMode": "torque"}, 1 / 60, 4, "cpu")
    bad = [dict(ltip_rb_index=17), dict(rtip_rb_index=-1), dict(mesh_bodies=[3, 4, 17]), dict(mesh_bodies=[-1]), dict(num_rigid_body=16),
           dict(num_dofs=11), dict(num_dofs=5, dof_lower=[0] * 5, dof_upper=[1] * 5), dict(dof_lower=[0] * 11, dof_upper=[1] * 11),
           dict(dof_lower=[0] * 12), dict(num_dofs=13, dof_lower=[0] * 12, dof_upper=[1] * 12)]
    for kw in bad:
        with pytest.raises(ValueError):
            MobileFranka({}, 1 / 60, 4, "cpu", **kw)
    with pytest.raises(ValueError, match="robot.dof"):
        MobileFranka({"dof": [0.0] * 9}, 1 / 60, 4, "cpu")
    with pytest.raises(ValueError, match="robot.root"):
        MobileFranka({"root": [0.0] * 3}, 1 / 60, 4, "cpu")


def drawer_args(fx):
    return (fx["rigid_body_mask"], fx["dof_state_mask"], fx["obj_id"], fx["part_bbox_init"], fx["part_axis_dir_init"], fx["joint_lo"],
            fx["joint_hi"], int(fx["num_objs"]))


def test_the_shipped_yaml_builds_with_a_mobile_franka_and_is_still_refused_without():
    from partmanip_amd.tasks import Franka, GraspCubeTensors, MobileFranka, OpenDrawerTensors
    fx = load("mobile_franka_ref_small")
    with open(os.path.join(ROOT, "cfg", "tasks", "open_drawer.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["robot"]["mobile"] is True
    robot = MobileFranka(cfg["robot"], 1 / 60, 5, "cpu")
    task = OpenDrawerTensors(5, "cpu", cfg, 1 / 60, *drawer_args(fx), robot=robot)
    assert task.num_obs["normal_state"] == cfg["obs_mode"]["normal_state"] == 53 and task.num_actions == 10
    assert tuple(task.obs_buf["normal_state"].shape) == (5, 53) and tuple(task.pos_act.shape) == (5, 12)
    assert tuple(task.robot_dof_state.shape) == (5, 12, 2) and tuple(task.pose_R.shape) == (5, 13, 3, 3)
    assert task.robot is robot and np.array_equal(task.robot_default_root.numpy(), np.float32([0, 0, 0, 0, 0, 0, 1]))
    # default part slots of both tasks: the robot's mesh bodies, then the link and the handle / the cube
    assert task.part_slot.tolist() == MESH + [17, 18] == fx["part_slot"].tolist() and np.array_equal(task.part_C.numpy(), fx["part_C"])
    cube = GraspCubeTensors(5, "cpu", {}, 1 / 60, num_bodies=18, robot=robot)
    assert cube.part_body.tolist() == MESH + [17] and tuple(cube.part_C.shape) == (12, 3, 3) and cube.num_actions == 10
    assert np.array_equal(cube.part_C.numpy()[:11], fx["part_C"][:11]) and np.array_equal(cube.part_C.numpy()[11], np.eye(3))
    assert cube.num_obs == {"normal_state": 43, "proprio_state": 31} and tuple(cube.pos_act.shape) == (5, 12)
    # explicit part lists still win; the fixed-base defaults are what they were
    assert OpenDrawerTensors(5, "cpu", cfg, 1 / 60, *drawer_args(fx), robot=robot, part_slot=[17, 18]).part_slot.tolist() == [17, 18]
    assert GraspCubeTensors(5, "cpu", {}, 1 / 60).part_body.tolist() == list(range(10)) + [11, 13]
    # without robot= the refusals stand
    with pytest.raises(NotImplementedError, match="mobile"):
        OpenDrawerTensors(5, "cpu", cfg, 1 / 60, *drawer_args(fx))
    with pytest.raises(NotImplementedError, match="mobile"):
        GraspCubeTensors(4, "cpu", {"robot": {"driveMode": "ik", "assetFile": "franka_panda_sdf_mobile"}}, 1 / 60)
    with pytest.raises(NotImplementedError, match="mobile"):
        Franka({"driveMode": "ik", "mobile": True}, 1 / 60, 4, "cpu")
    with pytest.raises(NotImplementedError, match="mobile"):
        Franka({"driveMode": "ik", "assetFile": "franka_panda_sdf_mobile"}, 1 / 60, 4, "cpu")
    for cls in (OpenDrawerTensors, GraspCubeTensors):
        doc = cls.__doc__ + __import__(cls.__module__, fromlist=["x"]).__doc__
        assert "mobile" in doc and "NotImplementedError" in doc and "MobileFranka" in doc
    assert "mobile" in OpenDrawerTensors.__doc__ and "NotImplementedError" in OpenDrawerTensors.__doc__
    # the wrappers refuse CPU tensors: there is no fall-back
    t = lambda k: torch.from_numpy(fx[k])                     # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        task.begin_step(t("actions"), t("jac"), t("dof_state_all"), t("root"), t("pos_act_all_before"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        task.end_step(t("rigid_body_all"), t("dof_state_all"), t("root"))


def test_abi_version():
    from partmanip_amd import _lib
    assert _lib.ABI_VERSION >= 158 and _lib.lib.pm_version() == _lib.ABI_VERSION
    assert "pm_franka_control_mobile_f32" in _lib.SIGNATURES


def test_c_entry_point_rejects_null_pointers_and_bad_sizes():
    from partmanip_amd._lib import lib
    one = ctypes.c_void_p(16)                                 # a non-null address that is never dereferenced on these paths

    def ctl(actions=one, A=10, N=4, nd=12, nl=16, jl=13, jr=15, jac=one, mode=0, slot=0, counters=one, act_stride=10, nbase=3, base_R=one,
            pos_act=one):
        return lib.pm_franka_control_mobile_f32(actions, act_stride, A, one, jac, N, nd, nl, jl, jr, one, one, one, 1 / 60, mode, nbase,
                                                base_R, one, one, one, 40, 200, 1, pos_act, one, one, one, one, counters, slot, None)

    assert ctl(nbase=0, A=7) == -1 and ctl(nbase=0) == -1 and ctl(nbase=2, A=9) == -1 and ctl(nbase=4, A=11) == -1 and ctl(nbase=-3) == -1
    assert ctl(base_R=None) == -1
    assert ctl(nd=5) == -1 and ctl(nd=5, mode=1, A=4, act_stride=4) == -1 and ctl(nd=65) == -1 and ctl(nd=65, mode=1, A=64, act_stride=64) == -1
    assert ctl(A=7) == -1 and ctl(A=11, act_stride=11) == -1 and ctl(mode=1, A=10) == -1 and ctl(mode=1, A=8, act_stride=8) == -1
    # everything the fixed-base entry point refuses
    assert ctl(actions=None) == -1 and ctl(N=0) == -1 and ctl(jac=None) == -1 and ctl(jl=16) == -1 and ctl(jr=-1) == -1 and ctl(nl=0) == -1
    assert ctl(mode=2) == -1 and ctl(slot=2) == -1 and ctl(counters=None) == -1 and ctl(act_stride=9) == -1 and ctl(pos_act=None) == -1
    assert ctl(mode=1, A=11, act_stride=10) == -1


def control_args(fx, **kw):
    N = fx["root"].shape[0]
    t = lambda k: torch.from_numpy(fx[k])                     # noqa: E731
    a = dict(actions=t("actions"), dof_state=torch.from_numpy(fx["dof_state_all"][fx["dof_state_mask"][:, :12]]), jac=t("jac"), jl=13, jr=15,
             dof_lo=t("dof_lo"), dof_hi=t("dof_hi"), default_dof_pos=t("default_dof_pos"), dt=1 / 60, drive_mode="ik", rew=torch.zeros(N),
             success=torch.zeros(N, dtype=torch.bool), progress=torch.zeros(N, dtype=torch.long), explore_step=40, max_episode_length=200,
             train=True, pos_act=torch.zeros(N, 12), epis_max_rew=torch.zeros(N), epis_max_step=torch.zeros(N, dtype=torch.long),
             reset=torch.zeros(N, dtype=torch.bool), reset_succ=torch.zeros(N, dtype=torch.bool), counters=torch.zeros(4, dtype=torch.int32),
             slot=0, num_base_dofs=3, base_R=torch.eye(3))
    a.update(kw)
    return a


def test_ops_franka_control_refuses_bad_mobile_arguments_and_cpu_tensors():
    from partmanip_amd import ops
    fx = load("mobile_franka_ref_small")
    t = lambda k: torch.from_numpy(fx[k])                     # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.franka_control(**control_args(fx))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.franka_control(**control_args(fx, drive_mode="pos", actions=t("actions_pos"), jac=None))
    bad = [dict(actions=t("actions")[:, :7]), dict(actions=t("actions_pos")), dict(drive_mode="pos"), dict(actions=t("actions").double()),
           dict(drive_mode="pos", actions=t("actions_pos")[:, :8]),
           dict(base_R=None), dict(base_R=torch.eye(4)), dict(base_R=torch.eye(3).reshape(9)), dict(base_R=torch.eye(3).double()),
           dict(base_R=torch.zeros(3, 6)[:, ::2]), dict(num_base_dofs=2), dict(jac=t("jac")[:, :, :, :9]), dict(jac=None), dict(jl=16),
           dict(dof_state=torch.zeros(5, 5, 2)), dict(pos_act=torch.zeros(5, 9)), dict(drive_mode="ik_abs")]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.franka_control(**control_args(fx, **kw))
    # the fixed-base call keeps its order: the device first
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.franka_control(**control_args(fx, num_base_dofs=0, base_R=None))
