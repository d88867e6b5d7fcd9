"""Host side of the kinematic articulation: the URDF parser (partmanip_amd/urdf.py) on the two shipped Franka assets and on small
URDFs written here, and the tests' own float64 reference (tests/kinematics_ref.py) held against closed forms and against central
differences of itself.  No GPU."""
import os

import numpy as np
import pytest

from partmanip_amd.urdf import FIXED, PRISMATIC, REVOLUTE, load_urdf, rpy_to_quat
from tests import kinematics_ref as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXED_URDF = os.path.join(GOLDEN, "franka_panda_sdf.urdf")
MOBILE_URDF = os.path.join(GOLDEN, "franka_panda_sdf_mobile.urdf")
ARM = [f"panda_link{i}" for i in range(8)] + ["panda_hand", "panda_leftfinger", "panda_lefttip", "panda_rightfinger", "panda_righttip"]

TOY = """<robot name="toy">
  <link name="base"/><link name="slider"/><link name="l1"/><link name="l2"/><link name="tip"/>
  <joint name="slide" type="prismatic"><parent link="base"/><child link="slider"/><axis xyz="2 0 0"/>
    <limit lower="-1" upper="1" velocity="0.5"/></joint>
  <joint name="j1" type="revolute"><parent link="slider"/><child link="l1"/><axis xyz="0 0 1"/>
    <limit lower="-3" upper="3" velocity="2"/></joint>
  <joint name="j2" type="continuous"><parent link="l1"/><child link="l2"/><origin xyz="1 0 0"/><axis xyz="0 0 1"/></joint>
  <joint name="jt" type="fixed"><parent link="l2"/><child link="tip"/><origin xyz="0.5 0 0"/></joint>
</robot>"""


def test_fixed_base_franka_parses_to_the_existing_defaults():
    from partmanip_amd.tasks.franka import PANDA_DOF_LOWER, PANDA_DOF_UPPER, Franka
    tree = load_urdf(FIXED_URDF)
    assert (tree.num_bodies, tree.num_dofs) == (13, 9) and tree.names == ARM
    assert tree.parent.tolist() == [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 11]
    assert tree.jtype.tolist() == [FIXED] + [REVOLUTE] * 7 + [FIXED, PRISMATIC, FIXED, PRISMATIC, FIXED]
    assert tree.dof.tolist() == [-1, 0, 1, 2, 3, 4, 5, 6, -1, 7, -1, 8, -1]
    assert tuple(tree.lower) == PANDA_DOF_LOWER and tuple(tree.upper) == PANDA_DOF_UPPER
    assert tree.velocity.tolist() == [2.175] * 4 + [2.61] * 3 + [0.2, 0.2]
    assert (tree.body_index("panda_lefttip"), tree.body_index("panda_righttip")) == (10, 12)
    assert "panda_link8" not in tree.names                    # commented out in the asset
    assert tree.anc_mask.tolist() == [0, 1, 3, 7, 15, 31, 63, 127, 127, 127 | 128, 127 | 128, 127 | 256, 127 | 256]
    kw = tree.robot_kwargs()
    assert "mesh_bodies" not in kw and kw["num_rigid_body"] == 13 and kw["num_dofs"] == 9
    r = Franka({"driveMode": "ik"}, 1 / 60, 4, "cpu", **kw)
    d = Franka({"driveMode": "ik"}, 1 / 60, 4, "cpu")        # the asset gives what the defaults assume
    assert (r.ltip_rb_index, r.rtip_rb_index, r.num_rigid_body) == (d.ltip_rb_index, d.rtip_rb_index, d.num_rigid_body)
    assert np.array_equal(r.dof_lower_limits_tensor.numpy(), d.dof_lower_limits_tensor.numpy())
    with pytest.raises(KeyError, match="panda_link8"):
        tree.body_index("panda_link8")


def test_mobile_franka_parses_to_16_bodies_not_the_17_of_the_defaults():
    from partmanip_amd.tasks.franka import MOBILE_BASE_LOWER, MOBILE_BASE_UPPER, PANDA_DOF_LOWER, PANDA_DOF_UPPER, MobileFranka
    tree = load_urdf(MOBILE_URDF)
    assert (tree.num_bodies, tree.num_dofs) == (16, 12)
    assert tree.names == ["panda_base0", "panda_base1", "panda_base2"] + ARM
    assert tree.jtype[:4].tolist() == [FIXED, PRISMATIC, PRISMATIC, PRISMATIC] and tree.dof[:4].tolist() == [-1, 0, 1, 2]
    assert tuple(tree.lower) == MOBILE_BASE_LOWER + PANDA_DOF_LOWER and tuple(tree.upper) == MOBILE_BASE_UPPER + PANDA_DOF_UPPER
    assert tree.mesh_bodies() == (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14)
    kw = tree.robot_kwargs()
    assert (kw["ltip_rb_index"], kw["rtip_rb_index"], kw["mesh_bodies"]) == (13, 15, tree.mesh_bodies())
    r = MobileFranka({"driveMode": "ik"}, 1 / 60, 4, "cpu", **kw)
    assert (r.num_rigid_body, r.num_dofs, r.num_actions, r.mesh_bodies) == (16, 12, 10, tree.mesh_bodies())
    assert np.array_equal(tree.axis[1:4], np.eye(3))


def test_rpy_convention_and_unit_quaternions():
    tree = load_urdf(MOBILE_URDF)
    assert np.abs(np.linalg.norm(tree.origin_q, axis=1) - 1).max() < 1e-15
    assert np.abs(np.linalg.norm(tree.axis[tree.jtype != FIXED], axis=1) - 1).max() < 1e-15
    rng = np.random.default_rng(3)
    for rpy in rng.uniform(-3, 3, (8, 3)):
        assert np.abs(K.quat_matrix(rpy_to_quat(rpy), np.float64) - K.rpy_matrix(rpy)).max() < 1e-14
    # roll about the fixed x axis first, yaw about the fixed z axis last: e_y -> e_z -> e_z (the other order gives -e_x)
    assert np.allclose(K.rpy_matrix([np.pi / 2, 0, np.pi / 2]) @ [0, 1, 0], [0, 0, 1], atol=1e-15)


def test_toy_urdf_matches_the_planar_closed_form():
    tree = load_urdf(TOY)
    assert tree.names == ["base", "slider", "l1", "l2", "tip"] and tree.dof.tolist() == [-1, 0, 1, 2, -1]
    assert tree.axis[1].tolist() == [1, 0, 0]                 # normalised
    assert tree.lower.tolist() == [-1, -3, -np.inf] and tree.upper.tolist() == [1, 3, np.inf] and tree.velocity[2] == np.inf
    rng = np.random.default_rng(0)
    q = rng.uniform(-1, 1, (16, 3)) * [1, 3, 3]
    qd = rng.normal(size=(16, 3))
    out = K.fk(tree, q, qd, [0, 0, 0, 0, 0, 0, 1])
    s, c1, s1, c12, s12 = q[:, 0], np.cos(q[:, 1]), np.sin(q[:, 1]), np.cos(q[:, 1] + q[:, 2]), np.sin(q[:, 1] + q[:, 2])
    z, o = np.zeros(16), np.ones(16)
    assert np.abs(out["pos"][:, 3] - np.stack([s + c1, s1, z], 1)).max() < 1e-15
    assert np.abs(out["pos"][:, 4] - np.stack([s + c1 + 0.5 * c12, s1 + 0.5 * s12, z], 1)).max() < 1e-15
    J = np.stack([np.stack([o, -s1 - 0.5 * s12, -0.5 * s12], 1), np.stack([z, c1 + 0.5 * c12, 0.5 * c12], 1), np.stack([z, z, z], 1),
                  np.stack([z, z, z], 1), np.stack([z, z, z], 1), np.stack([z, o, o], 1)], 1)
    assert np.abs(out["jac"][:, 3] - J).max() < 1e-15
    assert np.abs(out["jac"][:, 1, :, 2]).max() == 0 and np.abs(out["jac"][:, 0, :, 1:]).max() == 0      # not ancestors
    assert np.abs(out["vel"][:, 4] - np.einsum("nrd,nd->nr", J, qd)).max() < 1e-14
    Rz = np.stack([np.stack([c12, -s12, z], 1), np.stack([s12, c12, z], 1), np.stack([z, z, o], 1)], 1)
    assert np.abs(out["R"][:, 4] - Rz).max() < 1e-15


@pytest.mark.parametrize("path", [FIXED_URDF, MOBILE_URDF])
def test_reference_jacobian_is_the_derivative_of_its_own_poses(path):
    tree = load_urdf(path)
    rng = np.random.default_rng(11)
    q = tree.lower + rng.uniform(0, 1, (32, tree.num_dofs)) * (tree.upper - tree.lower)
    base = [0.3, -0.1, 0.05, 0.2, -0.3, 0.6, 0.7]
    out = K.fk(tree, q, np.zeros_like(q), base)
    h, worst_lin, worst_ang = 1e-6, 0.0, 0.0
    for d in range(tree.num_dofs):
        e = np.zeros(tree.num_dofs)
        e[d] = h
        hi, lo = K.fk(tree, q + e, np.zeros_like(q), base), K.fk(tree, q - e, np.zeros_like(q), base)
        lin = (hi["pos"] - lo["pos"])[:, 1:] / (2 * h)
        W = ((hi["R"] - lo["R"]) / (2 * h)) @ out["R"].transpose(0, 1, 3, 2)       # dR R^T = [omega]x
        ang = np.stack([W[..., 2, 1] - W[..., 1, 2], W[..., 0, 2] - W[..., 2, 0], W[..., 1, 0] - W[..., 0, 1]], -1)[:, 1:] / 2
        worst_lin = max(worst_lin, np.abs(lin - out["jac"][:, :, :3, d]).max())
        worst_ang = max(worst_ang, np.abs(ang - out["jac"][:, :, 3:, d]).max())
    print(f"{os.path.basename(path)}: jacobian against central differences: linear {worst_lin:.2e}, angular {worst_ang:.2e}")
    assert worst_lin < 1e-5 and worst_ang < 1e-5


def test_reference_fp32_switch_and_quaternion_round_trip():
    tree = load_urdf(FIXED_URDF)
    q = (tree.lower + tree.upper)[None] / 2
    o64, o32 = K.fk(tree, q, q * 0, [0, 0, 0, 0, 0, 0, 1]), K.fk(tree, q, q * 0, [0, 0, 0, 0, 0, 0, 1], dtype=np.float32)
    assert all(v.dtype == np.float32 for v in o32.values()) and all(v.dtype == np.float64 for v in o64.values())
    assert 0 < np.abs(o32["pos"] - o64["pos"]).max() < 1e-5
    assert np.abs(K.quat_matrix(o64["quat"], np.float64) - o64["R"]).max() < 1e-14


def _broken(old, new):
    assert old in TOY
    return TOY.replace(old, new)


@pytest.mark.parametrize("text, joint, what", [
    (_broken('name="j2" type="continuous"', 'name="j2" type="floating"'), "j2", "not supported"),
    (_broken('name="j1" type="revolute"', 'name="j1" type="planar"'), "j1", "not supported"),
    (_broken('<link name="tip"/>', '<link name="tip"/><link name="b2"/><link name="c2"/><joint name="stray" type="fixed">'
             '<parent link="b2"/><child link="c2"/></joint>'), "stray", "more than one root"),
    (_broken('<link name="tip"/>', '<link name="tip"/><link name="x"/><link name="y"/><joint name="xy" type="fixed"><parent link="x"/>'
             '<child link="y"/></joint><joint name="yx" type="fixed"><parent link="y"/><child link="x"/></joint>'), "yx", "cycle"),
    (_broken('<joint name="slide" type="prismatic"><parent link="base"/>', '<joint name="back" type="fixed"><parent link="tip"/>'
             '<child link="base"/></joint><joint name="slide" type="prismatic"><parent link="base"/>'), "back", "cycle"),
    (_broken('<parent link="l1"/>', '<parent link="nowhere"/>'), "j2", "unknown parent"),
])
def test_malformed_urdfs_raise_a_value_error_that_names_the_joint(text, joint, what):
    with pytest.raises(ValueError, match=what) as e:
        load_urdf(text)
    assert joint in str(e.value)


def test_limits_of_64_bodies_and_dofs():
    def chain(n):
        links = "".join(f'<link name="b{i}"/>' for i in range(n + 1))
        joints = "".join(f'<joint name="j{i}" type="revolute"><parent link="b{i}"/><child link="b{i + 1}"/><axis xyz="0 0 1"/>'
                         f'<limit lower="-1" upper="1"/></joint>' for i in range(n))
        return f"<robot>{links}{joints}</robot>"
    with pytest.raises(ValueError, match="outside"):
        load_urdf(chain(64))                                  # 65 bodies
    tree = load_urdf(chain(63))
    assert (tree.num_bodies, tree.num_dofs) == (64, 63) and int(tree.anc_mask[-1]) == 2 ** 63 - 1


def test_c_entry_refuses_bad_arguments_without_a_gpu():
    """The checks of pm_articulation_step_f32 run before any launch, so they can be held here: the pointers below are never read."""
    from partmanip_amd._lib import lib
    N, dt, p = 3, 1 / 60, 64
    good = dict(parent=p, jtype=p, dof=p, origin_q=p, origin_t=p, axis=p, anc_mask=p, dof_lo=p, dof_hi=p, vmax=0, dt=dt, base_pose=p,
                base_stride=0, dof_state=p, dof_rows=N * 9, targets=p, tgt_stride=9, reset=0, rb_row0=0, rb_stride=14, rb_rows=N * 14,
                dof_row0=0, dof_stride=9, N=N, nb=13, nd=9, rigid_body=p, jac=p, stream=0)
    bad = [dict(parent=0), dict(anc_mask=0), dict(dof_hi=0), dict(base_pose=0), dict(dof_state=0), dict(N=0), dict(nb=0), dict(nb=65),
           dict(nd=0), dict(nd=65), dict(base_stride=6), dict(base_stride=-7), dict(tgt_stride=8), dict(rb_stride=12), dict(dof_stride=8),
           dict(dt=0.0), dict(dt=-dt), dict(dt=float("nan")), dict(rb_rows=N * 14 - 2), dict(dof_rows=N * 9 - 1), dict(rb_rows=2 ** 31)]
    for change in bad:
        assert lib.pm_articulation_step_f32(*{**good, **change}.values()) == -1, change


def test_python_surface_refuses_malformed_trees_and_cpu_tensors():
    import torch
    from partmanip_amd import ops
    from partmanip_amd.kinematics import Articulation
    tree = load_urdf(TOY)
    tree.parent[2] = 3                                        # a parent that does not precede its child
    with pytest.raises(ValueError, match="precedes"):
        Articulation(tree, 2, "cpu")
    tree = load_urdf(TOY)
    tree.dof[3] = 1                                           # a DOF named twice
    with pytest.raises(ValueError, match="once each"):
        Articulation(tree, 2, "cpu")
    art = Articulation(load_urdf(TOY), 2, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        art.forward(torch.zeros(2, 3, 2), torch.tensor([0, 0, 0, 0, 0, 0, 1.0]))
    assert ops.articulation_step.__doc__
