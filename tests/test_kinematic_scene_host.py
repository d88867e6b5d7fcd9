"""Host side of the kinematic scene (one cabinet of its own type per environment): kinematics.ObjectLibrary's tables,
urdf.load_urdf(scale=), tasks.open_drawer.load_drawer_assets on the synthetic cabinets of tests/cabinet_fixtures.py, KinematicSim's
row tables against build_masks, and the C entry's header / ctypes / ABI.  No GPU."""
import inspect
import json
import os
import re

import numpy as np
import pytest

from partmanip_amd.kinematics import KinematicSim, ObjectLibrary
from partmanip_amd.tasks.open_drawer import OBJ_DEFAULT_ROOT, build_masks, load_drawer_assets
from partmanip_amd.urdf import FIXED, PRISMATIC, REVOLUTE, load_urdf
from tests import cabinet_fixtures as CF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MOBILE_URDF = os.path.join(GOLDEN, "franka_panda_sdf_mobile.urdf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_cabinets_have_the_stated_shapes():
    a, b, c = CF.tree_of("A"), CF.tree_of("B"), CF.tree_of("C")
    assert (a.num_bodies, a.num_dofs, b.num_bodies, b.num_dofs, c.num_bodies, c.num_dofs) == (2, 1, 7, 3, 64, 64)
    assert b.names == ["base", "frame", "drawer_1", "handle_1", "drawer_2", "handle_2", "door"] and b.names != CF.JSON_ORDER["B"]
    assert b.jtype.tolist() == [FIXED, FIXED, PRISMATIC, FIXED, PRISMATIC, FIXED, REVOLUTE] and b.parent.tolist() == [-1, 0, 1, 2, 1, 4, 0]
    assert sorted(set(c.jtype.tolist())) == [REVOLUTE, PRISMATIC]


def test_object_library_offsets_and_tables_equal_the_per_tree_tables():
    trees = [CF.tree_of("A"), CF.tree_of("B", 0.5), CF.tree_of("C")]
    lib = ObjectLibrary(trees, "cpu")
    assert lib.body_off.tolist() == [0, 2, 9, 73] and lib.dof_off.tolist() == [0, 1, 4, 68]
    assert (lib.num_bodies, lib.num_dofs, lib.max_bodies, lib.max_dofs, lib.num_types) == ([2, 7, 64], [1, 3, 64], 64, 64, 3)
    for k, tree in enumerate(trees):
        b0, b1, d0, d1 = lib.body_off[k], lib.body_off[k + 1], lib.dof_off[k], lib.dof_off[k + 1]
        assert lib.parent[b0:b1].tolist() == tree.parent.tolist() and lib.dof[b0:b1].tolist() == tree.dof.tolist()      # local indices
        assert lib.jtype[b0:b1].tolist() == tree.jtype.tolist()
        for got, want in ((lib.origin_q, tree.origin_q), (lib.origin_t, tree.origin_t), (lib.axis, tree.axis)):
            assert np.array_equal(got[b0:b1].numpy(), want.astype(np.float32))
        assert np.array_equal(lib.anc_mask[b0:b1].numpy().view(np.uint64), tree.anc_mask)
        assert np.array_equal(lib.dof_lower[d0:d1].numpy(), tree.lower.astype(np.float32))
        assert np.array_equal(lib.dof_upper[d0:d1].numpy(), tree.upper.astype(np.float32))
    order = lib.order_of(np.arange(10) % 3).tolist()
    assert order == [0, 3, 6, 9, 1, 4, 7, 2, 5, 8]
    with pytest.raises(ValueError, match="obj_type"):
        lib.order_of(np.array([0, 3]))
    bad = CF.tree_of("B")
    bad.parent[2] = 3
    with pytest.raises(ValueError, match="tree 1.*precedes"):
        ObjectLibrary([trees[0], bad], "cpu")
    with pytest.raises(ValueError, match="at least one"):
        ObjectLibrary([], "cpu")


def test_load_urdf_scale_scales_origins_and_prismatic_limits_and_nothing_else():
    one, half = load_urdf(CF.URDF_B), load_urdf(CF.URDF_B, scale=0.5)
    assert np.array_equal(load_urdf(CF.URDF_B, scale=1.0).origin_t, one.origin_t)       # the default changes nothing
    assert np.array_equal(half.origin_t, one.origin_t * 0.5) and np.abs(one.origin_t).max() > 0
    assert half.dof_names == ["slide_1", "slide_2", "hinge"]
    assert half.lower.tolist() == [0, 0, 0] and half.upper.tolist() == [0.2, 0.25, 1.5]       # the hinge keeps its radians
    assert one.upper.tolist() == [0.4, 0.5, 1.5]
    for name in ("origin_rpy", "origin_q", "axis", "velocity", "parent", "jtype", "dof", "anc_mask"):
        assert np.array_equal(getattr(half, name), getattr(one, name)), name
    assert half.names == one.names
    mob = load_urdf(MOBILE_URDF, scale=2.0)
    ref = load_urdf(MOBILE_URDF)
    pris = ref.jtype[ref.jtype != FIXED] == PRISMATIC
    assert np.array_equal(mob.upper[pris], ref.upper[pris] * 2) and np.array_equal(mob.upper[~pris], ref.upper[~pris])
    assert np.array_equal(mob.lower[pris], ref.lower[pris] * 2) and np.array_equal(mob.velocity, ref.velocity)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            load_urdf(CF.URDF_A, scale=bad)


def test_load_drawer_assets_parses_names_and_json(tmp_path):
    folders = [CF.write_cabinet(tmp_path, "A", 0, "40147"), CF.write_cabinet(tmp_path, "B", 1, "45162"), CF.write_cabinet(tmp_path, "B1", 2)]
    assets = load_drawer_assets(folders, scale=0.5)
    assert assets.num_objs == 3 and assets.names[1] == ("45162", "drawer_2", "handle_2", "slide_2")
    assert assets.num_bodies.tolist() == [2, 7, 7] and assets.num_dofs.tolist() == [1, 3, 3]
    # body rows follow the tree's depth-first order, the bbox arrays the json's order
    assert assets.target_link.tolist() == [1, 4, 2] and assets.target_handle.tolist() == [1, 5, 3] and assets.target_dof.tolist() == [0, 1, 0]
    info = CF.bbox_info("B")
    assert info["link_name"].index("handle_2") == 2 != 5 and info["link_name"].index("drawer_2") == 3 != 4
    assert np.array_equal(assets.part_bbox_init[1], np.asarray(info["bbox_world"][2]) * 0.5)
    assert np.array_equal(assets.part_axis_dir_init[1], info["axis_dir_world"][3])
    assert np.array_equal(assets.part_axis_xyz_init[1], info["axis_xyz_world"][3])
    assert abs(np.linalg.norm(assets.part_axis_dir_init[1]) - 1) < 1e-12
    # the reference's expressions: upper * scale, lower as in the file
    assert assets.part_joint_upper_limits.tolist() == [0.2, 0.25, 0.2] and assets.part_joint_lower_limits.tolist() == [0, 0, 0]
    assert assets.trees[1].upper.tolist() == [0.2, 0.25, 1.5] and np.array_equal(assets.trees[1].origin_t, load_urdf(CF.URDF_B).origin_t * 0.5)
    envs = assets.for_envs(7)
    assert envs.obj_id.tolist() == [0, 1, 2, 0, 1, 2, 0] and envs.num_objs == 3
    assert envs.obj_bodies.tolist() == [2, 7, 7, 2, 7, 7, 2] and envs.target_dof.tolist() == [0, 1, 0, 0, 1, 0, 0]
    assert envs.part_bbox_init.shape == (7, 8, 3) and envs.part_bbox_init.dtype == np.float32
    assert np.array_equal(envs.part_bbox_init[4], assets.part_bbox_init[1].astype(np.float32))
    assert set(envs.task_kwargs()) == {"obj_id", "part_bbox_init", "part_axis_dir_init", "part_joint_lower_limits", "part_joint_upper_limits",
                                       "num_objs"}
    rb, dm, B, D = envs.masks(16, 12)
    want = build_masks(16, 12, envs.obj_bodies, envs.obj_dofs, envs.target_link, envs.target_handle, envs.target_dof)
    assert np.array_equal(rb, want[0]) and np.array_equal(dm, want[1]) and (B, D) == want[2:] == (7 * 16 + 34, 7 * 12 + 15)
    assert "depth-first" in load_drawer_assets.__doc__ and "json" in load_drawer_assets.__doc__


def test_load_drawer_assets_raises_value_errors_that_name_the_problem(tmp_path):
    good = CF.write_cabinet(tmp_path / "good", "B")
    load_drawer_assets([good])

    def variant(name, kind="B", edit=None, drop=None):
        link, handle, joint = CF.TARGETS[kind]
        folder = tmp_path / name / f"cab-1-{link}-{handle}-{joint}-0"
        os.makedirs(folder)
        info, text = CF.bbox_info(kind), CF.urdf_text(kind)
        if edit:
            info, text = edit(info, text)
        if drop != "json":
            (folder / "bbox_info.json").write_text(json.dumps(info))
        if drop != "urdf":
            (folder / "mobility_new.urdf").write_text(text)
        return str(folder)

    with pytest.raises(ValueError, match="bbox_info.json"):
        load_drawer_assets([variant("nojson", drop="json")])
    with pytest.raises(ValueError, match="mobility_new.urdf"):
        load_drawer_assets([variant("nourdf", drop="urdf")])
    with pytest.raises(ValueError, match="handle_2"):
        load_drawer_assets([variant("nolink", edit=lambda i, t: (dict(i, link_name=[n.replace("handle_2", "knob") for n in i["link_name"]]), t))])
    with pytest.raises(ValueError, match="handle_2"):
        load_drawer_assets([variant("nobody", edit=lambda i, t: (i, t.replace("handle_2", "knob")))])
    with pytest.raises(ValueError, match="slide_2"):
        load_drawer_assets([variant("nojoint", edit=lambda i, t: (i, t.replace('name="slide_2"', 'name="rail"')))])
    with pytest.raises(ValueError, match="slide_2.*fixed"):
        load_drawer_assets([variant("fixed", edit=lambda i, t: (i, t.replace('name="slide_2" type="prismatic"', 'name="slide_2" type="fixed"')))])
    bad = tmp_path / "a-b"
    os.makedirs(bad)
    with pytest.raises(ValueError, match="does not parse"):
        load_drawer_assets([str(bad)])
    with pytest.raises(ValueError, match="at least one"):
        load_drawer_assets([])


def test_kinematic_sim_rejects_bad_object_arguments_before_any_launch():
    robot = load_urdf(MOBILE_URDF)
    lib = ObjectLibrary([CF.tree_of("A", 0.5), CF.tree_of("B", 0.5)], "cpu")
    with pytest.raises(ValueError, match="obj_type"):
        KinematicSim(robot, 3, "cpu", 1 / 60, objects=lib, obj_type=[0, 1, 2])
    with pytest.raises(ValueError, match="target_dof"):
        KinematicSim(robot, 3, "cpu", 1 / 60, objects=lib, obj_type=[0, 1, 0], target_dof=[0, 1, 1])
    with pytest.raises(ValueError, match="tips"):
        KinematicSim(robot, 3, "cpu", 1 / 60, objects=lib, obj_type=[0, 1, 0], tips=(13, 16))
    with pytest.raises(ValueError, match="row tables"):
        KinematicSim(robot, 3, "cpu", 1 / 60, objects=lib, obj_type=[0, 1, 0], rb_row0=[0, 18, 41], dof_row0=[0, 13, 28])
    with pytest.raises(ValueError, match="objects="):
        KinematicSim(robot, 3, "cpu", 1 / 60, obj_type=[0, 1, 0])
    with pytest.raises(ValueError, match="actor 1"):
        KinematicSim(robot, 3, "cpu", 1 / 60, objects=lib, obj_type=[0, 1, 0], num_actors=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # the constructor's first forward(): the tables were accepted
        KinematicSim(robot, 3, "cpu", 1 / 60, objects=lib, obj_type=[0, 1, 0], target_dof=[0, 1, 0], tips=(13, 15))


def test_kinematic_sim_row_tables_equal_build_masks_columns(monkeypatch):
    robot = load_urdf(MOBILE_URDF)
    trees = [CF.tree_of("A", 0.5), CF.tree_of("B", 0.5), CF.tree_of("C")]
    lib = ObjectLibrary(trees, "cpu")
    N = 8
    k = np.arange(N) % 3
    link, handle, tdof = np.array([1, 4, 63])[k], np.array([1, 5, 63])[k], np.array([0, 1, 7])[k]
    monkeypatch.setattr(KinematicSim, "forward", lambda self: None)        # no launch: the layout is decided on the host
    sim = KinematicSim(robot, N, "cpu", 1 / 60, objects=lib, obj_type=k, target_dof=tdof, tips=(13, 15))
    rb, dm, B, D = build_masks(16, 12, np.array(lib.num_bodies)[k], np.array(lib.num_dofs)[k], link, handle, tdof)
    assert (sim.B, sim.D) == (B, D) and tuple(sim.rigid_body.shape) == (B, 13) and tuple(sim.dof_state.shape) == (D, 2)
    assert np.array_equal(sim.rb_row0.numpy(), rb[:, 0]) and np.array_equal(sim.dof_row0.numpy(), dm[:, 0])
    assert np.array_equal(sim.obj_rb_row0.numpy() + link, rb[:, -2]) and np.array_equal(sim.obj_rb_row0.numpy() + handle, rb[:, -1])
    assert np.array_equal(sim.obj_dof_row0.numpy() + tdof, dm[:, -1])
    assert np.array_equal(sim.tip_rows.numpy(), rb[:, [13, 15]]) and np.array_equal(sim.target_dof.numpy(), tdof)
    assert tuple(sim.root.shape) == (N, 2, 13) and np.allclose(sim.root[:, 1, :7].numpy(), np.asarray(OBJ_DEFAULT_ROOT, dtype=np.float32))
    assert sorted(sim._order.tolist()) == list(range(N)) and (np.diff(k[sim._order.numpy()]) >= 0).all()
    plain = KinematicSim(robot, N, "cpu", 1 / 60)             # without objects= nothing changes
    assert tuple(plain.root.shape) == (N, 1, 13) and plain.objects is None and tuple(plain.rigid_body.shape) == (N, 16, 13)


def header_text():
    with open(os.path.join(ROOT, "include", "partmanip_hip.h")) as f:
        return f.read()


def test_header_ctypes_abi_and_wrapper_argument_order():
    import ctypes
    from partmanip_amd import _lib, ops
    src = header_text()
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 163 == _lib.ABI_VERSION == _lib.lib.pm_version()
    m = re.search(r"int pm_articulation_objects_step_f32\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["body_off", "dof_off", "K", "total_bodies", "total_dofs", "max_nb", "max_nd", "parent", "jtype", "dof", "origin_q",
                     "origin_t", "axis", "anc_mask", "dof_lo", "dof_hi", "obj_type", "order", "obj_pose", "pose_stride", "obj_rb_row0",
                     "obj_dof_row0", "dof_state", "dof_rows", "rigid_body", "rb_rows", "hold", "reset", "target_dof", "tip_rows", "dt", "N",
                     "stream"]
    res, args = _lib.SIGNATURES["pm_articulation_objects_step_f32"]
    assert res is ctypes.c_int and len(args) == len(names) == 33
    assert list(inspect.signature(ops.articulation_objects_step).parameters) == [
        "body_off", "dof_off", "parent", "jtype", "dof", "origin_q", "origin_t", "axis", "anc_mask", "dof_lo", "dof_hi", "max_nb", "max_nd",
        "obj_type", "obj_pose", "obj_rb_row0", "obj_dof_row0", "dof_state", "rigid_body", "order", "hold", "reset", "target_dof", "tip_rows",
        "dt"]
    for word in ("hold", "No Jacobian", "no dynamics", "stores nothing"):
        assert word in src[src.index("kinematic objects"):src.index("int pm_articulation_objects_step_f32")], word


def test_c_entry_refuses_bad_arguments_without_a_gpu():
    """The checks run before any launch, so they can be held here: the pointers below are never read."""
    from partmanip_amd._lib import lib
    p = 64
    good = dict(body_off=p, dof_off=p, K=3, total_bodies=73, total_dofs=68, max_nb=64, max_nd=64, parent=p, jtype=p, dof=p, origin_q=p,
                origin_t=p, axis=p, anc_mask=p, dof_lo=p, dof_hi=p, obj_type=p, order=0, obj_pose=p, pose_stride=26, obj_rb_row0=p,
                obj_dof_row0=p, dof_state=p, dof_rows=100, rigid_body=p, rb_rows=100, hold=p, reset=p, target_dof=p, tip_rows=p, dt=1 / 60,
                N=5, stream=0)
    bad = [{k: 0} for k in ("body_off", "dof_off", "parent", "jtype", "dof", "origin_q", "origin_t", "axis", "anc_mask", "dof_lo", "dof_hi",
                            "obj_type", "obj_pose", "obj_rb_row0", "obj_dof_row0", "dof_state", "rigid_body", "N", "K", "total_bodies",
                            "total_dofs", "max_nb", "max_nd", "dof_rows", "rb_rows", "hold", "reset", "target_dof", "tip_rows")]
    bad += [dict(max_nb=65), dict(max_nd=65), dict(pose_stride=6), dict(pose_stride=-7), dict(dof_rows=2 ** 31), dict(rb_rows=2 ** 31),
            dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(N=-1)]
    for change in bad:
        assert lib.pm_articulation_objects_step_f32(*{**good, **change}.values()) == -1, change
