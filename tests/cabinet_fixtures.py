"""Synthetic cabinets for the kinematic-scene tests: URDF text and, in the reference's folder layout, `mobility_new.urdf` plus
`bbox_info.json` written into a directory the test owns (tmp_path).  Nothing here is read from the reference's assets.

  A: 2 bodies, 1 prismatic DOF; the drawer is its own handle.
  B: 7 bodies, 3 DOFs: base -> frame (fixed) -> two prismatic drawers, each with a handle as a fixed child; base -> a revolute door.
     The drawers open along the object's -x (with the task's default object pose, turned half a turn about z, that is the world's +x).
  C: the chain at the kernel's limit, 64 bodies and 64 DOFs (the root's own joint included), revolute and prismatic mixed; it has no
     folder, a URDF's root link carries no joint.

bbox_info.json lists the links in an order that is NOT the depth-first body order, so an index taken from the wrong list shows.
A handle's box is centred `HANDLE_OFFSET` (in the handle's frame) off the handle body's origin at q = 0, with its `out` edge
(corner 0 - corner 4) along the target joint's axis; corners as the task reads them: out = c0 - c4, long = c1 - c0, short = c3 - c0,
centre = (c0 + c6) / 2.  All geometry is in the object's frame at scale 1, as in the reference's files."""
import json
import os

import numpy as np

from tests import kinematics_ref as K

URDF_A = """<robot name="cab_a">
  <link name="base"/><link name="drawer"/>
  <joint name="slide" type="prismatic"><parent link="base"/><child link="drawer"/><origin xyz="-0.3 0.1 0.2" rpy="0 0 0.2"/>
    <axis xyz="-1 0 0"/><limit lower="0" upper="0.4" velocity="1"/></joint>
</robot>"""

URDF_B = """<robot name="cab_b">
  <link name="base"/><link name="frame"/><link name="drawer_1"/><link name="handle_1"/><link name="drawer_2"/><link name="handle_2"/>
  <link name="door"/>
  <joint name="fix_frame" type="fixed"><parent link="base"/><child link="frame"/><origin xyz="0.05 0 0.1" rpy="0 0 0.1"/></joint>
  <joint name="slide_1" type="prismatic"><parent link="frame"/><child link="drawer_1"/><origin xyz="-0.2 0 0.3" rpy="0 0.05 0"/>
    <axis xyz="-1 0 0"/><limit lower="0" upper="0.4" velocity="1"/></joint>
  <joint name="grip_1" type="fixed"><parent link="drawer_1"/><child link="handle_1"/><origin xyz="-0.25 0 0.05"/></joint>
  <joint name="slide_2" type="prismatic"><parent link="frame"/><child link="drawer_2"/><origin xyz="-0.2 0 0.6" rpy="0 0 -0.1"/>
    <axis xyz="-1 0.2 0"/><limit lower="0" upper="0.5" velocity="1"/></joint>
  <joint name="grip_2" type="fixed"><parent link="drawer_2"/><child link="handle_2"/><origin xyz="-0.3 0.02 0.04" rpy="0.1 0 0"/></joint>
  <joint name="hinge" type="revolute"><parent link="base"/><child link="door"/><origin xyz="0.5 0.25 0.125"/>
    <axis xyz="0 0 1"/><limit lower="0" upper="1.5" velocity="1"/></joint>
</robot>"""

JSON_ORDER = {"A": ["drawer", "base"], "B": ["base", "door", "handle_2", "drawer_2", "handle_1", "drawer_1", "frame"]}
TARGETS = {"A": ("drawer", "drawer", "slide"), "B": ("drawer_2", "handle_2", "slide_2"), "B1": ("drawer_1", "handle_1", "slide_1"),
           "Bdoor": ("door", "door", "hinge")}
HANDLE_OFFSET = np.array([-0.02, 0.01, 0.03])
HANDLE_HALF = np.array([0.015, 0.06, 0.01])                   # out, long, short


def urdf_text(kind):
    return {"A": URDF_A, "B": URDF_B}[kind[0]]


def tree_of(kind, scale=1.0):
    from partmanip_amd.urdf import load_urdf
    return tree_c() if kind == "C" else load_urdf(urdf_text(kind), scale=scale)


def tree_c():
    """64 bodies, 64 DOFs: every third joint prismatic."""
    from partmanip_amd.urdf import KinematicTree
    rng = np.random.default_rng(64)
    ax = rng.normal(size=(64, 3))
    jt = np.where(np.arange(64) % 3 == 2, 2, 1).astype(np.int32)
    lim = [(-1.0, 1.0, 2.0) if t == 1 else (-0.05, 0.05, 1.0) for t in jt]
    return KinematicTree([f"b{i}" for i in range(64)], [f"j{i}" for i in range(64)], np.arange(64) - 1, jt, rng.uniform(-0.05, 0.05, (64, 3)),
                         rng.uniform(-1, 1, (64, 3)), ax / np.linalg.norm(ax, axis=1, keepdims=True), lim, np.zeros(64, dtype=bool))


def box_corners(centre, out, long_, short, half=HANDLE_HALF):
    """The 8 corners in the task's order from the centre, three orthonormal directions and the half sizes."""
    o, l, s = (np.asarray(v, dtype=np.float64) * h for v, h in zip((out, long_, short), half))
    c4 = np.asarray(centre, dtype=np.float64) - o - l - s
    return np.stack([c4 + 2 * o, c4 + 2 * o + 2 * l, c4 + 2 * o + 2 * l + 2 * s, c4 + 2 * o + 2 * s, c4, c4 + 2 * l, c4 + 2 * l + 2 * s, c4 + 2 * s])


def bbox_info(kind):
    """The json of cabinet A or B: per link (in JSON_ORDER) a box about its own origin at q = 0, its `out` edge along the axis of the
    nearest moving joint above it, and that joint's axis as axis_dir_world (zeros for the base)."""
    tree = tree_of(kind[0])
    out = K.fk(tree, np.zeros((1, tree.num_dofs)), np.zeros((1, tree.num_dofs)), [0, 0, 0, 0, 0, 0, 1])
    info = dict(link_name=list(JSON_ORDER[kind[0]]), bbox_world=[], axis_xyz_world=[], axis_dir_world=[])
    for name in info["link_name"]:
        b = tree.names.index(name)
        moving = K.ancestors(tree, b)
        if moving:
            jb = moving[0]
            a = out["R"][0, jb] @ tree.axis[jb]
            origin = out["pos"][0, jb]
        else:
            a, origin = np.array([1.0, 0.0, 0.0]), out["pos"][0, b]
        long_ = np.cross([0.0, 0.0, 1.0] if abs(a[2]) < 0.9 else [1.0, 0.0, 0.0], a)
        long_ /= np.linalg.norm(long_)
        short = np.cross(a, long_)
        centre = out["pos"][0, b] + out["R"][0, b] @ HANDLE_OFFSET
        info["bbox_world"].append(box_corners(centre, a, long_, short).tolist())
        info["axis_xyz_world"].append(origin.tolist())
        info["axis_dir_world"].append((a if moving else np.zeros(3)).tolist())
    return info


def write_cabinet(root, kind, index=0, asset="1000"):
    """Folder `cab-<asset>-<link>-<handle>-<joint>-<index>` under root with the two files; returns its path."""
    link, handle, joint = TARGETS[kind]
    folder = os.path.join(os.fspath(root), f"cab-{asset}-{link}-{handle}-{joint}-{index}")
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "mobility_new.urdf"), "w") as f:
        f.write(urdf_text(kind))
    with open(os.path.join(folder, "bbox_info.json"), "w") as f:
        json.dump(bbox_info(kind), f)
    return folder
