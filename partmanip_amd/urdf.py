"""URDF -> kinematic tree, on the host (numpy and the standard library's xml.etree only).

    tree = load_urdf("franka_panda_sdf.urdf")         # a path, or the XML text itself
    robot = Franka(cfg, dt, N, device, **tree.robot_kwargs())

What the tree fixes, as this project's own stated choices (neither has been checked against Isaac Gym, whose asset importer is
closed):
  * body order: depth first from the root link, children in the order their joints appear in the file.  It reproduces the 13-body
    Franka defaults of tasks/franka.py (link0-7, hand, left finger, left tip, right finger, right tip);
  * `rpy` is fixed-axis roll-pitch-yaw, R = Rz(yaw) Ry(pitch) Rx(roll), computed in float64 and kept as a unit quaternion (x, y, z, w).
DOFs are numbered in body order.  `<mimic>` is ignored, as the reference's simulator does (both fingers are DOFs); a `continuous`
joint is a revolute one without limits.  Any other joint type, a second root, a cycle or an unknown link raises a ValueError that
names the joint.  At most 64 bodies and 64 DOFs (the ancestor masks are 64-bit and the kernel stages one robot per lane).

    meshes = load_urdf_visuals("mobility_new.urdf", scale=0.5)    # per body, in that order: (vertices, faces) in the body's frame, or None"""
import os
import xml.etree.ElementTree as ET

import numpy as np

FIXED, REVOLUTE, PRISMATIC = 0, 1, 2
JOINT_TYPES = {"fixed": FIXED, "revolute": REVOLUTE, "continuous": REVOLUTE, "prismatic": PRISMATIC}
MAX_BODIES = MAX_DOFS = 64


def rpy_to_quat(rpy):
    """Fixed-axis roll-pitch-yaw -> the unit quaternion (x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll), in float64."""
    r, p, y = (float(v) / 2.0 for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    q = np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                  cr * cp * cy + sr * sp * sy], dtype=np.float64)
    return q / np.linalg.norm(q)


def _floats(text, n, what):
    v = [float(s) for s in (text or "").split()]
    if len(v) != n:
        raise ValueError(f"{what}: expected {n} numbers, got {text!r}")
    return np.array(v, dtype=np.float64)


class KinematicTree:
    """Arrays over the nb bodies: names, parent (int32, -1 for the root), jtype (FIXED / REVOLUTE / PRISMATIC), dof (int32, -1 for a
    fixed joint), joint_names (None for the root), origin_t (nb, 3), origin_rpy (nb, 3), origin_q (nb, 4) unit (x, y, z, w), axis
    (nb, 3) unit (zero for a fixed joint), anc_mask (nb) uint64 = the DOFs on the body's path to the root, has_mesh (nb) bool.
    Over the nd DOFs: lower, upper, velocity (float64; -inf / inf / inf where the file gives none), dof_names."""

    def __init__(self, names, joint_names, parent, jtype, origin_t, origin_rpy, axis, limits, has_mesh):
        nb = len(names)
        self.names, self.joint_names = list(names), list(joint_names)
        self.parent = np.asarray(parent, dtype=np.int32)
        self.jtype = np.asarray(jtype, dtype=np.int32)
        self.origin_t = np.asarray(origin_t, dtype=np.float64).reshape(nb, 3)
        self.origin_rpy = np.asarray(origin_rpy, dtype=np.float64).reshape(nb, 3)
        self.origin_q = np.stack([rpy_to_quat(r) for r in self.origin_rpy])
        self.axis = np.asarray(axis, dtype=np.float64).reshape(nb, 3)
        self.has_mesh = np.asarray(has_mesh, dtype=bool)
        self.dof = np.full(nb, -1, dtype=np.int32)
        moving = np.flatnonzero(self.jtype != FIXED)
        self.dof[moving] = np.arange(moving.size, dtype=np.int32)
        self.num_bodies, self.num_dofs = nb, int(moving.size)
        self.dof_names = [self.joint_names[b] for b in moving]
        lim = np.array([limits[b] for b in moving], dtype=np.float64).reshape(-1, 3)
        self.lower, self.upper, self.velocity = lim[:, 0].copy(), lim[:, 1].copy(), lim[:, 2].copy()
        if not 1 <= nb <= MAX_BODIES or not 1 <= self.num_dofs <= MAX_DOFS:
            raise ValueError(f"a tree of {nb} bodies and {self.num_dofs} DOFs is outside [1, {MAX_BODIES}] x [1, {MAX_DOFS}]")
        mask = [0] * nb
        for b in range(nb):
            p = int(self.parent[b])
            if not (p == -1 and b == 0) and not 0 <= p < b:
                raise ValueError(f"body {b} ({self.names[b]}): parent {p} does not precede it")
            mask[b] = (mask[p] if p >= 0 else 0) | ((1 << int(self.dof[b])) if self.dof[b] >= 0 else 0)
        self.anc_mask = np.array(mask, dtype=np.uint64)

    def body_index(self, name):
        try:
            return self.names.index(name)
        except ValueError:
            raise KeyError(f"no body named {name!r}; bodies: {self.names}") from None

    def mesh_bodies(self):
        """The bodies that carry a <collision> or <visual> mesh, in body order."""
        return tuple(int(b) for b in np.flatnonzero(self.has_mesh))

    def robot_kwargs(self, ltip="panda_lefttip", rtip="panda_righttip", mobile=None):
        """The keyword arguments tasks.franka.Franka / MobileFranka take, from the asset instead of from their defaults.  mobile
        (None: the tree's first DOF is prismatic, i.e. base slides in front of the arm) adds MobileFranka's `mesh_bodies`."""
        if mobile is None:
            mobile = bool(self.jtype[self.dof == 0][0] == PRISMATIC)
        kw = dict(num_dofs=self.num_dofs, num_rigid_body=self.num_bodies, dof_lower=tuple(float(v) for v in self.lower),
                  dof_upper=tuple(float(v) for v in self.upper), ltip_rb_index=self.body_index(ltip),
                  rtip_rb_index=self.body_index(rtip))
        if mobile:
            kw["mesh_bodies"] = self.mesh_bodies()
        return kw


def _has_mesh(link):
    return any(g.find("geometry/mesh") is not None for tag in ("collision", "visual") for g in link.findall(tag))


def load_urdf(path_or_string, scale=1.0):
    """A URDF file's path, or its text (anything that starts with '<'), -> KinematicTree.  scale multiplies the joint-origin
    translations and the lower / upper limits of prismatic joints, and nothing else (not rpy, axes, revolute limits or velocity
    limits): what the simulator's actor scale does to a tree's kinematics (the reference's set_actor_scale, 0.5 for its cabinets);
    prismatic joint positions are then in scaled metres.  The default changes nothing."""
    scale = float(scale)
    if not scale > 0 or not np.isfinite(scale):
        raise ValueError(f"scale: expected a positive finite number, got {scale}")
    text = path_or_string
    if not str(text).lstrip().startswith("<"):
        with open(os.fspath(path_or_string), encoding="utf-8") as f:
            text = f.read()
    robot = ET.fromstring(text)                               # comments are dropped by the parser
    links = {}
    for ln in robot.findall("link"):
        links[ln.get("name")] = ln
    children, child_of = {name: [] for name in links}, {}
    for j in robot.findall("joint"):
        jn, jt = j.get("name"), j.get("type")
        if jt not in JOINT_TYPES:
            raise ValueError(f"joint {jn!r}: type {jt!r} is not supported (supported: {sorted(JOINT_TYPES)})")
        par, ch = j.find("parent"), j.find("child")
        par = None if par is None else par.get("link")
        ch = None if ch is None else ch.get("link")
        if par not in links:
            raise ValueError(f"joint {jn!r}: unknown parent link {par!r}")
        if ch not in links:
            raise ValueError(f"joint {jn!r}: unknown child link {ch!r}")
        if ch in child_of:
            raise ValueError(f"joint {jn!r}: link {ch!r} already is the child of joint {child_of[ch].get('name')!r}")
        child_of[ch] = j
        children[par].append(j)
    if not links:
        raise ValueError("the URDF has no link")
    roots = [name for name in links if name not in child_of]
    if not roots:
        raise ValueError(f"joint {next(iter(child_of.values())).get('name')!r} is part of a cycle: no link is a root")
    if len(roots) > 1:
        via = children[roots[1]][0].get("name") if children[roots[1]] else None
        raise ValueError(f"more than one root link: {roots} (joint {via!r} hangs off the second)")
    names, joint_names, parent, jtype, origin_t, origin_rpy, axis, limits, has_mesh = [], [], [], [], [], [], [], [], []
    stack = [(roots[0], -1, None)]
    while stack:                                              # depth first, a link's children in file order
        name, par, j = stack.pop()
        b = len(names)
        names.append(name), parent.append(par), has_mesh.append(_has_mesh(links[name]))
        t, rpy, ax, lim, jt = np.zeros(3), np.zeros(3), np.zeros(3), (-np.inf, np.inf, np.inf), FIXED
        if j is not None:
            jn = j.get("name")
            jt = JOINT_TYPES[j.get("type")]
            o = j.find("origin")
            if o is not None:
                t = _floats(o.get("xyz", "0 0 0"), 3, f"joint {jn!r} origin xyz")
                rpy = _floats(o.get("rpy", "0 0 0"), 3, f"joint {jn!r} origin rpy")
                t = t * scale
            if jt != FIXED:
                a = j.find("axis")
                ax = _floats(a.get("xyz", "1 0 0"), 3, f"joint {jn!r} axis") if a is not None else np.array([1.0, 0.0, 0.0])
                n = np.linalg.norm(ax)
                if not n > 0:
                    raise ValueError(f"joint {jn!r}: a zero axis")
                ax = ax / n
                le = j.find("limit")
                if le is not None:
                    lo, hi = (-np.inf, np.inf) if j.get("type") == "continuous" else (float(le.get("lower", 0)), float(le.get("upper", 0)))
                    if jt == PRISMATIC:
                        lo, hi = lo * scale, hi * scale
                    lim = (lo, hi, float(le.get("velocity", np.inf)))
        joint_names.append(None if j is None else j.get("name"))
        jtype.append(jt), origin_t.append(t), origin_rpy.append(rpy), axis.append(ax), limits.append(lim)
        for cj in reversed(children[name]):
            stack.append((cj.find("child").get("link"), b, cj))
    if len(names) != len(links):
        lost = next(n for n in links if n not in names)
        raise ValueError(f"joint {child_of[lost].get('name')!r} is part of a cycle: link {lost!r} is not reachable from the root "
                         f"{roots[0]!r}")
    return KinematicTree(names, joint_names, parent, jtype, origin_t, origin_rpy, axis, limits, has_mesh)


def _rpy_matrix(rpy):
    """Rz(yaw) Ry(pitch) Rx(roll) in float64: the rotation rpy_to_quat encodes."""
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], dtype=np.float64)


def load_urdf_visuals(path, scale=1.0):
    """The visual meshes of a URDF file, one entry per body in load_urdf's body order: (vertices (n, 3) float32, faces (f, 3) int64)
    in the body's frame, or None for a body without a mesh.  A body's mesh is every <visual> of its link that has a geometry/mesh,
    concatenated in file order; where no visual has one, the <collision> meshes instead.  A mesh is read by meshio.load_mesh from
    its file name taken relative to the URDF's folder (a leading `package://` is dropped), multiplied by the mesh tag's `scale`
    (default 1 1 1), moved by the visual's <origin xyz rpy> (rpy as in rpy_to_quat: Rz Ry Rx), then multiplied by `scale` -- the
    simulator's actor scale, as in load_urdf; all in float64, rounded to float32 once.  Textures and materials are not read.
    ValueError, naming the file and the link: a missing mesh file, a mesh that cannot be read, a face index out of range."""
    from . import meshio
    scale = float(scale)
    if not scale > 0 or not np.isfinite(scale):
        raise ValueError(f"scale: expected a positive finite number, got {scale}")
    path = os.fspath(path)
    tree = load_urdf(path)
    folder = os.path.dirname(os.path.abspath(path))
    with open(path, encoding="utf-8") as f:
        links = {ln.get("name"): ln for ln in ET.fromstring(f.read()).findall("link")}
    out = []
    for name in tree.names:
        shapes = []
        for tag in ("visual", "collision"):
            shapes = [e for e in links[name].findall(tag) if e.find("geometry/mesh") is not None]
            if shapes:
                break
        verts, faces, base = [], [], 0
        for e in shapes:
            mesh = e.find("geometry/mesh")
            fn = mesh.get("filename") or ""
            if fn.startswith("package://"):
                fn = fn[len("package://"):]
            file = os.path.join(folder, fn)
            if not fn or not os.path.isfile(file):
                raise ValueError(f"{file}: missing mesh file of link {name!r}")
            try:
                v, fa = meshio.load_mesh(file)
            except ValueError as err:
                raise ValueError(f"{file}: the mesh of link {name!r} cannot be read ({err})") from None
            fa = np.asarray(fa, dtype=np.int64).reshape(-1, 3)
            if fa.size and (fa.min() < 0 or fa.max() >= len(v)):
                raise ValueError(f"{file}: a face index of the mesh of link {name!r} lies outside [0, {len(v)})")
            ms = _floats(mesh.get("scale", "1 1 1"), 3, f"link {name!r} mesh scale")
            o = e.find("origin")
            t = _floats(o.get("xyz", "0 0 0"), 3, f"link {name!r} origin xyz") if o is not None else np.zeros(3)
            rpy = _floats(o.get("rpy", "0 0 0"), 3, f"link {name!r} origin rpy") if o is not None else np.zeros(3)
            x = np.asarray(v, dtype=np.float64).reshape(-1, 3) * ms
            verts.append(((x @ _rpy_matrix(rpy).T + t) * scale).astype(np.float32))
            faces.append(fa + base)
            base += len(v)
        nf = sum(len(fa) for fa in faces)
        out.append((np.concatenate(verts), np.concatenate(faces)) if nf else None)
    return out
