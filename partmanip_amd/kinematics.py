"""A kinematic stand-in for the simulator's robot: body poses, velocities and the Jacobian of a URDF tree, one HIP launch per step
(csrc/articulation.hip through ops.articulation_step).

    tree = load_urdf("franka_panda_sdf.urdf")
    sim = KinematicSim(tree, N, device, dt, base_pose=(0, 0, 0, 0, 0, 0, 1), num_bodies=14, num_actors=2)
    sim.set_dof_state(robot.default_dof_pos)
    rigid_body, dof_state, jacobian = sim.step(pos_act, reset)     # what the task steps call the simulator's three tensors

It is not physics: no dynamics, no contact forces, no gravity; the joints follow their position targets (exactly, or at most
max_velocity fast) inside their limits.  The one contact rule is opt-in and blocks, it does not push: step(guard=) stops the whole
robot at the last of S parts of the step before a sensing point would enter a target (contact.StepGuard).  Rows of the tensors that are not the robot's (the cube, a cabinet) belong to the caller and are never
written after construction, unless one of the two scenes below is asked for.

With `free_body=True` and tips=(ltip, rtip) every environment also holds one free rigid body (the cube of grasp_cube: the last body
row, actor 1), and a second launch per step (csrc/free_body.hip through ops.free_body_step) moves it by a stated rule: reset puts it
back at free_body_pose, `hold` latches its pose in the hand frame (the mean of the two tips, the left tip's orientation) and carries
it from then on, a released body sinks at fall_speed down to rest_z or, at the default 0, stays where it is (include/partmanip_hip.h
states it in full).  `grip` (N, 8), the latched relative pose and the latch, belongs to the sim.

With `objects=` (an ObjectLibrary of cabinet trees, tasks.open_drawer.load_drawer_assets) every environment also holds one object of
its own type, laid out after the robot's rows as tasks.open_drawer.build_masks lays them out, and a second launch per step
(csrc/articulation_objects.hip through ops.articulation_objects_step) poses it from root[:, 1, :7].  An object's joints keep their
state; the one rule that moves one is the HOLD RULE: where `hold` is set, the target joint takes the displacement that the mean
velocity of the robot's two tips asks of it along its own freedom, inside its limits (include/partmanip_hip.h states it in full).
That is a kinematic rule the caller switches on, not a grasp: nothing here knows whether the gripper touches the handle."""
import numpy as np
import torch

from . import ops
from .urdf import FIXED, PRISMATIC, REVOLUTE

RESET_RANGE = 0.15                                            # the cube's random_reset range (the reference's grasp_cube.py:17-21)


def _checked_tables(tree):
    """(parent, jtype, dof) int64 of a tree, after what the kernels rely on and the C entries cannot see."""
    nb, nd = tree.num_bodies, tree.num_dofs
    parent, jtype, dof = (np.asarray(a, dtype=np.int64) for a in (tree.parent, tree.jtype, tree.dof))
    if parent[0] != -1 or any(not 0 <= parent[b] < b for b in range(1, nb)):
        raise ValueError("tree.parent: the root comes first and every parent precedes its children")
    if any(t not in (FIXED, REVOLUTE, PRISMATIC) for t in jtype):
        raise ValueError("tree.jtype: expected 0 (fixed), 1 (revolute) or 2 (prismatic)")
    moving = jtype != FIXED
    if sorted(dof[moving]) != list(range(nd)) or any(dof[~moving] != -1):
        raise ValueError(f"tree.dof: the moving joints must name the DOFs 0 .. {nd - 1} once each and fixed joints -1")
    return parent, jtype, dof


class Articulation:
    """The tree's tables on the device, uploaded once, and the pure forward-kinematics call."""

    def __init__(self, tree, num_envs, device):
        nb, nd = tree.num_bodies, tree.num_dofs
        parent, jtype, dof = _checked_tables(tree)
        self.tree, self.num_envs, self.device = tree, int(num_envs), device
        self.num_bodies, self.num_dofs = nb, nd
        f = dict(dtype=torch.float32, device=device)
        i = dict(dtype=torch.int32, device=device)
        self.parent, self.jtype, self.dof = (torch.as_tensor(np.asarray(a, dtype=np.int32), **i).contiguous() for a in (parent, jtype, dof))
        self.origin_q = torch.as_tensor(tree.origin_q, **f).contiguous()
        self.origin_t = torch.as_tensor(tree.origin_t, **f).contiguous()
        self.axis = torch.as_tensor(tree.axis, **f).contiguous()
        self.anc_mask = torch.as_tensor(np.asarray(tree.anc_mask, dtype=np.uint64).view(np.int64), dtype=torch.int64, device=device)
        self.dof_lower = torch.as_tensor(tree.lower, **f).contiguous()
        self.dof_upper = torch.as_tensor(tree.upper, **f).contiguous()

    def _tables(self):
        return (self.parent, self.jtype, self.dof, self.origin_q, self.origin_t, self.axis, self.anc_mask, self.dof_lower,
                self.dof_upper)

    def step(self, dof_state, base_pose, targets=None, reset=None, vmax=None, dt=0.0, rigid_body=None, jacobian=None, rb_row0=None,
             dof_row0=None):
        """ops.articulation_step on this tree; every tensor is the caller's."""
        ops.articulation_step(*self._tables(), base_pose, dof_state, targets=targets, reset=reset, vmax=vmax, dt=dt,
                              rigid_body=rigid_body, jac=jacobian, rb_row0=rb_row0, dof_row0=dof_row0)

    def sweep(self, dof_state, base_pose, targets, dt, *sensing, reset=None, free=None, vmax=None, dof_row0=None, **kw):
        """ops.articulation_sweep on this tree: the swept contact test of the step from dof_state towards targets, which writes no
        state.  `sensing` and the other keywords are that function's arguments from `fields` on (contact.StepGuard holds them).
        Returns (sweep_dist, steps, targets_out)."""
        return ops.articulation_sweep(*self._tables(), base_pose, dof_state, targets, dt, *sensing, reset=reset, free=free, vmax=vmax,
                                      dof_row0=dof_row0, **kw)

    def forward(self, dof_state, base_pose, rigid_body=None, jacobian=None, rb_row0=None, dof_row0=None):
        """Pure forward kinematics of dof_state (N, nd, 2), which is only read: (rigid_body (N, nb, 13), jacobian (N, nb - 1, 6, nd)),
        written into the caller's tensors where given (rigid_body may be wider, or flat with rb_row0) and into new ones otherwise."""
        N = self.num_envs
        f = dict(dtype=torch.float32, device=self.device)
        if rigid_body is None:
            if rb_row0 is not None:
                raise ValueError("rb_row0 needs the flat rigid_body it indexes")
            rigid_body = torch.zeros(N, self.num_bodies, 13, **f)
        if jacobian is None:
            jacobian = torch.zeros(N, self.num_bodies - 1, 6, self.num_dofs, **f)
        self.step(dof_state, base_pose, rigid_body=rigid_body, jacobian=jacobian, rb_row0=rb_row0, dof_row0=dof_row0)
        return rigid_body, jacobian


class ObjectLibrary:
    """K object trees laid end to end on the device, for ops.articulation_objects_step: body_off / dof_off (K + 1) int32, the
    per-body tables of Articulation over all the trees' bodies (parent and dof local to their tree), dof_lower / dof_upper over all
    their DOFs, and on the host num_bodies[k], num_dofs[k], max_bodies, max_dofs.  Each tree is validated exactly as Articulation
    validates its own (the ValueError names the tree)."""

    def __init__(self, trees, device):
        trees = list(trees)
        if not trees:
            raise ValueError("ObjectLibrary: expected at least one tree")
        cols = []
        for k, tree in enumerate(trees):
            try:
                cols.append(_checked_tables(tree))
            except ValueError as err:
                raise ValueError(f"tree {k}: {err}") from None
        self.trees, self.device, self.num_types = trees, device, len(trees)
        self.num_bodies = [t.num_bodies for t in trees]
        self.num_dofs = [t.num_dofs for t in trees]
        self.max_bodies, self.max_dofs = max(self.num_bodies), max(self.num_dofs)
        f = dict(dtype=torch.float32, device=device)
        i = dict(dtype=torch.int32, device=device)
        off = lambda n: torch.as_tensor(np.concatenate([[0], np.cumsum(n)]).astype(np.int32), **i)      # noqa: E731
        self.body_off, self.dof_off = off(self.num_bodies), off(self.num_dofs)
        cat = lambda j: torch.as_tensor(np.concatenate([c[j] for c in cols]).astype(np.int32), **i).contiguous()     # noqa: E731
        self.parent, self.jtype, self.dof = cat(0), cat(1), cat(2)
        catf = lambda name: torch.as_tensor(np.concatenate([np.asarray(getattr(t, name)) for t in trees]), **f).contiguous()   # noqa: E731
        self.origin_q, self.origin_t, self.axis = catf("origin_q"), catf("origin_t"), catf("axis")
        mask = np.concatenate([np.asarray(t.anc_mask, dtype=np.uint64) for t in trees])
        self.anc_mask = torch.as_tensor(mask.view(np.int64), dtype=torch.int64, device=device)
        self.dof_lower, self.dof_upper = catf("lower"), catf("upper")

    def _tables(self):
        return (self.body_off, self.dof_off, self.parent, self.jtype, self.dof, self.origin_q, self.origin_t, self.axis, self.anc_mask,
                self.dof_lower, self.dof_upper, self.max_bodies, self.max_dofs)

    def types_of(self, obj_type, N):
        """obj_type checked on the host -> (N) int64 numpy."""
        k = np.asarray(obj_type.cpu() if torch.is_tensor(obj_type) else obj_type)
        if k.dtype.kind not in "iu" or k.shape != (N,) or (k < 0).any() or (k >= self.num_types).any():
            raise ValueError(f"obj_type: expected {N} integers in [0, {self.num_types})")
        return k.astype(np.int64)

    def order_of(self, obj_type):
        """The environments grouped by type (a stable sort), (N) int32 on the device: which lane computes which environment, and
        nothing else (the kernel's results do not depend on it)."""
        k = self.types_of(obj_type, len(obj_type))
        return torch.as_tensor(np.argsort(k, kind="stable").astype(np.int32), device=self.device)

    def step(self, obj_type, obj_pose, obj_rb_row0, obj_dof_row0, dof_state, rigid_body, order=None, hold=None, reset=None,
             target_dof=None, tip_rows=None, dt=0.0):
        """ops.articulation_objects_step on this library; every tensor is the caller's."""
        ops.articulation_objects_step(*self._tables(), obj_type, obj_pose, obj_rb_row0, obj_dof_row0, dof_state, rigid_body,
                                      order=order, hold=hold, reset=reset, target_dof=target_dof, tip_rows=tip_rows, dt=dt)


def _row_table(rows, name, N, n, device):
    """A per-environment first-row table -> ((N) int32 on the device, rows needed), checked on the host: n rows per environment,
    no two environments overlapping."""
    t = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows, dtype=np.int64).reshape(-1)
    if t.size != N or (t < 0).any():
        raise ValueError(f"{name}: expected {N} non-negative first rows")
    s = np.sort(t)
    if (np.diff(s) < n).any():
        raise ValueError(f"{name}: two environments' {n} rows overlap")
    return torch.as_tensor(t.astype(np.int32), device=device).contiguous(), int(s[-1]) + n


class KinematicSim:
    """Owns rigid_body, dof_state, root and jacobian in the layouts the task classes take and steps the robot's rows.

    Dense (the grasp_cube layout): rigid_body (N, num_bodies, 13) with the robot's nb rows first, dof_state (N, nd, 2), root
    (N, num_actors, 13) with the robot as actor 0, jacobian (N, nb - 1, 6, nd).  With rb_row0 / dof_row0 (N first rows, the open_drawer
    layout) rigid_body is flat (num_bodies, 13) and dof_state flat (num_dof_rows, 2); both tables are then needed.  Rows that are not
    the robot's start at zero position and unit quaternion and belong to the caller.  base_pose: (7) or (N, 7), position and
    quaternion (x, y, z, w).  max_velocity: None (the joints reach their targets in one step), 'urdf' (the file's velocity limits) or
    (nd) values.

    objects=ObjectLibrary with obj_type (N) (the open_drawer layout, always flat): environment e holds the robot's nb rows and then
    the nb_k rows of its object, its DOF rows likewise, exactly the rows of tasks.open_drawer.build_masks; rb_row0 / dof_row0 /
    obj_rb_row0 / obj_dof_row0 (N) int32 and the totals B and D are attributes.  The object is actor 1: root[:, 1, :7] starts as
    obj_pose ((7) or (N, 7)) and is read by every launch, so a task reset that rewrites it moves the cabinet.  target_dof (N), local to
    the object, and tips=(ltip, rtip), the robot's tip bodies, are what step(hold=...) needs.  Without objects= nothing changes.

    free_body=True with tips=(ltip, rtip) (the dense layout, or rb_row0 layouts without objects=): one free rigid body per environment,
    actor 1 and the LAST body row of the dense tensor (num_bodies defaults to nb + 1; with rb_row0 the row after the robot's).  Its
    rows start at free_body_pose; rest_z, fall_speed and reset_range are the rule's constants (defaults: the task's cube).  grip
    (N, 8), free_body_row (N) and tip_rows (N, 2) (flat rows) are attributes.  forward() and set_dof_state() leave the body alone."""

    def __init__(self, tree, num_envs, device, dt, base_pose=(0, 0, 0, 0, 0, 0, 1), num_bodies=None, num_actors=None, max_velocity=None,
                 rb_row0=None, dof_row0=None, num_dof_rows=None, objects=None, obj_type=None, obj_pose=None, target_dof=None, tips=None,
                 free_body=False, free_body_pose=(0, 0, 0.025, 0, 0, 0, 1), rest_z=0.025, fall_speed=0.0, reset_range=RESET_RANGE):
        self.art = Articulation(tree, num_envs, device)
        N, nb, nd = int(num_envs), tree.num_bodies, tree.num_dofs
        self.num_envs, self.device, self.dt = N, device, float(dt)
        if not self.dt > 0:
            raise ValueError(f"dt: expected a positive step, got {dt}")
        f = dict(dtype=torch.float32, device=device)
        self.objects, self.free_body = objects, bool(free_body)
        fb_rows = 1 if self.free_body else 0                  # the free body's row comes right after the robot's
        if self.free_body:
            if objects is not None:
                raise ValueError("free_body= and objects= are two scenes: one free body or one cabinet per environment")
            if tips is None:
                raise ValueError("free_body= needs tips=(ltip, rtip), the robot's tip bodies")
            lt, rt = (int(v) for v in tips)
            if not (0 <= lt < nb and 0 <= rt < nb):
                raise ValueError(f"tips: expected two of the robot's {nb} bodies, got {tips}")
            if not float(fall_speed) >= 0 or not float(reset_range) >= 0 or float(rest_z) != float(rest_z):
                raise ValueError(f"fall_speed {fall_speed} and reset_range {reset_range}: expected non-negative numbers, rest_z {rest_z} a number")
            self.rest_z, self.fall_speed, self.reset_range = float(rest_z), float(fall_speed), float(reset_range)
            num_actors = 2 if num_actors is None else num_actors
            if int(num_actors) < 2:
                raise ValueError("num_actors: with free_body= the body is actor 1")
            if rb_row0 is None and num_bodies is None:
                num_bodies = nb + 1
            tips = None
        if objects is None:
            if any(a is not None for a in (obj_type, obj_pose, target_dof, tips)):
                raise ValueError("obj_type, obj_pose, target_dof and tips need objects= (tips: or free_body=)")
            num_actors = 1 if num_actors is None else num_actors
        else:
            if rb_row0 is not None or dof_row0 is not None:
                raise ValueError("with objects= the row tables are laid out here (robot first, then the object): pass none")
            num_actors = 2 if num_actors is None else num_actors
            if int(num_actors) < 2:
                raise ValueError("num_actors: with objects= the object is actor 1")
            k = objects.types_of(obj_type, N)
            onb, ond = np.asarray(objects.num_bodies)[k], np.asarray(objects.num_dofs)[k]
            rb_row0 = np.concatenate([[0], np.cumsum(nb + onb)[:-1]])
            dof_row0 = np.concatenate([[0], np.cumsum(nd + ond)[:-1]])
            need_B, need_D = int((nb + onb).sum()), int((nd + ond).sum())
            num_bodies = need_B if num_bodies is None else int(num_bodies)
            num_dof_rows = need_D if num_dof_rows is None else int(num_dof_rows)
            if num_bodies < need_B or num_dof_rows < need_D:
                raise ValueError(f"robots and objects need {need_B} body rows and {need_D} DOF rows, got {num_bodies} and {num_dof_rows}")
            i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32), device=device).contiguous()      # noqa: E731
            self.obj_type, self.obj_rb_row0, self.obj_dof_row0 = i32(k), i32(rb_row0 + nb), i32(dof_row0 + nd)
            self._order = objects.order_of(k)
            self.target_dof = self.tip_rows = None
            if target_dof is not None:
                td = np.asarray(target_dof.cpu() if torch.is_tensor(target_dof) else target_dof, dtype=np.int64).reshape(-1)
                if td.shape != (N,) or (td < 0).any() or (td >= ond).any():
                    raise ValueError(f"target_dof: expected {N} DOF indices local to each environment's object")
                self.target_dof = i32(td)
            if tips is not None:
                lt, rt = (int(v) for v in tips)
                if not (0 <= lt < nb and 0 <= rt < nb):
                    raise ValueError(f"tips: expected two of the robot's {nb} bodies, got {tips}")
                self.tip_rows = i32(np.stack([rb_row0 + lt, rb_row0 + rt], axis=1))
            self._no_flags = torch.zeros(N, dtype=torch.bool, device=device)
            # (flat row, environment, local DOF) of every object DOF, for set_dof_state(obj_q=)
            self._obj_dof_env = np.repeat(np.arange(N), ond)
            self._obj_dof_local = np.concatenate([np.arange(n) for n in ond])
            self._obj_dof_index = torch.as_tensor((dof_row0 + nd)[self._obj_dof_env] + self._obj_dof_local, device=device)
        if (rb_row0 is None) != (dof_row0 is None):
            raise ValueError("rb_row0 and dof_row0 come together (flat layouts) or not at all")
        self.flat = rb_row0 is not None
        if self.flat:
            self.rb_row0, need_rb = _row_table(rb_row0, "rb_row0", N, nb + fb_rows, device)
            self.dof_row0, need_dof = _row_table(dof_row0, "dof_row0", N, nd, device)
            B = need_rb if num_bodies is None else int(num_bodies)
            D = need_dof if num_dof_rows is None else int(num_dof_rows)
            if B < need_rb or D < need_dof:
                raise ValueError(f"the row tables need {need_rb} body rows and {need_dof} DOF rows, got {B} and {D}")
            self.rigid_body, self.dof_state = torch.zeros(B, 13, **f), torch.zeros(D, 2, **f)
            self._dof_index = (self.dof_row0.long()[:, None] + torch.arange(nd, device=device)[None]).reshape(-1)
        else:
            self.rb_row0 = self.dof_row0 = None
            nbt = nb if num_bodies is None else int(num_bodies)
            if nbt < nb + fb_rows:
                raise ValueError(f"num_bodies {nbt} below the robot's {nb}" + (" and the free body's row" if fb_rows else ""))
            self.rigid_body, self.dof_state = torch.zeros(N, nbt, 13, **f), torch.zeros(N, nd, 2, **f)
        self.rigid_body[..., 6] = 1.0
        bp = torch.as_tensor(base_pose, **f)
        if tuple(bp.shape) not in ((7,), (N, 7)):
            raise ValueError(f"base_pose: expected (7) or ({N}, 7), got {tuple(bp.shape)}")
        self.base_pose = bp.contiguous()
        if int(num_actors) < 1:
            raise ValueError("num_actors: the robot is actor 0")
        self.root = torch.zeros(N, int(num_actors), 13, **f)
        self.root[..., 6] = 1.0
        self.root[:, 0, :7] = self.base_pose
        if objects is not None:
            from .tasks.open_drawer import OBJ_DEFAULT_ROOT
            op = torch.as_tensor(OBJ_DEFAULT_ROOT if obj_pose is None else obj_pose, **f)
            if tuple(op.shape) not in ((7,), (N, 7)):
                raise ValueError(f"obj_pose: expected (7) or ({N}, 7), got {tuple(op.shape)}")
            self.root[:, 1, :7] = op
            self.B, self.D = self.rigid_body.shape[0], self.dof_state.shape[0]
        if self.free_body:
            # flat rows of rigid_body: dense, the LAST body row of each environment; with rb_row0, the row after the robot's
            first = self.rb_row0.long() if self.flat else torch.arange(N, device=device) * self.rigid_body.shape[1]
            body = first + nb if self.flat else first + self.rigid_body.shape[1] - 1
            self.free_body_row = body.to(torch.int32).contiguous()
            self.tip_rows = torch.stack([first + lt, first + rt], dim=1).to(torch.int32).contiguous()
            fp = torch.as_tensor(free_body_pose, **f)
            if tuple(fp.shape) != (7,):
                raise ValueError(f"free_body_pose: expected (7), got {tuple(fp.shape)}")
            self.free_body_pose = fp.contiguous()
            self.grip = torch.zeros(N, 8, **f)                # rel_t, rel_q, latch: the free-body launch's own state
            self.root[:, 1, :7] = fp
            self.rigid_body.view(-1, 13)[self.free_body_row.long(), :7] = fp
            self._no_flags = torch.zeros(N, dtype=torch.bool, device=device)
        self.jacobian = torch.zeros(N, nb - 1, 6, nd, **f)
        if max_velocity is None:
            self.max_velocity = None
        elif isinstance(max_velocity, str):
            if max_velocity != "urdf":
                raise ValueError(f"max_velocity: expected None, 'urdf' or {nd} values, got {max_velocity!r}")
            self.max_velocity = torch.as_tensor(tree.velocity, **f).contiguous()
        else:
            self.max_velocity = torch.as_tensor(max_velocity, **f).reshape(-1).contiguous()
            if self.max_velocity.numel() != nd:
                raise ValueError(f"max_velocity: expected {nd} values, got {self.max_velocity.numel()}")
        self.forward()

    def _objects_step(self, reset=None, hold=None):
        group = {}
        if hold is not None:
            if self.target_dof is None or self.tip_rows is None:
                raise ValueError("hold needs target_dof= and tips= at construction")
            group = dict(hold=hold, reset=self._no_flags if reset is None else reset, target_dof=self.target_dof, tip_rows=self.tip_rows,
                         dt=self.dt)
        self.objects.step(self.obj_type, self.root[:, 1, :7], self.obj_rb_row0, self.obj_dof_row0, self.dof_state, self.rigid_body,
                          order=self._order, **group)

    def forward(self):
        """Body rows and Jacobian of the joint state as it stands (one launch, and one for the objects; dof_state is only read)."""
        self.art.step(self.dof_state, self.base_pose, rigid_body=self.rigid_body, jacobian=self.jacobian, rb_row0=self.rb_row0,
                      dof_row0=self.dof_row0)
        if self.objects is not None:
            self._objects_step()
        return self.rigid_body, self.dof_state, self.jacobian

    def set_dof_state(self, q, qd=None, obj_q=None):
        """Joint positions q (nd) or (N, nd) and velocities qd (zero where None), then the body rows and the Jacobian they give.
        obj_q (with objects=): a number, or (N, max_dofs) of which environment e's first nd_k columns are its object's joint
        positions (at rest); None leaves the objects' joints as they are."""
        if obj_q is not None:
            if self.objects is None:
                raise ValueError("obj_q needs objects=")
            v = torch.as_tensor(obj_q, dtype=torch.float32, device=self.device)
            if v.dim() == 0:
                v = v.expand(self.num_envs, self.objects.max_dofs)
            if tuple(v.shape) != (self.num_envs, self.objects.max_dofs):
                raise ValueError(f"obj_q: expected a number or ({self.num_envs}, {self.objects.max_dofs}), got {tuple(v.shape)}")
            rows = torch.zeros(self._obj_dof_index.numel(), 2, dtype=torch.float32, device=self.device)
            rows[:, 0] = v[torch.as_tensor(self._obj_dof_env, device=self.device), torch.as_tensor(self._obj_dof_local, device=self.device)]
            self.dof_state[self._obj_dof_index] = rows
        N, nd = self.num_envs, self.art.num_dofs
        f = dict(dtype=torch.float32, device=self.device)
        s = torch.zeros(N, nd, 2, **f)
        s[..., 0] = torch.as_tensor(q, **f)
        if qd is not None:
            s[..., 1] = torch.as_tensor(qd, **f)
        if self.flat:
            self.dof_state[self._dof_index] = s.reshape(-1, 2)
        else:
            self.dof_state.copy_(s)
        return self.forward()

    def _free_body_step(self, hold, reset, u):
        ops.free_body_step(self.rigid_body, self.tip_rows, self.free_body_row, self.root, 1, self._no_flags if hold is None else hold,
                           self._no_flags if reset is None else reset, self.grip, self.free_body_pose, self.dt, u=u,
                           reset_range=self.reset_range, rest_z=self.rest_z, fall_speed=self.fall_speed)

    def reset_free_body(self, u=None):
        """The free body's launch alone with reset set everywhere: every environment's body goes back to free_body_pose, moved by u
        (N, 3) in [0, 1) where given, at rest and unlatched.  The robot is not touched."""
        if not self.free_body:
            raise ValueError("reset_free_body needs free_body=")
        self._free_body_step(None, ~self._no_flags, u)
        return self.rigid_body, self.dof_state, self.jacobian

    def step(self, pos_act, reset=None, hold=None, u=None, guard=None):
        """One launch: the joints move towards pos_act (N, nd), environments with reset set snap to it at rest; returns
        (rigid_body, dof_state, jacobian), updated in place.  With objects= a second launch on the same stream then poses every
        environment's object from root[:, 1, :7] and its DOF rows as they stand (a task reset has already written them).  hold (N)
        bool / uint8, or None: where set (and reset is not) the object's target joint follows the tips' mean velocity of THIS step
        (the hold rule); where not, it keeps its position at zero velocity; None: the objects' DOF rows are only read.
        With free_body= the second launch is the free body's (ops.free_body_step): hold (None: nowhere) latches and carries it, reset
        puts it back at free_body_pose, moved by u (N, 3) in [0, 1) where given (xy inside +-reset_range and a yaw).
        guard: None, or a contact.StepGuard (contact blocking).  One more launch first: the swept test of this step
        (ops.articulation_sweep) cuts it into guard.substeps parts and finds, per environment, the last part the robot can reach
        without a sensing point coming within guard.margin of a target or deeper into one; the articulation launch then runs on
        guard.targets with no rate limit (the sweep has applied it), so the joints stop at that candidate bit for bit.  Environments
        with reset or hold set are not guarded (a held cube or drawer moves with the hand).  The whole robot stops, nothing slides or
        is pushed, and the rule sees the scene as guard's pose table has it (the caller's last observation).  None: exactly the
        launches above."""
        if u is not None and not self.free_body:
            raise ValueError("u needs free_body=")
        vmax = self.max_velocity
        if guard is not None:
            pos_act = guard.sweep(self, pos_act, reset, hold)
            vmax = None
        self.art.step(self.dof_state, self.base_pose, targets=pos_act, reset=reset, vmax=vmax, dt=self.dt,
                      rigid_body=self.rigid_body, jacobian=self.jacobian, rb_row0=self.rb_row0, dof_row0=self.dof_row0)
        if self.objects is not None:
            self._objects_step(reset, hold)
        elif self.free_body:
            self._free_body_step(hold, reset, u)
        elif hold is not None:
            raise ValueError("hold needs objects= or free_body=")
        return self.rigid_body, self.dof_state, self.jacobian
