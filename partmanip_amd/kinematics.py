"""A kinematic stand-in for the simulator's robot: body poses, velocities and the Jacobian of a URDF tree, one HIP launch per step
(csrc/articulation.hip through ops.articulation_step).

    tree = load_urdf("franka_panda_sdf.urdf")
    sim = KinematicSim(tree, N, device, dt, base_pose=(0, 0, 0, 0, 0, 0, 1), num_bodies=14, num_actors=2)
    sim.set_dof_state(robot.default_dof_pos)
    rigid_body, dof_state, jacobian = sim.step(pos_act, reset)     # what the task steps call the simulator's three tensors

It is not physics: no dynamics, no contact, no gravity; the joints follow their position targets (exactly, or at most max_velocity
fast) inside their limits.  Rows of the tensors that are not the robot's (the cube, a cabinet) belong to the caller and are never
written after construction."""
import numpy as np
import torch

from . import ops
from .urdf import FIXED, PRISMATIC, REVOLUTE


class Articulation:
    """The tree's tables on the device, uploaded once, and the pure forward-kinematics call."""

    def __init__(self, tree, num_envs, device):
        nb, nd = tree.num_bodies, tree.num_dofs
        parent, jtype, dof = (np.asarray(a, dtype=np.int64) for a in (tree.parent, tree.jtype, tree.dof))
        # what the kernel relies on and the C entry cannot see
        if parent[0] != -1 or any(not 0 <= parent[b] < b for b in range(1, nb)):
            raise ValueError("tree.parent: the root comes first and every parent precedes its children")
        if any(t not in (FIXED, REVOLUTE, PRISMATIC) for t in jtype):
            raise ValueError("tree.jtype: expected 0 (fixed), 1 (revolute) or 2 (prismatic)")
        moving = jtype != FIXED
        if sorted(dof[moving]) != list(range(nd)) or any(dof[~moving] != -1):
            raise ValueError(f"tree.dof: the moving joints must name the DOFs 0 .. {nd - 1} once each and fixed joints -1")
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
    (nd) values."""

    def __init__(self, tree, num_envs, device, dt, base_pose=(0, 0, 0, 0, 0, 0, 1), num_bodies=None, num_actors=1, max_velocity=None,
                 rb_row0=None, dof_row0=None, num_dof_rows=None):
        self.art = Articulation(tree, num_envs, device)
        N, nb, nd = int(num_envs), tree.num_bodies, tree.num_dofs
        self.num_envs, self.device, self.dt = N, device, float(dt)
        if not self.dt > 0:
            raise ValueError(f"dt: expected a positive step, got {dt}")
        f = dict(dtype=torch.float32, device=device)
        if (rb_row0 is None) != (dof_row0 is None):
            raise ValueError("rb_row0 and dof_row0 come together (flat layouts) or not at all")
        self.flat = rb_row0 is not None
        if self.flat:
            self.rb_row0, need_rb = _row_table(rb_row0, "rb_row0", N, nb, device)
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
            if nbt < nb:
                raise ValueError(f"num_bodies {nbt} below the robot's {nb}")
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

    def forward(self):
        """Body rows and Jacobian of the joint state as it stands (one launch; dof_state is only read)."""
        self.art.step(self.dof_state, self.base_pose, rigid_body=self.rigid_body, jacobian=self.jacobian, rb_row0=self.rb_row0,
                      dof_row0=self.dof_row0)
        return self.rigid_body, self.dof_state, self.jacobian

    def set_dof_state(self, q, qd=None):
        """Joint positions q (nd) or (N, nd) and velocities qd (zero where None), then the body rows and the Jacobian they give."""
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

    def step(self, pos_act, reset=None):
        """One launch: the joints move towards pos_act (N, nd), environments with reset set snap to it at rest; returns
        (rigid_body, dof_state, jacobian), updated in place."""
        self.art.step(self.dof_state, self.base_pose, targets=pos_act, reset=reset, vmax=self.max_velocity, dt=self.dt,
                      rigid_body=self.rigid_body, jacobian=self.jacobian, rb_row0=self.rb_row0, dof_row0=self.dof_row0)
        return self.rigid_body, self.dof_state, self.jacobian
