"""The robot side of the task step, mirroring the reference's `tasks/load_robot.py:franka` without a simulator: the constants the
kernels need (DOF limits, default pose, tip body indices, the mesh-frame matrices of compute_scene_pose) and the action count of
each drive mode.  The arithmetic of `control` / `solve_ik` / `update_state` lives in csrc/task_grasp_cube.hip.

A simulator supplies what the reference asks Isaac Gym for: pass `num_dofs`, `num_rigid_body`, the limits and the tip indices of
your asset; the defaults are the Franka Panda with two finger-tip bodies (13 bodies: link0-7, hand, left finger, left tip, right
finger, right tip).  `MobileFranka` is the robot of the reference's cfg/tasks/open_drawer.yaml: three virtual prismatic base joints in
front of the same arm (12 DOFs, 17 bodies)."""
import torch

# joint limits of the Franka Emika Panda (manufacturer's data sheet, rad) and of its two finger slides (m)
PANDA_DOF_LOWER = (-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, 0.0, 0.0)
PANDA_DOF_UPPER = (2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04)
# travel of the mobile asset's three virtual base slides (x, y, z; m)
MOBILE_BASE_LOWER = (-0.2, -0.2, -0.1)
MOBILE_BASE_UPPER = (0.2, 0.2, 0.1)
# the 11 bodies of the mobile asset that carry a mesh (link0-7, hand, left finger, right finger) in its depth-first body order
MOBILE_MESH_BODIES = (3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15)
SUPPORTED_DRIVE_MODES = ("ik", "pos")
LEFT_OUT_DRIVE_MODES = ("ik_abs", "heuristic")


def coordinate_transform_matrix(device=None):
    """load_robot.py:52-56: the matrices that take the 11 robot meshes' frames to their bodies' frames, (11, 3, 3)."""
    c = torch.zeros(11, 3, 3)
    c[:, 0, 0] = 1
    c[:, 1, 2] = -1
    c[:, 2, 1] = 1
    c[-1, 1, 2] = 1
    return c.to(device) if device is not None else c


def quat_to_mat(q):
    """utils/torch_jit_utils.quat_to_mat: q (..., 4) in the order (i, j, k, r), two_s = 2 / sum q^2, no normalisation -> (..., 3, 3),
    in q's dtype."""
    i, j, k, r = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


class Franka:
    """The fixed-base Franka.  num_base_dofs, mesh_bodies and base_R say what MobileFranka adds: no base joints, no list of mesh
    bodies (the tasks then pose the reference's own twelve parts), no base matrix."""
    mobile, num_base_dofs, mesh_bodies, base_R = False, 0, None, None
    _min_dofs = (3, "an arm and two fingers")
    _left_out = f"{LEFT_OUT_DRIVE_MODES} and mobile bases"
    _default_limits = (9, PANDA_DOF_LOWER, PANDA_DOF_UPPER)

    def __init__(self, robot_cfg, dt, num_envs, device, num_dofs=9, num_rigid_body=13, dof_lower=None, dof_upper=None,
                 ltip_rb_index=10, rtip_rb_index=12):
        self.device, self.num_envs, self.dt = device, num_envs, float(dt)
        self.driveMode = robot_cfg.get("driveMode", "ik")
        if self.driveMode in LEFT_OUT_DRIVE_MODES:
            raise NotImplementedError(f"drive mode {self.driveMode!r} is not built (left out: {self._left_out}); available: "
                                      f"{SUPPORTED_DRIVE_MODES}")
        if self.driveMode not in SUPPORTED_DRIVE_MODES:
            raise NotImplementedError(f"unknown drive mode {self.driveMode!r}; available: {SUPPORTED_DRIVE_MODES}")
        self._check_cfg(robot_cfg)
        self.num_dofs, self.num_rigid_body = int(num_dofs), int(num_rigid_body)
        if self.num_dofs < self._min_dofs[0]:
            raise ValueError(f"num_dofs must be at least {self._min_dofs[0]} ({self._min_dofs[1]}), got {num_dofs}")
        # load_robot.py:15-26 ('pos': 8 at 9 DOFs, 11 at the mobile robot's 12)
        self.num_actions = 7 + self.num_base_dofs if self.driveMode == "ik" else self.num_dofs - 1
        self.ltip_rb_index, self.rtip_rb_index = int(ltip_rb_index), int(rtip_rb_index)
        self._check_indices()
        if dof_lower is None and dof_upper is None and self.num_dofs == self._default_limits[0]:
            dof_lower, dof_upper = self._default_limits[1:]
        if dof_lower is None or dof_upper is None:
            raise ValueError(f"dof_lower / dof_upper are needed for a robot of {self.num_dofs} DOFs")
        self.dof_lower_limits_tensor = torch.as_tensor(dof_lower, dtype=torch.float32).reshape(-1).to(device).contiguous()
        self.dof_upper_limits_tensor = torch.as_tensor(dof_upper, dtype=torch.float32).reshape(-1).to(device).contiguous()
        if self.dof_lower_limits_tensor.numel() != self.num_dofs or self.dof_upper_limits_tensor.numel() != self.num_dofs:
            raise ValueError(f"dof limits: expected {self.num_dofs} entries each")
        dof = robot_cfg.get("dof")
        if dof is None:                                       # base at its origin, mid-range arm, open gripper
            mid = (self.dof_lower_limits_tensor + self.dof_upper_limits_tensor) / 2
            mid[:self.num_base_dofs] = 0
            mid[-2:] = self.dof_upper_limits_tensor[-2:]
            self.default_dof_pos = mid.contiguous()
        else:
            self.default_dof_pos = torch.as_tensor(dof, dtype=torch.float32).reshape(-1).to(device).contiguous()
        if self.default_dof_pos.numel() != self.num_dofs:
            raise ValueError(f"robot.dof: expected {self.num_dofs} entries, got {self.default_dof_pos.numel()}")
        self._set_root(robot_cfg.get("root"))
        self.coordinate_transform_matrix = coordinate_transform_matrix(device)

    def _check_cfg(self, robot_cfg):
        if robot_cfg.get("mobile", False) or "mobile" in str(robot_cfg.get("assetFile", "")):
            raise NotImplementedError("mobile bases are not built (left out together with the drive modes "
                                      f"{LEFT_OUT_DRIVE_MODES})")

    def _check_indices(self):
        pass                                                  # a simulator's own tip indices are taken as they come

    def _set_root(self, root):
        self.default_root = None if root is None else torch.as_tensor(root, dtype=torch.float32).to(self.device)


class MobileFranka(Franka):
    """The mobile Franka of the reference's shipped open_drawer task (load_robot.py with `mobile`): num_base_dofs = 3 virtual prismatic
    joints in front of the arm, so 12 DOFs, 17 bodies and an action row of [base 3 | arm | gripper].  It carries Franka's attributes
    plus mobile = True, num_base_dofs, mesh_bodies and base_R, the (3, 3) float32 matrix of the default root quaternion that
    pm_franka_control_mobile_f32 turns the base action by.  The task classes take it through their `robot=` argument; robot_cfg may or
    may not say `mobile: True` or name a mobile assetFile.

    The default body layout (17 bodies, tips 14 / 16, mesh_bodies) is the depth-first order of the reference's mobile asset: base0-2,
    link0-7, link8, hand, leftfinger, lefttip, rightfinger, righttip.  Nobody has checked this order against Isaac Gym: a simulator's
    own counts and indices override all of them."""
    mobile, num_base_dofs = True, 3
    _min_dofs = (6, "three base joints, an arm and two fingers")
    _left_out = f"{LEFT_OUT_DRIVE_MODES}"
    _default_limits = (12, MOBILE_BASE_LOWER + PANDA_DOF_LOWER, MOBILE_BASE_UPPER + PANDA_DOF_UPPER)

    def __init__(self, robot_cfg, dt, num_envs, device, num_dofs=12, num_rigid_body=17, dof_lower=None, dof_upper=None,
                 ltip_rb_index=14, rtip_rb_index=16, mesh_bodies=None):
        self.mesh_bodies = MOBILE_MESH_BODIES if mesh_bodies is None else mesh_bodies
        super().__init__(robot_cfg, dt, num_envs, device, num_dofs, num_rigid_body, dof_lower, dof_upper, ltip_rb_index, rtip_rb_index)

    def _check_cfg(self, robot_cfg):
        pass                                                  # `mobile: True` and a mobile assetFile name this very robot

    def _check_indices(self):
        self.mesh_bodies = tuple(int(b) for b in self.mesh_bodies)
        for name, idx in (("ltip_rb_index", (self.ltip_rb_index,)), ("rtip_rb_index", (self.rtip_rb_index,)),
                          ("mesh_bodies", self.mesh_bodies)):
            if any(not 0 <= b < self.num_rigid_body for b in idx):
                raise ValueError(f"{name}: expected indices in [0, {self.num_rigid_body}), got {idx}")

    def _set_root(self, root):
        root = torch.as_tensor((0, 0, 0, 0, 0, 0, 1) if root is None else root, dtype=torch.float32).reshape(-1)
        if root.numel() < 7:
            raise ValueError(f"robot.root: expected at least 7 entries (position, quaternion), got {root.numel()}")
        self.default_root = root.to(self.device)
        self.base_R = quat_to_mat(root[3:7]).to(self.device).contiguous()     # load_robot.py:99, once, in float32
