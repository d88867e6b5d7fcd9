"""The robot side of the task step, mirroring the reference's `tasks/load_robot.py:franka` without a simulator: the constants the
kernels need (DOF limits, default pose, tip body indices, the mesh-frame matrices of compute_scene_pose) and the action count of
each drive mode.  The arithmetic of `control` / `solve_ik` / `update_state` lives in csrc/task_grasp_cube.hip.

A simulator supplies what the reference asks Isaac Gym for: pass `num_dofs`, `num_rigid_body`, the limits and the tip indices of
your asset; the defaults are the Franka Panda with two finger-tip bodies (13 bodies: link0-7, hand, left finger, left tip, right
finger, right tip)."""
import torch

# joint limits of the Franka Emika Panda (manufacturer's data sheet, rad) and of its two finger slides (m)
PANDA_DOF_LOWER = (-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, 0.0, 0.0)
PANDA_DOF_UPPER = (2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04)
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


class Franka:
    def __init__(self, robot_cfg, dt, num_envs, device, num_dofs=9, num_rigid_body=13, dof_lower=None, dof_upper=None,
                 ltip_rb_index=10, rtip_rb_index=12):
        self.device, self.num_envs, self.dt = device, num_envs, float(dt)
        self.driveMode = robot_cfg.get("driveMode", "ik")
        if self.driveMode in LEFT_OUT_DRIVE_MODES:
            raise NotImplementedError(f"drive mode {self.driveMode!r} is not built (left out: {LEFT_OUT_DRIVE_MODES} and mobile "
                                      f"bases); available: {SUPPORTED_DRIVE_MODES}")
        if self.driveMode not in SUPPORTED_DRIVE_MODES:
            raise NotImplementedError(f"unknown drive mode {self.driveMode!r}; available: {SUPPORTED_DRIVE_MODES}")
        if robot_cfg.get("mobile", False) or "mobile" in str(robot_cfg.get("assetFile", "")):
            raise NotImplementedError("mobile bases are not built (left out together with the drive modes "
                                      f"{LEFT_OUT_DRIVE_MODES})")
        self.mobile = False
        self.num_dofs, self.num_rigid_body = int(num_dofs), int(num_rigid_body)
        if self.num_dofs < 3:
            raise ValueError(f"num_dofs must be at least 3 (an arm and two fingers), got {num_dofs}")
        self.num_actions = 7 if self.driveMode == "ik" else self.num_dofs - 1           # load_robot.py:15-18 ('pos': 8 at 9 DOFs)
        self.ltip_rb_index, self.rtip_rb_index = int(ltip_rb_index), int(rtip_rb_index)
        if dof_lower is None and dof_upper is None and self.num_dofs == 9:
            dof_lower, dof_upper = PANDA_DOF_LOWER, PANDA_DOF_UPPER
        if dof_lower is None or dof_upper is None:
            raise ValueError(f"dof_lower / dof_upper are needed for a robot of {self.num_dofs} DOFs")
        self.dof_lower_limits_tensor = torch.as_tensor(dof_lower, dtype=torch.float32).reshape(-1).to(device).contiguous()
        self.dof_upper_limits_tensor = torch.as_tensor(dof_upper, dtype=torch.float32).reshape(-1).to(device).contiguous()
        if self.dof_lower_limits_tensor.numel() != self.num_dofs or self.dof_upper_limits_tensor.numel() != self.num_dofs:
            raise ValueError(f"dof limits: expected {self.num_dofs} entries each")
        dof = robot_cfg.get("dof")
        if dof is None:                                       # mid-range arm, open gripper
            mid = (self.dof_lower_limits_tensor + self.dof_upper_limits_tensor) / 2
            mid[-2:] = self.dof_upper_limits_tensor[-2:]
            self.default_dof_pos = mid.contiguous()
        else:
            self.default_dof_pos = torch.as_tensor(dof, dtype=torch.float32).reshape(-1).to(device).contiguous()
        if self.default_dof_pos.numel() != self.num_dofs:
            raise ValueError(f"robot.dof: expected {self.num_dofs} entries, got {self.default_dof_pos.numel()}")
        root = robot_cfg.get("root")
        self.default_root = None if root is None else torch.as_tensor(root, dtype=torch.float32).to(device)
        self.coordinate_transform_matrix = coordinate_transform_matrix(device)
