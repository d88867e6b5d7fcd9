"""What the reference's tasks/hand_base.py gives every task, without a simulator: the robot, the episode buffers, the posed-part list,
the step before physics (hand_base.pre_physics_step: joint targets and episode bookkeeping, ops.franka_control) and
compute_scene_pose.  GraspCubeTensors and OpenDrawerTensors add their own state, observation and reward on top."""
import torch

from .. import ops
from .franka import Franka


def franka_parts(finger):
    """hand_base.py:433-435: the robot parts the reference poses, its first ten bodies and one finger body."""
    return list(range(10)) + [finger]


class TaskTensors:
    def __init__(self, num_envs, device, cfg, dt, robot=None):
        self.num_envs, self.device, self.dt = int(num_envs), device, float(dt)
        self.robot = robot if robot is not None else Franka(cfg.get("robot", {}), dt, num_envs, device)
        self.num_actions = self.robot.num_actions
        self.max_episode_length = int(cfg.get("maxEpisodeLength", 200))
        self.explore_step = int(cfg.get("explore_step", 40))
        self.train_test_flag = "train"
        # a caller's own robot object need not know about base joints or mesh bodies: it is then a fixed-base Franka
        nbase = getattr(self.robot, "num_base_dofs", 0)
        self._base = dict(num_base_dofs=nbase, base_R=self.robot.base_R) if nbase else {}
        self._mesh_bodies = getattr(self.robot, "mesh_bodies", None)

    def _parts(self, part, part_C, default, n, extra):
        """The posed parts as ((M) int32, (M, 3, 3) float32 or None).  part None: the robot's mesh bodies and then the slots `extra`,
        or the task's default(n) (franka_parts and the same slots) where the robot names none; part_C "default" is then the Franka's
        mesh-frame matrices with the identity for `extra`, and None for a caller's own list."""
        f = dict(dtype=torch.float32, device=self.device)
        if part is None:
            part = default(n) if self._mesh_bodies is None else list(self._mesh_bodies) + list(extra)
            if isinstance(part_C, str):
                part_C = torch.cat([self.robot.coordinate_transform_matrix.to(self.device), torch.eye(3, **f).expand(len(extra), 3, 3)])
        elif isinstance(part_C, str):
            part_C = None
        part = torch.as_tensor(part, dtype=torch.int32).reshape(-1).to(self.device).contiguous()
        return part, None if part_C is None else torch.as_tensor(part_C, dtype=torch.float32).to(self.device).contiguous()

    def _buffers(self, num_parts, extras_columns):
        """Reward, flags, episode counters, joint targets, part poses and the extras (one (N, columns) buffer and its column views)."""
        N, device = self.num_envs, self.device
        f = dict(dtype=torch.float32, device=device)
        b = dict(dtype=torch.bool, device=device)
        self.rew_buf = torch.zeros(N, **f)
        self.success, self.is_reached = torch.zeros(N, **b), torch.zeros(N, **b)
        self.reset_buf, self.reset_succ = torch.zeros(N, **b), torch.zeros(N, **b)
        self.progress_buf = torch.zeros(N, dtype=torch.long, device=device)
        self.epis_max_rew = torch.full((N,), -100.0, **f)
        self.epis_max_step = torch.zeros(N, dtype=torch.long, device=device)
        self.pos_act = torch.zeros(N, self.robot.num_dofs, **f)
        self.pose_R = torch.zeros(N, num_parts, 3, 3, **f)
        self.pose_T = torch.zeros(N, num_parts, 3, **f)
        self._extras = torch.zeros(N, len(extras_columns), **f)
        self.extras = {k: self._extras[:, i] for i, k in enumerate(extras_columns)}
        self.extras["is_reached"] = self.is_reached
        self._counters = torch.zeros(4, dtype=torch.int32, device=device)
        self._slot = 1

    def _train(self):
        """True in 'train', False in 'test'; begin_step refuses any other train_test_flag before it looks at its arguments."""
        if self.train_test_flag not in ("train", "test"):
            raise NotImplementedError(f"train_test_flag {self.train_test_flag!r}")
        return self.train_test_flag == "train"

    def _control(self, actions, dof_state, jacobian):
        """hand_base.pre_physics_step up to the simulator calls: joint targets into pos_act, the episode bookkeeping on the reward
        and success of the last end_step, the buffer resets of the environments that start over, extras['succ_rate']."""
        train = self._train()
        self._slot ^= 1
        r = self.robot
        ops.franka_control(actions, dof_state, jacobian, r.ltip_rb_index - 1, r.rtip_rb_index - 1, r.dof_lower_limits_tensor,
                           r.dof_upper_limits_tensor, r.default_dof_pos, self.dt, r.driveMode, self.rew_buf, self.success,
                           self.progress_buf, self.explore_step, self.max_episode_length, train, self.pos_act, self.epis_max_rew,
                           self.epis_max_step, self.reset_buf, self.reset_succ, self._counters, self._slot, **self._base)
        if train:                                             # hand_base.py:373
            c = self._counters[2 * self._slot:2 * self._slot + 2]
            self.extras["succ_rate"] = c[0:1] / torch.clamp(c[1], min=1)

    def compute_scene_pose(self):
        """(rot (N, M, 3, 3), pos (N, M, 3)) of the last end_step: hand_base.py:431-441, the input of query_tsdf / query_pc."""
        return self.pose_R, self.pose_T
