"""The tensor program of the reference's grasp_cube task (tasks/grasp_cube.py, tasks/hand_base.py:363-392, 431-441) without a
simulator: raw state tensors in, observation rows, reward, reset flags, part poses and joint targets out.

    task = GraspCubeTensors(num_envs, device, cfg, dt)
    pos_act, reset = task.begin_step(actions, dof_state, jacobian)        # one launch; then: your simulator's step
    obs, rew, reset, extras = task.end_step(rigid_body, dof_state, root)  # one launch (+ the progress counter's increment)
    rot, pos = task.compute_scene_pose()                                  # -> TSDFfromMesh.query_tsdf / PCfromMesh.query_pc

What stays with the caller is what the reference does through Isaac Gym: stepping the simulator, writing DOF / root states of the
environments in `reset_buf` back into it (grasp_cube.reset_idx:152-182) and handing `pos_act` to its position drive.  The buffer
part of reset_idx (pos_act, progress_buf, success, epis_max_rew, epis_max_step) happens inside begin_step.

The mobile Franka comes in through `robot=MobileFranka(robot_cfg, dt, num_envs, device)` with `num_bodies=18` (its 17 bodies + the
cube); it is driven by pm_franka_control_mobile_f32 and its posed parts are its mesh_bodies + the cube.

Left out: building a mobile base from the cfg alone (NotImplementedError naming "mobile", from Franka: a config cannot say how many
bodies the asset has; pass robot=MobileFranka(...)), the drive modes 'ik_abs' (the reference's own code raises a shape error for more
than one environment) and 'heuristic' (a debugging mode that ends the process): NotImplementedError naming them; the reference's
"Jacobian has problem" exit (a host synchronisation) and extras['step_id'] (it is `progress_buf.float()`)."""
import torch

from .. import ops
from .base import TaskTensors, franka_parts

EXTRAS_COLUMNS = ("reaching_reward", "close_reward", "rot_reward", "reaching_goal_reward", "obj_movement", "raw_reward",
                  "obj_height", "obj_up_flag")
RESET_RANGE = 0.15                                            # grasp_cube.py:17-21


def default_part_body(num_bodies):
    """hand_base.py:433-435: rigid_body[:, :12] with the last two entries taken from [-3] and [-1]."""
    if num_bodies < 12:
        raise ValueError(f"the default part list needs at least 12 bodies, got {num_bodies}")
    return franka_parts(num_bodies - 3) + [num_bodies - 1]


class GraspCubeTensors(TaskTensors):
    """cfg: the task's dictionary (cfg/tasks/grasp_cube.yaml: robot.driveMode, explore_step, maxEpisodeLength, optionally robot.dof).
    num_bodies / num_actors / obj_actor describe the simulator's tensors (defaults: the Franka's 13 bodies + the cube, actors
    0 = robot, 1 = object); part_body (M) and part_C (M, 3, 3) or None choose the posed parts (defaults: the reference's 12; with a
    robot that names its mesh_bodies, those + the last body)."""

    def __init__(self, num_envs, device, cfg, dt, num_bodies=14, num_actors=2, obj_actor=1, robot=None, part_body=None,
                 part_C="default", goal=(0.0, 0.0, 0.2), goal_thresh=0.025, obj_default_pos=(0.0, 0.0, 0.025)):
        super().__init__(num_envs, device, cfg, dt, robot)
        nd = self.robot.num_dofs
        self.num_bodies, self.num_actors, self.obj_actor = int(num_bodies), int(num_actors), int(obj_actor)
        self.num_obs = {"normal_state": 19 + 2 * nd, "proprio_state": 7 + 2 * nd}
        self.goal_thresh = float(goal_thresh)
        f = dict(dtype=torch.float32, device=device)
        self.pose_lower_limit = torch.tensor([-RESET_RANGE, -RESET_RANGE, 0.0, -1, -1, -1, -1], **f)
        self.pose_upper_limit = torch.tensor([RESET_RANGE, RESET_RANGE, 0.4, 1, 1, 1, 1], **f)
        self.success_pos = torch.tensor(goal, **f)
        self.obj_default_pos = torch.tensor(obj_default_pos, **f)
        self.part_body, self.part_C = self._parts(part_body, part_C, default_part_body, self.num_bodies, [self.num_bodies - 1])
        self.obs_buf = {k: torch.zeros(self.num_envs, w, **f) for k, w in self.num_obs.items()}
        self._buffers(self.part_body.numel(), EXTRAS_COLUMNS)

    def begin_step(self, actions, dof_state, jacobian=None):
        """hand_base.pre_physics_step: joint targets from the actions, the episode bookkeeping on the reward and success of the last
        end_step, and the buffer resets of the environments that start over.  Returns (pos_act, reset_buf)."""
        self._control(actions, dof_state, jacobian)
        return self.pos_act, self.reset_buf

    def reset(self):
        """The buffer half of hand_base.reset's reset_idx(ones): every environment's targets, counters and flags start over.  The
        caller then puts the robot at pos_act and the cube at its default pose (KinematicSim.reset_free_body) and calls end_step.
        Returns pos_act."""
        self.pos_act.copy_(self.robot.default_dof_pos.expand_as(self.pos_act))
        self.progress_buf.zero_()
        self.success.zero_()
        self.epis_max_rew.fill_(-100.0)
        self.epis_max_step.zero_()
        return self.pos_act

    def end_step(self, rigid_body, dof_state, root, obs_out=None):
        """hand_base.post_physics_step: progress_buf += 1, then observation rows, reward, flags and part poses in one launch.
        obs_out: a 2-D float32 buffer (N, D) whose last 7 + 2 nd columns receive the proprio row (its head is for query_pc /
        query_tsdf with out=obs_out[:, :D - 25]); obs_buf['proprio_state'] is then that view."""
        self.progress_buf += 1
        Wp = self.num_obs["proprio_state"]
        if obs_out is not None:
            if obs_out.dim() != 2 or obs_out.shape[0] != self.num_envs or obs_out.shape[1] < Wp:
                raise ValueError(f"obs_out: expected ({self.num_envs}, >= {Wp}), got {tuple(obs_out.shape)}")
            self.obs_buf["proprio_state"] = obs_out[:, obs_out.shape[1] - Wp:]
        r = self.robot
        ops.grasp_cube_post(rigid_body, dof_state, root, self.obj_actor, r.ltip_rb_index, r.rtip_rb_index,
                            r.dof_lower_limits_tensor, r.dof_upper_limits_tensor, self.pose_lower_limit, self.pose_upper_limit,
                            self.success_pos, self.goal_thresh, self.obj_default_pos, self.part_body, self.part_C,
                            normal_state=self.obs_buf["normal_state"], proprio=self.obs_buf["proprio_state"], rew=self.rew_buf,
                            success=self.success, is_reached=self.is_reached, extras=self._extras, pose_R=self.pose_R,
                            pose_T=self.pose_T)
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras
