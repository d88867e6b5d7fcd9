"""The tensor program of the reference's open_drawer task (tasks/open_drawer.py compute_observations / compute_reward / reset_idx,
tasks/hand_base.py:363-392) around any simulator whose environments differ: flat state tensors and two index tables in, observation
rows, reward, reset flags, part poses, joint targets and the reset rows of the state tensors out.

    task = OpenDrawerTensors(num_envs, device, cfg, dt, rigid_body_mask, dof_state_mask, obj_id, part_bbox_init,
                             part_axis_dir_init, part_joint_lower_limits, part_joint_upper_limits, num_objs)
    pos_act_all, reset = task.begin_step(actions, jacobian, dof_state_all, root, pos_act_all)   # two launches; then: your step
    obs, rew, reset, extras = task.end_step(rigid_body_all, dof_state_all, root)                # one launch (+ progress_buf += 1)
    rot, pos = task.compute_scene_pose()                                  # -> TSDFfromMesh.query_tsdf / PCfromMesh.query_pc

What stays with the caller is what the reference does through Isaac Gym: stepping the simulator, handing `pos_act_all` to its
position drive and pushing the rewritten rows of `dof_state_all` / `root` into it with its indexed setters.  The index lists those
setters want (`global_indices[env_ids]`) are built by the caller from `reset_buf`: that is a host read or a nonzero(), which this
class never does.

The shipped cfg/tasks/open_drawer.yaml asks for the mobile Franka (three virtual base joints, 12 DOFs, 17 bodies).  A config file
cannot say how many bodies the asset has or where its tips are, so that robot comes in through `robot=`:

    task = OpenDrawerTensors(num_envs, device, cfg, dt, ..., robot=MobileFranka(cfg["robot"], dt, num_envs, device))

Left out: building a mobile base from the cfg alone (the cfg-only constructor raises NotImplementedError naming "mobile", from Franka;
pass robot=MobileFranka(...)), the drive modes 'ik_abs' (the reference's own code raises a shape error for more than one environment)
and 'heuristic' (a debugging mode that ends the process): NotImplementedError naming them; the reference's random STREAM (see
begin_step) and extras['step_id'] (it is `progress_buf.float()`)."""
import json
import math
import os

import numpy as np
import torch

from .. import ops
from ..urdf import FIXED, load_urdf
from .base import TaskTensors, franka_parts

EXTRAS_COLUMNS = ("is_open", "is_open_notgrasp", "reaching_reward", "close_reward", "rot_reward", "joint_state_reward", "raw_reward",
                  "is_grasped")
OBJ_DEFAULT_ROOT = (-0.6, 0.0, 0.5, 0.0, 0.0, 1.0, 0.0)        # open_drawer.py:44
RESET_T_RANGE, RESET_R_RANGE = 0.05, math.pi / 12             # open_drawer.py:46-47
SUC_PROP = 0.5                                                # open_drawer.py:84


def default_part_slot(num_rigid_body):
    """The 11 robot parts GraspCubeTensors poses (bodies 0-9 and the right finger), then the target link and the handle, as slots of
    an environment's gathered rows."""
    if num_rigid_body < 12:
        raise ValueError(f"the default part list needs at least 12 robot bodies, got {num_rigid_body}")
    return franka_parts(num_rigid_body - 2) + [num_rigid_body, num_rigid_body + 1]


def build_masks(num_robot_bodies, num_robot_dofs, obj_bodies, obj_dofs, target_link, target_handle, target_dof):
    """The index tables as open_drawer.py:58-70 builds them, for environments laid out one after the other (robot first): obj_bodies /
    obj_dofs (N) are each cabinet's body and DOF counts, target_link / target_handle / target_dof (N) index into the cabinet.
    Returns (rigid_body_mask (N, nrb + 2), dof_state_mask (N, nd + 1)) int32 numpy and the totals (B, D)."""
    N = len(obj_bodies)
    rb = np.zeros((N, num_robot_bodies + 2), dtype=np.int32)
    dm = np.zeros((N, num_robot_dofs + 1), dtype=np.int32)
    rigid_count = dof_count = 0
    for i in range(N):
        dm[i, :num_robot_dofs] = np.arange(dof_count, dof_count + num_robot_dofs)
        dm[i, -1] = dof_count + num_robot_dofs + int(target_dof[i])
        rb[i, :num_robot_bodies] = np.arange(rigid_count, rigid_count + num_robot_bodies)
        rb[i, -2] = rigid_count + num_robot_bodies + int(target_link[i])
        rb[i, -1] = rigid_count + num_robot_bodies + int(target_handle[i])
        dof_count += num_robot_dofs + int(obj_dofs[i])
        rigid_count += num_robot_bodies + int(obj_bodies[i])
    return rb, dm, rigid_count, dof_count


class DrawerEnvs:
    """DrawerAssets.for_envs(N): every per-environment array that build_masks, OpenDrawerTensors and kinematics.KinematicSim take, as
    numpy: obj_id, obj_bodies, obj_dofs, target_link, target_handle, target_dof (N) int32; part_bbox_init (N, 8, 3), part_axis_dir_init
    (N, 3), part_joint_lower_limits, part_joint_upper_limits (N) float32; num_objs."""

    def __init__(self, assets, N):
        oid = (np.arange(int(N)) % assets.num_objs).astype(np.int32)          # open_drawer.py:145
        self.num_envs, self.num_objs, self.obj_id = int(N), assets.num_objs, oid
        pick = lambda a, dt: np.ascontiguousarray(np.asarray(a)[oid], dtype=dt)      # noqa: E731
        self.obj_bodies, self.obj_dofs = pick(assets.num_bodies, np.int32), pick(assets.num_dofs, np.int32)
        self.target_link, self.target_handle = pick(assets.target_link, np.int32), pick(assets.target_handle, np.int32)
        self.target_dof = pick(assets.target_dof, np.int32)
        self.part_bbox_init, self.part_axis_dir_init = pick(assets.part_bbox_init, np.float32), pick(assets.part_axis_dir_init, np.float32)
        self.part_joint_lower_limits = pick(assets.part_joint_lower_limits, np.float32)
        self.part_joint_upper_limits = pick(assets.part_joint_upper_limits, np.float32)

    def masks(self, num_robot_bodies, num_robot_dofs):
        """build_masks for these environments: (rigid_body_mask, dof_state_mask, B, D)."""
        return build_masks(num_robot_bodies, num_robot_dofs, self.obj_bodies, self.obj_dofs, self.target_link, self.target_handle,
                           self.target_dof)

    def task_kwargs(self):
        """The per-object keyword arguments of OpenDrawerTensors."""
        return dict(obj_id=self.obj_id, part_bbox_init=self.part_bbox_init, part_axis_dir_init=self.part_axis_dir_init,
                    part_joint_lower_limits=self.part_joint_lower_limits, part_joint_upper_limits=self.part_joint_upper_limits,
                    num_objs=self.num_objs)


class DrawerAssets:
    """What load_drawer_assets read, per object k: trees[k] (urdf.KinematicTree at `scale`), names[k] = (asset, link, handle, joint),
    target_link[k] / target_handle[k] (body rows of the tree), target_dof[k] (DOF of the tree), part_bbox_init (K, 8, 3),
    part_axis_xyz_init, part_axis_dir_init (K, 3), part_joint_lower_limits, part_joint_upper_limits (K), num_bodies, num_dofs."""

    def __init__(self, folders, scale, trees, names, target_link, target_handle, target_dof, bbox, axis_xyz, axis_dir, lower, upper):
        self.folders, self.scale, self.trees, self.names, self.num_objs = list(folders), float(scale), list(trees), list(names), len(trees)
        self.target_link, self.target_handle, self.target_dof = (np.asarray(a, dtype=np.int32) for a in (target_link, target_handle, target_dof))
        self.part_bbox_init = np.asarray(bbox, dtype=np.float64).reshape(-1, 8, 3)
        self.part_axis_xyz_init = np.asarray(axis_xyz, dtype=np.float64).reshape(-1, 3)
        self.part_axis_dir_init = np.asarray(axis_dir, dtype=np.float64).reshape(-1, 3)
        self.part_joint_lower_limits, self.part_joint_upper_limits = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
        self.num_bodies = np.array([t.num_bodies for t in trees], dtype=np.int32)
        self.num_dofs = np.array([t.num_dofs for t in trees], dtype=np.int32)

    def for_envs(self, N):
        """Environment e holds object e % num_objs (open_drawer.py:145)."""
        return DrawerEnvs(self, N)


def load_drawer_assets(folders, scale=0.5):
    """The reference's object folders (open_drawer.py:98-140) -> DrawerAssets, on the host.  A folder's name parses as
    `...-asset-link-handle-joint-...` (`name.split('-')[-5:-1]`); it holds bbox_info.json (link_name, bbox_world, axis_xyz_world,
    axis_dir_world) and mobility_new.urdf, loaded at `scale` (urdf.load_urdf: the effect of the reference's set_actor_scale, 0.5).
    part_bbox_init = bbox_world[handle] * scale; the axes are those of the link; the limits are the reference's expressions: the
    file's upper limit of the target joint times scale, its lower limit as in the file.

    One difference from the reference, stated: it uses the json's link index as the BODY index too, trusting the simulator's body
    order to be the json's.  Here the bbox and axis arrays are indexed by the json's order, and the body rows (target_link,
    target_handle) by tree.body_index(name), i.e. this project's depth-first body order; nothing is claimed about Isaac Gym's.

    ValueError, naming it: a missing file, a folder name that does not parse, a link missing from the json or from the URDF, an
    unknown target joint, a target joint that is fixed."""
    folders = [os.fspath(f) for f in folders]
    if not folders:
        raise ValueError("load_drawer_assets: expected at least one folder")
    cols = {k: [] for k in ("trees", "names", "link", "handle", "dof", "bbox", "xyz", "dir", "lower", "upper")}
    for folder in folders:
        name = os.path.basename(os.path.normpath(folder))
        parts = name.split("-")[-5:-1]
        if len(parts) != 4:
            raise ValueError(f"{name!r}: the folder name does not parse as ...-asset-link-handle-joint-...")
        asset_id, link_name, handle_name, joint_name = parts
        info_path, urdf_path = os.path.join(folder, "bbox_info.json"), os.path.join(folder, "mobility_new.urdf")
        for path in (info_path, urdf_path):
            if not os.path.isfile(path):
                raise ValueError(f"{path}: missing file")
        with open(info_path, "rb") as f:
            info = json.load(f)
        for key in ("link_name", "bbox_world", "axis_xyz_world", "axis_dir_world"):
            if key not in info:
                raise ValueError(f"{info_path}: no {key!r}")
        for ln in (link_name, handle_name):
            if ln not in info["link_name"]:
                raise ValueError(f"{info_path}: unknown link {ln!r}; link_name: {info['link_name']}")
        link_id, handle_id = info["link_name"].index(link_name), info["link_name"].index(handle_name)
        tree, unscaled = load_urdf(urdf_path, scale=scale), load_urdf(urdf_path)
        for ln in (link_name, handle_name):
            if ln not in tree.names:
                raise ValueError(f"{urdf_path}: unknown link {ln!r}; links: {tree.names}")
        if joint_name not in tree.joint_names:
            raise ValueError(f"{urdf_path}: unknown joint {joint_name!r}; joints: {[j for j in tree.joint_names if j]}")
        jb = tree.joint_names.index(joint_name)
        if tree.jtype[jb] == FIXED:
            raise ValueError(f"{urdf_path}: the target joint {joint_name!r} is fixed")
        d = int(tree.dof[jb])
        cols["trees"].append(tree), cols["names"].append((asset_id, link_name, handle_name, joint_name))
        cols["link"].append(tree.body_index(link_name)), cols["handle"].append(tree.body_index(handle_name)), cols["dof"].append(d)
        cols["bbox"].append(np.asarray(info["bbox_world"][handle_id], dtype=np.float64).reshape(8, 3) * float(scale))
        cols["xyz"].append(info["axis_xyz_world"][link_id]), cols["dir"].append(info["axis_dir_world"][link_id])
        cols["lower"].append(float(unscaled.lower[d])), cols["upper"].append(float(unscaled.upper[d]) * float(scale))
    return DrawerAssets(folders, scale, cols["trees"], cols["names"], cols["link"], cols["handle"], cols["dof"], cols["bbox"], cols["xyz"],
                        cols["dir"], cols["lower"], cols["upper"])


def load_drawer_meshes(assets):
    """DrawerAssets -> one list per object of (vertices, faces)-or-None per body, in the tree's body order: the visual meshes of each
    folder's mobility_new.urdf at the assets' scale (urdf.load_urdf_visuals).  It is the `groups=` of mesh2depth.DepthFromMesh and
    the `scene_meshes=` of envs.make_open_drawer_env."""
    from ..urdf import load_urdf_visuals
    return [load_urdf_visuals(os.path.join(folder, "mobility_new.urdf"), scale=assets.scale) for folder in assets.folders]


def _host_ints(x, name, shape):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name}: expected an integer array, got {a.dtype}")
    if a.shape != tuple(shape):
        raise ValueError(f"{name}: expected {tuple(shape)}, got {a.shape}")
    return a.astype(np.int64)


class OpenDrawerTensors(TaskTensors):
    """cfg: the task's dictionary (robot.driveMode, robot.dof, robot.root, explore_step, maxEpisodeLength, random_reset).  Without
    `robot=` the robot is the fixed-base Franka with the 'ik' and 'pos' drives: a cfg that asks for a mobile base
    (cfg/tasks/open_drawer.yaml does) or for 'ik_abs' / 'heuristic' then raises NotImplementedError.  robot=MobileFranka(cfg["robot"],
    dt, num_envs, device) is the mobile Franka of that yaml (num_actions 10, normal_state 53 columns); a robot with num_base_dofs > 0
    is driven by pm_franka_control_mobile_f32 with its base_R.  robot.root defaults to the identity pose at the origin.

    rigid_body_mask (N, nrb + 2) and dof_state_mask (N, nd + 1): row indices into the simulator's flat rigid-body and DOF tensors
    (build_masks), checked here once on the host: every index >= 0 (and below num_rigid_bodies / num_dof_states when those totals
    are given; the tensors handed to begin_step / end_step must have at least max index + 1 rows either way), no index twice in
    dof_state_mask; ValueError otherwise.  obj_id (N) in [0, num_objs); part_bbox_init (N, 8, 3) already scaled;
    part_joint_upper_limits already multiplied by the object scale.  part_slot (M) / part_C (M, 3, 3) or None choose the posed
    parts among an environment's nrb + 2 gathered rows (default: default_part_slot, or the robot's mesh_bodies + [nrb, nrb + 1]
    where it names them, with the Franka's mesh-frame matrices, identity for the link and the handle)."""

    def __init__(self, num_envs, device, cfg, dt, rigid_body_mask, dof_state_mask, obj_id, part_bbox_init, part_axis_dir_init,
                 part_joint_lower_limits, part_joint_upper_limits, num_objs, num_rigid_bodies=None, num_dof_states=None,
                 num_actors=2, robot_actor=0, obj_actor=1, robot=None, part_slot=None, part_C="default",
                 obj_default_root=OBJ_DEFAULT_ROOT, suc_prop=SUC_PROP):
        super().__init__(num_envs, device, cfg, dt, robot)
        N = self.num_envs
        nd, nrb = self.robot.num_dofs, self.robot.num_rigid_body
        self.num_actors, self.robot_actor, self.obj_actor = int(num_actors), int(robot_actor), int(obj_actor)
        if not (0 <= self.robot_actor < self.num_actors and 0 <= self.obj_actor < self.num_actors) or self.robot_actor == self.obj_actor:
            raise ValueError(f"robot_actor {robot_actor} / obj_actor {obj_actor}: expected two different actors of {num_actors}")
        self.num_objs = int(num_objs)
        if self.num_objs < 1:
            raise ValueError(f"num_objs must be at least 1, got {num_objs}")
        rbm = _host_ints(rigid_body_mask, "rigid_body_mask", (N, nrb + 2))
        dfm = _host_ints(dof_state_mask, "dof_state_mask", (N, nd + 1))
        for a, name, total in ((rbm, "rigid_body_mask", num_rigid_bodies), (dfm, "dof_state_mask", num_dof_states)):
            hi = int(total) if total is not None else 2 ** 31 - 1
            if a.min() < 0 or a.max() >= hi:
                raise ValueError(f"{name}: indices must lie in [0, {hi}), got [{a.min()}, {a.max()}]")
        if np.unique(dfm).size != dfm.size:
            raise ValueError("dof_state_mask: an index appears twice (two environments would write one DOF row)")
        self.num_rigid_bodies = int(num_rigid_bodies) if num_rigid_bodies is not None else int(rbm.max()) + 1
        self.num_dof_states = int(num_dof_states) if num_dof_states is not None else int(dfm.max()) + 1
        oid = _host_ints(obj_id, "obj_id", (N,))
        if oid.min() < 0 or oid.max() >= self.num_objs:
            raise ValueError(f"obj_id: values must lie in [0, {self.num_objs}), got [{oid.min()}, {oid.max()}]")
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)   # noqa: E731
        self.rigid_body_mask, self.dof_state_mask, self.obj_id = i32(rbm), i32(dfm), i32(oid)
        f = dict(dtype=torch.float32, device=device)

        def const(x, name, shape):
            v = torch.as_tensor(x, dtype=torch.float32).to(device).contiguous()
            if tuple(v.shape) != shape:
                raise ValueError(f"{name}: expected {shape}, got {tuple(v.shape)}")
            return v

        self.part_bbox_init = const(part_bbox_init, "part_bbox_init", (N, 8, 3))
        self.part_axis_dir_init = const(part_axis_dir_init, "part_axis_dir_init", (N, 3))
        self.part_joint_lower_limits = const(part_joint_lower_limits, "part_joint_lower_limits", (N,))
        self.part_joint_upper_limits = const(part_joint_upper_limits, "part_joint_upper_limits", (N,))
        self.obj_default_root = const(obj_default_root, "obj_default_root", (7,))
        root = self.robot.default_root
        self.robot_default_root = const((0, 0, 0, 0, 0, 0, 1) if root is None else root.reshape(-1)[:7], "robot.root", (7,))
        self.num_obs = {"normal_state": 29 + 2 * nd}
        self.random_reset = bool(cfg.get("random_reset", False))
        self.reset_t_range, self.reset_r_range, self.suc_prop = RESET_T_RANGE, RESET_R_RANGE, float(suc_prop)
        self.part_slot, self.part_C = self._parts(part_slot, part_C, default_part_slot, nrb, [nrb, nrb + 1])
        self.obs_buf = {"normal_state": torch.zeros(N, self.num_obs["normal_state"], **f)}
        self._buffers(self.part_slot.numel(), EXTRAS_COLUMNS)
        self.succ_objid_lst = torch.zeros(self.num_objs, dtype=torch.bool, device=device)
        self.extras["success_objnum"] = self.succ_objid_lst
        self.robot_dof_state = torch.zeros(N, nd, 2, **f)
        self.part_dof_state = torch.zeros(N, 2, **f)
        self.part_bbox = torch.zeros(N, 8, 3, **f)

    def _check_state(self, rigid_body_all, dof_state_all, root, pos_act_all):
        if rigid_body_all is not None and (rigid_body_all.dim() != 2 or rigid_body_all.shape[0] < self.num_rigid_bodies):
            raise ValueError(f"rigid_body_all: expected (>= {self.num_rigid_bodies}, 13), got {tuple(rigid_body_all.shape)}")
        if dof_state_all.dim() != 2 or dof_state_all.shape[0] < self.num_dof_states:
            raise ValueError(f"dof_state_all: expected (>= {self.num_dof_states}, 2), got {tuple(dof_state_all.shape)}")
        if tuple(root.shape) != (self.num_envs, self.num_actors, 13):
            raise ValueError(f"root: expected {(self.num_envs, self.num_actors, 13)}, got {tuple(root.shape)}")
        if pos_act_all is not None and pos_act_all.numel() != dof_state_all.shape[0]:
            raise ValueError(f"pos_act_all: expected {dof_state_all.shape[0]} elements, got {pos_act_all.numel()}")

    def _reset_launch(self, flags, dof_state_all, root, pos_act_all, u):
        if self.random_reset and u is None:
            u = torch.rand(self.num_envs, 4, dtype=torch.float32, device=root.device)
        r = self.robot
        ops.open_drawer_reset(flags, self.pos_act, self.dof_state_mask, root, dof_state_all, pos_act_all, self.robot_actor,
                              self.obj_actor, self.robot_default_root, self.obj_default_root, r.default_dof_pos,
                              self.part_joint_lower_limits, u if self.random_reset else None, self.reset_t_range, self.reset_r_range,
                              robot_dof_state=self.robot_dof_state, part_dof_state=self.part_dof_state)

    def begin_step(self, actions, jacobian, dof_state_all, root, pos_act_all, u=None):
        """hand_base.pre_physics_step with open_drawer.reset_idx: joint targets from the actions and the robot DOF state of the last
        end_step (or reset), the episode bookkeeping, then in one more launch the scatter of the targets into pos_act_all (D) and, for
        the environments that start over, the default rows of root (N, na, 13) and dof_state_all (D, 2), in place.

        u (N, 4) in [0, 1) drives the perturbation when cfg['random_reset'] is set (row e: translation x, y, z and yaw of environment e);
        None draws it with torch.rand.  The random STREAM is therefore not the reference's, whose number of draws depends on how many
        environments reset (a host read here); the distribution is the same.  Returns (pos_act_all, reset_buf)."""
        self._train()                                         # a bad flag is refused before a bad argument
        self._check_state(None, dof_state_all, root, pos_act_all)
        self._control(actions, self.robot_dof_state, jacobian)
        self._reset_launch(self.reset_buf, dof_state_all, root, pos_act_all, u)
        return pos_act_all, self.reset_buf

    def reset(self, dof_state_all, root, pos_act_all, u=None):
        """hand_base.reset's reset_idx(ones): every environment's buffers and state rows start over (the same launch as in begin_step
        with every flag set).  The caller then pushes the state into its simulator, steps it once and calls end_step."""
        self._check_state(None, dof_state_all, root, pos_act_all)
        self.pos_act.copy_(self.robot.default_dof_pos.expand_as(self.pos_act))
        self.progress_buf.zero_()
        self.success.zero_()
        self.epis_max_rew.fill_(-100.0)
        self.epis_max_step.zero_()
        self._reset_launch(torch.ones(self.num_envs, dtype=torch.bool, device=root.device), dof_state_all, root, pos_act_all, u)
        return pos_act_all

    def end_step(self, rigid_body_all, dof_state_all, root):
        """hand_base.post_physics_step: progress_buf += 1, then the gather, observation rows, reward, flags, the per-object success
        flags and part poses in one launch.  rigid_body_all (B, 13), dof_state_all (D, 2), root (N, na, 13)."""
        self._check_state(rigid_body_all, dof_state_all, root, None)
        self.progress_buf += 1
        r = self.robot
        ops.open_drawer_post(rigid_body_all, dof_state_all, root, self.rigid_body_mask, self.dof_state_mask, self.obj_actor,
                             r.ltip_rb_index, r.rtip_rb_index, self.part_bbox_init, self.part_axis_dir_init,
                             self.part_joint_lower_limits, self.part_joint_upper_limits, r.dof_lower_limits_tensor,
                             r.dof_upper_limits_tensor, self.suc_prop, obj_id=self.obj_id, part_slot=self.part_slot, part_C=self.part_C,
                             normal_state=self.obs_buf["normal_state"], rew=self.rew_buf, success=self.success,
                             is_reached=self.is_reached, part_bbox=self.part_bbox, extras=self._extras,
                             succ_objid=self.succ_objid_lst, robot_dof_state=self.robot_dof_state,
                             part_dof_state=self.part_dof_state, pose_R=self.pose_R, pose_T=self.pose_T)
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras
