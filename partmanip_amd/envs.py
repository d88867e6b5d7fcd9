"""A vec-env over a task object and the kinematic stand-in: the duck type the runners consume (feeder.py's docstring: `reset() ->
{mode: (N, D)}`, `step(a) -> (obs, rew, reset, extras)` and the attributes num_envs / num_obs / num_actions / max_episode_length /
reset_succ / rew_buf / success / progress_buf / train_test_flag / dagger_reward_reset), so that `ppo` / `dagger` can `run()` on the
simulator-free loop of INTEGRATION.md instead of on noise.

    env = make_grasp_cube_env(cfg_task, num_envs, device, "franka_panda_sdf.urdf", dt, base_pose=..., observers={"mesh_pc": pc_observer(pc)})
    obs = env.reset()
    obs, rew, reset, extras = env.step(actions)               # begin_step, sim.step, end_step, the observers; no host synchronisation

Not physics (kinematics.py says what the stand-in is).  What closes the grasp_cube loop is the free body's carry rule
(csrc/free_body.hip) under the GRASP PREDICATE, a stated choice like `near = 0.01` elsewhere and not a contact:
hold = is_reached & (|p_l - p_r| <= grasp_width), from the last end_step, grasp_width = 0.055 (the 0.05 cube plus 0.005).  For
open_drawer the predicate is the task's own extras['is_grasped'] > 0 and the rule is the hold rule of kinematics.py.
KinematicEnv(contact=ContactSensor) senses, on every observation, how far the hand and the fingers are from the cube's or the
cabinet's baked grids (contact.py; extras['contact_dist'] / ['in_contact'] / ['penetration']) and grasp='contact' latches the cube on
finger contact instead of on the gap; it reports and resolves nothing.

A returned observation stays valid until the second step after it (two sets of rows, used in turn): the runners store the previous
observation after they have stepped."""
import numpy as np
import torch

from . import ops
from .kinematics import KinematicSim, ObjectLibrary
from .png import write_png
from .tasks import Franka, GraspCubeTensors, MobileFranka, OpenDrawerTensors
from .urdf import load_urdf

FORWARDED = ("num_envs", "num_actions", "max_episode_length", "reset_succ", "rew_buf", "success", "progress_buf", "train_test_flag",
             "dagger_reward_reset")
GRASP_WIDTH = 0.055


class _Observer:
    """width: the columns the observer fills at the head of a row; write(pose_R, pose_T, out): fill them, out a (N, >= width) view."""

    def __init__(self, width, write):
        self.width, self.write = int(width), write


def pc_observer(pc, sel=None, mask=False):
    """mesh2pc.PCfromMesh -> 3 * num_points columns.  sel (K) int32 on the device: the subset of the scene's points, drawn once here
    from torch's CPU generator where None (the reference draws one per call; a fixed one keeps the step free of host work).  A cloud
    built with groups= gives its own default, pc.group_sel(): (N, K) rows, every environment's from its own cabinet's cloud.
    mask=True: 4 * num_points columns, rows (x, y, z, pc.labels[part])."""
    if sel is None and getattr(pc, "groups", False):
        sel = pc.group_sel()
    elif sel is None:
        sel = torch.randperm(pc.pts.shape[0])[:pc.num_points].to(torch.int32).to(pc.device)
    obs = _Observer((4 if mask else 3) * sel.shape[-1], lambda R, T, out: pc.query_pc(R, T, out=out, sel=sel, mask=bool(mask)))
    obs.sel = sel
    return obs


def tsdf_observer(tsdf):
    """mesh2sdf.TSDFfromMesh -> resolution^3 columns."""
    res = int(tsdf.resolution)
    return _Observer(res ** 3, lambda R, T, out: tsdf.query_tsdf(R, T, out=out))


def depth_pc_observer(cam, volume, num_points=1024, mask=False, zero_label=0.0):
    """mesh2depth.DepthFromMesh and a depth2tsdf.TSDFVolume with the same cameras registered -> 3 * num_points columns: the rendered
    depth images back-projected and thinned (depth2pc returns its own tensor, so this one copies into the row).
    mask=True: 4 * num_points columns, rows (x, y, z, label): one render_frame gives the depth and the part image (cam's labels),
    and depth2pc_masked writes the sampled rows straight into the observation row (no copy); zero_label: the label of the point
    (0, 0, 0) that stands for everything outside the workspace."""
    if mask:
        def write_masked(R, T, out):
            frame = cam.render_frame(R, T, depth=True, seg=True, rgb=False)
            volume.depth2pc_masked(frame.depth, frame.seg, K=num_points, out=out, zero_label=zero_label)
        return _Observer(4 * num_points, write_masked)

    def write(R, T, out):
        out[:, :3 * num_points].copy_(volume.depth2pc(cam.render(R, T), K=num_points).reshape(out.shape[0], -1))
    return _Observer(3 * num_points, write)


def depth_img_observer(cam):
    """mesh2depth.DepthFromMesh -> V * im_h * im_w columns: the depth images themselves, rendered straight into the row (the
    `depth_img` mode of hand_base.py:337-341)."""
    return _Observer(cam.num_view * cam.im_h * cam.im_w, lambda R, T, out: cam.render(R, T, out=out))


def rgb_img_observer(cam, view=0):
    """mesh2depth.DepthFromMesh -> 3 * im_h * im_w columns: the colour image of camera `view` as three float planes (3, im_h, im_w),
    raw 0..255 (the `rgb_img` mode of hand_base.py:344-353, which takes camera 0 and permutes it so): one render_frame (rgb only)
    and one ops.rgb_planes launch straight into the row.  The colours are this package's palette and headlight shading."""
    view = int(view)
    if not 0 <= view < cam.num_view:
        raise ValueError(f"rgb_img_observer: view {view} outside [0, {cam.num_view})")

    def write(R, T, out):
        ops.rgb_planes(cam.render_frame(R, T, depth=False, seg=False, rgb=True).rgb, view, out)
    return _Observer(3 * cam.im_h * cam.im_w, write)


def depth_tsdf_observer(cam, volume):
    """mesh2depth.DepthFromMesh and a depth2tsdf.TSDFVolume with the same cameras registered -> resolution^3 columns: the rendered
    depth images integrated into the volume (the `depth_tsdf` mode of hand_base.py:325-327; integrate returns its own tensor, so
    this one copies into the row)."""
    n = int(volume._resolution) ** 3

    def write(R, T, out):
        out[:, :n].copy_(volume.integrate(cam.render(R, T)).reshape(out.shape[0], -1))
    return _Observer(n, write)


def depth_sparse_observer(cam, volume, K=1024):
    """The same pair -> 4 * K columns: rows (x, y, z, tsdf) of K voxels near the surface (the `depth_sparse` mode of
    hand_base.py:335-336, TSDFVolume.sparse_voxel)."""
    def write(R, T, out):
        out[:, :4 * K].copy_(volume.sparse_voxel(cam.render(R, T), K=K).reshape(out.shape[0], -1))
    return _Observer(4 * K, write)


def frame_recorder(cam, env=0, view=0):
    """mesh2depth.DepthFromMesh -> record(pose_R, pose_T, path): the colour image of environment `env` in view `view` written to
    `path` as a PNG (the image hand_base.py:355-357 saves).  Only that environment is rendered (b = 1, a slice of the poses, rgb
    only; a camera built with groups= is told that environment's object).  The copy to the host SYNCHRONISES the stream; it happens only for a frame somebody asked for."""
    env, view = int(env), int(view)
    if not 0 <= view < cam.num_view:
        raise ValueError(f"frame_recorder: view {view} outside [0, {cam.num_view})")

    def record(pose_R, pose_T, path):
        if not 0 <= env < pose_R.shape[0]:
            raise ValueError(f"frame_recorder: environment {env} outside [0, {pose_R.shape[0]})")
        group = cam.group_of[env:env + 1] if getattr(cam, "groups", False) else None
        frame = cam.render_frame(pose_R[env:env + 1], pose_T[env:env + 1], depth=False, seg=False, rgb=True, group_of=group)
        write_png(path, frame.rgb[0, view].cpu().numpy())
    return record


class KinematicEnv:
    """task: GraspCubeTensors over sim = KinematicSim(free_body=True), or OpenDrawerTensors over KinematicSim(objects=...).
    observers: {mode: pc_observer(...) / tsdf_observer(...) / depth_pc_observer(...) / depth_img_observer(...) / rgb_img_observer(...) /
    depth_tsdf_observer(...) / depth_sparse_observer(...)}; with add_proprio_obs the proprio row is the
    tail of every such mode's row (for grasp_cube the first mode's tail is written by end_step(obs_out=) itself: no cat).
    num_obs reports the widths returned.  grasp_width: the grasp predicate's (grasp_cube); hold=False switches the rule off (the
    cube, or the drawer, then never moves), hold='always' sets the flag in every environment whatever the predicate says (the
    "held" of kinematics.py: a flag the caller sets).  random_reset: the cube's reset draws u with torch.rand (default: the task cfg's `random_reset`, False).
    recorder: frame_recorder(cam, ...) or None; with one, step(actions, save_image_path=p) writes the frame after the step to p (the
    runners pass such a path when `save_video` is set); without one the path is ignored.
    scene_rows (N, M) int32 on the device (rows of sim.rigid_body, -1 for an empty slot) with scene_C (MC, 3, 3) or None: observers
    and recorder are then handed the poses of these M bodies from one ops.body_pose_gather launch per step, in place of the task's
    own parts (make_open_drawer_env(scene_meshes=) builds the table).
    contact: None, or a contact.ContactSensor over the scene pose's slots: every observation then senses (one more launch per step,
    no host synchronisation) and step()'s extras gain contact_dist (N, NB), the sensor's body distances in metres; in_contact (N, NB)
    = contact_dist <= contact_margin; penetration (N) = max(0, -min_j contact_dist).  Sensing alone resolves nothing (resolve= below): the
    observation rows, rewards and flags are those of the same run without it.  grasp='contact' (grasp_cube only; needs a sensor
    with bodies named 'lfinger' and 'rfinger'): the hold predicate is in_contact[lfinger] & in_contact[rfinger] of the last
    observation, in place of the gap rule, one step late like it.
    resolve: None (the sensor reports and nothing is blocked) or 'block' (needs contact=): contact blocking.  Every step then runs
    one more launch first (contact.StepGuard, csrc/articulation_sweep.hip): the step is cut into block_substeps parts and the robot
    stops at the last part before a sensing point would come within block_margin of a target, or deeper into one it touches; the
    test reads the scene pose of the last observation.  extras gain blocked (N) bool = the step was cut, and step_fraction (N)
    float32 = parts taken / block_substeps.  The limits, as contact.py states them: one fraction per environment (the whole robot
    stops when any sensing body would touch); a thin target can be stepped over between two candidates; contact is sticky (motion
    that lowers the distance below the margin is refused even if mostly tangential, motion away is admitted); held and reset
    environments are not guarded (a held cube or drawer moves with the hand); no self-collision, no friction, nothing is pushed.
    The defaults leave every earlier code path as it was: the same launches, the same extras keys."""

    def __init__(self, task, sim, observers=None, add_proprio_obs=False, grasp_width=GRASP_WIDTH, hold=True, random_reset=False,
                 recorder=None, scene_rows=None, scene_C=None, contact=None, contact_margin=0.002, grasp="gap", resolve=None,
                 block_substeps=8, block_margin=0.0):
        self.task, self.sim = task, sim
        if grasp not in ("gap", "contact"):
            raise ValueError(f"grasp: expected 'gap' or 'contact', got {grasp!r}")
        if grasp == "contact":
            if not isinstance(task, GraspCubeTensors):
                raise ValueError("grasp='contact': for grasp_cube only -- an open_drawer environment's target link differs per cabinet "
                                 "and is not named anywhere, so there is no body to ask the fingers about")
            if contact is None:
                raise ValueError("grasp='contact': needs contact= (a contact.ContactSensor)")
            if contact.names is None or not {"lfinger", "rfinger"} <= set(contact.names):
                raise ValueError(f"grasp='contact': contact= needs segments named 'lfinger' and 'rfinger' (names=), got {contact.names}")
            self._fingers = (contact.body("lfinger"), contact.body("rfinger"))
        self.contact, self.contact_margin, self.grasp_rule = contact, float(contact_margin), grasp
        if resolve not in (None, "block"):
            raise ValueError(f"resolve: expected None or 'block', got {resolve!r}")
        if resolve == "block" and contact is None:
            raise ValueError("resolve='block': needs contact= (a contact.ContactSensor): its points and targets are what is swept")
        self.resolve, self._guard = resolve, None
        self._contact_extras = {}
        self.recorder, self._scene_pose = recorder, None
        self.scene_rows, self.scene_C = scene_rows, scene_C
        if scene_rows is not None:
            f32 = dict(dtype=torch.float32, device=sim.device)
            self._scene_R = [torch.empty(*scene_rows.shape, 3, 3, **f32) for _ in range(2)]     # two sets, used in turn like the rows
            self._scene_T = [torch.empty(*scene_rows.shape, 3, **f32) for _ in range(2)]
        self.grasp = isinstance(task, GraspCubeTensors)
        if self.grasp != bool(getattr(sim, "free_body", False)) or (not self.grasp and sim.objects is None):
            raise ValueError("KinematicEnv: a GraspCubeTensors needs KinematicSim(free_body=True), an OpenDrawerTensors KinematicSim(objects=...)")
        if task.num_envs != sim.num_envs:
            raise ValueError(f"KinematicEnv: the task has {task.num_envs} environments, the sim {sim.num_envs}")
        self.device = sim.device
        self.observers = dict(observers or {})
        if hold not in (True, False, "always"):
            raise ValueError(f"hold: expected True (the predicate), False or 'always', got {hold!r}")
        self.add_proprio_obs, self.grasp_width, self.random_reset = bool(add_proprio_obs), float(grasp_width), bool(random_reset)
        if not hasattr(task, "dagger_reward_reset"):
            task.dagger_reward_reset = None                   # dagger.py sets it; like the feeder, nothing here reads it
        N, nd = task.num_envs, task.robot.num_dofs
        self._Wn, self._Wp = task.num_obs["normal_state"], 7 + 2 * nd
        self.num_obs = {"normal_state": self._Wn, "proprio_state": self._Wp}
        tail = self._Wp if self.add_proprio_obs else 0
        for mode, ob in self.observers.items():
            if mode in self.num_obs:
                raise ValueError(f"observers: {mode!r} is the task's own mode")
            self.num_obs[mode] = ob.width + tail
        f = dict(dtype=torch.float32, device=self.device)
        self._slots = [{mode: torch.zeros(N, w, **f) for mode, w in self.num_obs.items()} for _ in range(2)]
        self._slot = 0
        self._hold = torch.zeros(N, dtype=torch.bool, device=self.device)
        self._fixed_hold = None if hold is True else torch.full((N,), hold == "always", dtype=torch.bool, device=self.device)
        self._gap = torch.zeros(N, **f)
        if not self.grasp:
            self._pos_act_all = torch.zeros(sim.D, **f)
        if resolve == "block":
            from .contact import StepGuard
            nb = sim.art.num_bodies
            if scene_rows is not None:
                row0 = sim.rb_row0.cpu().numpy() if sim.flat else np.arange(N) * sim.rigid_body.shape[1]
                slot_body, C = guard_slot_body(nb, scene_rows=scene_rows.cpu().numpy(), rb_row0=row0), scene_C
            else:
                slot_body, C = guard_slot_body(nb, part_body=(task.part_body if self.grasp else task.part_slot).cpu().numpy()), task.part_C
            self._guard = StepGuard(contact, slot_body, C, substeps=block_substeps, margin=block_margin)

    def __getattr__(self, name):                              # only reached for names the env itself does not hold
        if name in FORWARDED:
            return getattr(self.task, name)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in FORWARDED:
            setattr(self.task, name, value)                   # 'test' on the env switches the task's reset rule
        else:
            object.__setattr__(self, name, value)

    # ------------------------------------------------------------------------------------------- the two halves of a step
    def _observe(self):
        """end_step into the next set of rows, then the observers and the grasp predicate for the next step."""
        task, sim = self.task, self.sim
        self._slot ^= 1
        rows = self._slots[self._slot]
        task.obs_buf["normal_state"] = rows["normal_state"]
        first = next(iter(self.observers), None)
        if self.grasp:
            out = rows[first] if self.add_proprio_obs and first is not None else rows["proprio_state"]
            task.end_step(sim.rigid_body, sim.dof_state, sim.root, obs_out=out)
            proprio = task.obs_buf["proprio_state"]
            if proprio.data_ptr() != rows["proprio_state"].data_ptr():
                rows["proprio_state"].copy_(proprio)
            r = task.robot
            torch.linalg.vector_norm(sim.rigid_body[:, r.ltip_rb_index, :3] - sim.rigid_body[:, r.rtip_rb_index, :3], dim=-1, out=self._gap)
            torch.logical_and(task.is_reached, self._gap <= self.grasp_width, out=self._hold)
        else:
            task.end_step(sim.rigid_body, sim.dof_state, sim.root)
            ns = rows["normal_state"]                         # the tip's seven columns and the joint columns of normal_state
            rows["proprio_state"][:, :7].copy_(ns[:, :7])
            rows["proprio_state"][:, 7:].copy_(ns[:, self._Wn - (self._Wp - 7):])
            torch.gt(task.extras["is_grasped"], 0, out=self._hold)
        self._scene_pose = None
        if self.observers:
            R, T = self.compute_scene_pose()
            for mode, ob in self.observers.items():
                ob.write(R, T, rows[mode])
                if self.add_proprio_obs and not (self.grasp and mode == first):
                    rows[mode][:, ob.width:].copy_(rows["proprio_state"])
        if self.contact is not None:
            self._sense()
        return dict(rows)

    def _sense(self):
        """The contact sensor on the scene pose the observers use: one launch, the three extras, and with grasp='contact' the hold
        predicate of the next step.  It reports; blocking is the guard's (resolve='block'), one launch before the step."""
        R, T = self.compute_scene_pose()
        body = self.contact.sense(R, T, per_point=False).body_dist                # (N, NB)
        touch = body <= self.contact_margin
        self._contact_extras = {"contact_dist": body, "in_contact": touch, "penetration": torch.clamp(-body.min(dim=1)[0], min=0.0)}
        if self.grasp_rule == "contact":
            torch.logical_and(touch[:, self._fingers[0]], touch[:, self._fingers[1]], out=self._hold)

    def reset(self):
        """hand_base.reset: every environment starts over; the observation of the first frame.  progress_buf is 0 afterwards."""
        task, sim = self.task, self.sim
        if self.grasp:
            task.reset()
            sim.set_dof_state(task.robot.default_dof_pos)
            sim.reset_free_body(u=self._u())
        else:
            sim.set_dof_state(task.robot.default_dof_pos)
            task.reset(sim.dof_state, sim.root, self._pos_act_all)
            sim.forward()
        obs = self._observe()
        task.progress_buf.zero_()
        return obs

    def _u(self):
        return torch.rand(self.task.num_envs, 3, dtype=torch.float32, device=self.device) if self.random_reset else None

    def step(self, actions, save_image_path=None):
        """One step.  save_image_path: with a recorder set and a path given, the colour frame of the recorder's environment after this
        step is written there as a PNG; that copies an image to the host and so synchronises, on those steps only."""
        task, sim = self.task, self.sim
        hold = self._hold if self._fixed_hold is None else self._fixed_hold
        if self._guard is not None:
            # the scene as the last observation saw it: _sense() gathered and cached it, so in steady state this issues no launch
            # (a step() taken before any reset() would pose whatever rigid_body holds)
            self._guard.set_scene(*self.compute_scene_pose())
        if self.grasp:
            pos_act, reset = task.begin_step(actions, sim.dof_state, sim.jacobian)
            sim.step(pos_act, reset, hold=hold, u=self._u(), guard=self._guard)
        else:
            _, reset = task.begin_step(actions, sim.jacobian, sim.dof_state, sim.root, self._pos_act_all)
            sim.step(task.pos_act, reset, hold=hold, guard=self._guard)
        obs = self._observe()
        if save_image_path is not None and self.recorder is not None:
            R, T = self.compute_scene_pose()                              # the observers' pose where there are observers
            self.recorder(R, T, save_image_path)
        extras = dict(task.extras, **self._contact_extras)
        if self._guard is not None:
            g = self._guard
            extras["blocked"] = g.steps < g.substeps
            extras["step_fraction"] = g.steps.to(torch.float32) / g.substeps
        return obs, task.rew_buf, task.reset_buf, extras

    def compute_scene_pose(self):
        """(rot (N, M, 3, 3), pos (N, M, 3)) of the last step, as the observers and the recorder get them: the task's own parts, or
        with scene_rows the M bodies of the table (gathered once per step, on first use)."""
        if self._scene_pose is None:
            if self.scene_rows is None:
                self._scene_pose = self.task.compute_scene_pose()
            else:
                self._scene_pose = ops.body_pose_gather(self.sim.rigid_body, self.scene_rows, self.scene_C,
                                                        self._scene_R[self._slot], self._scene_T[self._slot])
        return self._scene_pose

    def save_scene_pose(self, path=None):
        """hand_base.save_scene_pose: the posed parts of the last step on the host (a synchronisation; the runners call it in eval)."""
        rot, pos = self.compute_scene_pose()
        return {"rot": rot.cpu().numpy(), "pos": pos.cpu().numpy()}


def guard_slot_body(nb, scene_rows=None, rb_row0=None, part_body=None):
    """The slot_body table of a contact.StepGuard, on the host: for every pose slot of the scene pose the robot-local body in [0, nb)
    that places it, or -1.  From scene_rows (N, M) (rows of the flat rigid-body tensor, -1 for an empty slot) and rb_row0 (N) (each
    environment's first robot row): the row minus rb_row0, -1 where that falls outside the robot's nb rows; the environments must
    agree (the robot's slots are the same columns everywhere).  Or from part_body (M), the task's posed-part list over an
    environment's own rows (the robot's come first): entries outside [0, nb) become -1."""
    if scene_rows is not None:
        rows, row0 = np.asarray(scene_rows, dtype=np.int64), np.asarray(rb_row0, dtype=np.int64).reshape(-1)
        if rows.ndim != 2 or row0.shape != (rows.shape[0],):
            raise ValueError(f"scene_rows / rb_row0: expected (N, M) and (N,), got {rows.shape} and {row0.shape}")
        rel = rows - row0[:, None]
        sb = np.where((rows >= 0) & (rel >= 0) & (rel < nb), rel, -1)
        if (sb != sb[:1]).any():
            raise ValueError("scene_rows: the robot's bodies must sit in the same slots of every environment")
        return sb[0].astype(np.int32)
    part = np.asarray(part_body, dtype=np.int64).reshape(-1)
    return np.where((part >= 0) & (part < nb), part, -1).astype(np.int32)


def _scene(base_pose, dof):
    bp = np.asarray((0, 0, 0, 0, 0, 0, 1) if base_pose is None else base_pose, dtype=np.float64).reshape(-1)
    if bp.size != 7:
        raise ValueError(f"base_pose: expected 7 numbers, got {bp.size}")
    bp[3:] /= np.linalg.norm(bp[3:])
    return tuple(float(v) for v in bp), None if dof is None else [float(v) for v in dof]


def make_grasp_cube_env(cfg_task, num_envs, device, urdf, dt, base_pose=None, dof=None, observers=None, add_proprio_obs=False,
                        grasp_width=GRASP_WIDTH, hold=True, max_velocity=None, free_body_pose=(0, 0, 0.025, 0, 0, 0, 1), rest_z=0.025,
                        fall_speed=0.0, reset_range=0.15, recorder=None, contact=None, contact_margin=0.002, grasp="gap", resolve=None,
                        block_substeps=8, block_margin=0.0):
    """GraspCubeTensors + KinematicSim(free_body=True) around the robot of `urdf` (a path or a loaded tree; fixed or mobile, through
    tree.robot_kwargs()).  cfg_task: cfg/tasks/grasp_cube.yaml as a dict; base_pose (7), divided by its norm, and dof (the default
    joint positions; None: cfg_task['robot']['dof'], else mid-range) place the robot."""
    tree = load_urdf(urdf) if isinstance(urdf, str) else urdf
    bp, dof = _scene(base_pose, dof)
    rcfg = dict(cfg_task.get("robot", {}))
    if dof is not None:
        rcfg["dof"] = dof
    kw = tree.robot_kwargs()
    robot = (MobileFranka if "mesh_bodies" in kw else Franka)(rcfg, dt, num_envs, device, **kw)
    task = GraspCubeTensors(num_envs, device, dict(cfg_task, robot=rcfg), dt, num_bodies=tree.num_bodies + 1, robot=robot,
                            obj_default_pos=tuple(free_body_pose[:3]))
    sim = KinematicSim(tree, num_envs, device, dt, base_pose=bp, max_velocity=max_velocity, free_body=True,
                       tips=(robot.ltip_rb_index, robot.rtip_rb_index), free_body_pose=free_body_pose, rest_z=rest_z, fall_speed=fall_speed,
                       reset_range=reset_range)
    return KinematicEnv(task, sim, observers=observers, add_proprio_obs=add_proprio_obs, grasp_width=grasp_width, hold=hold,
                        random_reset=bool(cfg_task.get("random_reset", False)), recorder=recorder, contact=contact,
                        contact_margin=contact_margin, grasp=grasp, resolve=resolve, block_substeps=block_substeps,
                        block_margin=block_margin)


def scene_row_table(part_slot, rb_row0, obj_rb_row0, obj_bodies, max_bodies=None):
    """The (N, M) int32 row table of a scene whose environments differ, on the host: slot p < len(part_slot) of environment e is the
    robot body rb_row0[e] + part_slot[p]; slot len(part_slot) + j is body j of the environment's object, obj_rb_row0[e] + j, and -1
    from the object's body count on.  M = len(part_slot) + max_bodies (default: the largest body count among the environments)."""
    part_slot, rb_row0, obj_rb_row0, obj_bodies = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (part_slot, rb_row0, obj_rb_row0,
                                                                                                          obj_bodies))
    most = int(obj_bodies.max()) if max_bodies is None else int(max_bodies)
    if most < int(obj_bodies.max()):
        raise ValueError(f"max_bodies {most} below an object's {int(obj_bodies.max())} bodies")
    j = np.arange(most)[None]
    cab = np.where(j < obj_bodies[:, None], obj_rb_row0[:, None] + j, -1)
    return np.ascontiguousarray(np.concatenate([rb_row0[:, None] + part_slot[None], cab], axis=1), dtype=np.int32)


def make_open_drawer_env(cfg_task, num_envs, device, urdf, assets, dt, observers=None, add_proprio_obs=False, hold=True,
                         max_velocity=None, recorder=None, scene_meshes=None, contact=None, contact_margin=0.002, grasp="gap",
                         resolve=None, block_substeps=8, block_margin=0.0):
    """OpenDrawerTensors + KinematicSim(objects=...) wired as INTEGRATION.md's loop: assets = load_drawer_assets(folders, scale),
    handed out as env % num_objs; the robot of `urdf` (the mobile Franka of the shipped config, or the fixed one).
    scene_meshes: None, or load_drawer_meshes(assets) -- the same list a DepthFromMesh(meshes=robot parts, groups=scene_meshes,
    group_of=env.task.obj_id) was built from.  Observers and recorder then get the poses of the robot's posed parts (with their
    mesh-frame matrices) followed by EVERY body of the environment's own cabinet, in the tree's body order, NaN past its body count:
    scene_row_table over the sim's rows, env.scene_rows, one body_pose_gather launch per step.  Without it they get the task's 13
    parts (the robot's, the target link, the handle), as before."""
    tree = load_urdf(urdf) if isinstance(urdf, str) else urdf
    envs = assets.for_envs(num_envs)
    kw = tree.robot_kwargs()
    robot = (MobileFranka if "mesh_bodies" in kw else Franka)(cfg_task.get("robot", {}), dt, num_envs, device, **kw)
    rb_mask, dof_mask, B, D = envs.masks(robot.num_rigid_body, robot.num_dofs)
    task = OpenDrawerTensors(num_envs, device, cfg_task, dt, rb_mask, dof_mask, num_rigid_bodies=B, num_dof_states=D, robot=robot,
                             **envs.task_kwargs())
    sim = KinematicSim(tree, num_envs, device, dt, max_velocity=max_velocity, objects=ObjectLibrary(assets.trees, device),
                       obj_type=envs.obj_id, target_dof=envs.target_dof, tips=(robot.ltip_rb_index, robot.rtip_rb_index))
    rows = C = None
    if scene_meshes is not None:
        if len(scene_meshes) != assets.num_objs:
            raise ValueError(f"scene_meshes: expected one list per object ({assets.num_objs}), got {len(scene_meshes)}")
        for k, bodies in enumerate(scene_meshes):
            if len(bodies) != int(assets.num_bodies[k]):
                raise ValueError(f"scene_meshes[{k}]: expected one entry per body ({int(assets.num_bodies[k])}), got {len(bodies)}")
        nr = task.part_slot.numel() - 2                       # the robot's posed parts; the last two are the target link and the handle
        rows = scene_row_table(task.part_slot[:nr].cpu().numpy(), sim.rb_row0.cpu().numpy(), sim.obj_rb_row0.cpu().numpy(),
                               envs.obj_bodies, max_bodies=int(assets.num_bodies.max()))
        rows = torch.from_numpy(rows).to(device)
        C = None if task.part_C is None else task.part_C[:nr].contiguous()
    return KinematicEnv(task, sim, observers=observers, add_proprio_obs=add_proprio_obs, hold=hold, recorder=recorder, scene_rows=rows,
                        scene_C=C, contact=contact, contact_margin=contact_margin, grasp=grasp, resolve=resolve,
                        block_substeps=block_substeps, block_margin=block_margin)
