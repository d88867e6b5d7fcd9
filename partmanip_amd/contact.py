"""Contact sensing: the signed distance of points that ride on the robot's bodies to the scene's baked part grids.

    sensor = ContactSensor.from_cloud(tsdf, pc, slots=(8, 9, 10), targets=(11, 12), names=("hand", "lfinger", "rfinger"))
    r = sensor.sense(pose_R, pose_T)            # r.dist (b, NP), r.arg (b, NP), r.body_dist (b, NB), r.body_point (b, NB)

`tsdf` is a mesh2sdf.TSDFfromMesh (its grids are what is sensed AGAINST), `pc` a mesh2pc.PCfromMesh over the same pose slots (its
surface samples are the points that sense).  One launch of pm_mesh_sdf_points_f32 (csrc/mesh_sdf_points.hip; the grouped entry when
the TSDF was built with groups=) poses every point by its carrier slot, samples the target ordinals' grids there with the arithmetic
of the mesh-TSDF observation, and reduces per body.  `targets` is an ordinal range of the TSDF -- the cube's grid for grasp_cube, the
environment's own cabinet rows for open_drawer -- so the robot never senses itself.

What the numbers are.  A grid holds distances clamped to the bake's truncation, and a trilinear sample of it is a distance only
within that band; outside every target's valid box the value is 1.0 ("far", the reference's own out-of-box value), not a distance.
body_dist <= margin is therefore a contact test, and max(0, -body_dist) a penetration depth up to the truncation.  The sensor
reports; nothing here pushes bodies apart or models friction.

Contact blocking.  StepGuard(sensor, slot_body, slot_C, substeps=8, margin=0.0) is the one contact RESPONSE: handed to
KinematicSim.step(guard=) (KinematicEnv(resolve='block') does that), it runs one launch of pm_articulation_sweep_f32
(csrc/articulation_sweep.hip) before the articulation's: the step is cut into `substeps` parts, every part's joint state is posed and
sensed with this sensor's points and targets, and the robot stops at the last part before the first that would bring a sensing
point within `margin` of a target, or deeper into one it already touches.  A stated rule, not physics, and its limits are these:
  - one fraction per environment: the WHOLE robot stops when any sensing body would touch;
  - a target thinner than the distance a sensing point covers in one part can be stepped over between two candidates;
  - contact is sticky: motion that lowers the distance below the margin is refused even when it is mostly tangential; motion that
    keeps or raises the distance is admitted, so the robot can always back out;
  - environments that are reset or held are not guarded (a held cube or drawer moves with the hand, the fingers keep closing);
  - no self-collision, no ground plane, no friction, nothing slides and nothing is pushed.

Layout.  The kernel's per-wave cull wants the 64 points of a wave to share one carrier and one bounding sphere, and its segment
reduction wants a segment to start on a chunk boundary: PointLayout sorts each segment's points by carrier (stably) and pads every
(segment, carrier) run but the last to a multiple of 64 with repeats of its last point, which carry id -1 and enter no segment result;
chunk_spheres bounds each chunk in its carrier's frame.  Both are built once per sensor."""
import collections

import numpy as np
import torch

CHUNK = 64
ContactReading = collections.namedtuple("ContactReading", "dist arg body_dist body_point")


def _ints(a, name, n=None):
    v = np.asarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    if v.dtype.kind not in "iu" or v.ndim != 1 or (n is not None and v.shape != (n,)):
        raise ValueError(f"{name}: expected {'a list of' if n is None else n} integers, got {v.dtype} {v.shape}")
    return v.astype(np.int64)


class PointLayout:
    """NP points, carrier (NP,) integers or None (all -1), segments a list of point counts that sum to NP or None (no segments).
    Attributes, all numpy: src (NPp,) the caller's index of every laid-out point, pt_id (NPp,) int32 the same with -1 on padding,
    carrier (NPp,) int32, seg_off (NS + 1,) int32 in laid-out points or None, pos (NP,) where each of the caller's points went;
    identity: the layout is the caller's order with nothing added."""

    def __init__(self, NP, carrier=None, segments=None):
        NP = int(NP)
        car = np.full(NP, -1, dtype=np.int64) if carrier is None else _ints(carrier, "carrier", NP)
        if segments is None:
            counts = [NP]
        else:
            counts = _ints(segments, "segments").tolist()
            if not counts or min(counts) < 0 or sum(counts) != NP:
                raise ValueError(f"segments: expected non-negative point counts that sum to {NP}, got {counts}")
        runs, o = [], 0
        for s, cnt in enumerate(counts):
            idx = np.arange(o, o + cnt)
            o += cnt
            order = idx[np.argsort(car[idx], kind="stable")]
            pieces = np.split(order, np.flatnonzero(np.diff(car[order])) + 1) if cnt else []
            runs.extend((s, r) for r in pieces)
        src, pid, seg_off = [], [], [0] * (len(counts) + 1)
        total = 0
        for k, (s, r) in enumerate(runs):
            pad = 0 if k == len(runs) - 1 else (-len(r)) % CHUNK     # the layout's last run may end inside a chunk
            src += [r, np.full(pad, r[-1])]
            pid += [r, np.full(pad, -1)]
            total += len(r) + pad
            seg_off[s + 1] = total
        for s in range(len(counts)):                                 # an empty segment ends where the one before it ends
            seg_off[s + 1] = max(seg_off[s + 1], seg_off[s])
        self.NP = NP
        self.src = np.concatenate(src).astype(np.int64) if src else np.zeros(0, dtype=np.int64)
        self.pt_id = np.concatenate(pid).astype(np.int32) if pid else np.zeros(0, dtype=np.int32)
        self.carrier = car[self.src].astype(np.int32)
        self.seg_off = None if segments is None else np.asarray(seg_off, dtype=np.int32)
        self.pos = np.zeros(NP, dtype=np.int64)
        real = self.pt_id >= 0
        self.pos[self.src[real]] = np.flatnonzero(real)
        self.identity = len(self.src) == NP and bool((self.src == np.arange(NP)).all())

    def on(self, device):
        """The device tables a call needs: (src, pt_id, carrier, seg_off or None, pos), src and pos int64, the others int32."""
        f = lambda a: None if a is None else torch.from_numpy(a).to(device)   # noqa: E731
        return f(self.src), f(self.pt_id), f(self.carrier), f(self.seg_off), f(self.pos)


def chunk_spheres(pts):
    """pts (NPp, 3) float32 laid-out points (any device) -> (ceil(NPp / 64), 4) float32: per chunk the centre of its bounding box
    and a radius that holds every point of it with 1e-4 to spare (fp32 round-off of this evaluation is 1e-7).  Padding points are
    repeats of a point of their own chunk, so they need no mask."""
    n = pts.shape[0]
    C = (n + CHUNK - 1) // CHUNK
    if C * CHUNK != n:
        pts = torch.cat([pts, pts[-1:].expand(C * CHUNK - n, 3)])
    x = pts.reshape(C, CHUNK, 3)
    c = (x.min(dim=1)[0] + x.max(dim=1)[0]) * 0.5
    r = (x - c[:, None]).square().sum(dim=-1).sqrt().max(dim=1)[0] * 1.0001 + 1e-7
    return torch.cat([c, r[:, None]], dim=1).contiguous()


class ContactSensor:
    """tsdf: TSDFfromMesh; points (NP, 3) in their carriers' frames; carrier (NP,) integers in [-1, tsdf.part_num), -1 for a point
    given in the world frame; segments: the point counts of the sensing bodies, in order (they sum to NP); targets (lo, hi): the
    ordinals of `tsdf` sensed against (parts, or with groups= an environment's own rows); names: None or one name per body.
    sense() is one launch.  Attributes: num_bodies, num_points, names, targets, layout (PointLayout), chunk_sphere."""

    def __init__(self, tsdf, points, carrier, segments, targets, names=None):
        pts = np.ascontiguousarray(points.detach().cpu().numpy() if torch.is_tensor(points) else points, dtype=np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
            raise ValueError(f"points: expected (NP > 0, 3), got {pts.shape}")
        NP = pts.shape[0]
        car = _ints(carrier, "carrier", NP)
        if car.min() < -1 or car.max() >= tsdf.part_num:
            raise ValueError(f"carrier: expected pose slots in [-1, {tsdf.part_num}) (the pose table of tsdf), got [{car.min()}, {car.max()}]")
        lo, hi = (int(v) for v in targets)
        top = tsdf._row_range()[1]
        if not 0 <= lo < hi <= top:
            raise ValueError(f"targets: expected a non-empty ordinal range inside [0, {top}), got ({lo}, {hi})")
        self.layout = PointLayout(NP, car, segments)
        NB = len(self.layout.seg_off) - 1
        if names is not None and (len(names) != NB or len(set(names)) != NB):
            raise ValueError(f"names: expected {NB} distinct names, one per segment, got {list(names)}")
        self.tsdf, self.targets, self.names = tsdf, (lo, hi), None if names is None else tuple(names)
        self.num_points, self.num_bodies, self.device = NP, NB, tsdf.device
        src, self._pt_id, self._carrier, self._seg_off, self._pos = self.layout.on(self.device)
        self._pts = torch.from_numpy(pts).to(self.device).index_select(0, src).contiguous()
        self.chunk_sphere = chunk_spheres(self._pts)

    @classmethod
    def from_cloud(cls, tsdf, pc, slots, targets, points_per_body=None, names=None):
        """The sensing points are rows of pc.pts (a mesh2pc.PCfromMesh): for every pose slot of `slots` -- for example hand, left
        finger, right finger -- the cloud's points of that slot, the first points_per_body of them when given."""
        if int(pc.part_num) != int(tsdf.part_num):
            raise ValueError(f"pc: its part_num {pc.part_num} differs from tsdf's {tsdf.part_num}: the two do not share a pose table")
        part_of, pts = pc.part_of.cpu().numpy(), pc.pts.detach().cpu().numpy()
        rows = []
        for s in slots:
            r = np.flatnonzero(part_of == int(s))
            r = r if points_per_body is None else r[:int(points_per_body)]
            if len(r) == 0:
                raise ValueError(f"slots: the cloud has no point on pose slot {s}")
            rows.append(r)
        allr = np.concatenate(rows)
        return cls(tsdf, pts[allr], part_of[allr], [len(r) for r in rows], targets, names)

    def body(self, name):
        """The segment index of a named body."""
        if self.names is None or name not in self.names:
            raise ValueError(f"names: the sensor has no body named {name!r} (names = {self.names})")
        return self.names.index(name)

    def sense(self, pose_R, pose_T, group_of=None, per_point=True, cull=True):
        """pose_R (b, part_num, 3, 3), pose_T (b, part_num, 3) -> ContactReading(dist (b, NP) metres, arg (b, NP) int32 the target
        ordinal nearest to each point or -1, body_dist (b, NB), body_point (b, NB) int32 the index of each body's nearest point, in
        the constructor's order).  per_point=False computes the two body results only (dist and arg are None).  group_of as in
        TSDFfromMesh.query_tsdf."""
        d, a, bd, bp = self.tsdf._sdf_points(pose_R, pose_T, self._pts, self._carrier, self.targets[0], self.targets[1], group_of,
                                             pt_id=self._pt_id, chunk_sphere=self.chunk_sphere, seg_off=self._seg_off,
                                             want_dist=per_point, want_arg=per_point, cull=cull)
        if per_point and not self.layout.identity:
            d, a = d.index_select(1, self._pos), a.index_select(1, self._pos)
        return ContactReading(d, a, bd, bp)


class StepGuard:
    """Contact blocking for KinematicSim.step(guard=): the tables of one swept test per step and its three outputs.

    sensor: a ContactSensor (its points, carriers, segments and targets are what is swept); slot_body: one integer per pose slot of
    the sensor's table, the ROBOT-LOCAL body in [0, nb) whose frame places that slot, or -1 for a slot the robot does not place (the
    cube, a cabinet's bodies: their pose is the table's); slot_C (MC, 3, 3) or None: the mesh-frame matrices of the first MC slots,
    as ops.body_pose_gather takes them; substeps S in [1, 63]; margin: the distance at or below which a candidate is contact.
    set_scene(pose_R, pose_T) hands over the scene pose the test reads for the slots the robot does not place (the caller's last
    observation); sweep() is what KinematicSim.step calls.  After a step: sweep_dist (N, S + 1) the candidates' distances, steps (N)
    int32 the parts taken, targets (N, nd) the joint state the robot was sent to.  The module docstring states the rule's limits."""

    def __init__(self, sensor, slot_body, slot_C=None, substeps=8, margin=0.0):
        M = int(sensor.tsdf.part_num)
        sb = _ints(slot_body, "slot_body", M)
        if sb.min() < -1:
            raise ValueError(f"slot_body: expected robot bodies or -1, got {int(sb.min())}")
        self.substeps, self.margin = int(substeps), float(margin)
        if not 1 <= self.substeps <= 63:
            raise ValueError(f"substeps: expected 1 .. 63 parts of a step, got {substeps}")
        if self.margin != self.margin:
            raise ValueError("margin: expected a number, got NaN")
        self.sensor, self.device = sensor, sensor.device
        self._slot_body_host = sb
        self.slot_body = torch.from_numpy(sb.astype(np.int32)).to(self.device)
        self.slot_C = None
        if slot_C is not None:
            C = torch.as_tensor(slot_C, dtype=torch.float32).to(self.device).contiguous()
            if C.dim() != 3 or tuple(C.shape[1:]) != (3, 3) or C.shape[0] > M:
                raise ValueError(f"slot_C: expected (MC <= {M}, 3, 3), got {tuple(C.shape)}")
            self.slot_C = C
        self._pose = None
        self.sweep_dist = self.steps = self.targets = None

    def set_scene(self, pose_R, pose_T, group_of=None):
        """The scene pose (N, M, 3, 3) / (N, M, 3) the next sweep reads; the slots the robot places are ignored."""
        self._pose = (pose_R, pose_T, group_of)

    def sweep(self, sim, pos_act, reset=None, hold=None, cull=True):
        """The sweep launch for sim's next step towards pos_act; returns the guarded targets (N, nd).  Environments with reset or
        hold set take the whole step."""
        if self._pose is None:
            raise ValueError("StepGuard: set_scene(pose_R, pose_T) comes before the first guarded step")
        nb = sim.art.num_bodies
        if self._slot_body_host.max() >= nb:
            raise ValueError(f"slot_body: expected bodies in [-1, {nb}), got {int(self._slot_body_host.max())}")
        s = self.sensor
        tables, R, T, groups = s.tsdf._point_tables(*self._pose)
        N, nd = sim.num_envs, sim.art.num_dofs
        if self.sweep_dist is None or self.sweep_dist.shape[0] != N or self.targets.shape[1] != nd:
            f = dict(dtype=torch.float32, device=self.device)
            self.sweep_dist = torch.empty(N, self.substeps + 1, **f)
            self.steps = torch.empty(N, dtype=torch.int32, device=self.device)
            self.targets = torch.empty(N, nd, **f)
        sim.art.sweep(sim.dof_state, sim.base_pose, pos_act, sim.dt, *tables, R, T, s._pts, s._carrier, s._seg_off, self.slot_body,
                      self.substeps, margin=self.margin, reset=reset, free=hold, vmax=sim.max_velocity, dof_row0=sim.dof_row0,
                      slot_C=self.slot_C, p0=s.targets[0], p1=s.targets[1], pt_id=s._pt_id, chunk_sphere=s.chunk_sphere, cull=cull,
                      sweep_dist=self.sweep_dist, steps=self.steps, targets_out=self.targets, **groups)
        return self.targets
