"""The posed mesh point cloud, mirroring the reference's `utils/mesh2pc.py:PCfromMesh`: a point-cloud observation of the scene
without a depth camera.

    pc = PCfromMesh(num_envs, device, num_points=1024)                                  # mesh2pc.py:13-29
    cloud = pc.query_pc(pose_R (b, m, 3, 3), pose_T (b, m, 3))  -> (b, num_points, 3)    # mesh2pc.py:56-65

The surface of every rigid part (eight Franka links, hand, two fingers, the object) is sampled once at construction
(`meshio.sample_surface` in place of trimesh); every step the points are put under their parts' poses and `num_points` of them
are returned.  The reference poses all m * p points of every environment (bmm, 600 MB at 4096 environments) and then gathers a
random subset through a host index; here one launch of pm_mesh_pc_query_f32 (csrc/mesh_pc.hip) computes the selected points only,
and with `out=` writes them straight into the left part of an (N, 3 * num_points + proprio) observation buffer.

One copy of the canonical points lives on the device (`part_pc (m, p, 3)`, its flat view `pts (m p, 3)`, `part_of (m p)`); the
reference's per-environment repeat is the property `all_pc`, materialised on demand.

A scene whose environments differ (open_drawer: every environment holds its own cabinet, env % num_objs):

    pc = PCfromMesh(N, device, meshes=robot_parts, groups=load_drawer_meshes(assets), group_of=envs.obj_id)

The point library `pts` is then the shared parts' points followed by `num_points` points of every body of every object; a point of
body j names slot len(meshes) + j (`part_of`), and an environment's own cloud is the shared rows plus the rows of its object.  The
kernel is the same one: it already takes a selection per environment, so `group_sel()` only has to draw every environment's rows
from its own cloud.
"""
import numpy as np
import torch

from . import meshio, ops, scene_groups

SELECT_MODES = ("random", "all", "fps")


def random_poses(b, m, generator, device):
    """Seeded poses from plain tensor ops: unit-quaternion rotations (b, m, 3, 3) and translations U(-0.25, 0.25) (b, m, 3), float32
    on `device`, drawn from `generator` (which lives on that device)."""
    q = torch.nn.functional.normalize(torch.randn(b, m, 4, generator=generator, device=device), dim=-1)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).view(b, m, 3, 3)
    T = torch.rand(b, m, 3, generator=generator, device=device) * 0.5 - 0.25
    return R.contiguous(), T.contiguous()


class PCfromMesh:
    """Constructor of the reference plus keyword extensions in the manner of TSDFfromMesh: `asset_root` (prefix of the reference's
    relative paths assets/franka_description/meshes/visual/* and assets/objs/cube/cube.obj), `meshes` (a list of (vertices, faces)
    used instead of the files), `part_pcs` (a ready (m, p, 3) array used instead of sampling) and `seed` (part i is sampled with
    torch.Generator().manual_seed(seed + i), so the two fingers, one file loaded twice, get different points as in the reference).
    groups: None, or one list per object with one entry per body: (vertices, faces), a ready (num_points, 3) array, or None for a
    body without a mesh (tasks.open_drawer.load_drawer_meshes); body j of object k is sampled with
    torch.Generator().manual_seed(seed + GROUP_SEED_STRIDE * (k + 1) + j).  group_of (num_envs,) ints in [-1, len(groups)): the object
    each environment holds, -1 for none (default: env % len(groups), the reference's rule).  part_num is then num_shared + the
    largest body count; attributes: num_shared, pts_shared (the shared rows of pts), group_off (numpy, rows of pts relative to
    pts_shared), group_of (numpy), max_group_points.  With groups, `meshes` may be empty.
    labels: None, or part_num numbers, the value query_pc(mask=True) puts in a point's fourth column, by pose SLOT (None: the slot
    index); with groups= slot num_shared + j is body j of whichever object the environment holds, so a label there names "body j",
    not a particular cabinet's link.  Kept as float32 on the device (`labels`)."""

    GROUP_SEED_STRIDE = 4096

    def __init__(self, num_envs, device, num_points=1024, asset_root='.', meshes=None, part_pcs=None, seed=0, groups=None, group_of=None,
                 labels=None):
        self.num_envs = num_envs
        self.device = device
        self.num_points = int(num_points)
        self.asset_root = asset_root
        self.seed = seed
        if self.num_points < 1:
            raise ValueError(f"num_points must be positive, got {num_points}")
        if part_pcs is not None:
            pcs = np.ascontiguousarray(part_pcs.cpu().numpy() if torch.is_tensor(part_pcs) else part_pcs, dtype=np.float32)
            if pcs.ndim != 3 or pcs.shape[2] != 3 or pcs.shape[0] == 0 or pcs.shape[1] == 0:
                raise ValueError(f"part_pcs: expected (m, p, 3), got {pcs.shape}")
        else:
            if meshes is None:
                meshes = [meshio.load_mesh(path) for path in meshio.scene_mesh_paths(asset_root)]
            if len(meshes) == 0 and not groups:
                raise ValueError("meshes: at least one part is needed")
            pcs = np.stack([self.load_pc_from_mesh(v, f, i) for i, (v, f) in enumerate(meshes)]) if len(meshes) else \
                np.zeros((0, self.num_points, 3), dtype=np.float32)
        if group_of is not None and groups is None:
            raise ValueError("group_of: needs groups=")
        self.part_num, self.points_per_part = int(pcs.shape[0]), int(pcs.shape[1])
        self.groups = groups is not None
        self.last_sel = None
        if self.groups:
            self._init_groups(pcs, groups, group_of)
            self._init_labels(labels)
            return
        self._init_labels(labels)
        self.part_pc = torch.from_numpy(pcs).to(self.device)                                   # (m, p, 3)
        self.pts = self.part_pc.view(-1, 3)                                                    # (m p, 3), the same memory
        self.part_of = torch.arange(self.part_num, dtype=torch.int32).repeat_interleave(self.points_per_part).to(self.device)
        self._full = None                                                                      # scratch of select='fps'
        self._fps_ws = None

    def _init_labels(self, labels):
        """labels (part_num,) float32 on the device: the given numbers, or the slot index."""
        m = self.part_num
        lab = np.arange(m) if labels is None else np.asarray(labels.cpu().numpy() if torch.is_tensor(labels) else labels)
        if lab.shape != (m,) or lab.dtype.kind not in "iuf":
            raise ValueError(f"labels: expected {m} numbers, one per part, got {lab.dtype} {lab.shape}")
        self.labels = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.float32)).to(self.device)

    def _init_groups(self, pcs, groups, group_of):
        """The point library of a scene whose environments differ: the shared parts' points, then every object's bodies."""
        S = self.part_num
        self._full = self._fps_ws = None
        self.part_pc = torch.from_numpy(pcs).to(self.device)                                   # (S, p, 3): the shared parts only
        clouds, part = [pcs.reshape(-1, 3)], [np.repeat(np.arange(S, dtype=np.int32), self.points_per_part)]

        def add(body, slot, what, k, j):
            if isinstance(body, (tuple, list)):
                pts = self.load_pc_from_mesh(body[0], body[1], self.GROUP_SEED_STRIDE * (k + 1) + j)
            else:
                pts = np.ascontiguousarray(body.cpu().numpy() if torch.is_tensor(body) else body, dtype=np.float32)
                if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
                    raise ValueError(f"{what}: expected (vertices, faces), a (p, 3) array of points or None, got {pts.shape}")
            clouds.append(pts)
            part.append(np.full(len(pts), slot, dtype=np.int32))
            return len(pts)

        sg = self._scene = scene_groups.SceneGroups(self.num_envs, self.device, S, groups, add, group_of)
        self.num_shared, self.part_num, self.group_of, self.max_group_points = S, sg.part_num, sg.group_of, sg.most
        self.group_off = sg.group_off.astype(np.int64)                                         # rows of pts, as before: int64
        self.pts_shared = S * self.points_per_part
        if self.pts_shared + self.max_group_points == 0:
            raise ValueError("meshes and groups: no mesh at all")
        self._group_of_long = sg.group_of_dev.long()                                           # the index type of group_sel's gather
        self.pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds), dtype=np.float32)).to(self.device)   # (Q, 3)
        self.part_of = torch.from_numpy(np.concatenate(part)).to(self.device)                  # (Q,) int32: the slot
        self._all_table = None

    def _call_groups(self, b, group_of):
        """(host ints or None, device int64 (b,)) of a call over b environments, by SceneGroups' rules, as the index group_sel gathers
        with: the constructor's table, a host list validated once and copied, or a device tensor (not read here) checked for its
        length and clamped."""
        if group_of is None:
            self._scene.for_call(b, None)                                                      # the slice rule
            return self.group_of, self._group_of_long
        if torch.is_tensor(group_of) and group_of.is_cuda:
            if tuple(group_of.shape) != (b,):
                raise ValueError(f"group_of: expected ({b},), got {tuple(group_of.shape)}")
            g = group_of.long()                                                                # an id outside [-1, G) counts as -1, as in the kernels
            return None, torch.where((g >= 0) & (g < len(self.group_off) - 1), g, torch.full_like(g, -1))
        host = self._scene.host_group_of(group_of, b)
        return host, torch.from_numpy(host).to(self.device).long()

    def own_rows(self, g):
        """The rows of `pts` that make the cloud of an environment holding object g (-1: none): the shared rows, then the object's."""
        rows = np.arange(self.pts_shared)
        if g >= 0:
            rows = np.concatenate([rows, self.pts_shared + np.arange(self.group_off[g], self.group_off[g + 1])])
        return rows

    def group_sel(self, generator=None, group_of=None):
        """(b, K) int32 rows of `pts` on the device, K = num_points: for every object in turn, and then once for 'no object' (-1), the
        first K entries of torch.randperm over that cloud (own_rows) drawn from `generator` (None: the CPU global generator), then
        row group_of[e] of that table for every environment e, gathered on the device.  An environment's points so come from the
        shared parts and its own object only; environments holding the same object share their selection, as the reference's
        environments all do.  The 'no object' row is drawn only when the shared cloud has K points; it is -1 (NaN points)
        otherwise, and asking for it from the host is an error."""
        if not self.groups:
            raise ValueError("group_sel: this cloud was built without groups=")
        host, dev = self._call_groups(self.num_envs if group_of is None else len(group_of), group_of)
        K, G = self.num_points, len(self.group_off) - 1
        table = np.full((G + 1, K), -1, dtype=np.int32)
        for g in list(range(G)) + [-1]:
            rows = self.own_rows(g)
            if len(rows) < K:
                if g >= 0 or (host is not None and (host < 0).any()):
                    raise ValueError(f"num_points {K} exceeds the {len(rows)} points of the cloud of " +
                                     (f"object {g}" if g >= 0 else "an environment without an object"))
                continue
            table[g] = rows[torch.randperm(len(rows), generator=generator)[:K].numpy()]
        return torch.from_numpy(table).to(self.device)[dev]                                    # index -1 is the last row

    def _all_sel(self, dev):
        """(b, pts_shared + max_group_points) int32: every row of every environment's own cloud, -1 (a NaN point) past its count."""
        if self._all_table is None:
            G = len(self.group_off) - 1
            table = np.full((G + 1, self.pts_shared + self.max_group_points), -1, dtype=np.int32)
            for g in list(range(G)) + [-1]:
                rows = self.own_rows(g)
                table[g, :len(rows)] = rows
            self._all_table = torch.from_numpy(table).to(self.device)
        return self._all_table[dev]

    def load_pc_from_mesh(self, vertices, faces, index=0):
        """`num_points` surface points of one part (mesh2pc.py:32-41) as float32 (p, 3), seeded with seed + index."""
        g = torch.Generator().manual_seed(self.seed + index)
        return meshio.sample_surface(vertices, faces, self.num_points, g)[0]

    @property
    def all_pc(self):
        """The reference's attribute (mesh2pc.py:27-28): the part clouds repeated per environment, (b m, p, 3).  Built on demand
        (600 MB at 4096 environments); nothing here reads it."""
        return self.part_pc.unsqueeze(0).repeat(self.num_envs, 1, 1, 1).reshape(-1, self.points_per_part, 3)

    def query_pc(self, pose_R, pose_T, out=None, sel=None, select='random', group_of=None, mask=False):
        """pose_R [b, m, 3, 3], pose_T [b, m, 3] (any b) -> [b, K, 3]; mask=True: [b, K, 4], the fourth column labels[part] of the
        point (pm_mesh_pc_query_labeled_f32), the first three the same bits; out then needs >= 4K columns.
        select='random' (the reference): the first num_points entries of torch.randperm(m p) from the CPU global generator, one
        subset for all environments (mesh2pc.py:63-64).  select='all': every point, K = m p.  select='fps': the posed cloud of all
        points is thinned to num_points per environment by farthest-point sampling (ops.fps, start index 0), so large parts are
        covered as densely as small ones.  sel: an int32 device tensor (K,) or (b, K) used instead (no host generator, no copy).
        out: None, or a 2-D float32 view (b, >= 3K) with unit inner stride (e.g. obs[:, :3K] of an observation buffer); the result
        is then a view of its first 3K columns.  `last_sel` holds the selection that was used (None for 'all').
        With groups=: 'random' draws group_sel() per call; 'all' gives K = pts_shared + max_group_points with NaN rows past an
        environment's own points; 'fps' is refused; sel keeps its meaning (rows of pts).  b = num_envs, or group_of= (b,) names the
        object of each row of this call."""
        Q = self.pts.shape[0]
        nf = 4 if mask else 3
        b, _ = ops.check_poses(pose_R, pose_T, self.part_num)
        if group_of is not None and not self.groups:
            raise ValueError("group_of: this cloud was built without groups=")
        if sel is not None:
            if sel.dtype != torch.int32 or sel.dim() not in (1, 2) or (sel.dim() == 2 and sel.shape[0] != b) or sel.shape[-1] == 0:
                raise ValueError(f"sel: expected an int32 tensor (K,) or ({b}, K), got {sel.dtype} {tuple(sel.shape)}")
            K = sel.shape[-1]
        elif select not in SELECT_MODES:
            raise ValueError(f"select: expected one of {SELECT_MODES}, got {select!r}")
        elif self.groups and select == 'fps':
            raise ValueError("select='fps': not available with groups= (the farthest-point kernel thins one cloud of a common size; "
                             "the environments' own clouds differ in size)")
        elif self.groups:
            K = self.pts_shared + self.max_group_points if select == 'all' else self.num_points
        else:
            K = Q if select == 'all' else min(self.num_points, Q)
        if out is not None:
            ops._out_rows(out, b, nf * K)                                                      # a bad view is reported before the device and any launch
        env = self._call_groups(b, group_of) if self.groups and sel is None else None          # ... and so is a slice without its group_of
        ops._req(pose_R, pose_T, sel, out, self.pts)
        pose_R, pose_T = pose_R.contiguous(), pose_T.contiguous()
        if sel is None and self.groups:
            sel = self.group_sel(group_of=group_of) if select == 'random' else self._all_sel(env[1])
        elif sel is None and select == 'random':
            randperm = torch.randperm(Q)
            sel = randperm[:self.num_points].to(torch.int32).to(self.device)
        elif sel is None and select == 'fps':
            if self.num_points > Q:
                raise ValueError(f"select='fps': num_points {self.num_points} exceeds the {Q} points of the scene")
            if self._full is None or self._full.shape[0] != b:
                self._full = torch.empty(b, Q * 3, dtype=torch.float32, device=pose_R.device)
                self._fps_ws = ops.Workspace(pose_R.device)
            ops.mesh_pc_query(self.pts, self.part_of, pose_R, pose_T, None, self._full)
            sel = ops.fps(self._full.view(b, Q, 3), self.num_points, self._fps_ws)
        res = ops.mesh_pc_query(self.pts, self.part_of, pose_R, pose_T, sel, out, labels=self.labels if mask else None)
        self.last_sel = sel
        return res[:, :nf * K].unflatten(1, (K, nf))
