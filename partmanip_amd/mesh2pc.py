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
"""
import numpy as np
import torch

from . import meshio, ops

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
    torch.Generator().manual_seed(seed + i), so the two fingers, one file loaded twice, get different points as in the reference)."""

    def __init__(self, num_envs, device, num_points=1024, asset_root='.', meshes=None, part_pcs=None, seed=0):
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
            if len(meshes) == 0:
                raise ValueError("meshes: at least one part is needed")
            pcs = np.stack([self.load_pc_from_mesh(v, f, i) for i, (v, f) in enumerate(meshes)])
        self.part_num, self.points_per_part = int(pcs.shape[0]), int(pcs.shape[1])
        self.part_pc = torch.from_numpy(pcs).to(self.device)                                   # (m, p, 3)
        self.pts = self.part_pc.view(-1, 3)                                                    # (m p, 3), the same memory
        self.part_of = torch.arange(self.part_num, dtype=torch.int32).repeat_interleave(self.points_per_part).to(self.device)
        self.last_sel = None
        self._full = None                                                                      # scratch of select='fps'
        self._fps_ws = None

    def load_pc_from_mesh(self, vertices, faces, index=0):
        """`num_points` surface points of one part (mesh2pc.py:32-41) as float32 (p, 3), seeded with seed + index."""
        g = torch.Generator().manual_seed(self.seed + index)
        return meshio.sample_surface(vertices, faces, self.num_points, g)[0]

    @property
    def all_pc(self):
        """The reference's attribute (mesh2pc.py:27-28): the part clouds repeated per environment, (b m, p, 3).  Built on demand
        (600 MB at 4096 environments); nothing here reads it."""
        return self.part_pc.unsqueeze(0).repeat(self.num_envs, 1, 1, 1).reshape(-1, self.points_per_part, 3)

    def query_pc(self, pose_R, pose_T, out=None, sel=None, select='random'):
        """pose_R [b, m, 3, 3], pose_T [b, m, 3] (any b) -> [b, K, 3].
        select='random' (the reference): the first num_points entries of torch.randperm(m p) from the CPU global generator, one
        subset for all environments (mesh2pc.py:63-64).  select='all': every point, K = m p.  select='fps': the posed cloud of all
        points is thinned to num_points per environment by farthest-point sampling (ops.fps, start index 0), so large parts are
        covered as densely as small ones.  sel: an int32 device tensor (K,) or (b, K) used instead (no host generator, no copy).
        out: None, or a 2-D float32 view (b, >= 3K) with unit inner stride (e.g. obs[:, :3K] of an observation buffer); the result
        is then a view of its first 3K columns.  `last_sel` holds the selection that was used (None for 'all')."""
        Q = self.pts.shape[0]
        b, _ = ops.check_poses(pose_R, pose_T, self.part_num)
        if sel is not None:
            if sel.dtype != torch.int32 or sel.dim() not in (1, 2) or (sel.dim() == 2 and sel.shape[0] != b) or sel.shape[-1] == 0:
                raise ValueError(f"sel: expected an int32 tensor (K,) or ({b}, K), got {sel.dtype} {tuple(sel.shape)}")
            K = sel.shape[-1]
        elif select not in SELECT_MODES:
            raise ValueError(f"select: expected one of {SELECT_MODES}, got {select!r}")
        else:
            K = Q if select == 'all' else min(self.num_points, Q)
        if out is not None:
            ops._out_rows(out, b, 3 * K)                                                       # a bad view is reported before the device and any launch
        ops._req(pose_R, pose_T, sel, out, self.pts)
        pose_R, pose_T = pose_R.contiguous(), pose_T.contiguous()
        if sel is None and select == 'random':
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
        res = ops.mesh_pc_query(self.pts, self.part_of, pose_R, pose_T, sel, out)
        self.last_sel = sel
        return res[:, :3 * K].unflatten(1, (K, 3))
