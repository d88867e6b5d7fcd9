"""The 'mesh_tsdf' observation (`obs_mode: 'mesh_tsdf'` of cfg/algos/dagger_tsdf.yaml and bc.yaml), mirroring the reference's
`utils/mesh2sdf.py:TSDFfromMesh` for the part that runs every environment step:

    tsdf = TSDFfromMesh(num_envs, size, resolution, device, vox_origin=...)        # mesh2sdf.py:16-54
    vol = tsdf.query_tsdf(pose_R (b, m, 3, 3), pose_T (b, m, 3))  -> (b, res, res, res)   # mesh2sdf.py:89-93, 119-139
    scene, obj = tsdf.query_tsdf_seperately(pose_R, pose_T)                               # mesh2sdf.py:95-117

The pre-baked signed-distance grid of every rigid part (eight Franka links, hand, two fingers, the object) is sampled
trilinearly at each workspace voxel under the part's pose; the minimum over the parts and the ground plane, divided by the
truncation distance and clamped to [-1, 1], is the volume.  One launch of pm_mesh_tsdf_query_f32 (csrc/mesh_tsdf.hip) does
that: the reference's (b, m, n, 3) / (b, m, n) intermediates (6 MB per environment each) never exist, and with `out=` the
volume is written straight into the left part of an (N, res^3 + proprio) observation buffer (the reference reshapes and
concatenates, tasks/grasp_cube.py:131,137).

The grids are NOT padded to a common shape (mesh2sdf.py:181-184 pads with 1s that are never read: validity is tested against
each part's own shape): `merge_sdf_field` keeps one flat buffer of concatenated grids and per-part tables of offset, shape,
bbox_min and voxel_size.

Baking a grid from a mesh (mesh2sdf.py:201-237; kaolin and ManifoldPlus there, neither of which exists for ROCm) is done by
pm_mesh_sdf_bake_f32 (csrc/mesh_bake.hip) when the object is built with `bake=True`: `mesh2sdf(mesh_path)` returns the reference's
dict, and `load_sdf` of an absent file bakes the mesh, saves the dict at the reference's path and goes on.  The grid layout is
the reference's fp32 expressions (`bake_grid_layout`); the magnitude is the exact point-to-triangle distance; the sign is the
generalised winding number (|w| >= 0.5 is inside), which equals kaolin's ray parity on a closed mesh and needs no manifold
pre-pass on an open one.  Without `bake=True` an absent grid raises as before.  Marching cubes, ManifoldPlus itself
and the debug dumps stay outside this build's scope: they raise NotImplementedError.

A scene whose environments differ (open_drawer: every environment holds its own cabinet, env % num_objs):

    groups = bake_groups(device, load_drawer_meshes(assets), trunc, voxel_size)
    tsdf = TSDFfromMesh(N, size, res, device, sdf_dicts=robot_grids, groups=groups, group_of=envs.obj_id)

The shared grids keep slots 0 .. S - 1; groups[k][j] is the grid dict of body j of object k, or None, and is placed by slot S + j in
whatever environment holds object k.  query_tsdf then takes (N, part_num, ...) poses with part_num = S + the largest body count --
the table make_open_drawer_env(scene_meshes=) hands its observers -- and is one launch of pm_mesh_tsdf_query_groups_f32: an
environment samples its own cabinet's grids only, and the NaN poses past its body count are never looked at.

Beyond the reference: query_points(points, pose_R, pose_T, carrier=...) samples the same grids at arbitrary posed points and returns
metres (pm_mesh_sdf_points_f32, csrc/mesh_sdf_points.hip; the per-part arithmetic is shared with the kernel above through
csrc/mesh_sdf_sample.h).  contact.py builds the contact sensor on it.
"""
import hashlib
import os

import numpy as np
import torch

from . import meshio, ops, scene_groups

OBJ_SDF_PATH = os.path.join("assets", "objs", "cube", "sdf.npy")                     # mesh2sdf.py:48


def bake_grid_layout(vertices, trunc, voxel_size):
    """Shape, centre and bbox_min of the bake grid of a mesh, with the reference's own fp32 tensor expressions (mesh2sdf.py:213-223),
    evaluated on the CPU: vertices (V, 3) -> ((X, Y, Z) ints, centre (3,) float32 tensor, bbox_min (3,) float32 tensor).
    Voxel (i, j, k) sits at (idx - shape // 2) * voxel_size + centre; bbox_min is voxel (0, 0, 0)."""
    v = torch.as_tensor(np.asarray(vertices, dtype=np.float32)).reshape(1, -1, 3)
    obj_center = (v.max(dim=1)[0] + v.min(dim=1)[0]) / 2
    max_range = v.max(dim=1)[0] - v.min(dim=1)[0] + 2 * trunc
    volume_shape = torch.ceil(max_range / voxel_size)
    shape = (int(volume_shape[0, 0]), int(volume_shape[0, 1]), int(volume_shape[0, 2]))
    bbox_min = ((torch.zeros(1, 3, dtype=torch.long) - volume_shape // 2) * voxel_size + obj_center)[0]
    return shape, obj_center[0], bbox_min


def bake_mesh(device, trunc, voxel_size, mesh_path=None, vertices=None, faces=None, tri_cull=True):
    """The bake behind TSDFfromMesh.mesh2sdf: a mesh file, or vertices (V, 3) + faces (F, 3) -> the reference's dict."""
    if mesh_path is not None:
        vertices, faces = meshio.load_mesh(mesh_path)
    vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = meshio.drop_double_corner_faces(vertices, np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    if len(faces) == 0:
        raise ValueError(f"{mesh_path or 'mesh'}: no triangle is left to bake")
    shape, centre, bbox_min = bake_grid_layout(vertices, trunc, voxel_size)
    tri = torch.from_numpy(vertices[faces]).to(device)                              # (F, 3, 3)
    sdf = ops.mesh_sdf_bake(tri, shape, voxel_size, centre.tolist(), trunc, tri_cull)
    return {'sdf': sdf.cpu().numpy(), 'bbox_min': bbox_min.numpy(), 'voxel_size': voxel_size}


def _fitting_voxel_size(vertices, trunc, voxel_size):
    """The smallest voxel size, found by growing `voxel_size` in steps of 1 %, whose bake grid has fewer than 2^31 cells."""
    vs = float(voxel_size)
    while int(np.prod(np.asarray(bake_grid_layout(vertices, trunc, vs)[0], dtype=np.float64))) >= 2 ** 31:
        vs *= 1.01
    return vs


def bake_groups(device, meshes, trunc, voxel_size, cache_dir=None):
    """tasks.open_drawer.load_drawer_meshes(assets) -- one list per object of (vertices, faces)-or-None per body -- baked into the
    `groups` of TSDFfromMesh: one grid dict per body (bake_mesh), None where the body has no mesh.  cache_dir: None, or a folder
    where every baked dict is kept as <digest>.npy (np.save of the dict, as load_sdf keeps the robot's), the digest being the SHA-256
    of the mesh's float32 vertices, int64 faces, trunc and voxel_size; a file that is there is loaded instead of baking.
    A body whose grid would hold 2^31 cells or more is refused with the voxel size that would fit, before anything is baked."""
    meshes = [list(bodies) for bodies in meshes]
    for k, bodies in enumerate(meshes):
        for j, mesh in enumerate(bodies):
            if mesh is None:
                continue
            v = np.ascontiguousarray(mesh[0], dtype=np.float32).reshape(-1, 3)
            shape = bake_grid_layout(v, trunc, voxel_size)[0]
            if int(np.prod(np.asarray(shape, dtype=np.float64))) >= 2 ** 31:
                raise ValueError(f"groups[{k}][{j}]: the grid of body {j} of object {k} would be {shape} = {np.prod(np.asarray(shape, dtype=np.float64)):.3g} "
                                 f"cells at voxel_size {voxel_size} (the limit is 2^31); a voxel_size of "
                                 f"{_fitting_voxel_size(v, trunc, voxel_size):.4g} or more fits")
    if cache_dir is not None:
        os.makedirs(cache_dir, exist_ok=True)
    groups = []
    for bodies in meshes:
        out = []
        for mesh in bodies:
            if mesh is None:
                out.append(None)
                continue
            v = np.ascontiguousarray(mesh[0], dtype=np.float32).reshape(-1, 3)
            f = np.ascontiguousarray(mesh[1], dtype=np.int64).reshape(-1, 3)
            path = None
            if cache_dir is not None:
                h = hashlib.sha256()
                for piece in (np.asarray(v.shape, dtype=np.int64), v, np.asarray(f.shape, dtype=np.int64), f,
                              np.asarray([trunc, voxel_size], dtype=np.float64)):
                    h.update(piece.tobytes())
                path = os.path.join(cache_dir, h.hexdigest() + ".npy")
            if path is not None and os.path.exists(path):
                out.append(np.load(path, allow_pickle=True).item())
                continue
            d = bake_mesh(device, trunc, voxel_size, vertices=v, faces=f)
            if path is not None:
                np.save(path, d)
            out.append(d)
        groups.append(out)
    return groups


class TSDFfromMesh:
    """Constructor of the reference plus three keyword extensions: `bake` (bake absent grids from their meshes on the GPU, module
    docstring; default False = an absent grid is an error), `sdf_dicts` (a list of {'sdf': (X,Y,Z) float32, 'bbox_min':
    (3,), 'voxel_size': float} used instead of reading the pre-stored files) and `asset_root` (prefix of the reference's relative
    paths assets/franka_description/sdf/visual/*.npy and assets/objs/cube/sdf.npy).  `vox_origin` may be None, a tensor or the
    yaml's list (the reference raises TypeError on a list, tasks/hand_base.py passes one).
    `parallel=False` is served by the same kernel: the reference's own naive path (query_tsdf_naive ->
    triplet_interpolation_query) indexes a 3-D field with a flat index and cannot run; the parallel path is the specification.
    groups: None, or one list per object of grid dict-or-None per body (bake_groups); group_of (num_envs,) ints in [-1, len(groups)):
    the object each environment holds, -1 for none (default: env % len(groups), the reference's rule).  part_num is then num_shared
    + the largest body count; attributes: num_shared, grid_slot, group_off (numpy), group_of (numpy), max_group_grids."""

    def __init__(self, num_envs, size, resolution, device, parallel=True, debug=False, vox_origin=None, sdf_dicts=None,
                 asset_root='.', bake=False, groups=None, group_of=None):
        if debug:
            raise NotImplementedError("debug dumps (surface points / marching cubes) are outside this build's scope (DESIGN.md)")
        self.num_envs = num_envs
        self.parallel = parallel
        self.device = device
        self.debug = debug
        self.asset_root = asset_root
        self.bake = bake

        self.resolution = resolution
        self.size = size
        self.vox_size = self.size / self.resolution
        self.sdf_trunc = 4 * self.vox_size
        if vox_origin is None:
            self.vox_origin = torch.tensor([-0.25, -0.25, -0.0503], device=self.device)
        else:
            self.vox_origin = torch.as_tensor(vox_origin, dtype=torch.float32).to(self.device)
        self._origin3 = [float(v) for v in self.vox_origin.cpu().tolist()]          # host copy: no device read per query

        # queried points of the workspace, with the reference's own tensor expressions (mesh2sdf.py:29-37)
        tmp = torch.arange(0, self.resolution)
        xv, yv, zv = torch.meshgrid(tmp, tmp, tmp, indexing="ij")
        vox_coords = torch.stack([xv.flatten(), yv.flatten(), zv.flatten()], dim=1).long().to(self.device)
        self.vox_coords = vox_coords * self.vox_size + self.vox_origin             # [n, 3]
        self.point_num = self.vox_coords.shape[0]
        # the ground plane: the voxel's world z.  The reference repeats it per environment (2 GB at 4096); same shape and
        # values here, as a broadcast view of one row (the kernel takes the row)
        self._ground = self.vox_coords[:, -1].contiguous()
        self.init_tsdf = self._ground.unsqueeze(0).expand(self.num_envs, -1)       # [b, n]
        self.ground_tsdf = self._ground.unsqueeze(0).expand(self.num_envs, -1)     # [b, n]
        self._init_base = self._ground                                             # (n,) or, after initialize_sdf, (b, n)

        self.pre_store_sdf_trunc = self.sdf_trunc
        self.pre_store_sdf_voxel_size = 0.002
        self.sdf_dict_list = []
        if sdf_dicts is not None:
            self.sdf_dict_list.extend(sdf_dicts)
        else:
            self.load_franka(os.path.join(asset_root, "assets", "franka_description"))
            self.load_sdf(os.path.join(asset_root, OBJ_SDF_PATH), os.path.join(asset_root, meshio.OBJ_MESH_PATH))
        if group_of is not None and groups is None:
            raise ValueError("group_of: needs groups=")
        self.groups = groups is not None
        self._group_dicts = []
        self._scene = None
        self._point_layouts = {}                              # query_points: (id(carrier), id(segments), NP) -> layout
        if self.groups:
            slot = list(range(len(self.sdf_dict_list)))

            def add(d, s, what, k, j):
                if not isinstance(d, dict) or not {'sdf', 'bbox_min', 'voxel_size'} <= set(d):
                    raise ValueError(f"{what}: expected a dict with 'sdf', 'bbox_min' and 'voxel_size', or None")
                self._group_dicts.append(d)
                slot.append(s)
                return 1

            sg = self._scene = scene_groups.SceneGroups(num_envs, self.device, len(slot), groups, add, group_of)
            if not slot:
                raise ValueError("sdf_dicts and groups: no grid at all")
            self.grid_slot = np.asarray(slot, dtype=np.int32)
            self._grid_slot = torch.from_numpy(self.grid_slot).to(self.device)
            self.num_shared, self.group_off, self.group_of, self.max_group_grids = sg.num_shared, sg.group_off, sg.group_of, sg.most
            self._group_of = sg.group_of_dev
        self.merge_sdf_field()
        if self.groups:
            self.part_num = sg.part_num                                              # pose slots, not merge_sdf_field's library rows

    # ------------------------------------------------------------------------------------------------ loading
    def load_franka(self, hand_base_path):
        """Parts in the reference's order: link0..link7, hand, finger, finger (mesh2sdf.py:141-156); the mesh of a part is
        meshes/visual/<name>, its grid the same path with 'meshes' -> 'sdf' and the extension -> '.npy'."""
        for name in meshio.FRANKA_MESHES:
            mesh_path = os.path.join(hand_base_path, "meshes", "visual", name)
            preprocess_path = os.path.join(hand_base_path, "manifoldplus", "visual", name) if name.endswith(".obj") else None
            sdf_path = os.path.join(hand_base_path, "sdf", "visual", name[:-4] + ".npy")
            self.load_sdf(sdf_path, mesh_path, preprocess_path)

    def load_sdf(self, sdf_path, mesh_path=None, preprocess_path=None):
        """Pre-stored grid -> appended to `sdf_dict_list` (mesh2sdf.py:70-73, 82).  An absent file is baked from `mesh_path`, saved
        at `sdf_path` and appended (mesh2sdf.py:74-82) if the object was built with bake=True, else an error.  `preprocess_path`
        (the reference's ManifoldPlus output) is accepted and ignored: the winding-number sign needs no manifold pre-pass."""
        if os.path.exists(sdf_path):
            sdf_dict = np.load(sdf_path, allow_pickle=True).item()
        elif not self.bake:
            raise NotImplementedError(f"{sdf_path} is missing: the reference bakes it from the mesh with kaolin (mesh2sdf.py:201-237); "
                                      "here pass bake=True to bake it on the GPU (pm_mesh_sdf_bake_f32), or pass the file")
        else:
            if mesh_path is None:
                raise ValueError(f"{sdf_path} is missing and no mesh path was given to bake it from")
            sdf_dict = self.mesh2sdf(mesh_path)
            os.makedirs(os.path.dirname(os.path.abspath(sdf_path)), exist_ok=True)
            np.save(sdf_path, sdf_dict)
        self.sdf_dict_list.append(sdf_dict)

    def mesh2sdf(self, mesh_path=None, vertices=None, faces=None, tri_cull=True):
        """The reference's bake (mesh2sdf.py:201-237) of a mesh file, or of `vertices` (V, 3) + `faces` (F, 3), on the GPU:
        {'sdf': float32 (X, Y, Z), 'bbox_min': float32 (3,), 'voxel_size': pre_store_sdf_voxel_size}."""
        if not self.bake:
            raise NotImplementedError("baking a signed-distance grid from a mesh (kaolin in the reference) is off: build the object "
                                      "with bake=True to bake on the GPU (pm_mesh_sdf_bake_f32)")
        return bake_mesh(self.device, self.pre_store_sdf_trunc, self.pre_store_sdf_voxel_size, mesh_path, vertices, faces, tri_cull)

    def preprocess_mesh(self, input_mesh_path, output_mesh_path):
        raise NotImplementedError("ManifoldPlus preprocessing is outside this build's scope (DESIGN.md)")

    def visualize(self, sdf_field, voxel_size, bbox_min, save_path):
        raise NotImplementedError("marching cubes is outside this build's scope (DESIGN.md)")

    def extract_surface_points_from_volume(self, vol, save_path):
        raise NotImplementedError("debug dumps are outside this build's scope (DESIGN.md)")

    def merge_sdf_field(self):
        """One flat buffer of the concatenated (un-padded) grids + per-part tables, on `device`:
        sdf_field (sum X*Y*Z), sdf_field_off (m) int64, sdf_field_res (m, 3) int32, sdf_bbox_min (m, 3), sdf_voxel_size (m)."""
        dicts = self.sdf_dict_list + self._group_dicts       # the shared grids, then every object's (the rows of the grid library)
        self.part_num = len(dicts)
        grids = [np.ascontiguousarray(d['sdf'], dtype=np.float32) for d in dicts]
        for g in grids:
            if g.ndim != 3 or g.size >= 2 ** 31:
                raise ValueError(f"a part's 'sdf' must be a 3-D grid of fewer than 2^31 cells, got shape {g.shape}")
        sizes = np.array([g.size for g in grids], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.sdf_field = torch.from_numpy(np.concatenate([g.reshape(-1) for g in grids])).to(self.device)
        self.sdf_field_off = torch.from_numpy(off).to(self.device)
        self.sdf_field_res = torch.tensor([list(g.shape) for g in grids], dtype=torch.int32).to(self.device)
        self.sdf_bbox_min = torch.tensor(np.stack([np.asarray(d['bbox_min'], dtype=np.float32).reshape(3) for d in dicts]),
                                         dtype=torch.float32).to(self.device)
        self.sdf_voxel_size = torch.tensor([float(d['voxel_size']) for d in dicts], dtype=torch.float32).to(self.device)

    # ------------------------------------------------------------------------------------------------ queries
    def initialize_sdf(self, nerf_pred_tsdf):
        """pred_tsdf [b, n] in truncation units replaces the ground plane as the scene's base field (mesh2sdf.py:57-61)."""
        self.init_tsdf = torch.as_tensor(nerf_pred_tsdf, dtype=torch.float32).to(self.device) * self.sdf_trunc
        self._init_base = self.init_tsdf.reshape(self.num_envs, self.point_num).contiguous()

    def _row_range(self):
        """(s, e) of a query: it covers rows [0, e), of which [0, s) are the scene's and [s, e) the object's -- the parts, or with
        groups the ordinals of an environment's own rows (the shared ones, then its group's)."""
        if self.groups:
            return self.num_shared, self.num_shared + self.max_group_grids
        return self.part_num - 1, self.part_num

    def _query(self, pose_R, pose_T, p0, p1, base, out, brick_skip=True, group_of=None):
        """Rows [p0, p1) of _row_range against `base`."""
        eg = None
        if self.groups:
            eg = self._scene.for_call(ops.check_poses(pose_R, pose_T, self.part_num)[0], group_of)
        elif group_of is not None:
            raise ValueError("group_of: this object was built without groups=")
        pose_R = pose_R.to(torch.float32).reshape(-1, self.part_num, 3, 3).contiguous()
        pose_T = pose_T.to(torch.float32).reshape(-1, self.part_num, 3).contiguous()
        n = self.point_num
        if base.dim() == 2 and base.shape[0] != pose_R.shape[0]:
            raise ValueError(f"initialize_sdf was given {base.shape[0]} environments, the poses have {pose_R.shape[0]}")
        if eg is not None:
            res = ops.mesh_tsdf_query_groups(self.sdf_field, self.sdf_field_off, self.sdf_field_res, self.sdf_bbox_min,
                                             self.sdf_voxel_size, self._grid_slot, self.num_shared, self._scene.group_off_dev, eg, pose_R,
                                             pose_T, self.resolution, self.vox_size, self._origin3, self.sdf_trunc, base, p0, p1, out,
                                             brick_skip, max_group_grids=self.max_group_grids)
        else:
            res = ops.mesh_tsdf_query(self.sdf_field, self.sdf_field_off, self.sdf_field_res, self.sdf_bbox_min, self.sdf_voxel_size,
                                      pose_R, pose_T, self.resolution, self.vox_size, self._origin3, self.sdf_trunc, base,
                                      p0, p1, out, brick_skip)
        r = self.resolution
        return res[:, :n].unflatten(1, (r, r, r))

    def query_tsdf(self, pose_R, pose_T, out=None, brick_skip=True, group_of=None):
        """pose_R [b, m, 3, 3], pose_T [b, m, 3] -> [b, res, res, res].  out: None, or a 2-D float32 view (b, >= res^3) with
        unit inner stride (e.g. obs[:, :res^3] of an observation buffer); the result is then a view of its first res^3 columns.
        brick_skip=False turns the brick-level part rejection off (same bits, slower; for tests).  With groups=: one launch of the
        grouped entry; b = num_envs, or group_of= (b,) names the object of each row of this call."""
        return self._query(pose_R, pose_T, 0, self._row_range()[1], self._init_base, out, brick_skip, group_of)

    query_tsdf_parallel = query_tsdf
    query_tsdf_naive = query_tsdf          # the reference's naive path cannot run (class docstring); same kernel

    # ------------------------------------------------------------------------------------------------ posed points (contact.py)
    def _point_tables(self, pose_R, pose_T, group_of=None):
        """What a point query over this object's tables takes: (the five part tables, pose_R, pose_T as contiguous float32, the group
        keywords of ops.mesh_sdf_points -- empty without groups=)."""
        eg = None
        if self.groups:
            eg = self._scene.for_call(ops.check_poses(pose_R, pose_T, self.part_num)[0], group_of)
        elif group_of is not None:
            raise ValueError("group_of: this object was built without groups=")
        pose_R = pose_R.to(torch.float32).reshape(-1, self.part_num, 3, 3).contiguous()
        pose_T = pose_T.to(torch.float32).reshape(-1, self.part_num, 3).contiguous()
        tables = (self.sdf_field, self.sdf_field_off, self.sdf_field_res, self.sdf_bbox_min, self.sdf_voxel_size)
        kw = {}
        if eg is not None:
            kw = dict(grid_slot=self._grid_slot, NG_shared=self.num_shared, group_off=self._scene.group_off_dev, env_group=eg,
                      max_group_grids=self.max_group_grids)
        return tables, pose_R, pose_T, kw

    def _sdf_points(self, pose_R, pose_T, pts, carrier, p0, p1, group_of=None, **kw):
        """ops.mesh_sdf_points over this object's tables, ordinals [p0, p1) of _row_range: the grouped entry with groups=."""
        tables, pose_R, pose_T, groups = self._point_tables(pose_R, pose_T, group_of)
        return ops.mesh_sdf_points(*tables, pose_R, pose_T, pts, carrier, p0, p1, **kw, **groups)

    def query_points(self, points, pose_R, pose_T, carrier=None, parts=None, group_of=None, segments=None, return_arg=False,
                     cull=True):
        """The signed distance, in metres, of posed points to the part grids (one launch of pm_mesh_sdf_points_f32, with groups= of
        the grouped entry): points (NP, 3) shared by all environments or (b, NP, 3); carrier: None (the points are in the world frame)
        or (NP,) integers, the pose slot whose body carries each point (-1: world); parts (lo, hi): the ordinals sensed against
        (default all: the parts, or with groups= an environment's own rows); segments: None or a list of point counts that sum to NP.
        Returns dist (b, NP) -- the minimum over the ordinals of the trilinear sample, 1.0 where no grid's valid box holds the point;
        a distance only within the grids' truncation band -- then, when asked for, arg (b, NP) int32 (the ordinal that attains it, -1
        for none) and (seg_min (b, NS), seg_arg (b, NS) int32: each segment's minimum and the index of the point that attains it).
        Points whose carriers are not sorted are sorted for the kernel and the results come back in the caller's order; that layout is
        built once per (carrier, segments) pair of objects and kept (a list changed in place afterwards is not noticed)."""
        from .contact import PointLayout, chunk_spheres
        points = torch.as_tensor(points, dtype=torch.float32)
        if points.dim() not in (2, 3) or points.shape[-1] != 3 or points.shape[-2] == 0:
            raise ValueError(f"points: expected (NP > 0, 3) or (b, NP, 3), got {tuple(points.shape)}")
        NP = int(points.shape[-2])
        top = self._row_range()[1]
        lo, hi = (0, top) if parts is None else (int(v) for v in parts)
        if not 0 <= lo < hi <= top:
            raise ValueError(f"parts: expected a non-empty ordinal range inside [0, {top}), got ({lo}, {hi})")
        key = (id(carrier), id(segments), NP)
        hit = self._point_layouts.get(key)
        if hit is None or hit[0] is not carrier or hit[1] is not segments:
            if carrier is not None:
                c = np.asarray(carrier.cpu().numpy() if torch.is_tensor(carrier) else carrier)
                if c.shape != (NP,) or c.dtype.kind not in "iu" or c.min() < -1 or c.max() >= self.part_num:
                    raise ValueError(f"carrier: expected {NP} pose slots in [-1, {self.part_num}), got {c.dtype} {c.shape}")
            lay = PointLayout(NP, carrier, segments)
            if len(self._point_layouts) >= 8:
                self._point_layouts.pop(next(iter(self._point_layouts)))
            hit = self._point_layouts[key] = (carrier, segments, lay, lay.on(self.device))
        lay, (src, pt_id, car, seg_off, pos) = hit[2], hit[3]
        points = points.to(self.device)
        pts = (points if lay.identity else points.index_select(-2, src)).contiguous()
        sphere = chunk_spheres(pts) if cull and pts.dim() == 2 else None         # per-environment points are not culled
        d, a, sm, sa = self._sdf_points(pose_R, pose_T, pts, car, lo, hi, group_of, pt_id=pt_id, chunk_sphere=sphere, seg_off=seg_off,
                                        want_arg=return_arg, cull=cull)
        if not lay.identity:
            d, a = d.index_select(1, pos), None if a is None else a.index_select(1, pos)
        out = (d,) + ((a,) if return_arg else ()) + (((sm, sa),) if segments is not None else ())
        return out[0] if len(out) == 1 else out

    def query_tsdf_seperately(self, pose_R, pose_T, out_scene=None, out_obj=None, group_of=None):
        """(scene, obj): the parts before the last against the base field, and the last part (the object) alone against the
        ground plane (mesh2sdf.py:95-117); min(scene, obj) == query_tsdf bit for bit.  Two launches over part ranges.
        With groups=: (the shared rows against the base field, the environment's own rows against the ground plane).  The equality
        holds while the base field is the ground plane, as in the reference (after initialize_sdf the object's volume still carries
        the ground)."""
        s, e = self._row_range()
        if self.groups and (s == 0 or e == s):
            raise ValueError("query_tsdf_seperately: needs at least one shared grid and one grid in a group")
        group_of = group_of if self.groups else None                                 # without groups it has always been ignored here
        scene = self._query(pose_R, pose_T, 0, s, self._init_base, out_scene, group_of=group_of)
        obj = self._query(pose_R, pose_T, s, e, self._ground, out_obj, group_of=group_of)
        return scene, obj
