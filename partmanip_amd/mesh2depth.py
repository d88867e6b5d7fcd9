"""Depth camera over the posed part meshes: the producer of the reference's four depth observations (`depth_pc`, `depth_tsdf`,
`depth_sparse`, `depth_img`, tasks/hand_base.py:312-343), which there comes from the simulator's camera sensors.

    cam = DepthFromMesh(num_envs, device, cam_pose (V, 4, 4), cam_intr (3, 3), im_h, im_w)     # register_camera's arguments
    depth = cam.render(pose_R (b, m, 3, 3), pose_T (b, m, 3))  -> (b, V, im_h, im_w)            # positive z-depth, misses at `far`
    frame = cam.render_frame(pose_R, pose_T)  -> .depth (b, V, im_h, im_w), .seg int32 (b, V, im_h, im_w), .rgb uint8 (b, V, im_h, im_w, 3)

The triangles of every rigid part (PCfromMesh's file list: eight Franka links, hand, two fingers, the object) are kept once on the
device; every step one call of pm_mesh_depth_render_f32 (csrc/mesh_depth.hip) puts them under their parts' poses -- the same
(pose_R, pose_T) that PCfromMesh.query_pc and TSDFfromMesh.query_tsdf take, as the task classes' end_step emits them -- and renders
them into every view.  With far = 100 the result is exactly the tensor hand_base.py:322-324 hands to TSDFVolume (the sensors'
negated depth with its infinities replaced by 100), so it feeds TSDFVolume.depth2pc, integrate and sparse_voxel unchanged, and
unlike the mesh cloud it holds only what a camera sees: hidden surfaces are not in it.

The image is defined bit for bit by a stated fp32 association (include/partmanip_hip.h), as the mesh cloud is.  Two choices are this
project's own and have not been checked against the simulator: `near` defaults to 0.01 (Isaac Gym's clip planes are not reproduced),
and culling is two-sided, both faces of a triangle count (for closed meshes the nearest hit is a front face either way).

render_frame (pm_mesh_frame_render_f32, csrc/mesh_frame.hip) keeps the winning triangle of every pixel as well and resolves it into
the same depth, a part label (the reference's IMAGE_SEGMENTATION, hand_base.py:222-227; `labels=[1] * 11 + [0]` gives its robot
mask, load_robot.py:83) and a shaded colour (the image hand_base.py:355-357 saves).  All three are defined bit for bit; the nearest
triangle wins a pixel, the smaller row of `faces` on a tie.  The shading -- a headlight along the optical axis over a fixed palette
-- is this project's choice, not Isaac Gym's renderer.  Sensor noise and `is_camera_rand` are out of scope.

A scene whose environments differ (open_drawer: every environment holds its own cabinet, env % num_objs):

    cam = DepthFromMesh(N, device, ..., meshes=robot_parts, groups=load_drawer_meshes(assets), group_of=envs.obj_id)

`meshes` are the parts every environment draws (slots 0 .. len(meshes) - 1); groups[k][j] is the mesh of body j of object k, or
None, and takes slot len(meshes) + j in whatever environment holds object k.  render / render_frame then take (N, part_num, ...)
poses with part_num = len(meshes) + the largest body count, and call the grouped entries (pm_mesh_depth_render_groups_f32,
pm_mesh_frame_render_groups_f32): an environment pays the triangle set-up of its own object only, not of the whole library.
Textures and materials are not read, and `is_camera_rand` stays out of scope.
"""
import collections

import numpy as np
import torch

from . import meshio, ops, scene_groups

# The default colours of the parts, cycled: twelve well-separated hues at moderate saturation (0..255).
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
           (210, 245, 60), (250, 190, 212), (0, 128, 128), (170, 110, 40))

Frame = collections.namedtuple("Frame", "depth seg rgb")


class DepthFromMesh:
    """cam_pose (V, 4, 4) camera->world (the camera looks along its +z axis, x to the right, y down), cam_intr (3, 3), im_h, im_w:
    exactly TSDFVolume.register_camera's arguments.  `meshes`: a list of (vertices, faces) used instead of the files under
    `asset_root` (assets/franka_description/meshes/visual/* and assets/objs/cube/cube.obj, read through meshio.load_mesh).
    near = 0.01 is this project's choice, not Isaac Gym's clip plane; both faces of a triangle are hit (two-sided).
    For render_frame: labels (M,) ints, the seg value of each part (None: the part index), miss_label the seg value where nothing
    is hit; palette (M, 3) colours in 0..255 (None: PALETTE, cycled); ambient in [0, 1], the share of a colour that a surface seen
    edge-on keeps; background, the colour where nothing is hit.
    groups: None, or one list per object of (vertices, faces)-or-None per body (tasks.open_drawer.load_drawer_meshes); group_of
    (num_envs,) ints in [-1, len(groups)): the object each environment holds, -1 for none (default: env % len(groups), the
    reference's rule).  Slots, labels and palette then cover part_num = len(meshes) + the largest body count; attributes: num_shared
    (the shared slots), face_shared, group_off (numpy), group_of (numpy), max_group_faces.  With groups, `meshes` may be empty."""

    def __init__(self, num_envs, device, cam_pose, cam_intr, im_h, im_w, asset_root='.', meshes=None, near=0.01, far=100.0,
                 labels=None, miss_label=-1, palette=None, ambient=0.25, background=(255, 255, 255), groups=None, group_of=None):
        self.num_envs = num_envs
        self.device = device
        self.asset_root = asset_root
        self.im_h, self.im_w = int(im_h), int(im_w)
        self.near, self.far = float(near), float(far)
        if self.im_h < 1 or self.im_w < 1:
            raise ValueError(f"image size: expected positive im_h and im_w, got {im_h} x {im_w}")
        if not (self.near > 0 and self.far > self.near):
            raise ValueError(f"clip planes: expected 0 < near < far, got near = {near}, far = {far}")
        pose = np.asarray(cam_pose.cpu().numpy() if torch.is_tensor(cam_pose) else cam_pose, dtype=np.float32)
        if pose.ndim != 3 or pose.shape[1:] != (4, 4) or pose.shape[0] == 0:
            raise ValueError(f"cam_pose: expected (V, 4, 4), got {pose.shape}")
        intr = np.asarray(cam_intr.cpu().numpy() if torch.is_tensor(cam_intr) else cam_intr, dtype=np.float64)
        if intr.shape != (3, 3):
            raise ValueError(f"cam_intr: expected (3, 3), got {intr.shape}")
        self.cam_intr = cam_intr
        self.fx, self.fy, self.cx, self.cy = float(intr[0, 0]), float(intr[1, 1]), float(intr[0, 2]), float(intr[1, 2])
        self.num_view = int(pose.shape[0])
        self.cam_pose = torch.from_numpy(np.ascontiguousarray(pose)).to(self.device)
        if meshes is None:
            meshes = [meshio.load_mesh(path) for path in meshio.scene_mesh_paths(asset_root)]
        if len(meshes) == 0 and not groups:
            raise ValueError("meshes: at least one part is needed")
        if group_of is not None and groups is None:
            raise ValueError("group_of: needs groups=")
        verts, part, faces, base = [], [], [], 0

        def add(mesh, slot, what, k=None, j=None):
            nonlocal base
            v, f = np.asarray(mesh[0], dtype=np.float32), np.asarray(mesh[1], dtype=np.int64)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or len(v) == 0 or len(f) == 0:
                raise ValueError(f"{what}: expected vertices (n > 0, 3) and faces (f > 0, 3), got {v.shape} and {f.shape}")
            if f.min() < 0 or f.max() >= len(v):
                raise ValueError(f"{what}: a face index lies outside [0, {len(v)})")
            verts.append(v)
            part.append(np.full(len(v), slot, dtype=np.int32))
            faces.append(f + base)
            base += len(v)
            return len(f)

        for i, mesh in enumerate(meshes):
            add(mesh, i, f"meshes[{i}]")
        self.num_shared = self.part_num = len(meshes)
        self.face_shared = sum(len(f) for f in faces)
        self.groups = groups is not None
        self._scene = None
        if self.groups:
            sg = self._scene = scene_groups.SceneGroups(num_envs, self.device, self.num_shared, groups, add, group_of)
            self.part_num, self.group_off, self.group_of, self.max_group_faces = sg.part_num, sg.group_off, sg.group_of, sg.most
            self._group_of = sg.group_of_dev
            if not verts:
                raise ValueError("meshes and groups: no mesh at all")
        self.verts = torch.from_numpy(np.ascontiguousarray(np.concatenate(verts))).to(self.device)               # (NV, 3)
        self.vert_part = torch.from_numpy(np.concatenate(part)).to(self.device)                                  # (NV,) int32
        self.faces = torch.from_numpy(np.ascontiguousarray(np.concatenate(faces).astype(np.int32))).to(self.device)   # (F, 3) int32
        m = self.part_num
        self.labels = None
        if labels is not None:
            lab = np.asarray(labels)
            if lab.shape != (m,) or lab.dtype.kind not in "iu":
                raise ValueError(f"labels: expected {m} integers, one per part, got {lab.dtype} {lab.shape}")
            self.labels = torch.from_numpy(lab.astype(np.int32)).to(self.device)
        self.miss_label = int(miss_label)
        pal = np.asarray([PALETTE[i % len(PALETTE)] for i in range(m)] if palette is None else palette, dtype=np.float32)
        if pal.shape != (m, 3) or not (np.isfinite(pal).all() and pal.min() >= 0 and pal.max() <= 255):
            raise ValueError(f"palette: expected ({m}, 3) values in [0, 255], got {pal.shape}")
        self.palette = torch.from_numpy(np.ascontiguousarray(pal)).to(self.device)
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError(f"ambient: expected a value in [0, 1], got {ambient}")
        self.ambient = float(np.float32(ambient))                                               # the two float32 values the kernel takes
        self.one_minus_ambient = float(np.float32(1) - np.float32(ambient))
        self.background = tuple(int(c) for c in background)
        if len(self.background) != 3 or min(self.background) < 0 or max(self.background) > 255:
            raise ValueError(f"background: expected three values in 0..255, got {background}")
        self._keys = ops.Workspace(self.device)                                                 # render_frame's 64-bit keys, grown on demand

    def _call_groups(self, b, group_of):
        """The (F_shared, group_off, env_group, max_group_faces) of a call over b environments; None without groups."""
        if self._scene is None:
            if group_of is not None:
                raise ValueError("group_of: this camera was built without groups=")
            return None
        return self.face_shared, self._scene.group_off_dev, self._scene.for_call(b, group_of), self.max_group_faces

    def render(self, pose_R, pose_T, out=None, group_of=None):
        """pose_R [b, m, 3, 3], pose_T [b, m, 3] (any b) -> [b, V, im_h, im_w] float32: the z-depth (not the ray length) of the
        nearest surface through every pixel centre, `far` where nothing is hit.
        out: None, or a 2-D float32 view (b, >= V h w) with unit inner stride (e.g. the head of a depth_img observation buffer); the
        result is then a view of its first V h w columns.  With groups=: b = num_envs, or group_of= (b,) names the object of each
        row of this call (frame_recorder's one-environment slice)."""
        b, _ = ops.check_poses(pose_R, pose_T, self.part_num)
        n = self.num_view * self.im_h * self.im_w
        if out is not None:
            ops._out_rows(out, b, n)                                                           # a bad view is reported before the device
        groups = self._call_groups(b, group_of)
        ops._req(pose_R, pose_T, out, self.verts)
        pose_R, pose_T = pose_R.contiguous(), pose_T.contiguous()
        res = ops.mesh_depth_render(self.verts, self.vert_part, self.faces, pose_R, pose_T, self.cam_pose, self.fx, self.fy, self.cx,
                                    self.cy, self.im_h, self.im_w, self.near, self.far, out, groups=groups)
        return res[:, :n].unflatten(1, (self.num_view, self.im_h, self.im_w))

    def render_frame(self, pose_R, pose_T, depth=True, seg=True, rgb=True, out_depth=None, group_of=None):
        """pose_R [b, m, 3, 3], pose_T [b, m, 3] (any b) -> Frame(depth, seg, rgb) from one rasterisation, each None when switched off:
        depth [b, V, im_h, im_w] float32, the bits render() gives; seg [b, V, im_h, im_w] int32, labels[part] of the nearest
        triangle (the smaller row of `faces` on a tie), miss_label where nothing is hit; rgb [b, V, im_h, im_w, 3] uint8, the part's
        palette colour times ambient + (1 - ambient) |n.z| with n the triangle's unit normal in camera space, `background`
        where nothing is hit.  out_depth: as render()'s out.  The keys' workspace (8 b V im_h im_w bytes) belongs to this object and
        is reused while b fits.  group_of: as render()'s."""
        b, _ = ops.check_poses(pose_R, pose_T, self.part_num)
        groups = self._call_groups(b, group_of)
        if not (depth or seg or rgb):
            raise ValueError("render_frame: depth, seg and rgb are all switched off")
        if out_depth is not None and not depth:
            raise ValueError("render_frame: out_depth given with depth switched off")
        V, h, w = self.num_view, self.im_h, self.im_w
        n = V * h * w
        if out_depth is not None:
            ops._out_rows(out_depth, b, n)                                                     # a bad view is reported before the device
        ops._req(pose_R, pose_T, out_depth, self.verts)
        pose_R, pose_T = pose_R.contiguous(), pose_T.contiguous()
        d, s, c = ops.mesh_frame_render(self.verts, self.vert_part, self.faces, pose_R, pose_T, self.cam_pose, self.fx, self.fy, self.cx,
                                        self.cy, h, w, self.near, self.far, self._keys.get(8 * b * n), part_label=self.labels,
                                        miss_label=self.miss_label, palette=self.palette if rgb else None, ambient=self.ambient,
                                        one_minus_ambient=self.one_minus_ambient, background=self.background,
                                        depth=(True if out_depth is None else out_depth) if depth else False, seg=bool(seg),
                                        rgb=bool(rgb), groups=groups)
        return Frame(None if d is None else d[:, :n].unflatten(1, (V, h, w)), None if s is None else s.unflatten(1, (V, h, w)),
                     None if c is None else c.unflatten(1, (V, h, w, 3)))
