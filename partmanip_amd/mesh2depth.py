"""Depth camera over the posed part meshes: the producer of the reference's four depth observations (`depth_pc`, `depth_tsdf`,
`depth_sparse`, `depth_img`, tasks/hand_base.py:312-343), which there comes from the simulator's camera sensors.

    cam = DepthFromMesh(num_envs, device, cam_pose (V, 4, 4), cam_intr (3, 3), im_h, im_w)     # register_camera's arguments
    depth = cam.render(pose_R (b, m, 3, 3), pose_T (b, m, 3))  -> (b, V, im_h, im_w)            # positive z-depth, misses at `far`

The triangles of every rigid part (PCfromMesh's file list: eight Franka links, hand, two fingers, the object) are kept once on the
device; every step one call of pm_mesh_depth_render_f32 (csrc/mesh_depth.hip) puts them under their parts' poses -- the same
(pose_R, pose_T) that PCfromMesh.query_pc and TSDFfromMesh.query_tsdf take, as the task classes' end_step emits them -- and renders
them into every view.  With far = 100 the result is exactly the tensor hand_base.py:322-324 hands to TSDFVolume (the sensors'
negated depth with its infinities replaced by 100), so it feeds TSDFVolume.depth2pc, integrate and sparse_voxel unchanged, and
unlike the mesh cloud it holds only what a camera sees: hidden surfaces are not in it.

The image is defined bit for bit by a stated fp32 association (include/partmanip_hip.h), as the mesh cloud is.  Two choices are this
project's own and have not been checked against the simulator: `near` defaults to 0.01 (Isaac Gym's clip planes are not reproduced),
and culling is two-sided, both faces of a triangle count (for closed meshes the nearest hit is a front face either way).  Colour,
segmentation masks and sensor noise are out of scope.
"""
import numpy as np
import torch

from . import meshio, ops


class DepthFromMesh:
    """cam_pose (V, 4, 4) camera->world (the camera looks along its +z axis, x to the right, y down), cam_intr (3, 3), im_h, im_w:
    exactly TSDFVolume.register_camera's arguments.  `meshes`: a list of (vertices, faces) used instead of the files under
    `asset_root` (assets/franka_description/meshes/visual/* and assets/objs/cube/cube.obj, read through meshio.load_mesh).
    near = 0.01 is this project's choice, not Isaac Gym's clip plane; both faces of a triangle are hit (two-sided)."""

    def __init__(self, num_envs, device, cam_pose, cam_intr, im_h, im_w, asset_root='.', meshes=None, near=0.01, far=100.0):
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
        if len(meshes) == 0:
            raise ValueError("meshes: at least one part is needed")
        verts, part, faces, base = [], [], [], 0
        for i, (v, f) in enumerate(meshes):
            v, f = np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int64)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or len(v) == 0 or len(f) == 0:
                raise ValueError(f"meshes[{i}]: expected vertices (n > 0, 3) and faces (f > 0, 3), got {v.shape} and {f.shape}")
            if f.min() < 0 or f.max() >= len(v):
                raise ValueError(f"meshes[{i}]: a face index lies outside [0, {len(v)})")
            verts.append(v)
            part.append(np.full(len(v), i, dtype=np.int32))
            faces.append(f + base)
            base += len(v)
        self.part_num = len(meshes)
        self.verts = torch.from_numpy(np.ascontiguousarray(np.concatenate(verts))).to(self.device)               # (NV, 3)
        self.vert_part = torch.from_numpy(np.concatenate(part)).to(self.device)                                  # (NV,) int32
        self.faces = torch.from_numpy(np.ascontiguousarray(np.concatenate(faces).astype(np.int32))).to(self.device)   # (F, 3) int32

    def render(self, pose_R, pose_T, out=None):
        """pose_R [b, m, 3, 3], pose_T [b, m, 3] (any b) -> [b, V, im_h, im_w] float32: the z-depth (not the ray length) of the
        nearest surface through every pixel centre, `far` where nothing is hit.
        out: None, or a 2-D float32 view (b, >= V h w) with unit inner stride (e.g. the head of a depth_img observation buffer); the
        result is then a view of its first V h w columns."""
        b, _ = ops.check_poses(pose_R, pose_T, self.part_num)
        n = self.num_view * self.im_h * self.im_w
        if out is not None:
            ops._out_rows(out, b, n)                                                           # a bad view is reported before the device
        ops._req(pose_R, pose_T, out, self.verts)
        pose_R, pose_T = pose_R.contiguous(), pose_T.contiguous()
        res = ops.mesh_depth_render(self.verts, self.vert_part, self.faces, pose_R, pose_T, self.cam_pose, self.fx, self.fy, self.cx,
                                    self.cy, self.im_h, self.im_w, self.near, self.far, out)
        return res[:, :n].unflatten(1, (self.num_view, self.im_h, self.im_w))
