"""The group table of a scene whose environments differ (open_drawer: every environment holds its own cabinet), shared by the
posed-part observers DepthFromMesh, TSDFfromMesh and PCfromMesh.

The rows of an observer's library (faces, grids, points) are a shared range followed by G groups, one per object.  Body j of object
k takes pose slot num_shared + j in whatever environment holds object k; a body without a mesh (None) gets no row.  An environment
names its object through group_of: default env % G (the reference's rule), -1 for none.  A call over all num_envs environments uses
the constructor's table as it stands on the device; a call over a slice has to name its rows' objects with group_of=.
"""
import numpy as np
import torch


class SceneGroups:
    """groups: one list per object with one entry per body, None for a body without a mesh.  add_rows(body, slot, what, k, j) appends
    body j of object k to the caller's library under pose slot `slot` and returns how many rows it added (`what` names the entry in
    the caller's messages; slot and what are the rule's to state, so they are handed over ready, k and j besides for a library that
    keys on the body itself, as the cloud seeds its sampling).  Attributes: num_shared, part_num = num_shared + the largest body count, group_off (G + 1) numpy int32
    (rows relative to the shared range), most (the largest group's row count), group_of (num_envs) numpy int32, and the device
    copies group_off_dev and group_of_dev (int32)."""

    def __init__(self, num_envs, device, num_shared, groups, add_rows, group_of=None):
        groups = [list(g) for g in groups]
        if not groups:
            raise ValueError("groups: at least one object is needed")
        self.num_envs, self.device, self.num_shared = int(num_envs), device, int(num_shared)
        off = [0]
        for k, bodies in enumerate(groups):
            off.append(off[-1] + sum(add_rows(body, self.num_shared + j, f"groups[{k}][{j}]", k, j) for j, body in enumerate(bodies)
                                     if body is not None))
        self.part_num = self.num_shared + max(len(bodies) for bodies in groups)
        self.group_off = np.asarray(off, dtype=np.int32)
        self.most = int(np.diff(self.group_off).max())
        self.group_of = self.host_group_of(np.arange(self.num_envs) % len(groups) if group_of is None else group_of, self.num_envs)
        self.group_off_dev = torch.from_numpy(self.group_off).to(device)
        self.group_of_dev = torch.from_numpy(self.group_of).to(device)

    def host_group_of(self, group_of, b):
        g = np.asarray(group_of.cpu().numpy() if torch.is_tensor(group_of) else group_of)
        G = len(self.group_off) - 1
        if g.shape != (b,) or g.dtype.kind not in "iu" or g.min() < -1 or g.max() >= G:
            raise ValueError(f"group_of: expected {b} integers in [-1, {G}), got {g.dtype} {g.shape}")
        return np.ascontiguousarray(g, dtype=np.int32)

    def for_call(self, b, group_of):
        """The (b,) device table of a call over b environments: the constructor's, or the call's own group_of (b ints on the host,
        or a tensor on the device, which is not read here)."""
        if group_of is None:
            if b != self.num_envs:
                raise ValueError(f"poses: expected {self.num_envs} environments (the group table's), got {b}; pass group_of= for a slice")
            return self.group_of_dev
        if torch.is_tensor(group_of) and group_of.is_cuda:
            return group_of
        return torch.from_numpy(self.host_group_of(group_of, b)).to(self.device)
