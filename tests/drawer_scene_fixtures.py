"""A drawer scene whose environments differ, for the tests of the grouped cameras (DepthFromMesh(groups=), csrc/mesh_raster.h's
md_group_face) and of urdf.load_urdf_visuals.  Not product code; nothing is read from the reference's assets.

Three cabinets in the reference's folder layout, written into a directory the test owns:
  A: tests/cabinet_fixtures' cabinet A (2 bodies) with a <visual> box of 12 triangles on each link; the drawer's visual carries a
     non-trivial <origin xyz rpy> and a mesh `scale`.                                                            24 triangles
  B: cabinet B (7 bodies), one box per link.                                                                      84 triangles
  S: cabinet A's tree again: the base has no mesh at all, the drawer carries a closed 300-triangle ellipsoid.     300 triangles
The meshes are written with meshio.save_obj.  SPEC keeps what was written (mesh, mesh scale, origin), so a test can transform the
vertices by hand.

raw_scene(): the finger fixture (624 triangles, not a multiple of the rasteriser's 256-lane block) as the one shared part, the
three cabinets as groups, N = 5 environments over them (two share cabinet A, one holds none), seeded poses for every slot.  With
max_group_faces = 300 an environment has up to 924 face ordinals: the shared / group boundary (624) lies inside block 2, the group
of S straddles the block boundary at 768, and it ends the partial last block."""
import os

import numpy as np

from tests import cabinet_fixtures as CF
from tests import depth_render_ref as D
from tests import mesh_bake_ref as MB

F32 = np.float32
KINDS = ("A", "B", "S")
GROUP_OF = np.array([0, 1, 2, 0, -1], dtype=np.int32)        # environments 0 and 3 share cabinet A, environment 4 holds none
SCALE = 0.5


def ellipsoid_mesh(half, nu=15, nv=11):
    """Closed mesh of 2 nu (nv - 1) triangles (300 by default): nv - 1 rings of nu vertices and the two poles."""
    th = np.pi * np.arange(1, nv) / nv
    ph = 2 * np.pi * np.arange(nu) / nu
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(nu))], axis=-1)
    verts = np.concatenate([ring.reshape(-1, 3), [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]]) * np.asarray(half, dtype=np.float64)
    top, bottom = (nv - 1) * nu, (nv - 1) * nu + 1
    faces = []
    for j in range(nu):
        k = (j + 1) % nu
        faces.append((top, j, k))
        faces.append((bottom, (nv - 2) * nu + k, (nv - 2) * nu + j))
        for i in range(nv - 2):
            a, b, c, d = i * nu + j, i * nu + k, (i + 1) * nu + k, (i + 1) * nu + j
            faces += [(a, d, c), (a, c, b)]
    return verts.astype(F32), np.asarray(faces, dtype=np.int64)


def _box(half, centre=(0.0, 0.0, 0.0)):
    return MB.box_mesh(half, centre)


# kind -> link -> (mesh, mesh scale or None, origin xyz or None, origin rpy or None); a link that is not listed has no mesh
SPEC = {
    "A": {"base": (_box((0.20, 0.25, 0.30), (0.0, 0.0, 0.3)), None, None, None),
          "drawer": (_box((0.10, 0.40, 0.05)), (1.5, 0.5, 2.0), (0.01, -0.02, 0.03), (0.3, -0.2, 0.5))},
    "B": {"base": (_box((0.25, 0.30, 0.04)), None, None, None),
          "frame": (_box((0.10, 0.25, 0.40), (0.1, 0.0, 0.4)), None, None, None),      # behind the drawers, which stay in view
          "drawer_1": (_box((0.15, 0.22, 0.08)), None, (0.0, 0.0, 0.01), None),
          "handle_1": (_box((0.02, 0.08, 0.02)), None, None, None),
          "drawer_2": (_box((0.15, 0.22, 0.08)), None, None, (0.0, 0.0, 0.05)),
          "handle_2": (_box((0.02, 0.08, 0.02)), None, None, None),
          "door": (_box((0.02, 0.20, 0.30)), None, (0.0, -0.2, 0.3), None)},
    "S": {"drawer": (ellipsoid_mesh((0.25, 0.30, 0.20)), None, None, None)},
}


def urdf_text(kind):
    """The tree of cabinet_fixtures (A for S) with a <visual> on every link SPEC lists: mesh file `meshes/<link>.obj`."""
    text = CF.urdf_text("A" if kind == "S" else kind)
    for link, (_, mscale, xyz, rpy) in SPEC[kind].items():
        origin = ""
        if xyz is not None or rpy is not None:
            origin = '<origin xyz="%s" rpy="%s"/>' % (" ".join(repr(float(v)) for v in (xyz or (0, 0, 0))),
                                                       " ".join(repr(float(v)) for v in (rpy or (0, 0, 0))))
        scale = "" if mscale is None else ' scale="%s"' % " ".join(repr(float(v)) for v in mscale)
        visual = f'<visual>{origin}<geometry><mesh filename="meshes/{link}.obj"{scale}/></geometry></visual>'
        old = f'<link name="{link}"/>'
        assert old in text, (kind, link)
        text = text.replace(old, f'<link name="{link}">{visual}</link>')
    return text


def write_cabinet(root, kind, index=0):
    """cabinet_fixtures.write_cabinet's folder (for S: cabinet A's json and targets) with the visual URDF and the mesh files."""
    from partmanip_amd import meshio
    folder = CF.write_cabinet(root, "A" if kind == "S" else kind, index)
    with open(os.path.join(folder, "mobility_new.urdf"), "w") as f:
        f.write(urdf_text(kind))
    os.makedirs(os.path.join(folder, "meshes"), exist_ok=True)
    for link, ((v, fa), _, _, _) in SPEC[kind].items():
        meshio.save_obj(os.path.join(folder, "meshes", f"{link}.obj"), v, fa)
    return folder


def write_cabinets(root):
    return [write_cabinet(root, kind, i) for i, kind in enumerate(KINDS)]


def rpy_matrix64(rpy):
    """Rz(yaw) Ry(pitch) Rx(roll), multiplied out of the three axis rotations in float64."""
    r, p, y = (float(v) for v in rpy)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def expected_visual(kind, link, scale=SCALE):
    """(vertices float64, faces) of a link of SPEC, transformed by hand: mesh scale, origin, then `scale`; None without a mesh."""
    if link not in SPEC[kind]:
        return None
    (v, fa), mscale, xyz, rpy = SPEC[kind][link]
    x = v.astype(np.float64) * np.asarray(mscale or (1, 1, 1), dtype=np.float64)
    x = x @ rpy_matrix64(rpy or (0, 0, 0)).T + np.asarray(xyz or (0, 0, 0), dtype=np.float64)
    return x * scale, fa


def load_groups(root):
    """(assets, groups) of the three cabinets written under root, at SCALE."""
    from partmanip_amd.tasks.open_drawer import load_drawer_assets, load_drawer_meshes
    assets = load_drawer_assets(write_cabinets(root), scale=SCALE)
    return assets, load_drawer_meshes(assets)


# ------------------------------------------------------------------------------------------------------------ the raw scene
def concat_groups(shared, groups):
    """The arrays DepthFromMesh(meshes=shared, groups=groups) keeps, built independently: verts, vert_part (a group's body j takes
    slot len(shared) + j), faces, F_shared, group_off, part_num."""
    verts, part, faces, base = [], [], [], 0

    def add(mesh, slot):
        nonlocal base
        verts.append(np.asarray(mesh[0], dtype=F32))
        part.append(np.full(len(mesh[0]), slot, dtype=np.int32))
        faces.append(np.asarray(mesh[1], dtype=np.int64) + base)
        base += len(mesh[0])
        return len(mesh[1])
    F_shared = sum(add(m, i) for i, m in enumerate(shared))
    off = [0]
    for bodies in groups:
        off.append(off[-1] + sum(add(m, len(shared) + j) for j, m in enumerate(bodies) if m is not None))
    empty = np.zeros((0, 3))
    return dict(verts=np.concatenate(verts + [empty]).astype(F32), vert_part=np.concatenate(part + [np.zeros(0, np.int32)]).astype(np.int32),
                faces=np.concatenate(faces + [empty]).astype(np.int32), F_shared=F_shared, group_off=np.asarray(off, dtype=np.int32),
                part_num=len(shared) + max(len(b) for b in groups))


def raw_scene(groups, shared=None, group_of=GROUP_OF, seed=17, views=2, H=24, W=40):
    """The grouped arrays plus seeded poses for every slot of every environment (R, T), the cameras of depth_render_ref.seeded_scene
    (0.3 m from the origin, fx = fy = 60), and env_group.  The cabinet meshes are shrunk to the finger's size (x 0.15) so that all
    parts share the images."""
    rng = np.random.RandomState(seed)
    shared = [D.finger_mesh()] if shared is None else shared
    small = [[None if m is None else (np.asarray(m[0], dtype=F32) * F32(0.15), m[1]) for m in bodies] for bodies in groups]
    sc = concat_groups(shared, small)
    N, M = len(group_of), sc["part_num"]
    cams = []
    for _ in range(views):
        d = rng.standard_normal(3)
        d[2] = abs(d[2]) + 0.3
        cams.append(D.look_at(0.3 * d / np.linalg.norm(d)))
    sc.update(R=D.rotations(rng, (N, M)), T=rng.uniform(-0.06, 0.06, size=(N, M, 3)).astype(F32), cam_pose=np.stack(cams), fx=60.0,
              fy=60.0, cx=W / 2.0, cy=H / 2.0, H=H, W=W, near=0.01, far=100.0, env_group=np.asarray(group_of, dtype=np.int32))
    return sc


CAMERA_KEYS = ("cam_pose", "fx", "fy", "cx", "cy", "H", "W", "near", "far")


def env_rows(sc, b, env_group=None, max_group_faces=None):
    """The rows of faces environment b draws, by the definition: the shared rows, then its group's (cut to max_group_faces rows)."""
    g = int((sc["env_group"] if env_group is None else env_group)[b])
    rows = np.arange(sc["F_shared"])
    if 0 <= g < len(sc["group_off"]) - 1:
        lo, hi = (sc["F_shared"] + int(sc["group_off"][g + i]) for i in (0, 1))
        rows = np.concatenate([rows, np.arange(lo, hi if max_group_faces is None else min(hi, lo + max_group_faces))])
    return rows


def subset_depth(sc, env_group=None):
    """(N, V, H, W): render_f32 of every environment's own face subset under its own poses."""
    cam = {k: sc[k] for k in CAMERA_KEYS}
    return np.concatenate([D.render_f32(sc["verts"], sc["vert_part"], sc["faces"][env_rows(sc, b, env_group)], sc["R"][b:b + 1],
                                        sc["T"][b:b + 1], **cam) for b in range(len(sc["R"]))])


def all_in_one(sc):
    """The only scene the ungrouped entry offers: every object's bodies get slots of their own (object k's body j: 1 + sum of the
    body counts before k + j, after the shared slots) and an environment gives the absent objects NaN poses.  Returns (vert_part,
    R, T) of that scene; verts and faces are unchanged.  `sc` must carry `group_bodies`, the body count of each group."""
    ns = int(sc["vert_part"][sc["faces"][:sc["F_shared"]]].max()) + 1 if sc["F_shared"] else 0
    bodies = np.asarray(sc["group_bodies"])
    first = ns + np.concatenate([[0], np.cumsum(bodies)[:-1]])
    part = sc["vert_part"].copy()
    face_group = np.searchsorted(sc["group_off"], np.arange(len(sc["faces"]) - sc["F_shared"]), side="right") - 1
    for k in range(len(bodies)):
        vs = np.unique(sc["faces"][sc["F_shared"]:][face_group == k])
        part[vs] = first[k] + (sc["vert_part"][vs] - ns)
    N, M = len(sc["R"]), ns + int(bodies.sum())
    R, T = np.full((N, M, 3, 3), np.nan, dtype=F32), np.full((N, M, 3), np.nan, dtype=F32)
    R[:, :ns], T[:, :ns] = sc["R"][:, :ns], sc["T"][:, :ns]
    for b, g in enumerate(sc["env_group"]):
        if g >= 0:
            R[b, first[g]:first[g] + bodies[g]] = sc["R"][b, ns:ns + bodies[g]]
            T[b, first[g]:first[g] + bodies[g]] = sc["T"][b, ns:ns + bodies[g]]
    return part, R, T
