"""Yardsticks of the frame camera (partmanip_amd/mesh2depth.py: DepthFromMesh.render_frame, csrc/mesh_frame.hip).  Not product code.

frame_f32: the definition of the three images (include/partmanip_hip.h, pm_mesh_frame_render_f32) evaluated in numpy float32 over ALL
pixel x triangle pairs: z of every pair exactly as tests/depth_render_ref.render_f32 computes it, the winner as the lexicographic
minimum of (bits(z), f) through one uint64 key per pair, then the shade lines op by op in np.float32 (numpy rounds every float32
product, sum and difference on its own; its float32 sqrt and division are IEEE).  The GPU images must equal it byte for byte.

read_png: a decoder for what partmanip_amd.png.write_png writes (signature, IHDR, the inflated IDAT data, filter type 0), so that a
round trip does not depend on an imaging library.

The scenes are those of tests/depth_render_ref (seeded_scene, dyadic_triangle, concat_meshes, look_at)."""
import functools
import struct
import zlib

import numpy as np

from tests import depth_render_ref as D

F32 = np.float32
MISS_FACE = 0xFFFFFFFF


def default_palette(m):
    from partmanip_amd.mesh2depth import PALETTE
    return np.asarray([PALETTE[i % len(PALETTE)] for i in range(m)], dtype=F32)


def frame_f32(verts, vert_part, faces, R, T, cam_pose, fx, fy, cx, cy, H, W, near, far, part_label=None, miss_label=-1, palette=None,
              ambient=0.25, one_minus_ambient=None, background=(255, 255, 255), faces_per_chunk=256):
    """-> depth (B, V, H, W) float32, face (B, V, H, W) int64 (-1 at misses), seg (B, V, H, W) int32, rgb (B, V, H, W, 3) uint8."""
    verts, R, T, C = (np.asarray(a, dtype=F32) for a in (verts, R, T, cam_pose))
    vert_part, faces = np.asarray(vert_part).astype(np.int64), np.asarray(faces).astype(np.int64)
    NV, (B, M), V, nF = len(verts), R.shape[:2], len(C), len(faces)
    fx, fy, cx, cy, near, far = (F32(a) for a in (fx, fy, cx, cy, near, far))
    ambient = F32(ambient)
    oma = F32(1) - ambient if one_minus_ambient is None else F32(one_minus_ambient)
    palette = default_palette(M) if palette is None else np.asarray(palette, dtype=F32)
    face_ok = ((faces >= 0) & (faces < NV)).all(axis=1)
    safe_faces = np.where(face_ok[:, None], faces, 0)
    part = vert_part[safe_faces]
    face_ok &= ((part >= 0) & (part < M)).all(axis=1)
    safe_part = np.where((vert_part >= 0) & (vert_part < M), vert_part, 0)
    dx = ((np.arange(W).astype(F32) - cx) / fx)[None, :, None]
    dy = ((np.arange(H).astype(F32) - cy) / fy)[:, None, None]
    fill = (np.uint64(np.asarray(far, dtype=F32).view(np.uint32)) << np.uint64(32)) | np.uint64(MISS_FACE)
    keys = np.full((B, V, H, W), fill, dtype=np.uint64)
    cam_tri = np.zeros((B, V, nF, 3, 3), dtype=F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            Rv, Tv = R[b][safe_part], T[b][safe_part]
            x = verts
            xw = np.stack([((x[:, 0] * Rv[:, j, 0] + x[:, 1] * Rv[:, j, 1]) + x[:, 2] * Rv[:, j, 2]) + Tv[:, j] for j in range(3)], axis=1)
            for v in range(V):
                d = xw - C[v, :3, 3][None]
                p = np.stack([(d[:, 0] * C[v, 0, k] + d[:, 1] * C[v, 1, k]) + d[:, 2] * C[v, 2, k] for k in range(3)], axis=1)
                assert p.dtype == F32
                tri = p[safe_faces]
                cam_tri[b, v] = tri
                ok = face_ok & np.isfinite(tri).all(axis=(1, 2))
                index = np.nonzero(ok)[0]
                tri = tri[ok]
                img = keys[b, v]
                for lo in range(0, len(tri), faces_per_chunk):
                    p0, p1, p2 = (tri[lo:lo + faces_per_chunk, i] for i in range(3))

                    def cross(a, c):
                        return (a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0])
                    w = [(dx * n[0] + dy * n[1]) + n[2] for n in (cross(p1, p2), cross(p2, p0), cross(p0, p1))]
                    s = (w[0] + w[1]) + w[2]
                    z = ((w[0] * p0[:, 2] + w[1] * p1[:, 2]) + w[2] * p2[:, 2]) / s
                    assert z.dtype == F32
                    same = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
                    hit = same & (s != 0) & (z > near) & (z < far)
                    key = (np.ascontiguousarray(z).view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[lo:lo + faces_per_chunk].astype(np.uint64)
                    np.minimum(img, np.where(hit, key, fill).min(axis=2), out=img)
        low = (keys & np.uint64(MISS_FACE)).astype(np.int64)
        hit = low != MISS_FACE
        face = np.where(hit, low, -1)
        depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), far).astype(F32)
        fsafe = np.where(hit, low, 0)
        pp = vert_part[faces[fsafe, 0]]                                                    # (B, V, H, W): the winner's part
        pp = np.where(hit, pp, 0)
        label = pp if part_label is None else np.asarray(part_label).astype(np.int64)[pp]
        seg = np.where(hit, label, miss_label).astype(np.int32)
        bi, vi = np.arange(B)[:, None, None, None], np.arange(V)[None, :, None, None]
        corners = cam_tri[bi, vi, fsafe]                                                    # (B, V, H, W, 3, 3)
        p0, p1, p2 = corners[..., 0, :], corners[..., 1, :], corners[..., 2, :]
        e1, e2 = p1 - p0, p2 - p0
        gx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
        gy = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
        gz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
        q = (gx * gx + gy * gy) + gz * gz
        good = (q > 0) & np.isfinite(q)
        light = np.where(good, np.abs(gz) / np.sqrt(np.where(good, q, F32(1))), F32(0)).astype(F32)
        k = ambient + oma * light
        assert k.dtype == F32 and q.dtype == F32
        shade = palette[pp] * k[..., None] + F32(0.5)
        assert shade.dtype == F32
        rgb = np.where(hit[..., None], shade.astype(np.int32), np.asarray(background, dtype=np.int32)).astype(np.uint8)
    return depth, face, seg, rgb


@functools.lru_cache(maxsize=None)
def seeded_frame():
    """(scene, depth, face, seg, rgb) of tests/depth_render_ref.seeded_scene() with the default labels, palette, ambient and
    background, computed once per process; callers do not modify them."""
    sc = D.seeded_scene()
    out = frame_f32(**sc)
    for a in out:
        a.setflags(write=False)
    return (sc,) + out


def read_png(path):
    """-> (h, w, 3) or (h, w) uint8 of an 8-bit RGB or grey PNG without interlace whose rows all use filter type 0."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG signature"
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, compression, filt, interlace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT")), dtype=np.uint8)
    rows = raw.reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all(), "a filter type other than 0"
    img = rows[:, 1:].reshape(h, w, ch)
    return img.copy() if ch == 3 else img[..., 0].copy()
