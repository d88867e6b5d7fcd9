// The rasteriser shared by the depth camera (mesh_depth.hip) and the frame camera (mesh_frame.hip): camera-space vertices, the
// triangle set-up with its conservative pixel box, the per-pixel hit test and the walk over the box (lane path, and the whole-wave
// path for boxes over MD_WAVE_BOX).  Every formula is the definition of include/partmanip_hip.h (pm_mesh_depth_render_f32); the two
// kernels differ only in what a hit commits, which they hand to md_raster as `commit(dst, z, f)`: dst = the pixel's word of the
// kernel's own image of the view (img + r W + c), z the hit's depth, f the triangle's row in `faces`.  mesh_depth.hip's header has the definition, the properties that follow
// from it and the measurements that chose MD_WAVE_BOX.  Which triangle a lane takes is its kernel's choice (md_raster's `f`): the
// ungrouped kernels walk the rows of `faces` in order, the grouped ones take md_group_face's row of the environment's own subset.
#pragma once
#include "common.h"

#ifndef MD_WAVE_BOX
#define MD_WAVE_BOX 64                                       // boxes above this many pixels are walked by the whole wave
#endif
#define MD_THREADS 256
#define MD_MAX_TAB 12288                                     // W + H floats of LDS: 48 KB

struct md_cam {
    float c[12];                                             // rows 0..2 of the camera->world matrix: c[4 j + k], c[4 j + 3] = t_j
};

__device__ __forceinline__ md_cam md_load_cam(const float* __restrict__ cam_pose, int v) {
    md_cam cam;
#pragma unroll
    for (int i = 0; i < 12; ++i) cam.c[i] = cam_pose[16L * v + i];
    return cam;
}

// Camera-space position of vertex i; false if the vertex is to be skipped (bad index, bad part, non-finite result).
__device__ __forceinline__ bool md_vertex(const float* __restrict__ verts, const int32_t* __restrict__ vert_part, int NV, int M,
                                          const float* __restrict__ Rb, const float* __restrict__ Tb, const md_cam& cam, int i,
                                          float& px, float& py, float& pz) {
    px = py = pz = 0.f;
    if (i < 0 || i >= NV) return false;
    const int p = vert_part[i];
    if (p < 0 || p >= M) return false;
    const float x0 = verts[3L * i], x1 = verts[3L * i + 1], x2 = verts[3L * i + 2];
    const float* R = Rb + 9L * p;
    const float* T = Tb + 3L * p;
    float d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        d[j] = sub_rn(posed_coord(x0, x1, x2, R[3 * j], R[3 * j + 1], R[3 * j + 2], T[j]), cam.c[4 * j + 3]);
    }
    px = add_rn(add_rn(mul_rn(d[0], cam.c[0]), mul_rn(d[1], cam.c[4])), mul_rn(d[2], cam.c[8]));
    py = add_rn(add_rn(mul_rn(d[0], cam.c[1]), mul_rn(d[1], cam.c[5])), mul_rn(d[2], cam.c[9]));
    pz = add_rn(add_rn(mul_rn(d[0], cam.c[2]), mul_rn(d[1], cam.c[6])), mul_rn(d[2], cam.c[10]));
    return isfinite(px) && isfinite(py) && isfinite(pz);
}

struct md_tri {
    float n0x, n0y, n0z, n1x, n1y, n1z, n2x, n2y, n2z, z0, z1, z2;
    int x0, y0, bw, cnt;                                     // box origin, width and pixel count (0: nothing to do)
};

__device__ __forceinline__ float md_cross(float a, float b, float c, float d) { return sub_rn(mul_rn(a, b), mul_rn(c, d)); }

// One (pixel, triangle) test; a hit goes to commit(dst, z, f).  dst is this pixel's word of the kernel's image.
template <class Word, class Commit>
__device__ __forceinline__ void md_pixel(const md_tri& t, float dx, float dy, float near, float far, Word* dst, int f, Commit commit) {
    const float w0 = add_rn(add_rn(mul_rn(dx, t.n0x), mul_rn(dy, t.n0y)), t.n0z);
    const float w1 = add_rn(add_rn(mul_rn(dx, t.n1x), mul_rn(dy, t.n1y)), t.n1z);
    const float w2 = add_rn(add_rn(mul_rn(dx, t.n2x), mul_rn(dy, t.n2y)), t.n2z);
    const bool pos = w0 >= 0.f && w1 >= 0.f && w2 >= 0.f, neg = w0 <= 0.f && w1 <= 0.f && w2 <= 0.f;
    if (!(pos || neg)) return;
    const float s = add_rn(add_rn(w0, w1), w2);
    if (s == 0.f) return;
    const float z = __fdiv_rn(add_rn(add_rn(mul_rn(w0, t.z0), mul_rn(w1, t.z1)), mul_rn(w2, t.z2)), s);
    if (!(z > near && z < far)) return;                      // a NaN fails both
    commit(dst, z, f);
}

__device__ __forceinline__ float md_bcast(float x, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// Block blk of the raster grid -> its environment, view and chunk of MD_THREADS triangles.
__device__ __forceinline__ void md_block(long blk, int chunks, int V, long& b, int& v, int& chunk) {
    const long bv = blk / chunks;
    chunk = (int)(blk - bv * chunks);
    b = bv / V;
    v = (int)(bv - b * V);
}

// The face row of ordinal t of environment b in the grouped entries (include/partmanip_hip.h, pm_mesh_depth_render_groups_f32): the
// shared rows [0, F_shared) first, then the rows of the environment's group; -1 ("none") past them.  A group id outside [0, G) is no
// group; the group's rows are clamped to [F_shared, F) and to max_group_faces rows, so the row returned lies in [0, F) whatever the
// tables hold.  count: the environment's ordinals.  The host has checked 0 <= F_shared <= F and 0 <= max_group_faces <= F - F_shared.
__device__ __forceinline__ int md_group_face(int t, long b, int F, int F_shared, const int32_t* __restrict__ group_off, int G,
                                             const int32_t* __restrict__ env_group, int max_group_faces, int& count) {
    int lo = 0, n = 0;
    const int g = G > 0 ? env_group[b] : -1;
    if (g >= 0 && g < G) {
        const int room = F - F_shared;
        lo = min(max(group_off[g], 0), room);
        n = min(min(max(group_off[g + 1], lo), room) - lo, max_group_faces);
    }
    count = F_shared + n;
    return t < F_shared ? t : (t < count ? F_shared + lo + (t - F_shared) : -1);
}

// The raster work of one block: environment b, view v, one triangle per lane: f, its row in faces, chosen by the caller (the
// ungrouped kernels: chunk MD_THREADS + threadIdx.x; the grouped ones: md_group_face); a row outside [0, F) is "none".  md_tab: W + H
// floats of LDS; img: the (H, W) image of this environment and view, of whatever word the kernel keeps per pixel.  Every lane of the
// block must call it (a barrier and wave-wide broadcasts inside).  commit(img + r W + c, z, f) is called for every (pixel, triangle)
// hit with 0 <= r < H, 0 <= c < W and f the triangle's row in faces, 0 <= f < F.
template <class Word, class Commit>
__device__ __forceinline__ void md_raster(const float* __restrict__ verts, const int32_t* __restrict__ vert_part, int NV,
                                          const int32_t* __restrict__ faces, int F, const float* __restrict__ pose_R,
                                          const float* __restrict__ pose_T, int M, const float* __restrict__ cam_pose, long b, int v,
                                          int f, float fx, float fy, float cx, float cy, int H, int W, float near, float far,
                                          float* md_tab, Word* img, Commit commit) {
    for (int i = threadIdx.x; i < W + H; i += MD_THREADS)
        md_tab[i] = i < W ? __fdiv_rn(sub_rn((float)i, cx), fx) : __fdiv_rn(sub_rn((float)(i - W), cy), fy);

    const md_cam cam = md_load_cam(cam_pose, v);
    const float* Rb = pose_R + b * M * 9;
    const float* Tb = pose_T + b * M * 3;

    md_tri t = {};
    if ((unsigned)f < (unsigned)F) {
        float ax, ay, az, bx, by, bz, qx, qy, qz;
        const bool ok0 = md_vertex(verts, vert_part, NV, M, Rb, Tb, cam, faces[3L * f], ax, ay, az);
        const bool ok1 = md_vertex(verts, vert_part, NV, M, Rb, Tb, cam, faces[3L * f + 1], bx, by, bz);
        const bool ok2 = md_vertex(verts, vert_part, NV, M, Rb, Tb, cam, faces[3L * f + 2], qx, qy, qz);
        if (ok0 && ok1 && ok2) {
            t.n0x = md_cross(by, qz, bz, qy), t.n0y = md_cross(bz, qx, bx, qz), t.n0z = md_cross(bx, qy, by, qx);   // p1 x p2
            t.n1x = md_cross(qy, az, qz, ay), t.n1y = md_cross(qz, ax, qx, az), t.n1z = md_cross(qx, ay, qy, ax);   // p2 x p0
            t.n2x = md_cross(ay, bz, az, by), t.n2y = md_cross(az, bx, ax, bz), t.n2z = md_cross(ax, by, ay, bx);   // p0 x p1
            t.z0 = az, t.z1 = bz, t.z2 = qz;
            float ulo = 0.f, uhi = (float)(W - 1), vlo = 0.f, vhi = (float)(H - 1);
            if (az > near && bz > near && qz > near) {       // else: the whole image
                const float u0 = ax / az * fx + cx, u1 = bx / bz * fx + cx, u2 = qx / qz * fx + cx;
                const float v0 = ay / az * fy + cy, v1 = by / bz * fy + cy, v2 = qy / qz * fy + cy;
                ulo = fmaxf(floorf(fminf(fminf(u0, u1), u2)) - 1.f, ulo);
                uhi = fminf(ceilf(fmaxf(fmaxf(u0, u1), u2)) + 1.f, uhi);
                vlo = fmaxf(floorf(fminf(fminf(v0, v1), v2)) - 1.f, vlo);
                vhi = fminf(ceilf(fmaxf(fmaxf(v0, v1), v2)) + 1.f, vhi);
            }
            if (ulo <= uhi && vlo <= vhi) {                  // all four lie in [0, W - 1] x [0, H - 1] here (a NaN fails the test)
                t.x0 = (int)ulo, t.y0 = (int)vlo;
                t.bw = (int)uhi - t.x0 + 1;
                t.cnt = t.bw * ((int)vhi - t.y0 + 1);
            }
        }
    }
    __syncthreads();                                         // md_tab is complete

    const float* tdx = md_tab;
    const float* tdy = md_tab + W;
    const int lane = threadIdx.x & (PM_WAVE - 1);
    unsigned long long big = __ballot(t.cnt > MD_WAVE_BOX);
    while (big) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)big) - 1);
        big &= big - 1;
        md_tri s;
        s.n0x = md_bcast(t.n0x, l), s.n0y = md_bcast(t.n0y, l), s.n0z = md_bcast(t.n0z, l);
        s.n1x = md_bcast(t.n1x, l), s.n1y = md_bcast(t.n1y, l), s.n1z = md_bcast(t.n1z, l);
        s.n2x = md_bcast(t.n2x, l), s.n2y = md_bcast(t.n2y, l), s.n2z = md_bcast(t.n2z, l);
        s.z0 = md_bcast(t.z0, l), s.z1 = md_bcast(t.z1, l), s.z2 = md_bcast(t.z2, l);
        s.x0 = __builtin_amdgcn_readlane(t.x0, l), s.y0 = __builtin_amdgcn_readlane(t.y0, l);
        s.bw = __builtin_amdgcn_readlane(t.bw, l), s.cnt = __builtin_amdgcn_readlane(t.cnt, l);
        const int fl = __builtin_amdgcn_readlane(f, l);      // lane l's triangle
        for (int i = lane; i < s.cnt; i += PM_WAVE) {
            const int rr = i / s.bw;
            const int r = s.y0 + rr, c = s.x0 + (i - rr * s.bw);
            md_pixel(s, tdx[c], tdy[r], near, far, img + (long)r * W + c, fl, commit);
        }
    }
    if (t.cnt > 0 && t.cnt <= MD_WAVE_BOX) {
        const int bh = t.cnt / t.bw;
        for (int rr = 0; rr < bh; ++rr) {
            const int r = t.y0 + rr;
            const float dy = tdy[r];
            for (int cc = 0; cc < t.bw; ++cc) md_pixel(t, tdx[t.x0 + cc], dy, near, far, img + (long)r * W + t.x0 + cc, f, commit);
        }
    }
}
