// Frame camera over the posed part meshes: depth, part label and a shaded colour image from one rasterisation.  The reference reads
// a colour image and IMAGE_SEGMENTATION from the simulator's camera sensors (tasks/hand_base.py:222-227, 355-357); here they are
// rendered from the same (pose_R, pose_T) the depth camera takes.  mesh_depth.hip keeps the winning depth of a pixel; this file
// keeps the winning triangle as well, and resolves it.
//
// Definition (include/partmanip_hip.h has it in full).  The hit rule, z, the conservative box and the whole-wave path are the depth
// camera's, from the same code (mesh_raster.h).  A pixel's winner is the triangle of the smallest key (bits(z) << 32) | f over the
// triangles that hit it, f the triangle's row in faces: nearer first, then the smaller face index -- the stated tie-break, which
// two coincident triangles and the pixels exactly on a shared edge need.  z is positive, so the unsigned order of the key is that
// order.  z and f are functions of (triangle, pixel) alone and the minimum is order-free, so every output repeats bit for bit.
// depth = the winner's z (the bits pm_mesh_depth_render_f32 writes: the minimum of the high words is the minimum of the z),
// seg = the label of the winner's part, rgb = its palette colour under a headlight along the optical axis, two-sided:
// k = ambient + one_minus_ambient |g.z| / |g| with g = (p1 - p0) x (p2 - p0) in camera space, all fp32, every operation rounded on
// its own, the square root and the division IEEE.  The headlight and the palette are this project's choices, not Isaac Gym's
// renderer.
//
// Shape.  Three launches on one stream.  fill: every word of the (B, V, H, W) workspace of 64-bit keys becomes (bits(far) << 32) |
// 0xFFFFFFFF; every hit has z < far and beats it.  raster: mesh_raster.h's md_raster, one lane per (environment, view, triangle),
// whose commit is a 64-bit integer atomicMin on the key (no float atomics) after a relaxed 64-bit read that skips keys that cannot
// win; a stale read only costs a redundant update.  resolve: one lane per pixel reads its key, and for a hit poses the winner's three
// corners again with md_vertex (about 80 flops, against the three stores it feeds) and writes depth, seg and rgb; no image-sized
// intermediate besides the keys.
//
// Memory safety.  raster stores only keys, at r W + c with 0 <= r < H and 0 <= c < W of its (environment, view) image of the
// workspace, whose size the entry point has checked (md_raster's box is clamped to the image in float before it becomes an integer).
// A winner passed md_raster's index checks, so resolve reads nothing through a bad index; it repeats them all the same (f < F, the
// vertex index, the part) and writes a miss where one fails, so not even a workspace scribbled on between the launches can lead it
// out of bounds.  resolve writes columns [0, V H W) of a depth / seg row and bytes [0, 3 V H W) of an rgb row, nothing past them.
// Stream-ordered, never synchronises, allocates nothing.
//
// Atomic shape.  Scattered 8-byte integer-min atomics, one lane per triangle: the programming guide prices float adds only, so this
// shape is measured, not predicted (tools/time_mesh_frame.py, profiles/mesh_frame_timing.json).  If the ratio frame / depth is poor,
// the alternative without 64-bit atomics is a second raster pass after the depth kernel's own: a 32-bit atomicMin of f at the
// pixels where a triangle's z equals the settled depth.  It was not built.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): fill 6 VGPRs, 18 SGPRs; raster 54 VGPRs, 64 SGPRs, occupancy 8
// waves / SIMD, LDS (dynamic) 4 (W + H) bytes -- the depth raster's figures; resolve 68 VGPRs, 84 SGPRs, occupancy 7.  No scratch in
// any of the three.  Re-run when md_raster began to take the face row from its caller and the grouped entry was added
// (pm_mesh_frame_render_groups_f32: mesh_depth.hip's grouped raster with this file's commit; the key keeps the row in `faces`, so the
// tie-break and the resolve launch are the ungrouped entry's): fill, the ungrouped raster and resolve keep the figures above; the
// grouped raster kernel: 54 VGPRs, 66 SGPRs, no scratch, occupancy 8, the same LDS.
// Measured 2026-10-19 on one MI355X (tools/time_mesh_frame.py: the depth camera's scene, 133 200 triangles, 17 % of the pixels hit;
// ms per call, the three taken in turn): depth kernel / this file writing seg only / writing all three = 0.212 / 0.207 / 0.212
// (image rig 1 x 72 x 128, 64 environments), 2.83 / 2.79 / 2.86 (1024 environments), 1.21 / 1.18 / 1.37 (shipped rig 3 x 288 x 512,
// 64 environments, 226 MB of keys).  The raster with 8-byte keys is no slower than with 4-byte depths -- the relaxed read filters
// most updates there as well -- and what the full frame adds at the shipped rig is the resolve launch's larger output (it
// reads 226 MB of keys and writes 311 MB, the colour in single bytes).  The second-pass alternative has nothing to win at these ratios.
#include <string.h>

#include "mesh_raster.h"

#define MF_MISS_FACE 0xFFFFFFFFu

__global__ __launch_bounds__(MD_THREADS) void mesh_frame_fill_kernel(unsigned long long* __restrict__ keys, long total,
                                                                      unsigned long long key) {
    for (long i = (long)blockIdx.x * MD_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * MD_THREADS) keys[i] = key;
}

// The winner of one hit: nearer first, then the smaller face index.
struct mf_key_commit {
    __device__ __forceinline__ void operator()(unsigned long long* dst, float z, int f) const {
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)f;
        if (key < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(dst, key);
    }
};

__global__ __launch_bounds__(MD_THREADS) void mesh_frame_raster_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ vert_part, int NV, const int32_t* __restrict__ faces, int F,
    const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M, const float* __restrict__ cam_pose, int V, int chunks,
    float fx, float fy, float cx, float cy, int H, int W, float near, float far, unsigned long long* keys) {
    extern __shared__ float md_tab[];                        // dx of the W columns, then dy of the H rows
    long b;
    int v, chunk;
    md_block(blockIdx.x, chunks, V, b, v, chunk);
    unsigned long long* img = keys + (b * V + v) * ((long)H * W);
    md_raster(verts, vert_part, NV, faces, F, pose_R, pose_T, M, cam_pose, b, v, chunk * MD_THREADS + (int)threadIdx.x, fx, fy, cx, cy, H,
              W, near, far, md_tab, img, mf_key_commit());
}

// The grouped entry's raster (mesh_depth.hip's grouped kernel with this file's commit): the key's low word is the row in faces, so
// the tie-break and the resolve launch are the ungrouped entry's.
__global__ __launch_bounds__(MD_THREADS) void mesh_frame_raster_groups_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ vert_part, int NV, const int32_t* __restrict__ faces, int F,
    int F_shared, const int32_t* __restrict__ group_off, int G, const int32_t* __restrict__ env_group, int max_group_faces,
    const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M, const float* __restrict__ cam_pose, int V, int chunks,
    float fx, float fy, float cx, float cy, int H, int W, float near, float far, unsigned long long* keys) {
    extern __shared__ float md_tab[];
    long b;
    int v, chunk, count;
    md_block(blockIdx.x, chunks, V, b, v, chunk);
    const int f = md_group_face(chunk * MD_THREADS + (int)threadIdx.x, b, F, F_shared, group_off, G, env_group, max_group_faces, count);
    if (chunk * MD_THREADS >= count) return;
    unsigned long long* img = keys + (b * V + v) * ((long)H * W);
    md_raster(verts, vert_part, NV, faces, F, pose_R, pose_T, M, cam_pose, b, v, f, fx, fy, cx, cy, H, W, near, far, md_tab, img,
              mf_key_commit());
}

__global__ __launch_bounds__(MD_THREADS) void mesh_frame_resolve_kernel(
    const unsigned long long* __restrict__ keys, const float* __restrict__ verts, const int32_t* __restrict__ vert_part, int NV,
    const int32_t* __restrict__ faces, int F, const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M,
    const float* __restrict__ cam_pose, int V, long hw, long total, float far, const int32_t* __restrict__ part_label, int miss_label,
    const float* __restrict__ palette, float ambient, float one_minus_ambient, int bg_r, int bg_g, int bg_b, float* __restrict__ depth,
    long depth_stride, int32_t* __restrict__ seg, long seg_stride, uint8_t* __restrict__ rgb, long rgb_stride) {
    const long n = (long)V * hw;
    for (long i = (long)blockIdx.x * MD_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * MD_THREADS) {
        const long b = i / n;
        const long col = i - b * n;                          // (v H + r) W + c
        const int v = (int)(col / hw);
        const unsigned long long key = keys[i];
        const unsigned f = (unsigned)key;
        float z = far;
        int label = miss_label, cr = bg_r, cg = bg_g, cb = bg_b;
        const int i0 = f < (unsigned)F ? faces[3L * f] : -1;
        const int p = i0 >= 0 && i0 < NV ? vert_part[i0] : -1;
        if (p >= 0 && p < M) {                               // a hit
            z = __uint_as_float((unsigned)(key >> 32));
            label = part_label ? part_label[p] : p;
            if (rgb) {
                const md_cam cam = md_load_cam(cam_pose, v);
                const float* Rb = pose_R + b * M * 9;
                const float* Tb = pose_T + b * M * 3;
                float ax, ay, az, bx, by, bz, qx, qy, qz;
                md_vertex(verts, vert_part, NV, M, Rb, Tb, cam, i0, ax, ay, az);
                md_vertex(verts, vert_part, NV, M, Rb, Tb, cam, faces[3L * f + 1], bx, by, bz);
                md_vertex(verts, vert_part, NV, M, Rb, Tb, cam, faces[3L * f + 2], qx, qy, qz);
                const float e1x = sub_rn(bx, ax), e1y = sub_rn(by, ay), e1z = sub_rn(bz, az);
                const float e2x = sub_rn(qx, ax), e2y = sub_rn(qy, ay), e2z = sub_rn(qz, az);
                const float gx = md_cross(e1y, e2z, e1z, e2y), gy = md_cross(e1z, e2x, e1x, e2z), gz = md_cross(e1x, e2y, e1y, e2x);
                const float q = add_rn(add_rn(mul_rn(gx, gx), mul_rn(gy, gy)), mul_rn(gz, gz));
                const float l = q > 0.f && isfinite(q) ? __fdiv_rn(fabsf(gz), __fsqrt_rn(q)) : 0.f;
                const float k = add_rn(ambient, mul_rn(one_minus_ambient, l));
                cr = (int)add_rn(mul_rn(palette[3L * p], k), 0.5f);
                cg = (int)add_rn(mul_rn(palette[3L * p + 1], k), 0.5f);
                cb = (int)add_rn(mul_rn(palette[3L * p + 2], k), 0.5f);
            }
        }
        if (depth) depth[b * depth_stride + col] = z;
        if (seg) seg[b * seg_stride + col] = label;
        if (rgb) {
            uint8_t* px = rgb + b * rgb_stride + 3 * col;
            px[0] = (uint8_t)cr, px[1] = (uint8_t)cg, px[2] = (uint8_t)cb;
        }
    }
}

extern "C" size_t pm_mesh_frame_workspace_bytes(int B, int V, int H, int W) {
    if (B < 1 || V < 1 || H < 1 || W < 1) return 0;
    return (size_t)8 * (size_t)B * (size_t)V * (size_t)H * (size_t)W;
}

// Both entries: the checks and the three launches.  grouped: see mesh_depth.hip's md_render.
static int mf_render(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F, bool grouped, int F_shared,
                                        const int32_t* group_off, int G, const int32_t* env_group, int max_group_faces, const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V,
                                        float fx, float fy, float cx, float cy, int H, int W, float near, float far,
                                        const int32_t* part_label, int miss_label, const float* palette, float ambient,
                                        float one_minus_ambient, int bg_r, int bg_g, int bg_b, float* depth, long depth_stride,
                                        int32_t* seg, long seg_stride, uint8_t* rgb, long rgb_stride, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    PM_REQUIRE(verts && vert_part && faces && pose_R && pose_T && cam_pose && (depth || seg || rgb));
    PM_REQUIRE(NV >= 1 && F >= 1 && B >= 1 && M >= 1 && V >= 1 && H >= 1 && W >= 1);
    PM_REQUIRE(near > 0.f && far > near);                    // a NaN fails either
    PM_REQUIRE((long)W + H <= MD_MAX_TAB);
    const long hw = (long)H * W, n = (long)V * hw;
    PM_REQUIRE((!depth || depth_stride >= n) && (!seg || seg_stride >= n) && (!rgb || rgb_stride >= 3 * n));
    PM_REQUIRE(!rgb || palette);
    PM_REQUIRE(ambient >= 0.f && one_minus_ambient >= 0.f && ambient + one_minus_ambient <= 1.f);      // a NaN fails
    PM_REQUIRE(bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255);
    long ordinals = F;
    if (grouped) {
        PM_REQUIRE(F_shared >= 0 && F_shared <= F && G >= 0 && max_group_faces >= 0);
        PM_REQUIRE(G == 0 || (group_off && env_group));
        if (max_group_faces > F - F_shared) max_group_faces = F - F_shared;
        ordinals = (long)F_shared + max_group_faces;
    }
    const int chunks = (int)((ordinals + MD_THREADS - 1) / MD_THREADS);
    const long blocks = (long)chunks * V * B;
    PM_REQUIRE(blocks < (1L << 31) && hw < (1L << 31));
    if (!workspace || workspace_bytes < pm_mesh_frame_workspace_bytes(B, V, H, W)) return PM_EWORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return PM_EALIGN;
    unsigned long long* keys = (unsigned long long*)workspace;
    const long total = n * B;
    const long pixel_blocks = (total + MD_THREADS - 1) / MD_THREADS;
    const dim3 pixel_grid((unsigned)(pixel_blocks < (1L << 20) ? pixel_blocks : (1L << 20)));
    float far_f = far;
    unsigned far_bits;
    memcpy(&far_bits, &far_f, sizeof(far_bits));
    hipLaunchKernelGGL(mesh_frame_fill_kernel, pixel_grid, dim3(MD_THREADS), 0, pm_stream(stream), keys, total,
                       ((unsigned long long)far_bits << 32) | MF_MISS_FACE);
    PM_CHECK_LAUNCH();
    if (!grouped) {
        hipLaunchKernelGGL(mesh_frame_raster_kernel, dim3((unsigned)blocks), dim3(MD_THREADS), (size_t)(W + H) * sizeof(float),
                           pm_stream(stream), verts, vert_part, NV, faces, F, pose_R, pose_T, M, cam_pose, V, chunks, fx, fy, cx, cy,
                           H, W, near, far, keys);
        PM_CHECK_LAUNCH();
    } else if (blocks > 0) {                                 // no shared row and no group row: every pixel is a miss
        hipLaunchKernelGGL(mesh_frame_raster_groups_kernel, dim3((unsigned)blocks), dim3(MD_THREADS), (size_t)(W + H) * sizeof(float),
                           pm_stream(stream), verts, vert_part, NV, faces, F, F_shared, group_off, G, env_group, max_group_faces, pose_R,
                           pose_T, M, cam_pose, V, chunks, fx, fy, cx, cy, H, W, near, far, keys);
        PM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mesh_frame_resolve_kernel, pixel_grid, dim3(MD_THREADS), 0, pm_stream(stream), keys, verts, vert_part, NV,
                       faces, F, pose_R, pose_T, M, cam_pose, V, hw, total, far, part_label, miss_label, palette, ambient,
                       one_minus_ambient, bg_r, bg_g, bg_b, depth, depth_stride, seg, seg_stride, rgb, rgb_stride);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_mesh_frame_render_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F,
                                        const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V,
                                        float fx, float fy, float cx, float cy, int H, int W, float near, float far,
                                        const int32_t* part_label, int miss_label, const float* palette, float ambient,
                                        float one_minus_ambient, int bg_r, int bg_g, int bg_b, float* depth, long depth_stride,
                                        int32_t* seg, long seg_stride, uint8_t* rgb, long rgb_stride, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    return mf_render(verts, vert_part, NV, faces, F, false, 0, nullptr, 0, nullptr, 0,
                     pose_R, pose_T, B, M, cam_pose, V, fx, fy, cx, cy, H, W, near, far, part_label, miss_label, palette, ambient, one_minus_ambient,
                     bg_r, bg_g, bg_b, depth, depth_stride, seg, seg_stride, rgb, rgb_stride, workspace, workspace_bytes, stream);
}

extern "C" int pm_mesh_frame_render_groups_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F,
                                        int F_shared, const int32_t* group_off, int G, const int32_t* env_group, int max_group_faces,
                                        const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V,
                                        float fx, float fy, float cx, float cy, int H, int W, float near, float far,
                                        const int32_t* part_label, int miss_label, const float* palette, float ambient,
                                        float one_minus_ambient, int bg_r, int bg_g, int bg_b, float* depth, long depth_stride,
                                        int32_t* seg, long seg_stride, uint8_t* rgb, long rgb_stride, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    return mf_render(verts, vert_part, NV, faces, F, true, F_shared, group_off, G, env_group, max_group_faces,
                     pose_R, pose_T, B, M, cam_pose, V, fx, fy, cx, cy, H, W, near, far, part_label, miss_label, palette, ambient, one_minus_ambient,
                     bg_r, bg_g, bg_b, depth, depth_stride, seg, seg_stride, rgb, rgb_stride, workspace, workspace_bytes, stream);
}
