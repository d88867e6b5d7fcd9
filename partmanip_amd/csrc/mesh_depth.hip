// Depth camera over the posed part meshes: the producer of the reference's depth observations (tasks/hand_base.py:312-343 takes
// the image from the simulator's camera sensors; here it is rendered from the same (pose_R, pose_T) that query_pc and query_tsdf take).
//
// Definition (include/partmanip_hip.h has it in full).  All arithmetic is fp32, every product, sum and difference rounded on its
// own, divisions IEEE.  Vertex x of part j: xw = ((x0 R[j,0] + x1 R[j,1]) + x2 R[j,2]) + T[j] (common.h's posed_coord, shared with mesh_pc.hip), d = xw -
// C[:,3], p_k = (d0 C[0,k] + d1 C[1,k]) + d2 C[2,k] (the reference's bmm(world - t, R), depth2tsdf.py:47).  Triangle (p0, p1, p2):
// n0 = p1 x p2, n1 = p2 x p0, n2 = p0 x p1.  Pixel (row r, column c): dx = (float(c) - cx) / fx, dy = (float(r) - cy) / fy, w_i = (dx
// n_i.x + dy n_i.y) + n_i.z, s = (w0 + w1) + w2.  Hit iff the w_i are all >= 0 or all <= 0, s != 0 and z = ((w0 p0.z + w1 p1.z) + w2
// p2.z) / s lies in (near, far).  out = min z over the triangles that hit, else far.
//
// Properties that follow.
//  * w_i is the edge function of the edge opposite corner i, and it depends on that edge's two corners only.  Reversing the order
//    of the two corners negates the cross product exactly (a b - c d becomes c d - a b, both products rounded as before), so w_i is
//    negated exactly: two triangles that share an edge see edge values of exactly opposite sign at every pixel, the inclusive test
//    gives a pixel on the edge to both, and no crack opens between them.
//  * The minimum over triangles does not depend on their order and every z is a function of (triangle, pixel) alone, so the image
//    repeats bit for bit and a rasteriser and a ray caster give the same image -- as long as the rasteriser's pixel range is
//    conservative, i.e. contains every pixel that passes the hit rule.  Here the range is the box of the three projected corners
//    widened by one pixel on every side; a triangle with a corner at z <= near projects nowhere useful and gets the whole image.
//
// Shape.  One fill launch writes far; one raster launch follows in which a lane owns one (environment, view, triangle): it poses
// and projects the three corners itself (no per-vertex workspace; the poses and the camera are a few hundred bytes that stay in
// cache), sets up n0..n2 and its clamped pixel box, and walks it.  z is positive, so the unsigned order of its bits is the float
// order: the depth minimum is an integer atomicMin on the bits (no float atomics: the bits repeat).  A relaxed read of the current
// depth first skips a minimum that cannot win; a stale read only costs a redundant update.  A triangle whose box holds more than
// MD_WAVE_BOX pixels is handed to the whole wave (ballot, then its record broadcast lane by lane), so that a cube face, or a
// near-plane triangle with the whole image as its box, does not serialise on one lane; that is a schedule choice and cannot
// change the image.  dx and dy of every column and row are computed once per block into LDS ((W + H) floats), so a pixel test costs
// two ds_reads, 9 multiplies, 8 adds and the compares, and the division for z is paid by hits only.
//
// Memory safety.  A face index outside [0, NV), a part outside [0, M) or a non-finite camera-space coordinate skips the triangle;
// nothing is read through a bad index.  The box is clamped to the image in float before it becomes an integer, so no loop bound
// depends on an unclamped value, and every store lands in [0, V H W) of its environment's row: floats past V H W are never written.
// No workspace, stream-ordered, never synchronises.
//
// Atomic shape.  One lane per triangle issues scattered atomics, the shape the programming guide prices as slow; a tiled variant
// (a block owns an image tile, depths in LDS, every triangle tested against the tile) trades them for a bin pass or for F tests
// per tile.  It was not built and not measured: here the relaxed read filters most updates (a pixel's depth settles after its
// first few triangles; 17 % of the pixels are hit at all in the timed scene), and the figures below are what it would have to beat.
//
// Grouped entry (pm_mesh_depth_render_groups_f32; include/partmanip_hip.h has the definition).  The rows of `faces` split into a
// shared range [0, F_shared) and G groups behind it, and environment b draws the shared rows and the rows of group env_group[b]:
// open_drawer's environments each hold their own cabinet.  Same fill, same md_raster, same commit; what differs is the row a lane
// takes (mesh_raster.h, md_group_face): a lane owns (environment, view, face ordinal t < F_shared + max_group_faces), t maps to a row
// of the shared range or of the environment's group, and a block whose first ordinal lies past its environment's count returns
// before md_raster's barrier (the count depends on the block's environment only, so the branch is uniform over the block).  The image
// of an environment is therefore the definition applied to its own rows, bit for bit, and it pays the set-up of its own triangles;
// the alternative with the ungrouped entry -- every object of the library in one scene, NaN poses for the absent ones -- pays the
// set-up of the whole library in every environment (tools/time_drawer_scene.py, profiles/drawer_scene_timing.json).  A group id
// outside [0, G) is no group, a group's rows are clamped to [F_shared, F) and to max_group_faces: nothing is read through a bad index.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): raster 54 VGPRs, 64 SGPRs, no scratch, occupancy 8 waves / SIMD,
// LDS (dynamic) 4 (W + H) bytes = 3.2 KB at 512 x 288; fill 28 VGPRs, 51 SGPRs, no scratch.  Re-run when md_raster began to take the
// face row from its caller: the ungrouped raster kernel keeps 54 VGPRs / 64 SGPRs / no scratch / occupancy 8 / the same LDS (its
// device assembly differs from the previous one in the order of five scalar instructions and in one compare that became unsigned),
// fill unchanged; the grouped raster kernel: 54 VGPRs, 64 SGPRs, no scratch, occupancy 8, the same LDS.
// Measured A/B on one MI355X (tools/time_mesh_depth.py: 12 ellipsoids, 133 200 triangles, 1024 environments, random poses; the
// shipped rig 3 x 288 x 512 / the image rig 1 x 72 x 128, ms per call), MD_WAVE_BOX = 16 / 64 / 256: 56.65 / 18.97 / 18.99 and
// 10.63 / 2.85 / 2.85.  A box holds 27 / 18 pixels on average (a pixel-sized triangle widened by one pixel), so at 16 nearly every triangle
// takes the whole wave in turn and the launch serialises; between 64 and 256 few boxes fall and nothing changes; kept = 64.  At 64
// the shipped rig runs 1.10e10 pixel-triangle tests in 18.97 ms = 5.8e11 tests / s, 1.5 % of the output-bandwidth floor (0.288 ms for
// 1.8 GB): the kernel is bound by the tests and the triangle set-up, not by its output.
#include "mesh_raster.h"                                     // the rasteriser, shared with mesh_frame.hip; this file adds the depth commit

__global__ __launch_bounds__(MD_THREADS) void mesh_depth_fill_kernel(float* __restrict__ out, long out_stride, long n, long total,
                                                                      float far) {
    for (long i = (long)blockIdx.x * MD_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * MD_THREADS) {
        const long b = i / n;
        out[b * out_stride + (i - b * n)] = far;
    }
}

// The depth minimum of one hit.  dst is the pixel's word of the image, holding the bits of a positive float.
struct md_depth_commit {
    __device__ __forceinline__ void operator()(unsigned* dst, float z, int) const {
        const unsigned zb = __float_as_uint(z);
        if (zb < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(dst, zb);
    }
};

__global__ __launch_bounds__(MD_THREADS) void mesh_depth_raster_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ vert_part, int NV, const int32_t* __restrict__ faces, int F,
    const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M, const float* __restrict__ cam_pose, int V, int chunks,
    float fx, float fy, float cx, float cy, int H, int W, float near, float far, float* out, long out_stride) {
    extern __shared__ float md_tab[];                        // dx of the W columns, then dy of the H rows
    long b;
    int v, chunk;
    md_block(blockIdx.x, chunks, V, b, v, chunk);
    unsigned* img = (unsigned*)(out + b * out_stride + (long)v * H * W);
    md_raster(verts, vert_part, NV, faces, F, pose_R, pose_T, M, cam_pose, b, v, chunk * MD_THREADS + (int)threadIdx.x, fx, fy, cx, cy, H,
              W, near, far, md_tab, img, md_depth_commit());
}

// The grouped entry's raster: a lane owns (environment, view, face ordinal t), chunks = ceil((F_shared + max_group_faces) / 256).  A
// block whose first ordinal lies past its environment's count leaves before md_raster's barrier; the test is uniform over the block.
__global__ __launch_bounds__(MD_THREADS) void mesh_depth_raster_groups_kernel(
    const float* __restrict__ verts, const int32_t* __restrict__ vert_part, int NV, const int32_t* __restrict__ faces, int F,
    int F_shared, const int32_t* __restrict__ group_off, int G, const int32_t* __restrict__ env_group, int max_group_faces,
    const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M, const float* __restrict__ cam_pose, int V, int chunks,
    float fx, float fy, float cx, float cy, int H, int W, float near, float far, float* out, long out_stride) {
    extern __shared__ float md_tab[];
    long b;
    int v, chunk, count;
    md_block(blockIdx.x, chunks, V, b, v, chunk);
    const int f = md_group_face(chunk * MD_THREADS + (int)threadIdx.x, b, F, F_shared, group_off, G, env_group, max_group_faces, count);
    if (chunk * MD_THREADS >= count) return;
    unsigned* img = (unsigned*)(out + b * out_stride + (long)v * H * W);
    md_raster(verts, vert_part, NV, faces, F, pose_R, pose_T, M, cam_pose, b, v, f, fx, fy, cx, cy, H, W, near, far, md_tab, img,
              md_depth_commit());
}

// Both entries: the checks, the fill and one raster launch.  grouped: the ordinals of an environment are F_shared + max_group_faces
// (the latter cut to F - F_shared, which no group can exceed); else they are the F rows.
static int md_render(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F, bool grouped, int F_shared,
                     const int32_t* group_off, int G, const int32_t* env_group, int max_group_faces, const float* pose_R,
                     const float* pose_T, int B, int M, const float* cam_pose, int V, float fx, float fy, float cx, float cy, int H, int W,
                     float near, float far, float* out, long out_stride, void* stream) {
    PM_REQUIRE(verts && vert_part && faces && pose_R && pose_T && cam_pose && out);
    PM_REQUIRE(NV >= 1 && F >= 1 && B >= 1 && M >= 1 && V >= 1 && H >= 1 && W >= 1);
    PM_REQUIRE(near > 0.f && far > near);                    // a NaN fails either
    PM_REQUIRE((long)W + H <= MD_MAX_TAB);
    const long n = (long)V * H * W;
    PM_REQUIRE(out_stride >= n);
    long ordinals = F;
    if (grouped) {
        PM_REQUIRE(F_shared >= 0 && F_shared <= F && G >= 0 && max_group_faces >= 0);
        PM_REQUIRE(G == 0 || (group_off && env_group));
        if (max_group_faces > F - F_shared) max_group_faces = F - F_shared;
        ordinals = (long)F_shared + max_group_faces;
    }
    const int chunks = (int)((ordinals + MD_THREADS - 1) / MD_THREADS);
    const long blocks = (long)chunks * V * B;
    PM_REQUIRE(blocks < (1L << 31) && (long)H * W < (1L << 31));
    const long total = n * B;
    const long fill_blocks = (total + MD_THREADS - 1) / MD_THREADS;
    hipLaunchKernelGGL(mesh_depth_fill_kernel, dim3((unsigned)(fill_blocks < (1L << 20) ? fill_blocks : (1L << 20))),
                       dim3(MD_THREADS), 0, pm_stream(stream), out, out_stride, n, total, far);
    PM_CHECK_LAUNCH();
    if (!grouped) {
        hipLaunchKernelGGL(mesh_depth_raster_kernel, dim3((unsigned)blocks), dim3(MD_THREADS), (size_t)(W + H) * sizeof(float),
                           pm_stream(stream), verts, vert_part, NV, faces, F, pose_R, pose_T, M, cam_pose, V, chunks, fx, fy, cx, cy,
                           H, W, near, far, out, out_stride);
        PM_CHECK_LAUNCH();
    } else if (blocks > 0) {                                 // no shared row and no group row: the fill is the image
        hipLaunchKernelGGL(mesh_depth_raster_groups_kernel, dim3((unsigned)blocks), dim3(MD_THREADS), (size_t)(W + H) * sizeof(float),
                           pm_stream(stream), verts, vert_part, NV, faces, F, F_shared, group_off, G, env_group, max_group_faces, pose_R,
                           pose_T, M, cam_pose, V, chunks, fx, fy, cx, cy, H, W, near, far, out, out_stride);
        PM_CHECK_LAUNCH();
    }
    return PM_OK;
}

extern "C" int pm_mesh_depth_render_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F,
                                        const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V,
                                        float fx, float fy, float cx, float cy, int H, int W, float near, float far, float* out,
                                        long out_stride, void* stream) {
    return md_render(verts, vert_part, NV, faces, F, false, 0, nullptr, 0, nullptr, 0, pose_R, pose_T, B, M, cam_pose, V, fx, fy, cx, cy,
                     H, W, near, far, out, out_stride, stream);
}

extern "C" int pm_mesh_depth_render_groups_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F,
                                               int F_shared, const int32_t* group_off, int G, const int32_t* env_group,
                                               int max_group_faces, const float* pose_R, const float* pose_T, int B, int M,
                                               const float* cam_pose, int V, float fx, float fy, float cx, float cy, int H, int W,
                                               float near, float far, float* out, long out_stride, void* stream) {
    return md_render(verts, vert_part, NV, faces, F, true, F_shared, group_off, G, env_group, max_group_faces, pose_R, pose_T, B, M,
                     cam_pose, V, fx, fy, cx, cy, H, W, near, far, out, out_stride, stream);
}
