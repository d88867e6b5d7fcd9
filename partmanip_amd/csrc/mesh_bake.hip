// Baking a part's signed-distance grid from its triangle mesh (the reference's utils/mesh2sdf.py: TSDFfromMesh.mesh2sdf, :201-237,
// which needs kaolin's point_to_mesh_distance / check_sign and, for open meshes, ManifoldPlus -- none of which exists for ROCm).
//
// Contract ("mesh bake").  Voxel (i, j, k) of an (X, Y, Z) grid sits at (idx - shape / 2) * voxel_size + centre, the
// multiply and the add rounded separately as in the reference's tensor expression (:223).  Its value is
// clamp(sign * sqrt(min over faces of the squared point-to-triangle distance), -trunc, +trunc), sign = -1 iff |w| >= 0.5 with w
// the generalised winding number: sum over faces of the signed solid angle / 4 pi (van Oosterom-Strackee, tan(O/2) = a.(b x c) /
// (|a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), a, b, c = corners - point, through atan2).  On a closed mesh that is kaolin's
// parity test without its degenerate rays; on an open mesh it degrades smoothly (the stated deviation from the reference).
// A zero-area triangle counts as its longest edge for the distance and as nothing for the sign.
//
// Shape.  A lane owns a voxel, a wave a 4 x 4 x 4 brick (k fastest), a work-group four bricks consecutive along k.  A first small
// kernel turns every triangle into a 40-float record, computed in fp64 and rounded once: the corners, the unit normal, the unit
// direction and length of each edge, the in-plane inward normal of each edge, the bounding box, a "has an area" flag.  The bake
// kernel walks the records with a wave-uniform index, so they arrive through scalar loads into SGPRs (no LDS, no bank conflicts)
// and every lane keeps min d^2 and the running sum of atan2 in registers.  Per pair the distance is the minimum of the three
// clamped edge projections and, if the point projects inside the triangle, the plane distance -- no division in the loop (the
// divisions were done once per triangle in fp64); one correctly rounded sqrt, the compare against pi, the clamp and one store
// at the end.  No atomics, a fixed order of accumulation: two bakes of a mesh are bit-identical.
// Nothing approximate touches the magnitude: fused multiply-adds on fp32 inputs and one IEEE sqrt.  The raw v_sqrt (1 ulp) and the
// library atan2 appear only in the solid angles, whose sum decides a sign against pi with room to spare.
//
// Shortcut (tri_cull != 0).  A triangle whose bounding box is farther than 1.001 * trunc + 1e-6 from the brick's box of voxel
// centres cannot bring any of the brick's magnitudes below trunc, and everything at or above trunc is clamped to trunc: its
// distance part is skipped for the whole wave (its solid angle is still summed).  Output with and without it is bit-identical
// (tests/test_gpu_mesh_bake.py, whole grid).  The second shortcut one could think of -- one sign per brick that is farther than
// trunc from every triangle -- is exact on closed meshes only (the |w| = 0.5 surface of an open mesh leaves the mesh through its
// boundary edges and crosses free space), so it is not built.
//
// Memory safety.  Records are read at indices [0, F) only; a lane stores only when its (i, j, k) is inside the grid.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): mesh_bake_kernel<true>: 42 VGPRs, 44 SGPRs, no scratch, no LDS,
// occupancy 8 waves / SIMD; <false> (cull off, tests and timing only): 34 VGPRs, 44 SGPRs, no scratch, occupancy 8;
// mesh_bake_prep_kernel: 72 VGPRs, 16 SGPRs, no scratch, occupancy 7.  Inner loop of <true> in the disassembly: 134 VALU
// instructions for a pair that takes the distance path (4 of them v_sqrt / v_rcp), 71 for a pair the cull drops.
// Measured A/B on one MI355X, 100 x 100 torus (20 000 triangles, 151 x 151 x 70 voxels, tools/time_mesh_bake.py), kept = marked:
// cull off 88.3 ms -> cull on 68.2 / 68.6 ms with the area flag as a wave-uniform branch -> flag as a multiplier, no branch 65.3 ms
// (kept) -> + `#pragma unroll 2` 69.2 ms (not kept) -> + every record word pinned into an SGPR at the loop top, one wait per
// triangle instead of four, 65.8 / 65.3 ms (no gain: the other waves of the SIMD hide the scalar-load waits; not kept).
// Cull off the kernel runs at 0.62 of the VALU-issue floor (134 x pairs / 64 / 1.23e12 wave-instructions per second); the
// quarter-rate sqrt / rcp and the atan2 range reduction are what is left.  LDS tiles were not tried: the records already arrive
// at no VALU cost.
#include "common.h"

#define MB_BRICK 4                                           // brick edge in voxels; 4^3 = one wave
#define MB_WAVES 4                                           // bricks (waves) per work-group
#define MB_REC 40                                            // floats per triangle record
#define MB_PI 3.14159265358979323846f

// ---- per-triangle records, in fp64 ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_bake_prep_kernel(const float* __restrict__ tri, int F, float* __restrict__ rec) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float* t = tri + (long)f * 9;
    const double A[3] = {t[0], t[1], t[2]}, B[3] = {t[3], t[4], t[5]}, Cc[3] = {t[6], t[7], t[8]};
    double e[3][3];                                          // edges ab, bc, ca
    for (int d = 0; d < 3; ++d) {
        e[0][d] = B[d] - A[d];
        e[1][d] = Cc[d] - B[d];
        e[2][d] = A[d] - Cc[d];
    }
    // normal = ab x ac = ab x (-ca)
    double n[3] = {e[0][1] * -e[2][2] - e[0][2] * -e[2][1], e[0][2] * -e[2][0] - e[0][0] * -e[2][2],
                   e[0][0] * -e[2][1] - e[0][1] * -e[2][0]};
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const bool area = nn > 0.0;
    float* r = rec + (long)f * MB_REC;
    double u[3][3], L[3];
    for (int k = 0; k < 3; ++k) {
        L[k] = sqrt(e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2]);
        for (int d = 0; d < 3; ++d) u[k][d] = L[k] > 0.0 ? e[k][d] / L[k] : 0.0;
    }
    for (int d = 0; d < 3; ++d) {
        n[d] = area ? n[d] / nn : 0.0;
        r[d] = t[d];
        r[3 + d] = t[3 + d];
        r[6 + d] = t[6 + d];
        r[9 + d] = (float)n[d];
        r[33 + d] = fminf(fminf(t[d], t[3 + d]), t[6 + d]);
        r[36 + d] = fmaxf(fmaxf(t[d], t[3 + d]), t[6 + d]);
    }
    for (int k = 0; k < 3; ++k) {
        r[21 + k] = (float)L[k];
        // inward in-plane normal of edge k: n x u_k
        const double m[3] = {n[1] * u[k][2] - n[2] * u[k][1], n[2] * u[k][0] - n[0] * u[k][2], n[0] * u[k][1] - n[1] * u[k][0]};
        for (int d = 0; d < 3; ++d) {
            r[12 + 3 * k + d] = (float)u[k][d];
            r[24 + 3 * k + d] = (float)m[d];
        }
    }
    r[39] = area ? 1.0f : 0.0f;
}

// ---- the bake ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mb_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}
// squared distance from the origin to the segment {q + u t, 0 <= t <= L} (u a unit vector)
__device__ __forceinline__ float mb_seg(float qx, float qy, float qz, float ux, float uy, float uz, float L) {
    const float t = __builtin_amdgcn_fmed3f(-mb_dot(qx, qy, qz, ux, uy, uz), 0.0f, L);
    const float x = fmaf(ux, t, qx), y = fmaf(uy, t, qy), z = fmaf(uz, t, qz);
    return mb_dot(x, y, z, x, y, z);
}

template <bool CULL>
__global__ __launch_bounds__(64 * MB_WAVES) void mesh_bake_kernel(const float* __restrict__ rec, int F, int X, int Y, int Z, int nbj,
                                                                  int nbk, float voxel_size, float cx, float cy, float cz,
                                                                  float trunc, long bricks, float* __restrict__ sdf) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long brick = (long)blockIdx.x * MB_WAVES + wave;
    if (brick >= bricks) return;                             // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int bk = (int)(brick % nbk), bj = (int)((brick / nbk) % nbj), bi = (int)(brick / ((long)nbk * nbj));
    const int i = bi * MB_BRICK + (lane >> 4), j = bj * MB_BRICK + ((lane >> 2) & 3), k = bk * MB_BRICK + (lane & 3);
    const bool inside = i < X && j < Y && k < Z;
    // the reference's (idx - shape // 2) * voxel_size + centre, two roundings
    const float px = add_rn(mul_rn((float)(i - X / 2), voxel_size), cx);
    const float py = add_rn(mul_rn((float)(j - Y / 2), voxel_size), cy);
    const float pz = add_rn(mul_rn((float)(k - Z / 2), voxel_size), cz);
    // the brick's box of voxel centres (wave-uniform), widened by the reach of the cull
    const float reach = trunc * 1.001f + 1e-6f;
    const float lox = add_rn(mul_rn((float)(bi * MB_BRICK - X / 2), voxel_size), cx), hix = lox + (MB_BRICK - 1) * voxel_size * 1.001f;
    const float loy = add_rn(mul_rn((float)(bj * MB_BRICK - Y / 2), voxel_size), cy), hiy = loy + (MB_BRICK - 1) * voxel_size * 1.001f;
    const float loz = add_rn(mul_rn((float)(bk * MB_BRICK - Z / 2), voxel_size), cz), hiz = loz + (MB_BRICK - 1) * voxel_size * 1.001f;

    float best = __builtin_inff();                           // min d^2
    float turn = 0.0f;                                       // sum of atan2 = (sum of solid angles) / 2
    for (int f = 0; f < F; ++f) {
        const float* r = rec + (long)f * MB_REC;             // wave-uniform address: scalar loads
        const bool area = r[39] != 0.0f;                     // wave-uniform; false: the longest edge for the distance, nothing for the sign
        const float ax = r[0] - px, ay = r[1] - py, az = r[2] - pz;
        const float bx = r[3] - px, by = r[4] - py, bz = r[5] - pz;
        const float qx = r[6] - px, qy = r[7] - py, qz = r[8] - pz;      // q: corner c
        {                                                    // signed solid angle / 2
            const float la = __builtin_amdgcn_sqrtf(mb_dot(ax, ay, az, ax, ay, az));
            const float lb = __builtin_amdgcn_sqrtf(mb_dot(bx, by, bz, bx, by, bz));
            const float lc = __builtin_amdgcn_sqrtf(mb_dot(qx, qy, qz, qx, qy, qz));
            const float kx = fmaf(by, qz, -bz * qy), ky = fmaf(bz, qx, -bx * qz), kz = fmaf(bx, qy, -by * qx);   // b x c
            const float num = mb_dot(ax, ay, az, kx, ky, kz);
            const float den = fmaf(mb_dot(qx, qy, qz, ax, ay, az), lb,
                                   fmaf(mb_dot(bx, by, bz, qx, qy, qz), la, fmaf(mb_dot(ax, ay, az, bx, by, bz), lc, la * lb * lc)));
            turn = fmaf(r[39], atan2f(num, den), turn);      // flag 0: a triangle without area adds nothing (atan2 of finite numbers is finite)
        }
        bool near = true;
        if (CULL) {
            const float gx = fmaxf(fmaxf(r[33] - hix, lox - r[36]), 0.0f), gy = fmaxf(fmaxf(r[34] - hiy, loy - r[37]), 0.0f),
                        gz = fmaxf(fmaxf(r[35] - hiz, loz - r[38]), 0.0f);
            near = !(mb_dot(gx, gy, gz, gx, gy, gz) > reach * reach);    // wave-uniform
        }
        if (near) {
            const float e0 = mb_seg(ax, ay, az, r[12], r[13], r[14], r[21]);
            const float e1 = mb_seg(bx, by, bz, r[15], r[16], r[17], r[22]);
            const float e2 = mb_seg(qx, qy, qz, r[18], r[19], r[20], r[23]);
            // p - corner = -(corner - p): inside the prism over the triangle iff every inward edge normal sees p on its side
            const bool in = (int)area & (int)(mb_dot(ax, ay, az, r[24], r[25], r[26]) <= 0.0f) &      // no short circuit: no load behind a branch
                            (int)(mb_dot(bx, by, bz, r[27], r[28], r[29]) <= 0.0f) & (int)(mb_dot(qx, qy, qz, r[30], r[31], r[32]) <= 0.0f);
            const float h = mb_dot(ax, ay, az, r[9], r[10], r[11]);
            const float d2 = in ? h * h : fminf(e0, fminf(e1, e2));
            best = fminf(best, d2);
        }
    }
    if (inside) {
        const float d = sqrtf(best);                         // correctly rounded
        const float s = fabsf(turn) >= MB_PI ? -d : d;       // |w| >= 0.5  <=>  |sum atan2| >= pi
        sdf[((long)i * Y + j) * Z + k] = fminf(fmaxf(s, -trunc), trunc);
    }
}

extern "C" size_t pm_mesh_sdf_bake_workspace_bytes(int F) { return F > 0 ? (size_t)F * MB_REC * sizeof(float) : 0; }

extern "C" int pm_mesh_sdf_bake_f32(const float* tri, int F, int X, int Y, int Z, float voxel_size, float cx, float cy, float cz,
                                    float trunc, int tri_cull, float* sdf, void* workspace, size_t workspace_bytes, void* stream) {
    PM_REQUIRE(tri && sdf && workspace);
    PM_REQUIRE(F > 0 && F <= (1 << 26) && X > 0 && Y > 0 && Z > 0 && voxel_size > 0.f && trunc > 0.f);
    PM_REQUIRE((long)X * Y * Z < (1L << 31));
    PM_REQUIRE(workspace_bytes >= pm_mesh_sdf_bake_workspace_bytes(F));
    float* rec = (float*)workspace;
    hipLaunchKernelGGL(mesh_bake_prep_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, pm_stream(stream), tri, F, rec);
    PM_CHECK_LAUNCH();
    const int nbi = (X + MB_BRICK - 1) / MB_BRICK, nbj = (Y + MB_BRICK - 1) / MB_BRICK, nbk = (Z + MB_BRICK - 1) / MB_BRICK;
    const long bricks = (long)nbi * nbj * nbk;
    const dim3 grid((unsigned)((bricks + MB_WAVES - 1) / MB_WAVES)), block(64 * MB_WAVES);
    if (tri_cull)
        hipLaunchKernelGGL(mesh_bake_kernel<true>, grid, block, 0, pm_stream(stream), (const float*)rec, F, X, Y, Z, nbj, nbk,
                           voxel_size, cx, cy, cz, trunc, bricks, sdf);
    else
        hipLaunchKernelGGL(mesh_bake_kernel<false>, grid, block, 0, pm_stream(stream), (const float*)rec, F, X, Y, Z, nbj, nbk,
                           voxel_size, cx, cy, cz, trunc, bricks, sdf);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
