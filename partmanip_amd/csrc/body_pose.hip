// Body poses of a whole scene in one launch: the (pose_R, pose_T) the depth and the frame camera take, for every body an environment
// holds and not only the 13 parts the task kernels pose.  One lane per (environment, slot): slot m of environment b is row
// rows[b, m] of the flat rigid-body tensor; T = its position, R = quat_to_mat(its quaternion), times C_m for the first MC slots (the
// robot's mesh-frame matrices).  The arithmetic is task_common.h's, operation for operation: ts_quat_to_mat, and the product of
// ts_part_poses summed over the inner index left to right, so a slot the task kernels pose as well carries the same bits here.
//
// Memory safety.  A row index outside [0, nrows) gives a NaN pose (the rasteriser skips a triangle with a non-finite corner) and its
// address is never formed.  Every store lands in [0, 9 B M) of pose_R and [0, 3 B M) of pose_T.  No workspace, no atomics,
// stream-ordered, never synchronises.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 44 VGPRs, 25 SGPRs, no scratch, no LDS, occupancy 8 waves / SIMD.
#include "common.h"
#include "task_common.h"

#define BP_THREADS 256

__global__ __launch_bounds__(BP_THREADS) void body_pose_gather_kernel(const float* __restrict__ rigid_body, long nrows,
                                                                       const int32_t* __restrict__ rows, long total, int M,
                                                                       const float* __restrict__ part_C, int MC,
                                                                       float* __restrict__ pose_R, float* __restrict__ pose_T) {
    const long w = (long)blockIdx.x * BP_THREADS + threadIdx.x;
    if (w >= total) return;
    const int m = (int)(w % M);
    const long row = rows[w];
    float Rm[9], T[3];
    if (row < 0 || row >= nrows) {
#pragma unroll
        for (int c = 0; c < 9; ++c) Rm[c] = __builtin_nanf("");
        T[0] = T[1] = T[2] = __builtin_nanf("");
    } else {
        const float* src = rigid_body + row * 13;
        T[0] = src[0], T[1] = src[1], T[2] = src[2];
        float q[4] = {src[3], src[4], src[5], src[6]}, Q[9];
        ts_quat_to_mat(q, Q);
        if (m < MC) {
            const float* Cp = part_C + 9L * m;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rm[3 * i + j] = (Q[3 * i] * Cp[j] + Q[3 * i + 1] * Cp[3 + j]) + Q[3 * i + 2] * Cp[6 + j];
        } else {
#pragma unroll
            for (int c = 0; c < 9; ++c) Rm[c] = Q[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) pose_R[w * 9 + c] = Rm[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) pose_T[w * 3 + c] = T[c];
}

extern "C" int pm_body_pose_gather_f32(const float* rigid_body, long nrows, const int32_t* rows, int B, int M, const float* part_C,
                                       int MC, float* pose_R, float* pose_T, void* stream) {
    PM_REQUIRE(rigid_body && rows && pose_R && pose_T);
    PM_REQUIRE(nrows >= 1 && B >= 1 && M >= 1 && MC >= 0 && MC <= M && (MC == 0 || part_C));
    const long total = (long)B * M;
    const long blocks = (total + BP_THREADS - 1) / BP_THREADS;
    PM_REQUIRE(blocks < (1L << 31));
    hipLaunchKernelGGL(body_pose_gather_kernel, dim3((unsigned)blocks), dim3(BP_THREADS), 0, pm_stream(stream), rigid_body, nrows, rows,
                       total, M, part_C, MC, pose_R, pose_T);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
