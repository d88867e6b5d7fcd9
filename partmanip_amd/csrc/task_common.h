// What the task-step kernels share (task_grasp_cube.hip, task_open_drawer.hip): the small arithmetic helpers, each written once in the
// reference's association so that every kernel rounds it alike, the layout of a post kernel's scalars and the host rule for the
// environments per block.  The stages of the two post kernels (gather, part poses, rows out) are still written out in each file.
#pragma once

#define TS_SC 11                                             // a post kernel's scalars per environment: rew, extras[8], success, is_reached
#define TS_GRID_MIN 512                                      // blocks below which a launch takes fewer environments per block

// torch_jit_utils.py:375-403, q = (i, j, k, r)
__device__ __forceinline__ void ts_quat_to_mat(const float* q, float* m) {
    const float i = q[0], j = q[1], k = q[2], r = q[3];
    const float two_s = 2.0f / (((i * i + j * j) + k * k) + r * r);
    m[0] = 1.0f - two_s * (j * j + k * k);
    m[1] = two_s * (i * j - k * r);
    m[2] = two_s * (i * k + j * r);
    m[3] = two_s * (i * j + k * r);
    m[4] = 1.0f - two_s * (i * i + k * k);
    m[5] = two_s * (j * k - i * r);
    m[6] = two_s * (i * k - j * r);
    m[7] = two_s * (j * k + i * r);
    m[8] = 1.0f - two_s * (i * i + j * j);
}

__device__ __forceinline__ float ts_scale(float x, float lo, float hi) { return (2.0f * (x - lo)) / (hi - lo) - 1.0f; }
__device__ __forceinline__ float ts_norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// torch.max / torch.maximum of two tensors: NaN if either is.  torch.clamp with scalar bounds: a NaN passes through.
__device__ __forceinline__ float ts_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }
__device__ __forceinline__ float ts_clamp(float v, float lo, float hi) { return v != v ? v : fmaxf(fminf(v, hi), lo); }

// Environments per block of a post kernel: as many as LDS holds (eb_max at most, halving), fewer while the grid would leave most of the
// chip idle, but not below 4 for that reason (same bits either way).
static inline int ts_envs_per_block(int N, long bytes_per_env, int eb_max, long lds_max) {
    int eb = eb_max;
    while (eb > 1 && (eb * bytes_per_env > lds_max || (eb > 4 && (N + eb - 1) / eb < TS_GRID_MIN))) eb >>= 1;
    return eb;
}
