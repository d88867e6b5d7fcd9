// Device helpers shared by the task-step kernels (task_grasp_cube.hip, task_open_drawer.hip).
#pragma once

// torch_jit_utils.py:375-403, q = (i, j, k, r)
__device__ __forceinline__ void gc_quat_to_mat(const float* q, float* m) {
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

__device__ __forceinline__ float gc_scale(float x, float lo, float hi) { return (2.0f * (x - lo)) / (hi - lo) - 1.0f; }
__device__ __forceinline__ float gc_norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }
