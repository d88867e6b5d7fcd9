// What the task-step kernels share (task_grasp_cube.hip, task_open_drawer.hip): the small arithmetic helpers, each written once in the
// reference's association so that every kernel rounds it alike; the ONE description of a post kernel's dynamic LDS (ts_env_floats on
// host and device, ts_carve in the kernel); the task-independent stages of the two post kernels (flat ranges in and out, the root-row
// gather, the part poses of waves 1-3, the DOF columns, rows out, the flag stores); and the host side of a post
// launch (ts_post_launch: parts asked for, environments per block, LDS bytes, grid).  The stage helpers are plain
// __device__ __forceinline__ functions over their call sites' arguments: thread count and strides come in as arguments, nothing
// depends on a macro of the including file.  Both post kernels built from them keep the registers, occupancy and LDS they had with
// the stages written out, and give the same bits on the device (profiles/task_stage_sharing_ab.txt).
#pragma once

#define TS_SC 11                                             // a post kernel's scalars per environment: rew, extras[8], success, is_reached
#define TS_GRID_MIN 512                                      // blocks below which a launch takes fewer environments per block
#define TS_EB_MAX 32                                         // environments per block of a post kernel (at most; wave 0 holds one per lane)
#define TS_LDS_MAX 49152                                     // bytes of dynamic LDS a block may ask for

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

// ---------------------------------------------------------------------------------------------------- a post kernel's LDS
// In floats, per block of eb environments:
//   rb [eb][RB] | dof [eb][DF] | obj [eb][7] | ns [eb][W] | sc [eb][TS_SC] | extra [eb][X] | R [eb][M][9] | T [eb][M][3]
// RB, DF: the floats of an environment's staged rigid-body and DOF rows; W: the width of its normal_state row; X: the task's own
// segment (0 for grasp_cube, the 24 floats of open_drawer's handle box); M: the posed parts (0 when no pose is asked for).
// ts_env_floats is what the host sizes the launch with and ts_carve what the kernel addresses: a segment is added in both or in none.
struct ts_lds {
    float *rb, *dof, *obj, *ns, *sc, *extra, *R, *T;
};

__host__ __device__ __forceinline__ long ts_env_floats(int RB, int DF, int W, int X, int M) {
    return (long)RB + DF + 7 + W + TS_SC + X + (long)M * 12;
}

__device__ __forceinline__ ts_lds ts_carve(float* base, int eb, int RB, int DF, int W, int X, int M) {
    ts_lds s;
    s.rb = base;
    s.dof = s.rb + (long)eb * RB;
    s.obj = s.dof + eb * DF;
    s.ns = s.obj + eb * 7;
    s.sc = s.ns + eb * W;
    s.extra = s.sc + eb * TS_SC;
    s.R = s.extra + eb * X;
    s.T = s.R + eb * M * 9;
    return s;
}

// ---------------------------------------------------------------------------------------------------- the stages
// A flat range, thread i moving dword i: state into LDS, finished rows (pose_R, pose_T, part_bbox) out of it.
__device__ __forceinline__ void ts_copy(float* dst, const float* src, int n, int tid, int nt) {
    for (int i = tid; i < n; i += nt) dst[i] = src[i];
}

// The 7 pose floats of actor `actor`'s root row, for the neb environments from b0 on: obj [neb][7].
__device__ __forceinline__ void ts_gather_root(float* obj, const float* root, int b0, int neb, int na, int actor, int tid, int nt) {
    for (int i = tid; i < neb * 7; i += nt) {
        const int e = i / 7, c = i - e * 7;
        obj[i] = root[((long)(b0 + e) * na + actor) * 13 + c];
    }
}

// One (environment, part) pose per thread, w = w0, w0 + nw, ...: part p of environment e is row part_idx[p] of the nslots staged rows
// (rb [neb][RB]): T its position, R = quat_to_mat(its quaternion) C_p (sum over the inner index left to right), or the matrix itself
// without part_C.  An index outside [0, nslots) gives a NaN row; its address is never formed.
__device__ __forceinline__ void ts_part_poses(const float* rb, int RB, int neb, const int32_t* part_idx, int nslots, const float* part_C,
                                              int M, float* s_R, float* s_T, int w0, int nw) {
    for (int w = w0; w < neb * M; w += nw) {
        const int e = w / M, p = w - e * M;
        const int slot = part_idx[p];
        float Rm[9], T[3];
        if (slot < 0 || slot >= nslots) {
#pragma unroll
            for (int c = 0; c < 9; ++c) Rm[c] = __builtin_nanf("");
            T[0] = T[1] = T[2] = __builtin_nanf("");
        } else {
            const float* src = rb + e * RB + slot * 13;
            T[0] = src[0], T[1] = src[1], T[2] = src[2];
            float Q[9];
            ts_quat_to_mat(src + 3, Q);
            if (part_C) {
                const float* Cp = part_C + p * 9;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        Rm[3 * i + j] = (Q[3 * i] * Cp[j] + Q[3 * i + 1] * Cp[3 + j]) + Q[3 * i + 2] * Cp[6 + j];
            } else {
#pragma unroll
                for (int c = 0; c < 9; ++c) Rm[c] = Q[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) s_R[w * 9 + c] = Rm[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) s_T[w * 3 + c] = T[c];
    }
}

// Columns [col, col + nd) of a normal_state row: the scaled DOF positions; [col + nd, col + 2 nd): the velocities.  dof [nd][2].
__device__ __forceinline__ void ts_dof_columns(float* ns, int col, const float* dof, int nd, const float* dof_lo, const float* dof_hi) {
    for (int d = 0; d < nd; ++d) {
        ns[col + d] = ts_scale(dof[2 * d], dof_lo[d], dof_hi[d]);
        ns[col + nd + d] = dof[2 * d + 1];
    }
}

// neb rows of w floats, row e read at src + e * sstride and written at row b0 + e of g (gstride floats apart), thread i moving
// element i of the (row, column) list: runs of w consecutive dwords at the caller's stride.
__device__ __forceinline__ void ts_rows_out(float* g, long gstride, int b0, const float* src, int sstride, int w, int neb, int tid,
                                            int nt) {
    for (int i = tid; i < neb * w; i += nt) {
        const int e = i / w, c = i - e * w;
        g[(long)(b0 + e) * gstride + c] = src[e * sstride + c];
    }
}

// rew / success / is_reached of environment b from its scalars sc [TS_SC]; returns success.
__device__ __forceinline__ bool ts_store_flags(const float* sc, int b, float* rew, uint8_t* success, uint8_t* is_reached) {
    const bool succ = sc[9] != 0.0f;
    if (rew) rew[b] = sc[0];
    if (success) success[b] = succ;
    if (is_reached) is_reached[b] = sc[10] != 0.0f;
    return succ;
}

// ---------------------------------------------------------------------------------------------------- the host side
// Environments per block of a post kernel: as many as LDS holds (eb_max at most, halving), fewer while the grid would leave most of the
// chip idle, but not below 4 for that reason (same bits either way).
static inline int ts_envs_per_block(int N, long bytes_per_env, int eb_max, long lds_max) {
    int eb = eb_max;
    while (eb > 1 && (eb * bytes_per_env > lds_max || (eb > 4 && (N + eb - 1) / eb < TS_GRID_MIN))) eb >>= 1;
    return eb;
}

// What both post launchers do after their own argument checks: the parts the kernel poses (none unless a pose output is asked
// for), the environments per block, the bytes of dynamic LDS and the grid.  False where one environment does not fit the LDS cap.
struct ts_launch {
    int Mk, eb;
    size_t lds;
    unsigned grid;
};

static inline bool ts_post_launch(int N, int RB, int DF, int W, int X, bool poses, int M, ts_launch* L) {
    L->Mk = poses ? M : 0;
    const long env_bytes = 4 * ts_env_floats(RB, DF, W, X, L->Mk);
    L->eb = ts_envs_per_block(N, env_bytes, TS_EB_MAX, TS_LDS_MAX);
    L->lds = (size_t)(L->eb * env_bytes);
    L->grid = (unsigned)((N + L->eb - 1) / L->eb);
    return L->eb * env_bytes <= TS_LDS_MAX;
}
