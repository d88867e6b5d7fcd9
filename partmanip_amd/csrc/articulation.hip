// A batched kinematic articulation in one launch per step (pm_articulation_step_f32): position targets in, joint state, body
// poses / velocities and the geometric Jacobian out, in the simulator's layouts that the task kernels read (task_grasp_cube.hip,
// task_open_drawer.hip).  Not physics: no dynamics, no contact, no gravity.  The tree comes from a URDF (partmanip_amd/urdf.py).
//
// Shape.  Per environment the call writes nb * 13 + (nb - 1) * 6 * nd + 2 * nd floats, and the Jacobian is about 96 % of them
// (13 bodies, 9 DOFs: 169 + 648 + 18), while the chain of body frames is serially dependent.  A lane that walked the chain and
// stored its own Jacobian would write runs of a few dwords 2.6 KB apart from its neighbours'.  So a block takes `eb` consecutive
// environments and works in stages, everything between them in LDS:
//   0. drive: thread i owns one (environment, DOF) pair: q' from the target (rate limit, joint limits, reset), qd' = (q' - q) / dt,
//      both written back to dof_state (runs of 2 nd dwords) and left in LDS;
//   1. chain: the first wave owns one environment per lane and walks the bodies in order (a parent precedes its children):
//      frame = parent o origin o joint in quaternions, leaving per body position + quaternion and per DOF the world axis in LDS.
//      The chain alone runs in float64 (its own frames kept as doubles in LDS for the children, sin / cos included) and rounds once
//      on the way out: a 64-body chain would otherwise stack 64 float32 products, and at a few hundred flops per environment next
//      to a launch the wider arithmetic is not what is timed.  The tree tables are read at wave-uniform addresses; an
//      environment's LDS rows have odd strides, so the lanes of a wave sit on different banks;
//   2. the whole block writes the block's CONTIGUOUS Jacobian range as a flat range, thread i computing dword i from LDS and the
//      body's ancestor mask (a revolute column is a x (p_body - p_joint) | a, and p_joint is the origin of the joint's own body; a
//      prismatic one a | 0), then one thread per (environment, body, component) sums the same entries times qd' into the body's
//      velocity, and the body rows go out as runs of nb * 13 dwords.
// Every global store is lane-consecutive; the chain stores nothing to memory.
//
// Independence.  An environment is computed from its own rows in an order that does not depend on N, eb or the block it lands in:
// its bits are the same alone and inside any batch, and a NaN stays inside its environment.  No atomics, no synchronisation.
//
// Resources and times: profiles/kinematics_timing.json (tools/time_kinematics.py).  Dynamic LDS per environment is (7 nb) | 1
// doubles (the chain's frames) and (13 nb + 5 nd) | 1 floats: 1596 B for the Franka (13 bodies, 9 DOFs), 8204 B at the 64 x 64
// limit; eb is chosen by ts_envs_per_block (at most 64, one per lane of the chain's wave; fewer while the grid would fall under
// TS_GRID_MIN or LDS over TS_LDS_MAX).
#include "common.h"
#include "task_common.h"                                      // ts_clamp, ts_envs_per_block, TS_LDS_MAX
#include "articulation_common.h"                              // the quaternion helpers, the frame step, ar_jentry

__global__ __launch_bounds__(AR_THREADS) void articulation_step_kernel(
    const int32_t* __restrict__ parent, const int32_t* __restrict__ jtype, const int32_t* __restrict__ dof,
    const float* __restrict__ origin_q, const float* __restrict__ origin_t, const float* __restrict__ axis,
    const unsigned long long* __restrict__ anc_mask, const float* __restrict__ dof_lo, const float* __restrict__ dof_hi,
    const float* __restrict__ vmax, float dt, const float* __restrict__ base_pose, long base_stride, float* __restrict__ dof_state,
    long dof_rows, const float* __restrict__ targets, long tgt_stride, const uint8_t* __restrict__ reset,
    const int32_t* __restrict__ rb_row0, long rb_stride, long rb_rows, const int32_t* __restrict__ dof_row0, long dof_stride, int N,
    int nb, int nd, int eb, int DS, int ES, float* __restrict__ rigid_body, float* __restrict__ jac) {
    extern __shared__ double ar_chain[];                      // [eb][DS] doubles: the chain's frames [nb][7]; then [eb][ES] floats
    float* ar_lds = (float*)(ar_chain + (long)eb * DS);
    __shared__ unsigned long long s_mask[AR_MAX];
    __shared__ int s_info[AR_MAX];                            // per DOF: its body | its joint type << 8, -1 where no body names it
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * eb;
    const int neb = min(eb, N - b0);
    const int RB = nb * 13;                                   // an environment's LDS row: rb [nb][13] | q' [nd] | qd' [nd] | axis [nd][3]

    if (tid < AR_MAX) s_info[tid] = -1;
    __syncthreads();
    if (tid < nb) {
        s_mask[tid] = anc_mask[tid];
        const int d = dof[tid], jt = jtype[tid];
        if ((jt == AR_REVOLUTE || jt == AR_PRISMATIC) && d >= 0 && d < nd) s_info[d] = tid | (jt << 8);
    }

    // 0. drive.  An environment whose DOF rows would fall outside dof_state is computed as NaN and stores nothing there.
    for (int i = tid; i < neb * nd; i += AR_THREADS) {
        const int e = i / nd, d = i - e * nd;
        const long b = b0 + e;
        const long row = dof_row0 ? (long)dof_row0[b] : b * dof_stride;
        float* E = ar_lds + e * ES + RB;
        float q = __builtin_nanf(""), qd = __builtin_nanf("");
        if (row >= 0 && row + nd <= dof_rows) {
            float* s = dof_state + (row + d) * 2;
            q = s[0], qd = s[1];
            if (targets) {
                const float t = targets[b * tgt_stride + d], lo = dof_lo[d], hi = dof_hi[d];
                float qn;
                if (reset && reset[b]) {
                    qn = ts_clamp(t, lo, hi), qd = 0.0f;
                } else {
                    if (vmax) {
                        const float m = vmax[d] * dt;
                        qn = q + ts_clamp(t - q, -m, m);
                    } else {
                        qn = t;
                    }
                    qn = ts_clamp(qn, lo, hi);
                    qd = (qn - q) / dt;
                }
                q = qn;
                s[0] = q, s[1] = qd;
            }
        }
        E[d] = q, E[nd + d] = qd;
    }
    __syncthreads();

    // 1. the chain, one environment per lane of the first wave
    if (tid < 64) {
        for (int e = tid; e < neb; e += 64) {
            float* rb = ar_lds + e * ES;
            double* fr = ar_chain + e * DS;
            const float* qs = rb + RB;
            float* ax = rb + RB + 2 * nd;
            const float* bp = base_pose + (long)(b0 + e) * base_stride;
            double base[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) base[c] = bp[c];
            ar_qunit(base + 3);
            for (int b = 0; b < nb; ++b) {
                const int p = parent[b];
                double pp[3], pq[4], pos[3], fq[4];
#pragma unroll
                for (int c = 0; c < 3; ++c) pp[c] = (p >= 0 && p < b) ? fr[p * 7 + c] : base[c];
#pragma unroll
                for (int c = 0; c < 4; ++c) pq[c] = (p >= 0 && p < b) ? fr[p * 7 + 3 + c] : base[3 + c];
                ar_frame_origin(pp, pq, origin_t, origin_q, b, pos, fq);
                const int jt = jtype[b], d = dof[b];
                if ((jt == AR_REVOLUTE || jt == AR_PRISMATIC) && d >= 0 && d < nd) {
                    const double al[3] = {axis[b * 3], axis[b * 3 + 1], axis[b * 3 + 2]};
                    double aw[3];
                    ar_qrot(fq, al, aw);
#pragma unroll
                    for (int c = 0; c < 3; ++c) ax[d * 3 + c] = (float)aw[c];
                    ar_frame_joint(jt, al, aw, (double)qs[d], pos, fq);
                }
                ar_qunit(fq);
#pragma unroll
                for (int c = 0; c < 3; ++c) fr[b * 7 + c] = pos[c], rb[b * 13 + c] = (float)pos[c];
#pragma unroll
                for (int c = 0; c < 4; ++c) fr[b * 7 + 3 + c] = fq[c], rb[b * 13 + 3 + c] = (float)fq[c];
            }
        }
    }
    __syncthreads();

    // 2. the block's Jacobian range, flat: dword i of [neb][nb - 1][6][nd]
    if (jac) {
        const int per_body = 6 * nd, per_env = (nb - 1) * per_body;
        float* g = jac + (long)b0 * per_env;
        for (int i = tid; i < neb * per_env; i += AR_THREADS) {
            const int e = i / per_env, rem = i - e * per_env;
            const int l = rem / per_body, rem2 = rem - l * per_body;
            const int r = rem2 / nd, d = rem2 - r * nd;
            const int info = s_info[d];
            float v = 0.0f;
            if (info >= 0 && ((s_mask[l + 1] >> d) & 1ull)) {
                const float* rb = ar_lds + e * ES;
                v = ar_jentry(rb, rb + RB + 2 * nd, l + 1, r, d, info);
            }
            g[i] = v;
        }
    }
    if (rigid_body) {
        // velocities: (J qd')[r] per (environment, body), summed over the ancestor DOFs in ascending order
        for (int i = tid; i < neb * nb * 6; i += AR_THREADS) {
            const int e = i / (nb * 6), rem = i - e * nb * 6;
            const int b = rem / 6, r = rem - b * 6;
            float* rb = ar_lds + e * ES;
            const float* qd = rb + RB + nd;
            const unsigned long long m = s_mask[b];
            float s = 0.0f;
            for (int d = 0; d < nd; ++d) {
                const int info = s_info[d];
                if (info >= 0 && ((m >> d) & 1ull)) s = s + ar_jentry(rb, rb + RB + 2 * nd, b, r, d, info) * qd[d];
            }
            rb[b * 13 + 7 + r] = s;
        }
        __syncthreads();
        // rows out: runs of nb * 13 dwords at the caller's rows; an environment whose rows would fall outside the tensor is skipped
        for (int i = tid; i < neb * RB; i += AR_THREADS) {
            const int e = i / RB, c = i - e * RB;
            const long b = b0 + e;
            const long row = rb_row0 ? (long)rb_row0[b] : b * rb_stride;
            if (row >= 0 && row + nb <= rb_rows) rigid_body[row * 13 + c] = ar_lds[e * ES + c];
        }
    }
}

extern "C" int pm_articulation_step_f32(const int32_t* parent, const int32_t* jtype, const int32_t* dof, const float* origin_q,
                                        const float* origin_t, const float* axis, const uint64_t* anc_mask, const float* dof_lo,
                                        const float* dof_hi, const float* vmax, float dt, const float* base_pose, long base_stride,
                                        float* dof_state, long dof_rows, const float* targets, long tgt_stride, const uint8_t* reset,
                                        const int32_t* rb_row0, long rb_stride, long rb_rows, const int32_t* dof_row0, long dof_stride,
                                        int N, int nb, int nd, float* rigid_body, float* jac, void* stream) {
    PM_REQUIRE(parent && jtype && dof && origin_q && origin_t && axis && anc_mask && dof_lo && dof_hi && base_pose && dof_state);
    PM_REQUIRE(N >= 1 && nb >= 1 && nb <= AR_MAX && nd >= 1 && nd <= AR_MAX);
    PM_REQUIRE(base_stride == 0 || base_stride >= 7);
    PM_REQUIRE(dof_rows >= nd && dof_rows < 2147483648L && (dof_row0 || (dof_stride >= nd && (N - 1) * dof_stride + nd <= dof_rows)));
    if (targets) PM_REQUIRE(dt > 0.0f && tgt_stride >= nd);    // a NaN dt is refused too
    if (rigid_body) PM_REQUIRE(rb_rows >= nb && rb_rows < 2147483648L && (rb_row0 || (rb_stride >= nb && (N - 1) * rb_stride + nb <= rb_rows)));
    const int DS = (7 * nb) | 1, ES = (13 * nb + 5 * nd) | 1;
    const long env_bytes = 8L * DS + 4L * ES;
    const int eb = ts_envs_per_block(N, env_bytes, AR_MAX, TS_LDS_MAX);
    PM_REQUIRE(eb * env_bytes <= TS_LDS_MAX);
    const unsigned grid = (unsigned)((N + eb - 1) / eb);
    hipLaunchKernelGGL(articulation_step_kernel, dim3(grid), dim3(AR_THREADS), (size_t)(eb * env_bytes), pm_stream(stream), parent,
                       jtype, dof, origin_q, origin_t, axis, (const unsigned long long*)anc_mask, dof_lo, dof_hi, vmax, dt, base_pose,
                       base_stride, dof_state, dof_rows, targets, tgt_stride, reset, rb_row0, rb_stride, rb_rows, dof_row0, dof_stride,
                       N, nb, nd, eb, DS, ES, rigid_body, jac);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
