// The grasp_cube task step (the reference's tasks/grasp_cube.py, tasks/load_robot.py, tasks/hand_base.py:363-392, 431-441) as two
// launches: grasp_cube_post_kernel after physics (observation rows, reward, flags, part poses) and franka_control_kernel before it
// (joint targets by damped least squares, episode bookkeeping; instantiated for the fixed-base Franka and for the mobile one with
// three virtual base joints in front of the arm, pm_franka_control_f32 and pm_franka_control_mobile_f32).  The reference spends
// several dozen tensor-library launches per step on this (a 24-candidate gather / argmin, a batched 6 x 6 inverse, many cats), each
// of them launch-bound at 4096 environments.
//
// Shape.  An environment costs a few hundred flops over about 1 KB of state (14 bodies x 13 floats, 9 DOFs x 2, one root row, two
// 6 x 9 Jacobian rows) and writes about 0.9 KB (37 + 25 + 8 + 12 x 12 floats), so the question is how a wave reads and writes that
// state, not the arithmetic.  The state of consecutive environments is CONTIGUOUS in every simulator tensor, so a block takes `eb`
// consecutive environments and
//   1. copies their rigid-body and DOF rows into LDS as one flat range, lane i reading dword i (whole 256-byte wave loads whatever
//      nb and nd are), plus the 7 pose floats of the object's root row;
//   2. computes out of LDS: the first wave owns one environment per lane (tip pose, the 24-candidate rotation choice, reward,
//      flags: one serial chain per environment), the other three waves own one (environment, part) pose each; results go back to LDS
//      as rows laid out exactly as the outputs are;
//   3. copies the rows out, lane i writing dword i of a row range: pose_R / pose_T of the block are one contiguous range, and the
//      observation rows (row stride from the caller, 4-byte aligned only) are written as runs of 37 / 25 consecutive dwords.
// The environment rows in LDS have odd strides where the width is odd (19 + 2 nd, 9, 3), so per-lane row writes do not collide on
// banks; the rigid-body rows (stride 13 nb) are read two-way conflicted at nb = 14, which is a few dozen LDS cycles per block.
//
// Dropped without a measurement, by construction: one environment per lane reading its state straight from memory.  A lane would
// then walk a 728-byte row while its neighbours walk theirs: every load instruction of the wave touches 64 different cache lines
// for 4 bytes each, and the pose outputs would be 36-byte runs per lane.  Staging costs one barrier and 20-50 KB of LDS.  Also
// dropped: one kernel per output group (the launches are the cost this file removes) and 16-byte loads (the ranges start wherever
// eb * nb * 13 puts them and the whole input is 3 MB at 4096 environments).
//
// Arithmetic.  fp32, no contraction (-ffp-contract=off), each group in the reference's association so that the error against the
// float64 reference is the reference's own float32 error: sum q^2 left to right, 2 (x - lo) / (hi - lo) - 1 as written, the reward
// ((reaching + 0.5 rot) + 5 close) + 20 goal, then + 3 success.  The rotation choice compares the candidates' traces (the
// reference takes argmin acos(clamp((tr - 1) / 2)), the same choice away from ties; no acos here); the first maximum wins.
// The control kernel forms A = J J^T + 0.05^2 I (6 x 6, symmetric positive definite) in registers, factors it by Cholesky and
// solves twice; the reference inverts by LU, so this group differs from it by rounding only (tests: within 4 e_ref).
//
// Independence.  An environment is computed by one thread from its own rows, in an order that does not depend on N, eb or the
// block it lands in: its bits are the same alone and inside any batch, and a NaN stays inside its environment.  The only
// cross-environment values are the two int32 sums of the control kernel (one integer atomic per wave, exact in any order).
//
// What is shared.  The LDS layout (ts_env_floats / ts_carve), the flat copies, the root-row gather, the part poses of waves 1-3, the
// DOF columns, the row-out loops, the flag stores and the host side of the launch (ts_post_launch) are the helpers of task_common.h,
// shared with open_drawer_post_kernel; this file keeps the rotation choice, the per-environment chain of wave 0 and the proprio row.
// One stage stays written out in both files: the tip average with the gripper length.  As a shared helper (average, then length,
// then the caller's use of the average) it gives this kernel 78 VGPRs against the 76 of the loop written out (the loads of both
// tip rows then precede every store to the row in LDS), and a stage moves only if no kernel pays a register for it.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): grasp_cube_post_kernel 76 VGPRs, 106 SGPRs, no scratch, 6 waves /
// SIMD; dynamic LDS eb * ts_env_floats(13 nb, 2 nd, 19 + 2 nd, 0, M) floats (task_common.h) = eb * (13 nb + 4 nd + 37 + 12 M) floats =
// 1596 B per environment at nb = 14, nd = 9, M = 12: 12.8 KB with the 8
// environments per block chosen at 4096 environments (512 blocks), never more than 48 KB.  franka_control_kernel<0> 58 VGPRs, 58 SGPRs,
// no scratch, 8 waves / SIMD (as before it became a template); <3>, the mobile Franka, 62 VGPRs, 58 SGPRs, no scratch, 8 waves / SIMD; LDS
// eb * (6 na + 1) floats, na = nd - 2 - NB arm DOFs = 1.4 KB at 8 environments per block for either robot (na = 7).  Times:
// profiles/grasp_cube_timing.json and, for the mobile robot, profiles/mobile_franka_timing.json (tools/time_mobile_franka.py).
#include "common.h"
#include "task_common.h"                                      // ts_*: the helpers, stages and LDS layout shared with task_open_drawer.hip

#define GC_THREADS 256
#define FC_THREADS 64
#define FC_ND_MAX 64

// torch_jit_utils.py:412-425: candidate c takes columns (a, b) = IND[c % 6] of R, row 0 of both negated for c < 12, row 1 for
// 6 <= c < 18, third column = first x second; the candidate of largest trace, the lowest c on ties.  o: 3 x 3 row-major.
__device__ __forceinline__ void gc_deambiguity(const float* q, float* o) {
    float R[9];
    ts_quat_to_mat(q, R);
    float best = 0.f;
    int bc = 0;
#pragma unroll
    for (int c = 0; c < 24; ++c) {
        const int p = c % 6;
        const int a = p == 0 || p == 1 ? 0 : (p == 2 || p == 3 ? 1 : 2);
        const int b = p == 0 || p == 5 ? 1 : (p == 1 || p == 2 ? 2 : 0);
        const float a0 = c < 12 ? -R[a] : R[a], b0 = c < 12 ? -R[b] : R[b];
        const float a1 = (c >= 6 && c < 18) ? -R[3 + a] : R[3 + a], b1 = (c >= 6 && c < 18) ? -R[3 + b] : R[3 + b];
        const float tr = (a0 + b1) + (a0 * b1 - a1 * b0);
        if (c == 0 || tr > best) best = tr, bc = c;
    }
    const int p = bc % 6;
    const int a = p == 0 || p == 1 ? 0 : (p == 2 || p == 3 ? 1 : 2);
    const int b = p == 0 || p == 5 ? 1 : (p == 1 || p == 2 ? 2 : 0);
    const float s0 = bc < 12 ? -1.f : 1.f, s1 = (bc >= 6 && bc < 18) ? -1.f : 1.f;
    const float a0 = s0 * R[a], a1 = s1 * R[3 + a], a2 = R[6 + a];
    const float b0 = s0 * R[b], b1 = s1 * R[3 + b], b2 = R[6 + b];
    o[0] = a0, o[1] = b0, o[2] = a1 * b2 - a2 * b1;
    o[3] = a1, o[4] = b1, o[5] = a2 * b0 - a0 * b2;
    o[6] = a2, o[7] = b2, o[8] = a0 * b1 - a1 * b0;
}

__global__ __launch_bounds__(GC_THREADS) void grasp_cube_post_kernel(
    const float* __restrict__ rigid_body, const float* __restrict__ dof_state, const float* __restrict__ root, int N, int nb, int nd,
    int na, int obj_actor, int ltip, int rtip, const float* __restrict__ dof_lo, const float* __restrict__ dof_hi,
    const float* __restrict__ pose_lo, const float* __restrict__ pose_hi, const float* __restrict__ goal, float goal_thresh,
    const float* __restrict__ obj_default_pos, const int32_t* __restrict__ part_body, const float* __restrict__ part_C, int M, int eb,
    float* __restrict__ normal_state, long ns_stride, float* __restrict__ proprio, long pr_stride, float* __restrict__ rew,
    uint8_t* __restrict__ success, uint8_t* __restrict__ is_reached, float* __restrict__ extras, long ex_stride,
    float* __restrict__ pose_R, float* __restrict__ pose_T) {
    extern __shared__ float gc_lds[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * eb;
    const int neb = min(eb, N - b0);
    const int RB = nb * 13, DF = nd * 2, W = 19 + 2 * nd;
    const ts_lds sh = ts_carve(gc_lds, eb, RB, DF, W, 0, M);

    // 1. the block's state, flat
    ts_copy(sh.rb, rigid_body + (long)b0 * RB, neb * RB, tid, GC_THREADS);
    ts_copy(sh.dof, dof_state + (long)b0 * DF, neb * DF, tid, GC_THREADS);
    ts_gather_root(sh.obj, root, b0, neb, na, obj_actor, tid, GC_THREADS);
    __syncthreads();

    // 2. compute
    if (tid < 64) {
        for (int e = tid; e < neb; e += 64) {
            const float* L = sh.rb + e * RB + ltip * 13;
            const float* Rt = sh.rb + e * RB + rtip * 13;
            const float* obj = sh.obj + e * 7;
            float* ns = sh.ns + e * W;
            float tip[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                tip[c] = (L[c] + Rt[c]) / 2.0f;
                ns[c] = ts_scale(tip[c], pose_lo[c], pose_hi[c]);
            }
            const float gl = ts_norm3(L[0] - Rt[0], L[1] - Rt[1], L[2] - Rt[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) ns[7 + c] = ts_scale(obj[c], pose_lo[c], pose_hi[c]);
            float o[9], h[9];
            gc_deambiguity(obj + 3, o);
#pragma unroll
            for (int c = 0; c < 9; ++c) ns[10 + c] = o[c];
            ts_dof_columns(ns, 19, sh.dof + e * DF, nd, dof_lo, dof_hi);
            // grasp_cube.py:73-113
            const float dist = ts_norm3(tip[0] - obj[0], tip[1] - obj[1], tip[2] - obj[2]);
            const bool reached = dist < 0.02f;
            const float reaching = -dist;
            const float close = reached ? (0.1f - gl) : 0.1f * (gl - 0.1f);
            ts_quat_to_mat(tip + 3, h);
            const float down = -h[8];
            float p1 = 0.f, p2 = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float u1 = fabsf(h[3 * r] * o[3 * r]) + fabsf(h[3 * r + 1] * o[3 * r + 1]);
                const float u2 = fabsf(h[3 * r] * o[3 * r + 1]) + fabsf(h[3 * r + 1] * o[3 * r]);
                p1 = r == 0 ? u1 : p1 + u1;
                p2 = r == 0 ? u2 : p2 + u2;
            }
            const float rot = (down + ts_max(p1, p2)) - 3.0f;
            const float dgoal = ts_norm3(obj[0] - goal[0], obj[1] - goal[1], obj[2] - goal[2]);
            const float gap = 0.2f - dgoal;
            const float rgoal = reached ? (gap != gap ? gap : fmaxf(gap, 0.0f)) : 0.0f;
            const bool succ = (dgoal <= goal_thresh) && reached;
            float rw = ((reaching + 0.5f * rot) + 5.0f * close) + 20.0f * rgoal;
            rw = rw + (succ ? 3.0f : 0.0f);
            float* sc = sh.sc + e * TS_SC;
            sc[0] = rw;
            sc[1] = reaching, sc[2] = close, sc[3] = rot, sc[4] = rgoal;
            sc[5] = ts_norm3(obj[0] - obj_default_pos[0], obj[1] - obj_default_pos[1], obj[2] - obj_default_pos[2]);
            sc[6] = rw, sc[7] = obj[2], sc[8] = obj[2] > 0.1f ? 1.0f : 0.0f;
            sc[9] = succ ? 1.0f : 0.0f, sc[10] = reached ? 1.0f : 0.0f;
        }
    } else if (pose_R || pose_T) {
        ts_part_poses(sh.rb, RB, neb, part_body, nb, part_C, M, sh.R, sh.T, tid - 64, GC_THREADS - 64);
    }
    __syncthreads();

    // 3. rows out
    if (normal_state) ts_rows_out(normal_state, ns_stride, b0, sh.ns, W, W, neb, tid, GC_THREADS);
    if (proprio) {
        const int Wp = 7 + 2 * nd;
        for (int i = tid; i < neb * Wp; i += GC_THREADS) {
            const int e = i / Wp, c = i - e * Wp;
            proprio[(long)(b0 + e) * pr_stride + c] = sh.ns[e * W + (c < 7 ? c : c + 12)];
        }
    }
    if (extras) ts_rows_out(extras, ex_stride, b0, sh.sc + 1, TS_SC, 8, neb, tid, GC_THREADS);
    if (tid < neb) ts_store_flags(sh.sc + tid * TS_SC, b0 + tid, rew, success, is_reached);
    if (pose_R) ts_copy(pose_R + (long)b0 * M * 9, sh.R, neb * M * 9, tid, GC_THREADS);
    if (pose_T) ts_copy(pose_T + (long)b0 * M * 3, sh.T, neb * M * 3, tid, GC_THREADS);
}

extern "C" int pm_grasp_cube_post_f32(const float* rigid_body, const float* dof_state, const float* root, int N, int nb, int nd,
                                      int na, int obj_actor, int ltip, int rtip, const float* dof_lo, const float* dof_hi,
                                      const float* pose_lo, const float* pose_hi, const float* goal, float goal_thresh,
                                      const float* obj_default_pos, const int32_t* part_body, const float* part_C, int M,
                                      float* normal_state, long ns_stride, float* proprio, long pr_stride, float* rew,
                                      uint8_t* success, uint8_t* is_reached, float* extras, long ex_stride, float* pose_R,
                                      float* pose_T, void* stream) {
    PM_REQUIRE(rigid_body && dof_state && root && dof_lo && dof_hi && pose_lo && pose_hi && goal && obj_default_pos);
    PM_REQUIRE(N >= 1 && nb >= 1 && nd >= 1 && na >= 1);
    PM_REQUIRE(obj_actor >= 0 && obj_actor < na && ltip >= 0 && ltip < nb && rtip >= 0 && rtip < nb);
    PM_REQUIRE(!normal_state || ns_stride >= 19 + 2L * nd);
    PM_REQUIRE(!proprio || pr_stride >= 7 + 2L * nd);
    PM_REQUIRE(!extras || ex_stride >= 8);
    const bool poses = pose_R || pose_T;
    PM_REQUIRE(!poses || (part_body && M >= 1));
    PM_REQUIRE((long)nb * 13 + nd * 2 <= 12000);
    ts_launch L;
    PM_REQUIRE(ts_post_launch(N, nb * 13, nd * 2, 19 + 2 * nd, 0, poses, M, &L));
    hipLaunchKernelGGL(grasp_cube_post_kernel, dim3(L.grid), dim3(GC_THREADS), L.lds, pm_stream(stream), rigid_body, dof_state, root,
                       N, nb, nd, na, obj_actor, ltip, rtip, dof_lo, dof_hi, pose_lo, pose_hi, goal, goal_thresh, obj_default_pos,
                       part_body, part_C, L.Mk, L.eb, normal_state, ns_stride, proprio, pr_stride, rew, success, is_reached, extras,
                       ex_stride, pose_R, pose_T);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

// ---------------------------------------------------------------------------------------------------- before physics
// One wave per block, one environment per lane.  The block first averages the two link rows of the Jacobian over the arm DOFs into
// LDS (lane i reads element i of the block's (environment, row, DOF) list: runs of na consecutive dwords out of rows of nd),
// as [eb][6 * na + 1] (an odd stride where na is even, and 6 na is always even: the lanes' rows start on different banks).
//
// NB = the number of virtual prismatic base joints in front of the arm (load_robot.py's `self.mobile * 3`): 0 for the fixed-base
// Franka (pm_franka_control_f32), 3 for the mobile one (pm_franka_control_mobile_f32).  The arm is then DOFs [NB, nd - 2), na =
// nd - 2 - NB, and the loader starts each run at column NB: the base's Jacobian columns never reach LDS.  With NB = 3 the lane also
// reads the 9 floats of base_R (the same address in every lane: scalar loads), forms db = 0.005 a[:3], the base targets q + base_R^T
// db (sum over j left to right, as a matrix product does) and takes db off the first three entries of dpose.  One template, two
// instantiations: the Cholesky solve and the bookkeeping exist once, and NB = 0 compiles to the arithmetic it always had.
template <int NB>
__global__ __launch_bounds__(FC_THREADS) void franka_control_kernel(
    const float* __restrict__ actions, long act_stride, int A, const float* __restrict__ dof_state, const float* __restrict__ jac,
    int N, int nd, int nl, int jl, int jr, const float* __restrict__ dof_lo, const float* __restrict__ dof_hi,
    const float* __restrict__ default_dof_pos, float dt, int drive_mode, const float* __restrict__ base_R,
    const float* __restrict__ rew, uint8_t* __restrict__ success, int64_t* __restrict__ progress, int explore_step,
    int max_episode_length, int train, int eb, float* __restrict__ pos_act, float* __restrict__ epis_max_rew,
    int64_t* __restrict__ epis_max_step, uint8_t* __restrict__ reset, uint8_t* __restrict__ reset_succ, int32_t* __restrict__ counters,
    int slot) {
    extern __shared__ float fc_J[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * eb;
    const int neb = min(eb, N - b0);
    const int na = nd - 2 - NB, JS = 6 * na + 1;
    if (blockIdx.x == 0 && tid == 0) counters[2 * (1 - slot)] = 0, counters[2 * (1 - slot) + 1] = 0;
    if (drive_mode == 0) {
        for (int i = tid; i < neb * 6 * na; i += FC_THREADS) {
            const int e = i / (6 * na), rem = i - e * 6 * na, r = rem / na, k = rem - r * na;
            const long base = (long)(b0 + e) * nl;
            const float l = jac[((base + jl) * 6 + r) * nd + NB + k], rr = jac[((base + jr) * 6 + r) * nd + NB + k];
            fc_J[e * JS + rem] = (l + rr) / 2.0f;
        }
        __syncthreads();
    }
    const bool live = tid < neb;
    const long b = b0 + tid;
    int n_succ = 0, n_reset = 0;
    if (live) {
        const float* a = actions + b * act_stride;
        const float* qs = dof_state + b * nd * 2;
        float* out = pos_act + b * nd;
        bool rst;
        const bool succ = success[b] != 0;
        int64_t prog = progress[b];
        if (train) {
            const float r = rew[b], mr = epis_max_rew[b];
            int64_t ms = r < mr ? epis_max_step[b] : prog;
            const float nmr = ts_max(r, mr);                                            // torch.maximum
            rst = (prog >= ms + explore_step) || succ;
            reset_succ[b] = succ;
            epis_max_step[b] = rst ? 0 : ms;
            epis_max_rew[b] = rst ? -100.0f : nmr;
        } else {
            rst = prog >= max_episode_length;
            if (rst) epis_max_step[b] = 0, epis_max_rew[b] = -100.0f;
        }
        reset[b] = rst;
        n_succ = succ, n_reset = rst;
        if (rst) {
            progress[b] = 0;
            success[b] = 0;
            for (int d = 0; d < nd; ++d) out[d] = default_dof_pos[d];
        } else {
            float db[3] = {0.f, 0.f, 0.f};
            if (NB > 0) {                                       // load_robot.py:98-100
#pragma unroll
                for (int j = 0; j < 3; ++j) db[j] = a[j] * 0.005f;
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const float s = (base_R[i] * db[0] + base_R[3 + i] * db[1]) + base_R[6 + i] * db[2];
                    out[i] = ts_clamp(qs[2 * i] + s, dof_lo[i], dof_hi[i]);
                }
            }
            a += NB, qs += 2 * NB, out += NB;                   // the arm and the fingers, as load_robot.py's raw_output[..., 3:]
            const float* lo = dof_lo + NB;
            const float* hi = dof_hi + NB;
            const int nf = na + 2;
            if (drive_mode == 0) {
                const float* J = fc_J + tid * JS;
                float Am[6][6], x[6];
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = 0; j < 6; ++j) Am[i][j] = 0.f;
                for (int k = 0; k < na; ++k) {
                    float c[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) c[i] = J[i * na + k];
#pragma unroll
                    for (int i = 0; i < 6; ++i)
#pragma unroll
                        for (int j = 0; j <= i; ++j) Am[i][j] += c[i] * c[j];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) Am[i][i] += 0.0025f;
                // Cholesky A = L L^T in place (lower), then L y = dpose, L^T x = y
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    float d = Am[j][j];
#pragma unroll
                    for (int k = 0; k < j; ++k) d -= Am[j][k] * Am[j][k];
                    d = sqrtf(d);
                    Am[j][j] = d;
#pragma unroll
                    for (int i = j + 1; i < 6; ++i) {
                        float s = Am[i][j];
#pragma unroll
                        for (int k = 0; k < j; ++k) s -= Am[i][k] * Am[j][k];
                        Am[i][j] = s / d;
                    }
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    float s = a[i] * 0.005f;
                    if (NB > 0 && i < 3) s -= db[i];            // load_robot.py:112-113: the base carries the hand along
#pragma unroll
                    for (int k = 0; k < i; ++k) s -= Am[i][k] * x[k];
                    x[i] = s / Am[i][i];
                }
#pragma unroll
                for (int i = 5; i >= 0; --i) {
                    float s = x[i];
#pragma unroll
                    for (int k = i + 1; k < 6; ++k) s -= Am[k][i] * x[k];
                    x[i] = s / Am[i][i];
                }
                for (int k = 0; k < na; ++k) {
                    float u = 0.f;
#pragma unroll
                    for (int i = 0; i < 6; ++i) u = i == 0 ? J[k] * x[0] : u + J[i * na + k] * x[i];
                    out[k] = ts_clamp(qs[2 * k] + u, lo[k], hi[k]);
                }
                const float g = a[6] * dt / 5.0f;
                for (int k = na; k < nf; ++k) out[k] = ts_clamp(qs[2 * k] + g, lo[k], hi[k]);
            } else {
                for (int k = 0; k < na; ++k) out[k] = ts_clamp(qs[2 * k] + a[k] * dt * 20.0f, lo[k], hi[k]);
                const float g = a[na] * dt;
                for (int k = na; k < nf; ++k) out[k] = ts_clamp(qs[2 * k] + g, lo[k], hi[k]);
            }
        }
    }
    const int ts = __popcll(__ballot(n_succ)), tr = __popcll(__ballot(n_reset));
    if (tid == 0) {
        if (ts) atomicAdd(counters + 2 * slot, ts);
        if (tr) atomicAdd(counters + 2 * slot + 1, tr);
    }
}

// both entry points: the checks they share, the environments per block and the launch
template <int NB>
static int fc_launch(const float* actions, long act_stride, int A, const float* dof_state, const float* jac, int N, int nd, int nl,
                     int jl, int jr, const float* dof_lo, const float* dof_hi, const float* default_dof_pos, float dt, int drive_mode,
                     const float* base_R, const float* rew, uint8_t* success, int64_t* progress, int explore_step,
                     int max_episode_length, int train, float* pos_act, float* epis_max_rew, int64_t* epis_max_step, uint8_t* reset,
                     uint8_t* reset_succ, int32_t* counters, int slot, void* stream) {
    PM_REQUIRE(actions && dof_state && dof_lo && dof_hi && default_dof_pos && rew && success && progress && pos_act);
    PM_REQUIRE(epis_max_rew && epis_max_step && reset && reset_succ && counters);
    PM_REQUIRE(N >= 1 && nd >= NB + 3 && nd <= FC_ND_MAX && (slot == 0 || slot == 1));
    PM_REQUIRE(drive_mode == 0 || drive_mode == 1);
    if (drive_mode == 0) PM_REQUIRE(jac && A == 7 + NB && nl >= 1 && jl >= 0 && jl < nl && jr >= 0 && jr < nl);
    else PM_REQUIRE(A == nd - 1);
    PM_REQUIRE(act_stride >= A);
    int eb = FC_THREADS;
    while (eb > 8 && (N + eb - 1) / eb < TS_GRID_MIN) eb >>= 1;
    const size_t lds = drive_mode == 0 ? (size_t)eb * (6 * (nd - 2 - NB) + 1) * sizeof(float) : 0;
    const unsigned grid = (unsigned)((N + eb - 1) / eb);
    hipLaunchKernelGGL(franka_control_kernel<NB>, dim3(grid), dim3(FC_THREADS), lds, pm_stream(stream), actions, act_stride, A,
                       dof_state, jac, N, nd, nl, jl, jr, dof_lo, dof_hi, default_dof_pos, dt, drive_mode, base_R, rew, success,
                       progress, explore_step, max_episode_length, train, eb, pos_act, epis_max_rew, epis_max_step, reset, reset_succ,
                       counters, slot);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_franka_control_f32(const float* actions, long act_stride, int A, const float* dof_state, const float* jac, int N,
                                     int nd, int nl, int jl, int jr, const float* dof_lo, const float* dof_hi,
                                     const float* default_dof_pos, float dt, int drive_mode, const float* rew, uint8_t* success,
                                     int64_t* progress, int explore_step, int max_episode_length, int train, float* pos_act,
                                     float* epis_max_rew, int64_t* epis_max_step, uint8_t* reset, uint8_t* reset_succ,
                                     int32_t* counters, int slot, void* stream) {
    return fc_launch<0>(actions, act_stride, A, dof_state, jac, N, nd, nl, jl, jr, dof_lo, dof_hi, default_dof_pos, dt, drive_mode,
                        nullptr, rew, success, progress, explore_step, max_episode_length, train, pos_act, epis_max_rew,
                        epis_max_step, reset, reset_succ, counters, slot, stream);
}

extern "C" int pm_franka_control_mobile_f32(const float* actions, long act_stride, int A, const float* dof_state, const float* jac,
                                            int N, int nd, int nl, int jl, int jr, const float* dof_lo, const float* dof_hi,
                                            const float* default_dof_pos, float dt, int drive_mode, int nbase, const float* base_R,
                                            const float* rew, uint8_t* success, int64_t* progress, int explore_step,
                                            int max_episode_length, int train, float* pos_act, float* epis_max_rew,
                                            int64_t* epis_max_step, uint8_t* reset, uint8_t* reset_succ, int32_t* counters, int slot,
                                            void* stream) {
    PM_REQUIRE(nbase == 3 && base_R);
    return fc_launch<3>(actions, act_stride, A, dof_state, jac, N, nd, nl, jl, jr, dof_lo, dof_hi, default_dof_pos, dt, drive_mode,
                        base_R, rew, success, progress, explore_step, max_episode_length, train, pos_act, epis_max_rew,
                        epis_max_step, reset, reset_succ, counters, slot, stream);
}
