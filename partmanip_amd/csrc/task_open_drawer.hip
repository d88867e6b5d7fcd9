// The open_drawer task step (the reference's tasks/open_drawer.py compute_observations / compute_reward / reset_idx with
// load_robot.update_state) around heterogeneous environments: open_drawer_post_kernel after physics (handle frame, observation row,
// six-term reward, flags, per-object success tally, compact DOF state, part poses) and open_drawer_reset_kernel before physics, next
// to franka_control_kernel of task_grasp_cube.hip (target scatter and the state half of reset_idx).
//
// Shape.  Every environment holds another cabinet, so the simulator's rigid-body and DOF tensors are FLAT, (B, 13) and (D, 2), and an
// environment reaches its nrb + 2 bodies and nd + 1 DOFs through a row of indices (rigid_body_mask, dof_state_mask).  The kernel keeps
// the structure of grasp_cube_post_kernel: a block takes `eb` consecutive environments and
//   1. gathers their rows into LDS, lane i reading dword i of the block's (environment, slot, 13) list: the robot's nrb rows of an
//      environment are consecutive in memory and consecutive environments follow each other with a cabinet's rows between them, so the
//      wave loads stay runs of 13 nrb dwords with short gaps; the mask entry is one cached load per 13 lanes.  The 8 corners of the
//      handle box (N, 8, 3) and the 7 pose floats of the object's root row come in as flat ranges;
//   2. computes out of LDS: the first wave owns one environment per lane (tip pose, posed box, handle frame, reward: one serial chain
//      per environment), the other three waves one (environment, part) pose each; results go back to LDS laid out as the outputs;
//   3. copies rows out, lane i writing dword i: part_bbox, robot_dof_state, pose_R and pose_T of the block are contiguous ranges,
//      normal_state and extras rows (row stride from the caller) runs of 29 + 2 nd and 8 dwords.
//
// Arithmetic.  fp32, no contraction (-ffp-contract=off), each group in the reference's association: the box is (init + q axis), then
// the three products of a row of R summed left to right, then + position; norms as sqrt((x^2 + y^2) + z^2); the hand axes by Isaac
// Gym's quat_rotate on the AVERAGED (not unit) tip quaternion, a + b + c with a = v (2 w^2 - 1), b = 2 w (q x v), c = 2 q (q . v),
// evaluated on the full basis vector so that a NaN spreads as it does there; bool factors are multiplied as 0 / 1 floats;
// rew = base + |base| rot, then + 2 success.  clamp(max=), min and max propagate NaN, comparisons with NaN are false.
//
// Independence.  An environment is computed by one thread from its own rows in an order that does not depend on N, eb or the block
// it lands in.  The only cross-environment value is succ_objid: plain byte stores of the constant 1 (any order, any number of writers).
//
// Bounds.  A mask entry outside its tensor reads as NaN and is never dereferenced (post) or is skipped (reset); obj_id outside
// [0, num_objs) sets no flag.  The wrapper's constructor checks the masks once on the host.
//
// What is shared.  The LDS layout (ts_env_floats / ts_carve, the handle box in the task's own segment), the root-row gather, the flat
// copies, the part poses of waves 1-3, the DOF columns, the row-out loops, the flag stores and the host side of the launch
// (ts_post_launch) are the helpers of task_common.h, shared with grasp_cube_post_kernel; this file keeps the masked gather, the
// per-environment chain of wave 0, succ_objid and part_dof_state.  The tip average stays written out in both files (see
// task_grasp_cube.hip: as a helper it costs that kernel two registers).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): open_drawer_post_kernel 63 VGPRs, 104 SGPRs, no scratch, 7 waves /
// SIMD; open_drawer_reset_kernel 34 VGPRs, 54 SGPRs, no scratch, 8 waves / SIMD, no LDS.  Dynamic LDS of the post kernel:
// eb * ts_env_floats(13 (nrb + 2), 2 (nd + 1), 29 + 2 nd, 24, M) floats (task_common.h) = eb * (13 (nrb + 2) + 2 (nd + 1) + 7 +
// (29 + 2 nd) + 11 + 24 + 12 M) floats = 1840 B per environment at nrb = 13, nd = 9, M = 13: 14.4 KB
// with 8 environments per block, never more than 48 KB.  Times: profiles/open_drawer_timing.json.
#include "common.h"
#include "task_common.h"                                      // ts_*: the helpers, stages and LDS layout shared with task_grasp_cube.hip

#define OD_THREADS 256
#define OD_RS_THREADS 256

__device__ __forceinline__ float od_dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Isaac Gym's quat_rotate (q = (x, y, z, w), not normalised): v (2 w^2 - 1) + 2 w (q x v) + 2 q (q . v)
__device__ __forceinline__ void od_quat_rotate(const float* q, const float* v, float* o) {
    const float w = q[3];
    const float s = 2.0f * (w * w) - 1.0f;
    const float cx = q[1] * v[2] - q[2] * v[1], cy = q[2] * v[0] - q[0] * v[2], cz = q[0] * v[1] - q[1] * v[0];
    const float d = od_dot3(q, v);
    o[0] = (v[0] * s + (cx * w) * 2.0f) + (q[0] * d) * 2.0f;
    o[1] = (v[1] * s + (cy * w) * 2.0f) + (q[1] * d) * 2.0f;
    o[2] = (v[2] * s + (cz * w) * 2.0f) + (q[2] * d) * 2.0f;
}

__global__ __launch_bounds__(OD_THREADS) void open_drawer_post_kernel(
    const float* __restrict__ rigid_body_all, long B, const float* __restrict__ dof_state_all, long D, const float* __restrict__ root,
    int N, int nrb, int nd, int na, int obj_actor, int ltip, int rtip, const int32_t* __restrict__ rb_mask,
    const int32_t* __restrict__ dof_mask, const int32_t* __restrict__ obj_id, int num_objs, const float* __restrict__ bbox_init,
    const float* __restrict__ axis_dir, const float* __restrict__ joint_lo, const float* __restrict__ joint_hi,
    const float* __restrict__ dof_lo, const float* __restrict__ dof_hi, float suc_prop, const int32_t* __restrict__ part_slot,
    const float* __restrict__ part_C, int M, int eb, float* __restrict__ normal_state, long ns_stride, float* __restrict__ rew,
    uint8_t* __restrict__ success, uint8_t* __restrict__ is_reached, float* __restrict__ part_bbox, float* __restrict__ extras,
    long ex_stride, uint8_t* __restrict__ succ_objid, float* __restrict__ robot_dof_state, float* __restrict__ part_dof_state,
    float* __restrict__ pose_R, float* __restrict__ pose_T) {
    extern __shared__ float od_lds[];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * eb;
    const int neb = min(eb, N - b0);
    const int NS = nrb + 2, RB = NS * 13, DF = (nd + 1) * 2, W = 29 + 2 * nd;
    const ts_lds sh = ts_carve(od_lds, eb, RB, DF, W, 24, M);        // extra: the handle box, [eb][8][3]
    const float qnan = __builtin_nanf("");

    // 1. the block's state, gathered
    for (int i = tid; i < neb * RB; i += OD_THREADS) {
        const int e = i / RB, rem = i - e * RB, s = rem / 13, c = rem - s * 13;
        const long row = rb_mask[(long)(b0 + e) * NS + s];
        sh.rb[i] = (row >= 0 && row < B) ? rigid_body_all[row * 13 + c] : qnan;
    }
    for (int i = tid; i < neb * DF; i += OD_THREADS) {
        const int e = i / DF, rem = i - e * DF;
        const long row = dof_mask[(long)(b0 + e) * (nd + 1) + (rem >> 1)];
        sh.dof[i] = (row >= 0 && row < D) ? dof_state_all[row * 2 + (rem & 1)] : qnan;
    }
    ts_gather_root(sh.obj, root, b0, neb, na, obj_actor, tid, OD_THREADS);
    ts_copy(sh.extra, bbox_init + (long)b0 * 24, neb * 24, tid, OD_THREADS);
    __syncthreads();

    // 2. compute
    if (tid < 64) {
        for (int e = tid; e < neb; e += 64) {
            const float* L = sh.rb + e * RB + ltip * 13;
            const float* Rt = sh.rb + e * RB + rtip * 13;
            const float* obj = sh.obj + e * 7;
            float* ns = sh.ns + e * W;
            float* bb = sh.extra + e * 24;
            // load_robot.py:153-164
            float tip[7];
#pragma unroll
            for (int c = 0; c < 13; ++c) {
                const float v = (L[c] + Rt[c]) / 2.0f;
                if (c < 7) tip[c] = v;
                ns[c] = v;
            }
            const float gl = ts_norm3(L[0] - Rt[0], L[1] - Rt[1], L[2] - Rt[2]);
            const float q = sh.dof[e * DF + 2 * nd];
            // open_drawer.py:258-259
            {
                float Rm[9];
                ts_quat_to_mat(obj + 3, Rm);
                const float* ax = axis_dir + (long)(b0 + e) * 3;
                const float a0 = q * ax[0], a1 = q * ax[1], a2 = q * ax[2];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float p[3];
                    p[0] = bb[3 * k] + a0, p[1] = bb[3 * k + 1] + a1, p[2] = bb[3 * k + 2] + a2;
#pragma unroll
                    for (int j = 0; j < 3; ++j) bb[3 * k + j] = od_dot3(p, Rm + 3 * j) + obj[j];
                }
            }
            float h_out[3], h_long[3], h_short[3], mid[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                h_out[c] = bb[c] - bb[12 + c];
                h_long[c] = bb[3 + c] - bb[c];
                h_short[c] = bb[9 + c] - bb[c];
                mid[c] = (bb[c] + bb[18 + c]) / 2.0f;
            }
            const float len_out = ts_norm3(h_out[0], h_out[1], h_out[2]);
            const float len_long = ts_norm3(h_long[0], h_long[1], h_long[2]);
            const float len_short = ts_norm3(h_short[0], h_short[1], h_short[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                h_out[c] = h_out[c] / len_out, h_long[c] = h_long[c] / len_long, h_short[c] = h_short[c] / len_short;
                ns[13 + c] = mid[c], ns[16 + c] = h_out[c], ns[19 + c] = h_short[c], ns[22 + c] = h_long[c];
            }
            ns[25] = len_out, ns[26] = len_long, ns[27] = len_short;
            ts_dof_columns(ns, 28, sh.dof + e * DF, nd, dof_lo, dof_hi);
            ns[28 + 2 * nd] = q;
            // open_drawer.py:185-193
            float delta[3], dl[3], dr[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) delta[c] = tip[c] - mid[c], dl[c] = L[c] - mid[c], dr[c] = Rt[c] - mid[c];
            const float dist = ts_norm3(delta[0], delta[1], delta[2]);
            const bool r_out = fabsf(od_dot3(delta, h_out)) < len_out / 2.0f;
            const bool r_short = (od_dot3(dl, h_short) * od_dot3(dr, h_short)) < 0.0f;
            const bool r_long = fabsf(od_dot3(delta, h_long)) < len_long / 2.0f;
            const bool reached = r_out && r_short && r_long;
            const float reaching = -dist + 0.1f * ((r_out || r_short || r_long) ? 1.0f : 0.0f);
            // open_drawer.py:196-204
            float grip[3], sep[3], down[3];
            {
                const float ex[3] = {1.f, 0.f, 0.f}, ey[3] = {0.f, 1.f, 0.f}, ez[3] = {0.f, 0.f, 1.f};
                od_quat_rotate(tip + 3, ez, grip);
                od_quat_rotate(tip + 3, ey, sep);
                od_quat_rotate(tip + 3, ex, down);
            }
            const float ngrip[3] = {-grip[0], -grip[1], -grip[2]}, nsep[3] = {-sep[0], -sep[1], -sep[2]};
            const float ndown[3] = {-down[0], -down[1], -down[2]};
            const float dot1 = od_dot3(ngrip, h_out);
            const float dot2 = ts_max(od_dot3(sep, h_short), od_dot3(nsep, h_short));
            const float dot3 = ts_max(od_dot3(down, h_long), od_dot3(ndown, h_long));
            const float rot = ((dot1 + dot2) + dot3) - 3.0f;
            // open_drawer.py:207-234
            const float fr = reached ? 1.0f : 0.0f;
            const float close = (0.1f - gl) * fr + (0.1f * (gl - 0.1f)) * (1.0f - fr);
            const bool grasp = reached && (gl < len_short + 0.01f) && (rot > -0.2f);
            const float fg = grasp ? 1.0f : 0.0f;
            const float lo = joint_lo[b0 + e], hi = joint_hi[b0 + e];
            const float travel = q - lo;
            const float frac = travel / hi;
            const float capped = frac != frac ? frac : fminf(frac, suc_prop);
            const float jsr = fg * (0.1f + capped);
            const bool open_ng = frac > 0.1f;
            const bool open = grasp && open_ng;
            const float base = ((reaching + 0.5f * rot) + 5.0f * close) + 5.0f * jsr;
            float rw = base + fabsf(base) * rot;
            const bool succ = grasp && (travel >= suc_prop * hi);
            rw = rw + (succ ? 2.0f : 0.0f);
            float* sc = sh.sc + e * TS_SC;
            sc[0] = rw;
            sc[1] = open ? 1.0f : 0.0f, sc[2] = open_ng ? 1.0f : 0.0f, sc[3] = reaching, sc[4] = close, sc[5] = rot, sc[6] = jsr;
            sc[7] = rw, sc[8] = fg, sc[9] = succ ? 1.0f : 0.0f, sc[10] = fr;
        }
    } else if (pose_R || pose_T) {
        ts_part_poses(sh.rb, RB, neb, part_slot, NS, part_C, M, sh.R, sh.T, tid - 64, OD_THREADS - 64);
    }
    __syncthreads();

    // 3. rows out
    if (normal_state) ts_rows_out(normal_state, ns_stride, b0, sh.ns, W, W, neb, tid, OD_THREADS);
    if (extras) ts_rows_out(extras, ex_stride, b0, sh.sc + 1, TS_SC, 8, neb, tid, OD_THREADS);
    if (tid < neb) {
        const bool succ = ts_store_flags(sh.sc + tid * TS_SC, b0 + tid, rew, success, is_reached);
        if (succ_objid && succ) {
            const int o = obj_id[b0 + tid];
            if (o >= 0 && o < num_objs) succ_objid[o] = 1;
        }
        if (part_dof_state) {
            part_dof_state[(long)(b0 + tid) * 2] = sh.dof[tid * DF + 2 * nd];
            part_dof_state[(long)(b0 + tid) * 2 + 1] = sh.dof[tid * DF + 2 * nd + 1];
        }
    }
    if (part_bbox) ts_copy(part_bbox + (long)b0 * 24, sh.extra, neb * 24, tid, OD_THREADS);
    if (robot_dof_state) ts_rows_out(robot_dof_state, nd * 2, b0, sh.dof, DF, nd * 2, neb, tid, OD_THREADS);
    if (pose_R) ts_copy(pose_R + (long)b0 * M * 9, sh.R, neb * M * 9, tid, OD_THREADS);
    if (pose_T) ts_copy(pose_T + (long)b0 * M * 3, sh.T, neb * M * 3, tid, OD_THREADS);
}

extern "C" int pm_open_drawer_post_f32(const float* rigid_body_all, long B, const float* dof_state_all, long D, const float* root, int N,
                                       int nrb, int nd, int na, int obj_actor, int ltip, int rtip, const int32_t* rigid_body_mask,
                                       const int32_t* dof_state_mask, const int32_t* obj_id, int num_objs,
                                       const float* part_bbox_init, const float* part_axis_dir_init, const float* joint_lo,
                                       const float* joint_hi, const float* dof_lo, const float* dof_hi, float suc_prop,
                                       const int32_t* part_slot, const float* part_C, int M, float* normal_state, long ns_stride,
                                       float* rew, uint8_t* success, uint8_t* is_reached, float* part_bbox, float* extras,
                                       long ex_stride, uint8_t* succ_objid, float* robot_dof_state, float* part_dof_state,
                                       float* pose_R, float* pose_T, void* stream) {
    PM_REQUIRE(rigid_body_all && dof_state_all && root && rigid_body_mask && dof_state_mask && part_bbox_init && part_axis_dir_init);
    PM_REQUIRE(joint_lo && joint_hi && dof_lo && dof_hi);
    PM_REQUIRE(N >= 1 && nrb >= 1 && nd >= 1 && na >= 1 && B >= 1 && D >= 1 && B <= 0x7fffffffL && D <= 0x7fffffffL);
    PM_REQUIRE(obj_actor >= 0 && obj_actor < na && ltip >= 0 && ltip < nrb && rtip >= 0 && rtip < nrb);
    PM_REQUIRE(!succ_objid || (obj_id && num_objs >= 1));
    PM_REQUIRE(!normal_state || ns_stride >= 29 + 2L * nd);
    PM_REQUIRE(!extras || ex_stride >= 8);
    const bool poses = pose_R || pose_T;
    PM_REQUIRE(!poses || (part_slot && M >= 1));
    PM_REQUIRE((long)(nrb + 2) * 13 + (nd + 1) * 4 <= 12000);
    ts_launch L;
    PM_REQUIRE(ts_post_launch(N, (nrb + 2) * 13, (nd + 1) * 2, 29 + 2 * nd, 24, poses, M, &L));
    hipLaunchKernelGGL(open_drawer_post_kernel, dim3(L.grid), dim3(OD_THREADS), L.lds, pm_stream(stream), rigid_body_all, B,
                       dof_state_all, D, root, N, nrb, nd, na, obj_actor, ltip, rtip, rigid_body_mask, dof_state_mask, obj_id, num_objs,
                       part_bbox_init, part_axis_dir_init, joint_lo, joint_hi, dof_lo, dof_hi, suc_prop, part_slot, part_C, L.Mk, L.eb,
                       normal_state, ns_stride, rew, success, is_reached, part_bbox, extras, ex_stride, succ_objid, robot_dof_state,
                       part_dof_state, pose_R, pose_T);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

// ---------------------------------------------------------------------------------------------------- before physics
// One thread per element of three lists: the N (nd + 1) mask entries (coalesced mask reads; scattered 4 / 8-byte writes, which is what
// a scatter through an index table is), then the N na 13 root floats (coalesced).  Every write of an environment that is not reset
// is the pos_act_all scatter alone.  Isaac Gym's quat_mul in its own association (the factored form with the shared term qq).
// sin / cos of the fp32 yaw angle are the correctly rounded fp32 values (evaluated in double: four lanes of a resetting environment).
__global__ __launch_bounds__(OD_RS_THREADS) void open_drawer_reset_kernel(
    const uint8_t* __restrict__ reset, const float* __restrict__ pos_act, const int32_t* __restrict__ dof_mask, int N, int nd, int na,
    int robot_actor, int obj_actor, const float* __restrict__ robot_default_root, const float* __restrict__ obj_default_root,
    int random_reset, const float* __restrict__ u, float t_range, float r_range, const float* __restrict__ default_dof_pos,
    const float* __restrict__ joint_lo, float* __restrict__ root, float* __restrict__ dof_state_all, long D,
    float* __restrict__ pos_act_all, float* __restrict__ robot_dof_state, float* __restrict__ part_dof_state) {
    const long i = (long)blockIdx.x * OD_RS_THREADS + threadIdx.x;
    const long n_dof = (long)N * (nd + 1), n_root = (long)N * na * 13;
    if (i < n_dof) {
        const int e = (int)(i / (nd + 1)), k = (int)(i - (long)e * (nd + 1));
        const long row = dof_mask[i];
        const bool ok = row >= 0 && row < D;
        const bool rst = reset[e] != 0;
        if (k < nd) {
            if (ok) pos_act_all[row] = pos_act[(long)e * nd + k];
            if (rst) {
                const float v = default_dof_pos[k];
                if (ok) dof_state_all[row * 2] = v, dof_state_all[row * 2 + 1] = 0.0f;
                if (robot_dof_state) robot_dof_state[((long)e * nd + k) * 2] = v, robot_dof_state[((long)e * nd + k) * 2 + 1] = 0.0f;
            }
        } else if (rst) {
            const float v = joint_lo[e];
            if (ok) dof_state_all[row * 2] = v, dof_state_all[row * 2 + 1] = 0.0f;
            if (part_dof_state) part_dof_state[(long)e * 2] = v, part_dof_state[(long)e * 2 + 1] = 0.0f;
        }
    } else if (i < n_dof + n_root) {
        const long j = i - n_dof;
        const int e = (int)(j / (na * 13)), rem = (int)(j - (long)e * na * 13), a = rem / 13, c = rem - a * 13;
        if (!reset[e]) return;
        float v;
        if (c >= 7) {
            v = 0.0f;
        } else if (a == robot_actor) {
            v = robot_default_root[c];
        } else if (a == obj_actor) {
            v = obj_default_root[c];
            if (random_reset) {
                const float* ue = u + (long)e * 4;
                if (c < 3) {
                    v = v + (((ue[c] * t_range) * 2.0f) - t_range);
                } else {
                    const float ang = ((ue[3] * r_range) * 2.0f) - r_range;
                    const float x1 = obj_default_root[3], y1 = obj_default_root[4], z1 = obj_default_root[5], w1 = obj_default_root[6];
                    const float x2 = 0.0f, y2 = 0.0f, z2 = (float)sin((double)ang), w2 = (float)cos((double)ang);
                    const float ww = (z1 + x1) * (x2 + y2);
                    const float yy = (w1 - y1) * (w2 + z2);
                    const float zz = (w1 + y1) * (w2 - z2);
                    const float xx = (ww + yy) + zz;
                    const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
                    v = c == 6   ? (qq - ww) + (z1 - y1) * (y2 - z2)
                        : c == 3 ? (qq - xx) + (x1 + w1) * (x2 + w2)
                        : c == 4 ? (qq - yy) + (w1 - x1) * (y2 + z2)
                                 : (qq - zz) + (z1 + y1) * (w2 - x2);
                }
            }
        } else {
            return;
        }
        root[j] = v;
    }
}

extern "C" int pm_open_drawer_reset_f32(const uint8_t* reset, const float* pos_act, const int32_t* dof_state_mask, int N, int nd, int na,
                                        int robot_actor, int obj_actor, const float* robot_default_root,
                                        const float* obj_default_root, int random_reset, const float* u, float t_range, float r_range,
                                        const float* default_dof_pos, const float* joint_lo, float* root, float* dof_state_all, long D,
                                        float* pos_act_all, float* robot_dof_state, float* part_dof_state, void* stream) {
    PM_REQUIRE(reset && pos_act && dof_state_mask && robot_default_root && obj_default_root && default_dof_pos && joint_lo);
    PM_REQUIRE(root && dof_state_all && pos_act_all);
    PM_REQUIRE(N >= 1 && nd >= 1 && na >= 1 && D >= 1 && D <= 0x7fffffffL);
    PM_REQUIRE(robot_actor >= 0 && robot_actor < na && obj_actor >= 0 && obj_actor < na && robot_actor != obj_actor);
    PM_REQUIRE(!random_reset || u);
    const long total = (long)N * (nd + 1) + (long)N * na * 13;
    PM_REQUIRE(total < 0x7fffffffL * OD_RS_THREADS);
    const unsigned grid = (unsigned)((total + OD_RS_THREADS - 1) / OD_RS_THREADS);
    hipLaunchKernelGGL(open_drawer_reset_kernel, dim3(grid), dim3(OD_RS_THREADS), 0, pm_stream(stream), reset, pos_act, dof_state_mask,
                       N, nd, na, robot_actor, obj_actor, robot_default_root, obj_default_root, random_reset, u, t_range, r_range,
                       default_dof_pos, joint_lo, root, dof_state_all, D, pos_act_all, robot_dof_state, part_dof_state);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
