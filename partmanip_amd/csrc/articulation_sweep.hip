// A swept contact test of one kinematic step (pm_articulation_sweep_f32 / pm_articulation_sweep_groups_f32): how far along this step
// can the robot go before one of its sensing points enters a target grid.  The step from the joint state q to the drive rule's end
// state q' is cut into S parts; candidate k = 0 .. S is the joint state q_k on the way, each is posed (articulation.hip's float64
// chain, body_pose.hip's matrices) and sensed (mesh_sdf_points.hip's point query, mt_sample of mesh_sdf_sample.h), and the step is
// cut at the last candidate before the first that would take the robot into contact or deeper into it.  By definition
// (include/partmanip_hip.h) sweep_dist[b, k] has the bits that pm_articulation_step_f32 on q_k, pm_body_pose_gather_f32 and
// pm_mesh_sdf_points(_groups)_f32 give when run one after the other; this launch pays for none of the Jacobian (96 % of the
// articulation launch's output), for none of the S + 1 round trips of body rows and pose tables through memory, and walks the
// chain once for all candidates.  It is a stated rule, not physics: nothing slides, bounces or is pushed.
//
// Shape.  One work-group of four waves per environment, everything between the stages in LDS:
//   0. drive: thread i owns one (candidate, DOF) pair and computes q_k[d] from dof_state (only read), the target, the rate limit and
//      the joint limits -- articulation_step_kernel's stage 0, operation for operation, without its store;
//   1. chain: the first wave walks the bodies with lane = candidate, so the serially dependent float64 chain is paid once for all
//      S + 1 <= 64 candidates; the tree tables are read at wave-uniform addresses.  A lane keeps its frames as doubles in LDS for the
//      children (7 per body), and when its walk is over rewrites each body's 56 bytes in place as 12 floats: quat_to_mat of the
//      rounded quaternion and the rounded position, what a pose slot placed by that body is made of;
//   2. the poses that count are tested for non-finite entries, per candidate (the point query's rule 5 on the candidate's table);
//   3. all four waves take (candidate, segment, 64-point chunk) triples in turn, lane = point: the chunk loop of mesh_sdf_points.hip
//      with every pose read going through sw_pose -- the caller's table, or for a slot a robot body places the candidate's matrix
//      (times the slot's C in body_pose.hip's association).  Ordinal, row and slot are wave-uniform in the sample loop, so its table
//      reads stay scalar loads.  A chunk's minimum is reduced with shuffles over order-preserving integer keys (NaN -> 0, it wins)
//      and meets the other chunks of its candidate in LDS through an integer minimum: no floating-point atomics, no dependence on
//      timing, bit-reproducible;
//   4. one lane applies the admission rule along k, threads d < nd write the accepted candidate's joints.
// The cull helpers (sw_ordered, sw_out_of_reach, sw_pose_finite) are copies of mesh_sdf_points.hip's: that file's and mesh_tsdf.hip's
// instructions stay exactly as they were (sharing the brick test once moved mesh_tsdf_kernel<true>'s registers).
//
// Independence.  An environment is computed by its own work-group from its own rows: its bits do not depend on N or on the block it
// lands in, and a NaN (a target, a joint, a pose) stays inside its environment, where it makes every candidate it reaches NaN.
//
// Memory safety: segment offsets are cut to [0, NP] and made non-decreasing, carriers outside [-1, M) read no pose, a slot_body
// outside [-1, nb) reads no LDS row (the slot's pose is NaN), group tables are cut as in mesh_tsdf.hip, gathers stay behind the
// validity test, a chunk's sphere row is (start / 64) < ceil(NP / 64), an environment whose DOF rows would fall outside dof_state
// reads none of them (its candidates are NaN).  Every store lands in the environment's own S + 1, 1 and nd output elements.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): articulation_sweep_kernel: 79 VGPRs, 106 SGPRs, no scratch, 520
// bytes of static LDS, occupancy 6 waves / SIMD; articulation_sweep_groups_kernel: 79 VGPRs, 106 SGPRs, no scratch, 4616 bytes of
// static LDS (the slot bit set), occupancy 6.  Dynamic LDS is (S + 1) ((7 nb | 1) * 8 + 4 nd) bytes: 6876 B for the Franka (13
// bodies, 9 DOFs) at S = 8; SW_LDS_MAX bounds it.
// Timings: tools/time_guarded_step.py, profiles/guarded_step_timing.json.  The launch equals the composed launches' time from 1024
// environments on (the gathers bind both) and beats it only where that is launch-bound; at 64 environments its time grows with S,
// one work-group per environment leaving the chip idle.
#include "mesh_sdf_sample.h"
#include "task_common.h"                                      // ts_clamp, ts_quat_to_mat
#include "articulation_common.h"                              // the quaternion helpers and the frame step of the chain

#define SW_WAVES 4                                            // waves per work-group
#define SW_THREADS (64 * SW_WAVES)
#define SW_MAX_M 32768                                        // grouped entry: pose slots the LDS bit set has room for
#define SW_MAX_S 63                                           // S + 1 candidates are the lanes of the chain's wave
#define SW_LDS_MAX 57344                                      // bytes of dynamic LDS a work-group may ask for
#define SW_BODY 14                                            // floats of a body's LDS slot (7 doubles): Q [9] | T [3] | 2 unused

typedef float sw_af __attribute__((may_alias));              // the chain's doubles are rewritten in place as floats

__device__ __forceinline__ unsigned sw_ordered(float v) {    // unsigned order == float order; NaN -> 0 (below -inf): NaN wins a minimum
    const unsigned u = __float_as_uint(v);
    return v != v ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float sw_unordered(unsigned k) {
    return k == 0u ? __builtin_nanf("") : __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
#define SW_KEY_ONE 0xBF800000u                               // sw_ordered(1.0f): "far", the identity of the minimum

// mesh_sdf_points.hip's sp_out_of_reach, copied: nonzero iff NO point of the ball (centre b, radius brad, world frame) can give a
// valid sample of the part.  NaN / inf anywhere compares false: not skipped.
__device__ __forceinline__ int sw_out_of_reach(float bx, float by, float bz, float brad, float a0, float a1, float a2, const float* R,
                                               const float* T, float mn0, float mn1, float mn2, int rx, int ry, int rz, float iv) {
    const float d0 = bx - T[0], d1 = by - T[1], d2 = bz - T[2];
    int skip = 0;
#define SW_AXIS(ra, rb_, rc, mn, rn)                                                                        \
    {                                                                                                        \
        const float q = d0 * ra + d1 * rb_ + d2 * rc;                                                        \
        const float rad = brad * __builtin_amdgcn_sqrtf(ra * ra + rb_ * rb_ + rc * rc) * 1.001f;             \
        const float mag = a0 * fabsf(ra) + a1 * fabsf(rb_) + a2 * fabsf(rc) + fabsf(mn);                     \
        const float uc = (q - mn) * iv, ur = fabsf(rad * iv), mg = 0.02f + 1e-5f * fabsf(mag * iv);          \
        skip |= (int)(uc + ur < 1.0f - mg) | (int)(uc - ur > (float)(rn - 2) + mg);                          \
    }
    SW_AXIS(R[0], R[3], R[6], mn0, rx)
    SW_AXIS(R[1], R[4], R[7], mn1, ry)
    SW_AXIS(R[2], R[5], R[8], mn2, rz)
#undef SW_AXIS
    return skip;
}

__device__ __forceinline__ int sw_pose_finite(const float* R, const float* T) {
    int ok = 1;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok &= mt_fin(R[i]);
    return ok & mt_fin(T[0]) & mt_fin(T[1]) & mt_fin(T[2]);
}

// Where a candidate's pose table comes from: the caller's table (Rb, Tb: this environment's M slots) and the candidate's body
// matrices in LDS (cand: [nb][SW_BODY]).
struct sw_table {
    const float *Rb, *Tb;
    const int32_t* slot_body;
    const float* slot_C;
    int MC, nb;
    const sw_af* cand;
};

// Slot m in [0, M) of the candidate's table: the caller's pose where slot_body[m] == -1; for a body j in [0, nb) T = its position
// and R = quat_to_mat(its quaternion), times C_m for m < MC summed over the inner index left to right (body_pose.hip); any other
// slot_body: a NaN pose (what a row outside the rigid-body tensor gives there).
__device__ __forceinline__ void sw_pose(const sw_table& t, int m, float* R, float* T) {
    const int j = t.slot_body[m];
    if (j == -1) {
#pragma unroll
        for (int c = 0; c < 9; ++c) R[c] = t.Rb[m * 9 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) T[c] = t.Tb[m * 3 + c];
    } else if (j >= 0 && j < t.nb) {
        const sw_af* s = t.cand + j * SW_BODY;
        float Q[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) Q[c] = s[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) T[c] = s[9 + c];
        if (m < t.MC) {
            const float* Cp = t.slot_C + 9L * m;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) R[3 * i + jj] = (Q[3 * i] * Cp[jj] + Q[3 * i + 1] * Cp[3 + jj]) + Q[3 * i + 2] * Cp[6 + jj];
        } else {
#pragma unroll
            for (int c = 0; c < 9; ++c) R[c] = Q[c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 9; ++c) R[c] = __builtin_nanf("");
        T[0] = T[1] = T[2] = __builtin_nanf("");
    }
}

// GROUPS = false: ordinal p is part p, placed by pose slot p.  GROUPS = true: the grid library of mesh_tsdf.hip's grouped kernel.
template <bool GROUPS>
__device__ __forceinline__ void sw_body(
    const int32_t* __restrict__ parent, const int32_t* __restrict__ jtype, const int32_t* __restrict__ dof,
    const float* __restrict__ origin_q, const float* __restrict__ origin_t, const float* __restrict__ axis,
    const float* __restrict__ dof_lo, const float* __restrict__ dof_hi, const float* __restrict__ vmax, float dt,
    const float* __restrict__ base_pose, long base_stride, const float* __restrict__ dof_state, long dof_rows,
    const float* __restrict__ targets, long tgt_stride, const uint8_t* __restrict__ reset, const int32_t* __restrict__ dof_row0,
    long dof_stride, int nb, int nd, const float* __restrict__ fields, const int64_t* __restrict__ part_off,
    const int32_t* __restrict__ part_shape, const float* __restrict__ part_bbox_min, const float* __restrict__ part_voxel_size,
    const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M, int p0, int p1, const float* __restrict__ pts,
    long pts_env_stride, const int32_t* __restrict__ carrier, const int32_t* __restrict__ pt_id, const float* __restrict__ chunk_sphere,
    int NP, const int32_t* __restrict__ seg_off, int NS, int cull, const int32_t* __restrict__ slot_body,
    const float* __restrict__ slot_C, int MC, int S, float block_margin, const uint8_t* __restrict__ free_env, int FS,
    float* __restrict__ sweep_dist, int32_t* __restrict__ steps, float* __restrict__ targets_out, const int32_t* __restrict__ grid_slot,
    int NG, int NG_shared, const int32_t* __restrict__ group_off, int G, const int32_t* __restrict__ env_group, int max_group_grids) {
    extern __shared__ double sw_fr[];                         // [S + 1][FS] doubles: a candidate's frames [nb][7]; then q_k [S + 1][nd] floats
    __shared__ unsigned named[GROUPS ? SW_MAX_M / 32 : 1];
    __shared__ unsigned key_s[64];                            // per candidate: the ordered key of its minimum, then the distance's bits
    __shared__ int bad_s[64];                                 // per candidate: a pose that counts is not finite
    __shared__ int bad_tab, steps_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NC = S + 1;
    float* qk = (float*)(sw_fr + (long)NC * FS);
    const bool is_reset = reset && reset[b];

    // 0. drive: q_k[d] for every candidate.  An environment whose DOF rows would fall outside dof_state is NaN.
    {
        const long row = dof_row0 ? (long)dof_row0[b] : (long)b * dof_stride;
        const bool row_ok = row >= 0 && row + nd <= dof_rows;
        for (int i = tid; i < NC * nd; i += SW_THREADS) {
            const int k = i / nd, d = i - k * nd;
            float qc = __builtin_nanf("");
            if (row_ok) {
                const float q = dof_state[(row + d) * 2];
                const float t = targets[(long)b * tgt_stride + d], lo = dof_lo[d], hi = dof_hi[d];
                float qn;
                if (is_reset) {
                    qn = ts_clamp(t, lo, hi);
                } else {
                    if (vmax) {
                        const float m = vmax[d] * dt;
                        qn = q + ts_clamp(t - q, -m, m);
                    } else {
                        qn = t;
                    }
                    qn = ts_clamp(qn, lo, hi);
                }
                if (k == S) {
                    qc = qn;
                } else if (k == 0) {
                    qc = ts_clamp(q, lo, hi);
                } else {
                    const float a = __fdiv_rn((float)k, (float)S);
                    qc = ts_clamp(add_rn(q, mul_rn(a, sub_rn(qn, q))), lo, hi);
                }
            }
            qk[i] = qc;
        }
    }
    if (tid < 64) key_s[tid] = SW_KEY_ONE, bad_s[tid] = 0;
    if (tid == 0) bad_tab = 0;
    __syncthreads();

    // 1. the chain, one candidate per lane of the first wave (articulation_step_kernel's stage 1 without its float stores)
    if (tid < NC) {
        double* fr = sw_fr + (long)tid * FS;
        const float* qs = qk + tid * nd;
        const float* bp = base_pose + (long)b * base_stride;
        double base[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) base[c] = bp[c];
        ar_qunit(base + 3);
        for (int bd = 0; bd < nb; ++bd) {
            const int p = parent[bd];
            double pp[3], pq[4], pos[3], fq[4];
#pragma unroll
            for (int c = 0; c < 3; ++c) pp[c] = (p >= 0 && p < bd) ? fr[p * 7 + c] : base[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) pq[c] = (p >= 0 && p < bd) ? fr[p * 7 + 3 + c] : base[3 + c];
            ar_frame_origin(pp, pq, origin_t, origin_q, bd, pos, fq);
            const int jt = jtype[bd], d = dof[bd];
            if ((jt == AR_REVOLUTE || jt == AR_PRISMATIC) && d >= 0 && d < nd) {
                const double al[3] = {axis[bd * 3], axis[bd * 3 + 1], axis[bd * 3 + 2]};
                double aw[3];
                ar_qrot(fq, al, aw);
                ar_frame_joint(jt, al, aw, (double)qs[d], pos, fq);
            }
            ar_qunit(fq);
#pragma unroll
            for (int c = 0; c < 3; ++c) fr[bd * 7 + c] = pos[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) fr[bd * 7 + 3 + c] = fq[c];
        }
        // each body's frame, rounded once, as the matrix and the position a pose slot takes from its row
        for (int bd = 0; bd < nb; ++bd) {
            double v[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) v[c] = fr[bd * 7 + c];
            const float q4[4] = {(float)v[3], (float)v[4], (float)v[5], (float)v[6]};
            float Q[9];
            ts_quat_to_mat(q4, Q);
            sw_af* o = (sw_af*)(fr + bd * 7);
#pragma unroll
            for (int c = 0; c < 9; ++c) o[c] = Q[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[9 + c] = (float)v[c];
        }
    }

    // the environment's ordinals, cut as in mesh_tsdf.hip
    int n_ord = M, g_lo = 0;
    if constexpr (GROUPS) {
        const int g = G > 0 ? env_group[b] : -1;
        int cnt = 0;
        g_lo = NG_shared;
        if (g >= 0 && g < G) {
            const int span = NG - NG_shared;
            const int o0 = min(max(group_off[g], 0), span), o1 = min(max(group_off[g + 1], o0), span);
            g_lo = NG_shared + o0;
            cnt = min(o1 - o0, max_group_grids);
        }
        n_ord = NG_shared + cnt;
    }

    // 2. a non-finite pose in a slot that counts -> the candidate (a robot-placed slot) or the environment (a table slot) is NaN
    if constexpr (GROUPS) {
        for (int i = tid; i < (M + 31) / 32; i += SW_THREADS) named[i] = 0u;
        __syncthreads();
        for (int t = tid; t < n_ord; t += SW_THREADS) {
            const int s = grid_slot[t < NG_shared ? t : g_lo + (t - NG_shared)];
            if (s >= 0 && s < M) atomicOr(&named[s >> 5], 1u << (s & 31));
        }
        for (int n = tid; n < NP; n += SW_THREADS) {
            const int s = carrier[n];
            if (s >= 0 && s < M) atomicOr(&named[s >> 5], 1u << (s & 31));
        }
    }
    __syncthreads();
    sw_table tab = {pose_R + (long)b * M * 9, pose_T + (long)b * M * 3, slot_body, slot_C, MC, nb, nullptr};
    for (int s = tid; s < M; s += SW_THREADS) {               // one pass over the slots; only a robot-placed slot costs S + 1 looks
        bool look = true;
        if constexpr (GROUPS) look = (named[s >> 5] >> (s & 31)) & 1u;
        if (!look) continue;
        float R[9], T[3];
        if (slot_body[s] == -1) {                             // a table slot is the same for every candidate: looked at once
            sw_pose(tab, s, R, T);
            if (!sw_pose_finite(R, T)) bad_tab = 1;
        } else {
            for (int k = 0; k < NC; ++k) {
                tab.cand = (const sw_af*)(sw_fr + (long)k * FS);
                sw_pose(tab, s, R, T);
                if (!sw_pose_finite(R, T)) bad_s[k] = 1;
            }
        }
    }
    __syncthreads();

    // 3. (candidate, segment, chunk) triples, dealt to the waves in turn
    if (!bad_tab) {                                           // uniform over the work-group
        int dealt = 0;
        for (int s = 0; s < NS; ++s) {
            const int lo = min(max(seg_off[s], 0), NP);
            const int hi = min(max(seg_off[s + 1], lo), NP);
            const int nchunks = (hi - lo + 63) >> 6;
            const int items = NC * nchunks;
            for (int it = (wave - dealt) & (SW_WAVES - 1); it < items; it += SW_WAVES) {
                const int k = it / nchunks, c = it - k * nchunks;    // wave-uniform
                if (bad_s[k]) continue;
                tab.cand = (const sw_af*)(sw_fr + (long)k * FS);
                const int start = lo + c * 64;
                const int n = start + lane;
                const bool act = n < hi;
                const int nc = act ? n : hi - 1;              // a lane past the end reads the last point and counts for nothing
                const float* pp = pts + (long)b * pts_env_stride + 3L * nc;
                const float x0 = pp[0], x1 = pp[1], x2 = pp[2];
                const int ca = carrier[nc];
                const int id = pt_id ? pt_id[nc] : nc;
                const bool posed = ca >= 0 && ca < M;
                const bool ok = act && (posed || ca == -1);   // a carrier outside [-1, M): 1, no pose read through it
                float wx = x0, wy = x1, wz = x2;
                if (posed) {
                    float R[9], T[3];
                    sw_pose(tab, ca, R, T);
                    wx = posed_coord(x0, x1, x2, R[0], R[1], R[2], T[0]);
                    wy = posed_coord(x0, x1, x2, R[3], R[4], R[5], T[1]);
                    wz = posed_coord(x0, x1, x2, R[6], R[7], R[8], T[2]);
                }

                // the chunk's bounding sphere in the world frame (wave-uniform)
                const int c0 = __builtin_amdgcn_readfirstlane(ca);   // lane 0 is always a real point of the chunk
                const bool use_cull = cull && chunk_sphere && (start & 63) == 0 && __all(!act || ca == c0);
                float sx = 0.f, sy = 0.f, sz = 0.f, sr = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
                if (use_cull) {
                    const float* Sp = chunk_sphere + (long)(start >> 6) * 4;
                    const float ux = Sp[0], uy = Sp[1], uz = Sp[2];
                    sx = ux, sy = uy, sz = uz, sr = Sp[3];
                    e0 = fabsf(ux), e1 = fabsf(uy), e2 = fabsf(uz);
                    if (c0 >= 0 && c0 < M) {
                        float R[9], T[3];
                        sw_pose(tab, c0, R, T);
                        sx = ux * R[0] + uy * R[1] + uz * R[2] + T[0];
                        sy = ux * R[3] + uy * R[4] + uz * R[5] + T[1];
                        sz = ux * R[6] + uy * R[7] + uz * R[8] + T[2];
                        e0 = fabsf(ux * R[0]) + fabsf(uy * R[1]) + fabsf(uz * R[2]) + fabsf(T[0]);
                        e1 = fabsf(ux * R[3]) + fabsf(uy * R[4]) + fabsf(uz * R[5]) + fabsf(T[1]);
                        e2 = fabsf(ux * R[6]) + fabsf(uy * R[7]) + fabsf(uz * R[8]) + fabsf(T[2]);
                        float fro = 0.f;
#pragma unroll
                        for (int i = 0; i < 9; ++i) fro += R[i] * R[i];
                        sr = sr * __builtin_amdgcn_sqrtf(fro) * 1.001f;
                    }
                }

                float m = 1.0f;
                for (int pb = 0; pb < n_ord; pb += 64) {
                    // lane l looks at ordinal pb + l: is it in [p0, p1), one of the environment's own, and within the sphere's reach?
                    unsigned long long todo;
                    {
                        const int p = pb + lane;
                        int pc = p < M ? p : M - 1, ps = pc;
                        bool own = p < M;
                        if constexpr (GROUPS) {
                            own = p < n_ord;
                            pc = own ? (p < NG_shared ? p : g_lo + (p - NG_shared)) : 0;
                            const int sl = grid_slot[pc];
                            own = own && sl >= 0 && sl < M;
                            ps = own ? sl : 0;
                        }
                        int need = (int)(p >= p0) & (int)(p < p1) & (int)own;
                        if (use_cull) {
                            float R[9], T[3];
                            sw_pose(tab, ps, R, T);
                            const float iv = __builtin_amdgcn_rcpf(part_voxel_size[pc]);
                            need &= !sw_out_of_reach(sx, sy, sz, sr, e0 + fabsf(T[0]) + sr, e1 + fabsf(T[1]) + sr, e2 + fabsf(T[2]) + sr, R, T,
                                                     part_bbox_min[pc * 3], part_bbox_min[pc * 3 + 1], part_bbox_min[pc * 3 + 2],
                                                     part_shape[pc * 3], part_shape[pc * 3 + 1], part_shape[pc * 3 + 2], iv);
                        }
                        todo = __ballot(need != 0);
                    }
                    while (todo) {
                        const int t = pb + (int)__builtin_ctzll(todo);   // wave-uniform: the table loads below are scalar loads
                        todo &= todo - 1;
                        int p = t, slot = t;
                        if constexpr (GROUPS) {                  // the ordinal's row and the slot it names (in [0, M): the ballot saw to that)
                            p = t < NG_shared ? t : g_lo + (t - NG_shared);
                            slot = grid_slot[p];
                        }
                        float R[9], T[3];
                        sw_pose(tab, slot, R, T);
                        const mt_part P = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], T[0], T[1], T[2], part_bbox_min[p * 3],
                                           part_bbox_min[p * 3 + 1], part_bbox_min[p * 3 + 2], part_voxel_size[p], part_shape[p * 3],
                                           part_shape[p * 3 + 1], part_shape[p * 3 + 2], part_off[p]};
                        m = mt_min_nan(m, mt_sample(fields, P, wx, wy, wz, ok));
                    }
                }
                unsigned key = (act && id >= 0) ? sw_ordered(m) : SW_KEY_ONE;   // a negative id is a padding point: in no result
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned other = __shfl_xor(key, o, 64);
                    key = other < key ? other : key;
                }
                if (lane == 0) atomicMin(&key_s[k], key);
            }
            dealt = (dealt + items) & (SW_WAVES - 1);
        }
    }
    __syncthreads();

    // 4. the distances out, the cut, the guarded targets
    if (tid < NC) {
        const float d = (bad_tab || bad_s[tid]) ? __builtin_nanf("") : sw_unordered(key_s[tid]);
        sweep_dist[(long)b * NC + tid] = d;
        key_s[tid] = __float_as_uint(d);
    }
    __syncthreads();
    if (tid == 0) {
        int K = 0;
        bool open = true;
        float prev = __uint_as_float(key_s[0]);
        for (int k = 1; k <= S; ++k) {
            const float d = __uint_as_float(key_s[k]);
            open = open && (d > block_margin || d >= prev);   // a NaN is not admissible
            K = open ? k : K;
            prev = d;
        }
        if (is_reset || (free_env && free_env[b])) K = S;
        steps_s = K;
        steps[b] = K;
    }
    __syncthreads();
    if (tid < nd) targets_out[(long)b * nd + tid] = qk[steps_s * nd + tid];
}

#define SW_CHAIN_PARAMS                                                                                                              \
    const int32_t *__restrict__ parent, const int32_t *__restrict__ jtype, const int32_t *__restrict__ dof,                           \
        const float *__restrict__ origin_q, const float *__restrict__ origin_t, const float *__restrict__ axis,                       \
        const float *__restrict__ dof_lo, const float *__restrict__ dof_hi, const float *__restrict__ vmax, float dt,                 \
        const float *__restrict__ base_pose, long base_stride, const float *__restrict__ dof_state, long dof_rows,                    \
        const float *__restrict__ targets, long tgt_stride, const uint8_t *__restrict__ reset, const int32_t *__restrict__ dof_row0,  \
        long dof_stride, int nb, int nd, const float *__restrict__ fields, const int64_t *__restrict__ part_off,                      \
        const int32_t *__restrict__ part_shape, const float *__restrict__ part_bbox_min, const float *__restrict__ part_voxel_size
#define SW_CHAIN_ARGS                                                                                                                \
    parent, jtype, dof, origin_q, origin_t, axis, dof_lo, dof_hi, vmax, dt, base_pose, base_stride, dof_state, dof_rows, targets,     \
        tgt_stride, reset, dof_row0, dof_stride, nb, nd, fields, part_off, part_shape, part_bbox_min, part_voxel_size
#define SW_SENSE_PARAMS                                                                                                              \
    const float *__restrict__ pose_R, const float *__restrict__ pose_T, int M, int p0, int p1, const float *__restrict__ pts,         \
        long pts_env_stride, const int32_t *__restrict__ carrier, const int32_t *__restrict__ pt_id,                                  \
        const float *__restrict__ chunk_sphere, int NP, const int32_t *__restrict__ seg_off, int NS, int cull,                        \
        const int32_t *__restrict__ slot_body, const float *__restrict__ slot_C, int MC, int S, float block_margin,                   \
        const uint8_t *__restrict__ free_env, int FS, float *__restrict__ sweep_dist, int32_t *__restrict__ steps,                    \
        float *__restrict__ targets_out
#define SW_SENSE_ARGS                                                                                                                \
    pose_R, pose_T, M, p0, p1, pts, pts_env_stride, carrier, pt_id, chunk_sphere, NP, seg_off, NS, cull, slot_body, slot_C, MC, S,    \
        block_margin, free_env, FS, sweep_dist, steps, targets_out

__global__ __launch_bounds__(SW_THREADS) void articulation_sweep_kernel(SW_CHAIN_PARAMS, SW_SENSE_PARAMS) {
    sw_body<false>(SW_CHAIN_ARGS, SW_SENSE_ARGS, nullptr, 0, 0, nullptr, 0, nullptr, 0);
}

__global__ __launch_bounds__(SW_THREADS) void articulation_sweep_groups_kernel(
    SW_CHAIN_PARAMS, const int32_t* __restrict__ grid_slot, int NG, int NG_shared, const int32_t* __restrict__ group_off, int G,
    const int32_t* __restrict__ env_group, int max_group_grids, SW_SENSE_PARAMS) {
    sw_body<true>(SW_CHAIN_ARGS, SW_SENSE_ARGS, grid_slot, NG, NG_shared, group_off, G, env_group, max_group_grids);
}

// the argument rules the two entries share; *lds = the bytes of dynamic LDS, *FS = a candidate's doubles
static int sw_check(const void* parent, const void* jtype, const void* dof, const void* origin_q, const void* origin_t, const void* axis,
                    const void* dof_lo, const void* dof_hi, float dt, const void* base_pose, long base_stride, const void* dof_state,
                    long dof_rows, const void* targets, long tgt_stride, const void* dof_row0, long dof_stride, int N, int nb, int nd,
                    const void* pts, long pts_env_stride, const void* carrier, int NP, const void* seg_off, int NS, int M,
                    const void* slot_body, const void* slot_C, int MC, int S, float block_margin, const void* sweep_dist,
                    const void* steps, const void* targets_out, int* FS, size_t* lds) {
    PM_REQUIRE(parent && jtype && dof && origin_q && origin_t && axis && dof_lo && dof_hi && base_pose && dof_state && targets);
    PM_REQUIRE(N >= 1 && nb >= 1 && nb <= AR_MAX && nd >= 1 && nd <= AR_MAX);
    PM_REQUIRE(base_stride == 0 || base_stride >= 7);
    PM_REQUIRE(dof_rows >= nd && dof_rows < 2147483648L && (dof_row0 || (dof_stride >= nd && (N - 1) * dof_stride + nd <= dof_rows)));
    PM_REQUIRE(dt > 0.0f && tgt_stride >= nd);                 // a NaN dt is refused too
    PM_REQUIRE(pts && carrier && NP > 0 && NP <= (1 << 30) && NS >= 1 && seg_off);
    PM_REQUIRE(pts_env_stride == 0 || pts_env_stride >= 3L * NP);
    PM_REQUIRE(slot_body && MC >= 0 && MC <= M && (MC == 0 || slot_C));
    PM_REQUIRE(S >= 1 && S <= SW_MAX_S && block_margin == block_margin);
    PM_REQUIRE(sweep_dist && steps && targets_out);
    *FS = (7 * nb) | 1;
    *lds = (size_t)(S + 1) * (8u * (size_t)*FS + 4u * (size_t)nd);
    PM_REQUIRE(*lds <= SW_LDS_MAX);
    return PM_OK;
}

extern "C" int pm_articulation_sweep_f32(const int32_t* parent, const int32_t* jtype, const int32_t* dof, const float* origin_q,
                                         const float* origin_t, const float* axis, const float* dof_lo, const float* dof_hi,
                                         const float* vmax, float dt, const float* base_pose, long base_stride, const float* dof_state,
                                         long dof_rows, const float* targets, long tgt_stride, const uint8_t* reset,
                                         const int32_t* dof_row0, long dof_stride, int N, int nb, int nd, const float* fields,
                                         const int64_t* part_off, const int32_t* part_shape, const float* part_bbox_min,
                                         const float* part_voxel_size, const float* pose_R, const float* pose_T, int M, int p0, int p1,
                                         const float* pts, long pts_env_stride, const int32_t* carrier, const int32_t* pt_id,
                                         const float* chunk_sphere, int NP, const int32_t* seg_off, int NS, int cull,
                                         const int32_t* slot_body, const float* slot_C, int MC, int S, float block_margin,
                                         const uint8_t* free_env, float* sweep_dist, int32_t* steps, float* targets_out, void* stream) {
    PM_REQUIRE(fields && part_off && part_shape && part_bbox_min && part_voxel_size && pose_R && pose_T);
    PM_REQUIRE(M > 0 && p0 >= 0 && p0 < p1 && p1 <= M);
    int FS;
    size_t lds;
    if (int e = sw_check(parent, jtype, dof, origin_q, origin_t, axis, dof_lo, dof_hi, dt, base_pose, base_stride, dof_state, dof_rows,
                         targets, tgt_stride, dof_row0, dof_stride, N, nb, nd, pts, pts_env_stride, carrier, NP, seg_off, NS, M, slot_body,
                         slot_C, MC, S, block_margin, sweep_dist, steps, targets_out, &FS, &lds))
        return e;
    hipLaunchKernelGGL(articulation_sweep_kernel, dim3((unsigned)N), dim3(SW_THREADS), lds, pm_stream(stream), SW_CHAIN_ARGS,
                       SW_SENSE_ARGS);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_articulation_sweep_groups_f32(
    const int32_t* parent, const int32_t* jtype, const int32_t* dof, const float* origin_q, const float* origin_t, const float* axis,
    const float* dof_lo, const float* dof_hi, const float* vmax, float dt, const float* base_pose, long base_stride,
    const float* dof_state, long dof_rows, const float* targets, long tgt_stride, const uint8_t* reset, const int32_t* dof_row0,
    long dof_stride, int N, int nb, int nd, const float* fields, const int64_t* part_off, const int32_t* part_shape,
    const float* part_bbox_min, const float* part_voxel_size, const int32_t* grid_slot, int NG, int NG_shared, const int32_t* group_off,
    int G, const int32_t* env_group, int max_group_grids, const float* pose_R, const float* pose_T, int M, int t0, int t1,
    const float* pts, long pts_env_stride, const int32_t* carrier, const int32_t* pt_id, const float* chunk_sphere, int NP,
    const int32_t* seg_off, int NS, int cull, const int32_t* slot_body, const float* slot_C, int MC, int S, float block_margin,
    const uint8_t* free_env, float* sweep_dist, int32_t* steps, float* targets_out, void* stream) {
    PM_REQUIRE(fields && part_off && part_shape && part_bbox_min && part_voxel_size && grid_slot && pose_R && pose_T);
    PM_REQUIRE(M > 0 && M <= SW_MAX_M && NG > 0 && NG_shared >= 0 && NG_shared <= NG && G >= 0 && max_group_grids >= 0);
    PM_REQUIRE(t0 >= 0 && t0 < t1 && (long)t1 <= (long)NG_shared + max_group_grids);
    PM_REQUIRE(G == 0 || (group_off && env_group));
    int FS;
    size_t lds;
    if (int e = sw_check(parent, jtype, dof, origin_q, origin_t, axis, dof_lo, dof_hi, dt, base_pose, base_stride, dof_state, dof_rows,
                         targets, tgt_stride, dof_row0, dof_stride, N, nb, nd, pts, pts_env_stride, carrier, NP, seg_off, NS, M, slot_body,
                         slot_C, MC, S, block_margin, sweep_dist, steps, targets_out, &FS, &lds))
        return e;
    const int p0 = t0, p1 = t1;
    hipLaunchKernelGGL(articulation_sweep_groups_kernel, dim3((unsigned)N), dim3(SW_THREADS), lds, pm_stream(stream), SW_CHAIN_ARGS,
                       grid_slot, NG, NG_shared, group_off, G, env_group, max_group_grids, SW_SENSE_ARGS);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
