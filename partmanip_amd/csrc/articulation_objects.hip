// One articulated object per environment, each environment its own tree out of a library of K (pm_articulation_objects_step_f32):
// the cabinets of the open_drawer task next to the robot of articulation.hip, in the simulator's flat layouts (rigid_body (B, 13),
// dof_state (D, 2)) that task_open_drawer.hip reads.  Not physics: no dynamics, no contact, no gravity.  An object's joints keep their
// state; the one thing that moves a joint is the hold rule below, a stated kinematic rule and not a grasp.
//
// Shape.  Per environment the call writes nb_k * 13 floats (and the 2 of the target DOF row under the hold rule): no Jacobian, so the
// stores are small and the serially dependent chain of frames is what there is to do.  The reference hands its objects out as
// env % num_objs, so neighbouring environments hold different trees and one lane per environment in index order would read every
// table at 64 different addresses.  The host therefore passes `order` (N): the environments grouped by type, built once.  A block
// takes `eb` consecutive entries of it, one environment per lane of its first wave; except at the seam between two types a wave reads
// the tables at wave-uniform addresses.  Nothing else depends on `order`: an environment is computed by one lane from its own rows.
//   0. one thread per slot resolves its environment: type, table offsets, first rows, the hold flags; everything is checked here
//      and an environment that fails a check takes no further part (nb = 0); one thread then lays the slots' body counts end to end;
//   1. thread i owns one (slot, DOF): (q, qd) from dof_state into LDS (the target DOF of an environment that is not held gets
//      qd = 0 when the hold group is given); one (slot, body): the DOF's own body and joint type into LDS;
//   2. chain: as in articulation.hip, float64 frames rounded once (articulation_common.h, so the same tree gives the same bits in
//      both kernels).  Where the walk reaches the held target joint its world axis and origin are known and do not depend on its own
//      q, so q' is computed there, in float64 from the two tip rows as they stand in rigid_body, before the joint is applied;
//   3. one thread per (body, component) of the block's bodies sums J qd over the ancestor DOFs in ascending order, the entries from
//      the float32 rows exactly as the robot kernel forms them; then the body rows go out as runs of nb_k * 13 dwords and the
//      target DOF rows as runs of 2.
// Every global store is lane-consecutive within its run; the chain stores nothing to memory.
//
// Independence.  An environment's bits depend on its own rows only: not on N, on `order`, on its neighbours' types, on eb or on the
// block it lands in.  A NaN stays inside its environment.  No atomics, no synchronisation, no allocation.
//
// LDS.  Dynamic, per slot (7 max_nb) | 1 doubles and (13 max_nb + 6 max_nd) | 1 floats, sized for the LARGEST tree of the library
// (the host cannot see which types a block will meet): 8460 B where a 64 x 64 tree is in the library, so 4 environments per block
// there, and 64 per block for cabinets of a few bodies.  eb by ts_envs_per_block.  Times: profiles/kinematic_scene_timing.json.
#include "common.h"
#include "task_common.h"                                      // ts_clamp, ts_envs_per_block, TS_LDS_MAX
#include "articulation_common.h"

// the slot that holds body g of the block's bodies laid end to end: off [neb + 1] ascending, off[0] = 0, g < off[neb]
__device__ __forceinline__ int ao_slot_of(const int* off, int neb, int g) {
    int lo = 0, hi = neb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(AR_THREADS) void articulation_objects_step_kernel(
    const int32_t* __restrict__ body_off, const int32_t* __restrict__ dof_off, int K, int TB, int TD, int MB, int MD,
    const int32_t* __restrict__ parent, const int32_t* __restrict__ jtype, const int32_t* __restrict__ dof,
    const float* __restrict__ origin_q, const float* __restrict__ origin_t, const float* __restrict__ axis,
    const unsigned long long* __restrict__ anc_mask, const float* __restrict__ dof_lo, const float* __restrict__ dof_hi,
    const int32_t* __restrict__ obj_type, const int32_t* __restrict__ order, const float* __restrict__ obj_pose, long pose_stride,
    const int32_t* __restrict__ rb_row0, const int32_t* __restrict__ dof_row0, float* dof_state, long dof_rows, float* rigid_body,
    long rb_rows, const uint8_t* __restrict__ hold, const uint8_t* __restrict__ reset, const int32_t* __restrict__ target_dof,
    const int32_t* __restrict__ tip_rows, float dt, int N, int eb, int DS, int ES) {
    extern __shared__ double ao_chain[];                      // [eb][DS] doubles: the chain's frames [MB][7]; then [eb][ES] floats
    float* ao_lds = (float*)(ao_chain + (long)eb * DS);       // a slot's row: rb [MB][13] | q [MD] | qd [MD] | axis [MD][3] | info [MD]
    __shared__ int s_env[AR_MAX], s_bo[AR_MAX], s_do[AR_MAX], s_nb[AR_MAX], s_nd[AR_MAX], s_rb[AR_MAX], s_df[AR_MAX], s_tgt[AR_MAX];
    __shared__ int s_held[AR_MAX], s_tipl[AR_MAX], s_tipr[AR_MAX], s_off[AR_MAX + 1];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * eb;
    const int neb = min(eb, N - b0);
    const int RB = MB * 13;

    // 0. the slots.  nb = 0 marks an environment that stores nothing: no address is formed from a value that failed its check.
    if (tid < neb) {
        int nb = 0, nd = 0, bo = 0, dofo = 0, rr = 0, dr = 0, tgt = -1, held = 0, tl = 0, tr = 0;
        const int e = order ? order[b0 + tid] : b0 + tid;
        if (e >= 0 && e < N) {
            const int k = obj_type[e];
            if (k >= 0 && k < K) {
                const long bo_ = body_off[k], b1 = body_off[k + 1], do_ = dof_off[k], d1 = dof_off[k + 1];
                const long r_ = rb_row0[e], d_ = dof_row0[e];
                bool ok = bo_ >= 0 && b1 - bo_ >= 1 && b1 - bo_ <= MB && b1 <= TB && do_ >= 0 && d1 - do_ >= 1 && d1 - do_ <= MD && d1 <= TD &&
                          r_ >= 0 && r_ + (b1 - bo_) <= rb_rows && d_ >= 0 && d_ + (d1 - do_) <= dof_rows;
                if (ok && hold) {
                    tgt = target_dof[e], tl = tip_rows[2 * e], tr = tip_rows[2 * e + 1];
                    ok = tgt >= 0 && tgt < d1 - do_ && tl >= 0 && tl < rb_rows && tr >= 0 && tr < rb_rows;
                    held = hold[e] && !reset[e];
                }
                if (ok) nb = (int)(b1 - bo_), nd = (int)(d1 - do_), bo = (int)bo_, dofo = (int)do_, rr = (int)r_, dr = (int)d_;
            }
        }
        s_env[tid] = e, s_bo[tid] = bo, s_do[tid] = dofo, s_nb[tid] = nb, s_nd[tid] = nd, s_rb[tid] = rr, s_df[tid] = dr;
        s_tgt[tid] = nb ? tgt : -1, s_held[tid] = nb ? held : 0, s_tipl[tid] = tl, s_tipr[tid] = tr;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int s = 0; s < neb; ++s) s_off[s] = o, o += s_nb[s];
        s_off[neb] = o;
    }
    // 1. joint states and the DOFs' own bodies into LDS
    for (int i = tid; i < neb * MD; i += AR_THREADS) {
        const int s = i / MD, d = i - s * MD;
        float* E = ao_lds + s * ES + RB;
        if (d < s_nd[s]) {
            const float* g = dof_state + ((long)s_df[s] + d) * 2;
            E[d] = g[0];
            E[MD + d] = (hold && d == s_tgt[s] && !s_held[s]) ? 0.0f : g[1];
        }
        ((int*)(E + 5 * MD))[d] = -1;
    }
    __syncthreads();
    for (int i = tid; i < neb * MB; i += AR_THREADS) {
        const int s = i / MB, b = i - s * MB;
        if (b < s_nb[s]) {
            const int d = dof[s_bo[s] + b], jt = jtype[s_bo[s] + b];
            if ((jt == AR_REVOLUTE || jt == AR_PRISMATIC) && d >= 0 && d < s_nd[s]) ((int*)(ao_lds + s * ES + RB + 5 * MD))[d] = b | (jt << 8);
        }
    }
    __syncthreads();

    // 2. the chain, one environment per lane of the first wave (eb <= 64)
    if (tid < neb && s_nb[tid] > 0) {
        const int s = tid, nb = s_nb[s], nd = s_nd[s], bo = s_bo[s];
        float* rb = ao_lds + s * ES;
        double* fr = ao_chain + s * DS;
        float* qs = rb + RB;
        float* ax = rb + RB + 2 * MD;
        const float* bp = obj_pose + (long)s_env[s] * pose_stride;
        const int tgt = s_held[s] ? s_tgt[s] : -1;
        double base[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) base[c] = bp[c];
        ar_qunit(base + 3);
        for (int b = 0; b < nb; ++b) {
            const int p = parent[bo + b];
            double pp[3], pq[4], pos[3], fq[4];
#pragma unroll
            for (int c = 0; c < 3; ++c) pp[c] = (p >= 0 && p < b) ? fr[p * 7 + c] : base[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) pq[c] = (p >= 0 && p < b) ? fr[p * 7 + 3 + c] : base[3 + c];
            ar_frame_origin(pp, pq, origin_t + (long)bo * 3, origin_q + (long)bo * 4, b, pos, fq);
            const int jt = jtype[bo + b], d = dof[bo + b];
            if ((jt == AR_REVOLUTE || jt == AR_PRISMATIC) && d >= 0 && d < nd) {
                const float* al_ = axis + (long)(bo + b) * 3;
                const double al[3] = {al_[0], al_[1], al_[2]};
                double aw[3];
                ar_qrot(fq, al, aw);
#pragma unroll
                for (int c = 0; c < 3; ++c) ax[d * 3 + c] = (float)aw[c];
                if (d == tgt) {
                    // the hold rule: the joint follows the component of the tips' mean velocity that it can follow
                    const float* tl = rigid_body + (long)s_tipl[s] * 13;
                    const float* tr = rigid_body + (long)s_tipr[s] * 13;
                    double pm[3], vm[3], cv[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) pm[c] = 0.5 * ((double)tl[c] + (double)tr[c]), vm[c] = 0.5 * ((double)tl[7 + c] + (double)tr[7 + c]);
                    if (jt == AR_PRISMATIC) {
                        cv[0] = aw[0], cv[1] = aw[1], cv[2] = aw[2];
                    } else {
                        const double r0 = pm[0] - pos[0], r1 = pm[1] - pos[1], r2 = pm[2] - pos[2];
                        cv[0] = aw[1] * r2 - aw[2] * r1, cv[1] = aw[2] * r0 - aw[0] * r2, cv[2] = aw[0] * r1 - aw[1] * r0;
                    }
                    const double cc = (cv[0] * cv[0] + cv[1] * cv[1]) + cv[2] * cv[2];
                    const double cvv = (cv[0] * vm[0] + cv[1] * vm[1]) + cv[2] * vm[2];
                    const double dq = cc == 0.0 ? 0.0 : ((double)dt * cvv) / cc;
                    const float q0 = qs[d];
                    const float qn = ts_clamp((float)((double)q0 + dq), dof_lo[s_do[s] + d], dof_hi[s_do[s] + d]);
                    qs[d] = qn, qs[MD + d] = (qn - q0) / dt;
                }
                ar_frame_joint(jt, al, aw, (double)qs[d], pos, fq);
            }
            ar_qunit(fq);
#pragma unroll
            for (int c = 0; c < 3; ++c) fr[b * 7 + c] = pos[c], rb[b * 13 + c] = (float)pos[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) fr[b * 7 + 3 + c] = fq[c], rb[b * 13 + 3 + c] = (float)fq[c];
        }
    }
    __syncthreads();

    // 3. velocities: (J qd)[r] per body of the block, summed over the ancestor DOFs in ascending order
    const int bodies = s_off[neb];
    for (int i = tid; i < bodies * 6; i += AR_THREADS) {
        const int g = i / 6, r = i - g * 6;
        const int s = ao_slot_of(s_off, neb, g), b = g - s_off[s], nd = s_nd[s];
        float* rb = ao_lds + s * ES;
        const float* qd = rb + RB + MD;
        const int* info_ = (const int*)(rb + RB + 5 * MD);
        const unsigned long long m = anc_mask[s_bo[s] + b];
        float sum = 0.0f;
        for (int d = 0; d < nd; ++d) {
            const int info = info_[d];
            if (info >= 0 && ((m >> d) & 1ull)) sum = sum + ar_jentry(rb, rb + RB + 2 * MD, b, r, d, info) * qd[d];
        }
        rb[b * 13 + 7 + r] = sum;
    }
    __syncthreads();
    // rows out: runs of nb_k * 13 dwords at the object's first row; the target DOF rows: runs of 2
    for (int i = tid; i < bodies * 13; i += AR_THREADS) {
        const int g = i / 13, c = i - g * 13;
        const int s = ao_slot_of(s_off, neb, g), b = g - s_off[s];
        rigid_body[((long)s_rb[s] + b) * 13 + c] = ao_lds[s * ES + b * 13 + c];
    }
    if (hold) {
        for (int i = tid; i < neb * 2; i += AR_THREADS) {
            const int s = i >> 1, c = i & 1, d = s_tgt[s];
            if (s_nb[s] > 0 && d >= 0) dof_state[((long)s_df[s] + d) * 2 + c] = ao_lds[s * ES + RB + c * MD + d];
        }
    }
}

extern "C" int pm_articulation_objects_step_f32(const int32_t* body_off, const int32_t* dof_off, int K, int total_bodies, int total_dofs,
                                                int max_nb, int max_nd, const int32_t* parent, const int32_t* jtype, const int32_t* dof,
                                                const float* origin_q, const float* origin_t, const float* axis, const uint64_t* anc_mask,
                                                const float* dof_lo, const float* dof_hi, const int32_t* obj_type, const int32_t* order,
                                                const float* obj_pose, long pose_stride, const int32_t* obj_rb_row0,
                                                const int32_t* obj_dof_row0, float* dof_state, long dof_rows, float* rigid_body, long rb_rows,
                                                const uint8_t* hold, const uint8_t* reset, const int32_t* target_dof, const int32_t* tip_rows,
                                                float dt, int N, void* stream) {
    PM_REQUIRE(body_off && dof_off && parent && jtype && dof && origin_q && origin_t && axis && anc_mask && dof_lo && dof_hi);
    PM_REQUIRE(obj_type && obj_pose && obj_rb_row0 && obj_dof_row0 && dof_state && rigid_body);
    PM_REQUIRE(N >= 1 && K >= 1 && max_nb >= 1 && max_nb <= AR_MAX && max_nd >= 1 && max_nd <= AR_MAX);
    PM_REQUIRE(total_bodies >= 1 && total_dofs >= 1);
    PM_REQUIRE(pose_stride == 0 || pose_stride >= 7);
    PM_REQUIRE(dof_rows >= 1 && dof_rows < 2147483648L && rb_rows >= 1 && rb_rows < 2147483648L);
    const bool any = hold || reset || target_dof || tip_rows;
    if (any) PM_REQUIRE(hold && reset && target_dof && tip_rows && dt > 0.0f);       // the hold group comes together; a NaN dt is refused too
    const int DS = (7 * max_nb) | 1, ES = (13 * max_nb + 6 * max_nd) | 1;
    const long env_bytes = 8L * DS + 4L * ES;
    const int eb = ts_envs_per_block(N, env_bytes, AR_MAX, TS_LDS_MAX);
    PM_REQUIRE(eb * env_bytes <= TS_LDS_MAX);
    const unsigned grid = (unsigned)((N + eb - 1) / eb);
    hipLaunchKernelGGL(articulation_objects_step_kernel, dim3(grid), dim3(AR_THREADS), (size_t)(eb * env_bytes), pm_stream(stream),
                       body_off, dof_off, K, total_bodies, total_dofs, max_nb, max_nd, parent, jtype, dof, origin_q, origin_t, axis,
                       (const unsigned long long*)anc_mask, dof_lo, dof_hi, obj_type, order, obj_pose, pose_stride, obj_rb_row0,
                       obj_dof_row0, dof_state, dof_rows, rigid_body, rb_rows, hold, reset, target_dof, tip_rows, dt, N, eb, DS, ES);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
