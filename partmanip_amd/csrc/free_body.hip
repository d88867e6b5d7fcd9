// One free rigid body per environment (pm_free_body_step_f32): the cube of the grasp_cube task next to the robot of articulation.hip.
// Not physics: no dynamics, no contact, no friction.  The body keeps its pose; what moves it is a stated kinematic rule in the manner of
// the hold rule of articulation_objects.hip, first match wins (include/partmanip_hip.h states each in full):
//   1. reset: the default pose (with u: xy moved inside +-reset_range, a yaw), at rest, latch cleared;
//   2. hold, not latched: the body's pose in the hand frame is written to grip once (the latch); the pose stays, at rest;
//   3. hold, latched: the body is carried, pose = hand frame o grip; linear velocity from the displacement, angular the left tip's;
//   4. otherwise: latch cleared, orientation kept, z sinks at fall_speed down to rest_z (fall_speed = 0: it stays where it is).
// The hand frame is (mean of the two tip positions, the left tip's quaternion over its norm), read from rigid_body as the robot's launch
// on the same stream left it.  The body's own pose is read from root[e, obj_actor]; the same 13 values go back there and to the body's
// row of rigid_body.  Arithmetic: float64 from the float32 inputs through articulation_common.h's helpers, every output rounded once.
//
// Shape.  One thread per environment, 64 per block: about 40 loads, 30 stores and a few hundred float64 operations per environment, so
// even 4096 environments are 64 waves on 256 CUs.  The kernel is launch-bound like its siblings and is deliberately not tuned; the
// stores of an environment are 13 + 13 (+ 8) consecutive dwords of its own rows.  Times: profiles/free_body_timing.json.
//
// Independence.  An environment's bits depend on its own rows only, not on N or on the block it lands in; a NaN stays inside its
// environment.  An environment with a row outside [0, rb_rows) stores nothing and forms no address from that row.  No atomics, no
// synchronisation, no allocation, no LDS.
#include "common.h"
#include "articulation_common.h"

#define FB_THREADS 64

__global__ __launch_bounds__(FB_THREADS) void free_body_step_kernel(
    float* rigid_body, long rb_rows, const int32_t* __restrict__ tip_rows, const int32_t* __restrict__ body_row, float* root, int na,
    int obj_actor, const uint8_t* __restrict__ hold, const uint8_t* __restrict__ reset, float* grip, const float* __restrict__ default_pose,
    const float* __restrict__ u, float reset_range, float dt_, float rest_z, float fall_speed, int N) {
    const int e = blockIdx.x * FB_THREADS + threadIdx.x;
    if (e >= N) return;
    const long tl = tip_rows[2 * e], tr = tip_rows[2 * e + 1], br = body_row[e];
    if (tl < 0 || tl >= rb_rows || tr < 0 || tr >= rb_rows || br < 0 || br >= rb_rows) return;
    float* ro = root + ((long)e * na + obj_actor) * 13;
    float* bo = rigid_body + br * 13;
    float* g = grip + (long)e * 8;
    const double dt = dt_;
    float out[13];
#pragma unroll
    for (int c = 0; c < 7; ++c) out[c] = ro[c];               // the pose as it stands: rules 2 and 4 keep (most of) it
#pragma unroll
    for (int c = 7; c < 13; ++c) out[c] = 0.0f;
    const bool held = hold[e] != 0, latched = g[7] != 0.0f;

    if (reset[e]) {
        // 1. the default pose; with u the reference's random_reset (grasp_cube.py:162-167: the angle itself, not its half)
#pragma unroll
        for (int c = 0; c < 7; ++c) out[c] = default_pose[c];
        if (u) {
            const double r = reset_range;
            out[0] = (float)((double)default_pose[0] + (2.0 * (double)u[3 * e] - 1.0) * r);
            out[1] = (float)((double)default_pose[1] + (2.0 * (double)u[3 * e + 1] - 1.0) * r);
            const double th = 6.283185307179586476925286766559 * (double)u[3 * e + 2] - 3.1415926535897932384626433832795;
            const double dq[4] = {default_pose[3], default_pose[4], default_pose[5], default_pose[6]};
            const double yq[4] = {0.0, 0.0, sin(th), cos(th)};
            double q[4];
            ar_qmul(dq, yq, q);
#pragma unroll
            for (int c = 0; c < 4; ++c) out[3 + c] = (float)q[c];
        }
        g[7] = 0.0f;
    } else if (held) {
        const float* L = rigid_body + tl * 13;
        const float* R = rigid_body + tr * 13;
        double p[3], qh[4], c0[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = 0.5 * ((double)L[c] + (double)R[c]), c0[c] = ro[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) qh[c] = L[3 + c];
        ar_qunit(qh);
        if (!latched) {
            // 2. the latch: the body in the hand frame, rel_t = R_H^T (c - p), rel_q = q_H* o q_c
            const double qc[4] = {-qh[0], -qh[1], -qh[2], qh[3]};
            const double d[3] = {c0[0] - p[0], c0[1] - p[1], c0[2] - p[2]};
            const double qb[4] = {ro[3], ro[4], ro[5], ro[6]};
            double rt[3], rq[4];
            ar_qrot(qc, d, rt);
            ar_qmul(qc, qb, rq);
            float gv[8];
#pragma unroll
            for (int c = 0; c < 3; ++c) gv[c] = (float)rt[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) gv[3 + c] = (float)rq[c];
            gv[7] = 1.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) g[c] = gv[c];
        } else {
            // 3. carried: c' = p + R_H rel_t, q' = unit(q_H o rel_q); grip is only read, so nothing drifts
            const double rt[3] = {g[0], g[1], g[2]};
            const double rq[4] = {g[3], g[4], g[5], g[6]};
            double w[3], qn[4];
            ar_qrot(qh, rt, w);
            ar_qmul(qh, rq, qn);
            ar_qunit(qn);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double cn = p[c] + w[c];
                out[c] = (float)cn;
                out[7 + c] = (float)((cn - c0[c]) / dt);
                out[10 + c] = L[10 + c];
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) out[3 + c] = (float)qn[c];
        }
    } else {
        // 4. released: z sinks towards rest_z, never below it; at or under rest_z (or NaN) it is kept
        const double z = ro[2], zr = rest_z;
        if (z > zr) {
            const double zn = fmax(zr, z - (double)fall_speed * dt);
            out[2] = (float)zn;
            out[9] = (float)((zn - z) / dt);
        }
        g[7] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 13; ++c) ro[c] = out[c];
#pragma unroll
    for (int c = 0; c < 13; ++c) bo[c] = out[c];
}

extern "C" int pm_free_body_step_f32(float* rigid_body, long rb_rows, const int32_t* tip_rows, const int32_t* body_row, float* root, int na,
                                     int obj_actor, const uint8_t* hold, const uint8_t* reset, float* grip, const float* default_pose,
                                     const float* u, float reset_range, float dt, float rest_z, float fall_speed, int N, void* stream) {
    PM_REQUIRE(rigid_body && tip_rows && body_row && root && hold && reset && grip && default_pose);
    PM_REQUIRE(N >= 1 && na >= 1 && obj_actor >= 0 && obj_actor < na);
    PM_REQUIRE(rb_rows >= 1 && rb_rows < 2147483648L);
    PM_REQUIRE(dt > 0.0f && fall_speed >= 0.0f && reset_range >= 0.0f && rest_z == rest_z);        // a NaN is refused by each of them
    const unsigned grid = (unsigned)((N + FB_THREADS - 1) / FB_THREADS);
    hipLaunchKernelGGL(free_body_step_kernel, dim3(grid), dim3(FB_THREADS), 0, pm_stream(stream), rigid_body, rb_rows, tip_rows, body_row,
                       root, na, obj_actor, hold, reset, grip, default_pose, u, reset_range, dt, rest_z, fall_speed, N);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
