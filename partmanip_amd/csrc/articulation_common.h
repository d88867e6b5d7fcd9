// What the two kinematic kernels share (articulation.hip: one robot per environment; articulation_objects.hip: one object tree of
// the environment's own type): the quaternion helpers, the per-body frame step in its two halves (parent o origin, then the joint)
// and one Jacobian entry.  Each is written once so that both kernels round alike: a tree stepped as a robot and as an object gives
// the same body rows bit for bit.  Plain __device__ __forceinline__ functions over their call sites' arguments.
#pragma once

#define AR_THREADS 256
#define AR_MAX 64                                             // bodies and DOFs at most: 64-bit ancestor masks, the static tables
#define AR_REVOLUTE 1
#define AR_PRISMATIC 2

// Hamilton product of quaternions (x, y, z, w): the rotation b, then a
__device__ __forceinline__ void ar_qmul(const double* a, const double* b, double* o) {
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    o[1] = ((a[3] * b[1] - a[0] * b[2]) + a[1] * b[3]) + a[2] * b[0];
    o[2] = ((a[3] * b[2] + a[0] * b[1]) - a[1] * b[0]) + a[2] * b[3];
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
}

// v turned by the unit quaternion q: v + 2 w (u x v) + 2 u x (u x v)
__device__ __forceinline__ void ar_qrot(const double* q, const double* v, double* o) {
    const double cx = q[1] * v[2] - q[2] * v[1], cy = q[2] * v[0] - q[0] * v[2], cz = q[0] * v[1] - q[1] * v[0];
    const double dx = q[1] * cz - q[2] * cy, dy = q[2] * cx - q[0] * cz, dz = q[0] * cy - q[1] * cx;
    o[0] = v[0] + 2.0 * (q[3] * cx + dx);
    o[1] = v[1] + 2.0 * (q[3] * cy + dy);
    o[2] = v[2] + 2.0 * (q[3] * cz + dz);
}

__device__ __forceinline__ void ar_qunit(double* q) {
    const double s = 1.0 / sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] *= s, q[1] *= s, q[2] *= s, q[3] *= s;
}

// The first half of a body's frame step: parent (pp, pq) o origin (row b of origin_t / origin_q) -> the joint's frame (pos, fq)
// before the joint moves.
__device__ __forceinline__ void ar_frame_origin(const double* pp, const double* pq, const float* origin_t, const float* origin_q, int b,
                                                double* pos, double* fq) {
    double ot[3], oq[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) ot[c] = origin_t[b * 3 + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) oq[c] = origin_q[b * 4 + c];
    ar_qrot(pq, ot, pos);
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[c] = pp[c] + pos[c];
    ar_qmul(pq, oq, fq);
}

// The second half: the joint itself at position th, a rotation about the local axis al (revolute) or a translation along the world
// axis aw (prismatic).  The caller divides fq by its norm afterwards (ar_qunit), fixed joints included.
__device__ __forceinline__ void ar_frame_joint(int jt, const double* al, const double* aw, double th, double* pos, double* fq) {
    if (jt == AR_REVOLUTE) {
        const double h = 0.5 * th, sn = sin(h), cs = cos(h);
        const double jq[4] = {al[0] * sn, al[1] * sn, al[2] * sn, cs};
        double t4[4];
        ar_qmul(fq, jq, t4);
#pragma unroll
        for (int c = 0; c < 4; ++c) fq[c] = t4[c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) pos[c] = pos[c] + aw[c] * th;
    }
}

// Entry (r, d) of body `body`'s Jacobian, for a DOF d that IS an ancestor: rb = the environment's staged body rows, ax its world axes,
// info = the DOF's own body | its joint type << 8.
__device__ __forceinline__ float ar_jentry(const float* rb, const float* ax, int body, int r, int d, int info) {
    const float* a = ax + d * 3;
    if ((info >> 8) == AR_PRISMATIC) return r < 3 ? a[r] : 0.0f;
    if (r >= 3) return a[r - 3];
    const float* pb = rb + body * 13;
    const float* pj = rb + (info & 0xff) * 13;
    const int i = r == 2 ? 0 : r + 1, j = r == 0 ? 2 : r - 1;                       // (a x v)[r] = a[i] v[j] - a[j] v[i]
    return a[i] * (pb[j] - pj[j]) - a[j] * (pb[i] - pj[i]);
}
