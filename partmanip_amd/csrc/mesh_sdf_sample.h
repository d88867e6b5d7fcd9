// The arithmetic the mesh-TSDF observation (mesh_tsdf.hip) and the point query (mesh_sdf_points.hip) share: one trilinear sample of a
// part's signed-distance grid at a world point under the part's pose.  It is specified op by op (include/partmanip_hip.h) and exists
// here once.
#pragma once
#include "common.h"

typedef float mt_f2 __attribute__((ext_vector_type(2), aligned(4)));
__device__ __forceinline__ int mt_fin(float x) { return isfinite(x) ? 1 : 0; }
__device__ __forceinline__ float mt_min_nan(float m, float v) { return (v < m || v != v) ? v : m; }   // torch.min: NaN wins

// A part as one sample reads it: its pose (R row-major, T), the grid's bbox_min, voxel size, shape and offset into `fields`.
struct mt_part {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22, t0, t1, t2, mn0, mn1, mn2, vs;
    int rx, ry, rz;
    long off;
};

// The sample of the part's grid at the world point (cx, cy, cz): d = c - T, q = ((d0 R0j + d1 R1j) + d2 R2j), u = (q - bbox_min) /
// voxel_size with a true division, valid iff `inside` and 1 <= u_a, u_a - shape_a <= -2 on all three axes, then the reference's
// trilinear association (mesh2sdf.py:266-269); an invalid sample is 1 ("far").  Every operation is one correctly rounded fp32
// operation.  A gather happens only behind the validity test, so the eight corners lie inside the part's own grid whatever the
// pose and the point hold (false for NaN / inf).
__device__ __forceinline__ float mt_sample(const float* __restrict__ fields, const mt_part& P, float cx, float cy, float cz, bool inside) {
    const float d0 = sub_rn(cx, P.t0), d1 = sub_rn(cy, P.t1), d2 = sub_rn(cz, P.t2);
    const float q0 = add_rn(add_rn(mul_rn(d0, P.r00), mul_rn(d1, P.r10)), mul_rn(d2, P.r20));
    const float q1 = add_rn(add_rn(mul_rn(d0, P.r01), mul_rn(d1, P.r11)), mul_rn(d2, P.r21));
    const float q2 = add_rn(add_rn(mul_rn(d0, P.r02), mul_rn(d1, P.r12)), mul_rn(d2, P.r22));
    const float u0 = __fdiv_rn(sub_rn(q0, P.mn0), P.vs), u1 = __fdiv_rn(sub_rn(q1, P.mn1), P.vs), u2 = __fdiv_rn(sub_rn(q2, P.mn2), P.vs);
    const int rx = P.rx, ry = P.ry, rz = P.rz;
    const int valid = (int)inside & (int)(u0 >= 1.0f) & (int)(sub_rn(u0, (float)rx) <= -2.0f) & (int)(u1 >= 1.0f) &
                      (int)(sub_rn(u1, (float)ry) <= -2.0f) & (int)(u2 >= 1.0f) & (int)(sub_rn(u2, (float)rz) <= -2.0f);
    float val = 1.0f;
    if (valid) {                                             // 1 <= l_a <= r_a - 2: all eight corners inside the part's grid
        const int l0 = (int)u0, l1 = (int)u1, l2 = (int)u2;
        const float x = sub_rn(u0, (float)l0), y = sub_rn(u1, (float)l1), z = sub_rn(u2, (float)l2);
        const float* f = fields + P.off + ((unsigned)(l0 * ry + l1) * (unsigned)rz + (unsigned)l2);
        const unsigned sy = (unsigned)rz, sx = (unsigned)rz * (unsigned)ry;
        // the two corners along z are neighbours in memory: one 8-byte load each (4-byte aligned) -- the gathers are what
        // the kernels wait for (64 lanes x distinct cache lines per instruction), so four of them instead of eight
        const mt_f2 c00 = *(const mt_f2*)f, c01 = *(const mt_f2*)(f + sy), c10 = *(const mt_f2*)(f + sx),
                    c11 = *(const mt_f2*)(f + sx + sy);
        const float f000 = c00.x, f001 = c00.y, f010 = c01.x, f011 = c01.y;
        const float f100 = c10.x, f101 = c10.y, f110 = c11.x, f111 = c11.y;
        const float zc = sub_rn(1.0f, z), yc = sub_rn(1.0f, y), xc = sub_rn(1.0f, x);
        const float lo = add_rn(mul_rn(add_rn(mul_rn(f000, zc), mul_rn(f001, z)), yc),
                                mul_rn(add_rn(mul_rn(f010, zc), mul_rn(f011, z)), y));
        const float hi = add_rn(mul_rn(add_rn(mul_rn(f100, zc), mul_rn(f101, z)), yc),
                                mul_rn(add_rn(mul_rn(f110, zc), mul_rn(f111, z)), y));
        val = add_rn(add_rn(mul_rn(lo, xc), mul_rn(hi, x)), 0.0f);   // value * valid + 1 * !valid
    }
    return val;
}
