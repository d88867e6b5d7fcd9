// Mesh-TSDF observation (the reference's utils/mesh2sdf.py: TSDFfromMesh.query_tsdf_parallel, :119-132, 239-272) in one launch.
//
// Per environment b and workspace voxel v the reference samples the pre-baked signed-distance grid of every rigid part p
// trilinearly at the voxel's centre under the part's pose, takes the minimum over the parts and a base field (ground plane or a
// predicted volume), divides by the truncation distance and clamps to [-1, 1].  It does so in ~40 tensor passes over (b, m, n, 3)
// and (b, m, n) intermediates (6 MB per environment each); here nothing of size B*M*n exists: one thread owns one voxel, loops
// over the parts [p0, p1) and writes one float.
//
// Shape.  A wave owns a 4 x 4 x 4 brick of voxels of one environment (lane = (i & 3, j & 3, k & 3), k fastest), a work-group four
// consecutive bricks (consecutive along k, so that its 16-byte row pieces complete 64-byte runs in L2 before they leave it).
// Before the per-voxel work the wave tests the brick against every part's valid box (brick centre through the pose, circum-radius
// scaled by the column norms of R so that a non-orthonormal R stays conservative, a margin for fp32 round-off that scales with
// the operands' magnitudes).  Lane l tests part l, so the M tests cost one evaluation; the ballot of the answers is a scalar list
// of the parts the brick can reach, and the wave loops over its set bits only.  Everything such an iteration needs besides the
// voxel index -- pose, grid offset / shape / bbox_min / voxel_size -- is then indexed by wave-uniform values (blockIdx, the wave id
// through readfirstlane, the bit position): scalar loads and SGPR operands.  The test only ever skips samples the
// per-voxel test would have called invalid (value 1 = "far", the identity of the minimum once the base field is in), so the output
// with and without it (brick_skip = 0) is bit-identical (tests/test_gpu_mesh_tsdf.py).
//
// Rounding follows the reference's tensor expressions op by op where a comparison or the result depends on it: c_v = idx *
// vox_size + origin, u = (q - bbox_min) / voxel_size with a true division, validity u >= 1 && u - res <= -2 against the part's
// OWN shape, the interpolation in the reference's association (:266-269), value * valid + 1 * !valid, / sdf_trunc, clamp.  The
// 3x3 product of step 1 is evaluated as ((d0 R0j + d1 R1j) + d2 R2j) without contraction; the reference's bmm may round it in
// another order (covered by the tests' tolerance, which is taken from the reference's own fp32-vs-fp64 error).
//
// Memory safety.  A gather happens only behind 1 <= u_a <= res_a - 2 (false for NaN / inf), so the eight corners lie inside the
// part's own grid whatever the pose holds.  An environment with a non-finite entry anywhere in its M poses is written as NaN
// (what min / clamp would propagate in the reference, whose indexing is undefined there); other environments are unaffected.
//
// A scene whose environments differ (pm_mesh_tsdf_query_groups_f32, mesh_tsdf_groups_kernel): the part tables are a grid library, an
// environment owns the shared rows and the rows of its group, and a row names the pose slot it is placed by (grid_slot).  Both
// kernels are one body, mt_body<SKIP, GROUPS>: lane l tests ORDINAL pb + l of the environment's own rows, the ballot is the list of
// ordinals to sample, and an iteration turns its ordinal into (row, slot) with scalar arithmetic and one scalar load of grid_slot
// -- group id, group offsets, row and slot are all functions of blockIdx.y and the bit position, so every table and pose read of
// the sample loop is still a scalar load (checked in the disassembly: the loop's only vector loads are the four corner gathers).
// A non-finite pose counts only in a slot one of the environment's own rows names; the NaN poses a scene's row table leaves past a
// cabinet's body count are never read into a test.  Group ids, offsets, the row bound and the slots are cut to their ranges in
// the kernel, so tables that live on the device need no validation (include/partmanip_hip.h).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): mesh_tsdf_kernel<true>: 62 VGPRs, 96 SGPRs, no scratch, no LDS,
// occupancy 8 waves / SIMD; <false> (brick test off, tests only): 30 VGPRs, 104 SGPRs, no scratch, occupancy 7.
// mesh_tsdf_groups_kernel<true>: 58 VGPRs, 73 SGPRs, no scratch, no LDS, occupancy 8; <false>: 29 VGPRs, 71 SGPRs, occupancy 8.
// Sharing the body left mesh_tsdf_kernel<true> at its registers and occupancy; <false> went from 31 to 30 VGPRs, occupancy unchanged.
// Moving the sample into mesh_sdf_sample.h (mt_sample) left all four kernels' instructions as they were, line for line.
// Measured A/B on one MI355X at B = 1024, res = 50, 12 parts (tools/time_mesh_tsdf.py), kept = the last of each line:
// part loop with one brick test per (wave, part) 4.09 ms -> lane-parallel tests + ballot 2.25 ms -> branch-free test with every
// table load up front 2.11 ms -> raw rcp / sqrt in the test 2.07 ms -> corner pairs as 8-byte gathers 1.94 ms.  That is 4 % of
// the output-bandwidth floor: the time goes to the trilinear gathers (up to 64 distinct cache lines per load instruction).
#include "mesh_sdf_sample.h"                                 // mt_sample: the per-part sample, shared with mesh_sdf_points.hip

#define MT_BRICK 4                                           // brick edge in voxels; 4^3 = one wave
#define MT_WAVES 4                                           // bricks (waves) per work-group

// The body both kernels share.  GROUPS = false: ordinal p is part p, placed by pose slot p (every group argument is a constant the
// compiler folds away).  GROUPS = true: the part tables are a grid library and environment b owns the ordinals t < n_ord -- row t
// for t < NG_shared, row g_lo + (t - NG_shared) of its group after that -- each placed by pose slot grid_slot[row].
template <bool SKIP, bool GROUPS>
__device__ __forceinline__ void mt_body(
    const float* __restrict__ fields, const int64_t* __restrict__ part_off, const int32_t* __restrict__ part_shape,
    const float* __restrict__ part_bbox_min, const float* __restrict__ part_voxel_size, const float* __restrict__ pose_R,
    const float* __restrict__ pose_T, int M, int p0, int p1, int res, int nb /* bricks per axis */, float vox_size, float ox,
    float oy, float oz, float sdf_trunc, const float* __restrict__ base, long base_stride, float* __restrict__ out,
    long out_stride, const int32_t* __restrict__ grid_slot, int NG, int NG_shared, const int32_t* __restrict__ group_off, int G,
    const int32_t* __restrict__ env_group, int max_group_grids) {
    const int b = blockIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int brick = blockIdx.x * MT_WAVES + wave;
    if (brick >= nb * nb * nb) return;                       // wave-uniform; the kernel has no barrier
    const int lane = threadIdx.x & 63;
    const int bi = brick / (nb * nb), bj = (brick / nb) % nb, bk = brick % nb;
    const int i = bi * MT_BRICK + (lane >> 4), j = bj * MT_BRICK + ((lane >> 2) & 3), k = bk * MT_BRICK + (lane & 3);
    const bool inside = i < res && j < res && k < res;
    const long v = ((long)i * res + j) * res + k;
    float* dst = out + (long)b * out_stride + v;

    // voxel centre, as the reference's `vox_coords * vox_size + vox_origin`
    const float cx = add_rn(mul_rn((float)i, vox_size), ox);
    const float cy = add_rn(mul_rn((float)j, vox_size), oy);
    const float cz = add_rn(mul_rn((float)k, vox_size), oz);
    // brick centre and circum-radius of its voxel centres (wave-uniform)
    const float hc = 0.5f * (MT_BRICK - 1);
    const float bx = (bi * MT_BRICK + hc) * vox_size + ox, by = (bj * MT_BRICK + hc) * vox_size + oy,
                bz = (bk * MT_BRICK + hc) * vox_size + oz;
    const float brad = 1.7320508f * hc * vox_size * 1.001f;
    const float* Rb = pose_R + (long)b * M * 9;
    const float* Tb = pose_T + (long)b * M * 3;

    // The environment's ordinals (wave-uniform: b is blockIdx.y, so these are scalar loads).  A group id outside [0, G) owns the shared
    // rows only; the group's offsets are cut to [0, NG - NG_shared] and its rows to max_group_grids, whatever the tables hold.
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

    // Lane l looks at part pb + l: is its pose finite, and can the brick reach its valid box?  The ballot of the answers is the
    // wave's (scalar) list of parts to sample: the twelve brick tests cost one evaluation, not twelve.
    auto parts_of = [&](int pb, bool& bad) -> unsigned long long {
        // every table and pose read happens up front and unconditionally (clamped index): no load waits behind a branch
        const int p = pb + lane;
        int pc = p < M ? p : M - 1, ps = pc;                 // the row of the part tables and the pose slot this lane reads
        bool own = true;                                     // GROUPS: the ordinal exists and its row names a pose slot in [0, M)
        if constexpr (GROUPS) {
            own = p < n_ord;
            pc = own ? (p < NG_shared ? p : g_lo + (p - NG_shared)) : 0;
            const int s = grid_slot[pc];
            own = own && s >= 0 && s < M;
            ps = own ? s : 0;                                // no pose is read through a slot outside [0, M)
        }
        const float* R = Rb + ps * 9;
        const float* T = Tb + ps * 3;
        const float r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
        const float t0 = T[0], t1 = T[1], t2 = T[2];
        const float mn0 = part_bbox_min[pc * 3], mn1 = part_bbox_min[pc * 3 + 1], mn2 = part_bbox_min[pc * 3 + 2];
        const int rx = part_shape[pc * 3], ry = part_shape[pc * 3 + 1], rz = part_shape[pc * 3 + 2];
        const float iv = __builtin_amdgcn_rcpf(part_voxel_size[pc]);   // 1 ulp: inside the margin
        bad |= own && !(mt_fin(r00) & mt_fin(r01) & mt_fin(r02) & mt_fin(r10) & mt_fin(r11) & mt_fin(r12) & mt_fin(r20) & mt_fin(r21) &
                        mt_fin(r22) & mt_fin(t0) & mt_fin(t1) & mt_fin(t2));
        int need = (int)(p >= p0) & (int)(p < p1) & (int)own;
        if (SKIP) {
            // |((c_v - c) R)_a| <= |c_v - c| * |column a of R|; the margin covers fp32 round-off of both evaluations:
            // 1e-5 of the magnitudes that enter the sums (>= 30 x the bound of the handful of fp32 operations) + 0.02 cells
            const float d0 = bx - t0, d1 = by - t1, d2 = bz - t2;
            const float a0 = fabsf(bx) + fabsf(t0) + brad, a1 = fabsf(by) + fabsf(t1) + brad, a2 = fabsf(bz) + fabsf(t2) + brad;
            int skip = 0;
#define MT_AXIS(ra, rb_, rc, mn, rn)                                                                        \
    {                                                                                                        \
        const float q = d0 * ra + d1 * rb_ + d2 * rc;                                                        \
        const float rad = brad * __builtin_amdgcn_sqrtf(ra * ra + rb_ * rb_ + rc * rc) * 1.001f;             \
        const float mag = a0 * fabsf(ra) + a1 * fabsf(rb_) + a2 * fabsf(rc) + fabsf(mn);                     \
        const float uc = (q - mn) * iv, ur = fabsf(rad * iv), mg = 0.02f + 1e-5f * fabsf(mag * iv);          \
        skip |= (int)(uc + ur < 1.0f - mg) | (int)(uc - ur > (float)(rn - 2) + mg);                          \
    }
            MT_AXIS(r00, r10, r20, mn0, rx)
            MT_AXIS(r01, r11, r21, mn1, ry)
            MT_AXIS(r02, r12, r22, mn2, rz)
#undef MT_AXIS
            need &= !skip;                                   // NaN / inf anywhere above compares false: not skipped
        }
        return __ballot(need != 0);
    };

    // non-finite pose anywhere in this environment (GROUPS: in a slot one of its own rows names) -> the whole volume is NaN (and
    // nothing below runs on garbage)
    bool bad = false;
    const unsigned long long first = parts_of(0, bad);
    for (int pb = 64; pb < n_ord; pb += 64) (void)parts_of(pb, bad);
    if (__any(bad)) {
        if (inside) *dst = __builtin_nanf("");
        return;
    }

    float m = inside ? base[(long)b * base_stride + v] : 0.0f;
    for (int pb = 0; pb < n_ord; pb += 64) {
        unsigned long long todo = pb == 0 ? first : parts_of(pb, bad);
        while (todo) {
            int p = pb + (int)__builtin_ctzll(todo);         // wave-uniform: the loads below are scalar loads
            todo &= todo - 1;
            int slot = p;
            if constexpr (GROUPS) {                          // the ordinal's row and the slot it names (in [0, M): parts_of saw to that)
                p = p < NG_shared ? p : g_lo + (p - NG_shared);
                slot = grid_slot[p];
            }
            const float* R = Rb + slot * 9;
            const float* T = Tb + slot * 3;
            const mt_part P = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], T[0], T[1], T[2], part_bbox_min[p * 3],
                               part_bbox_min[p * 3 + 1], part_bbox_min[p * 3 + 2], part_voxel_size[p], part_shape[p * 3],
                               part_shape[p * 3 + 1], part_shape[p * 3 + 2], part_off[p]};
            const float val = mt_sample(fields, P, cx, cy, cz, inside);
            m = mt_min_nan(m, val);
        }
    }
    if (inside) {
        const float s = __fdiv_rn(m, sdf_trunc);
        *dst = s != s ? s : fminf(fmaxf(s, -1.0f), 1.0f);
    }
}

template <bool SKIP>
__global__ __launch_bounds__(64 * MT_WAVES) void mesh_tsdf_kernel(
    const float* __restrict__ fields, const int64_t* __restrict__ part_off, const int32_t* __restrict__ part_shape,
    const float* __restrict__ part_bbox_min, const float* __restrict__ part_voxel_size, const float* __restrict__ pose_R,
    const float* __restrict__ pose_T, int M, int p0, int p1, int res, int nb, float vox_size, float ox, float oy, float oz,
    float sdf_trunc, const float* __restrict__ base, long base_stride, float* __restrict__ out, long out_stride) {
    mt_body<SKIP, false>(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, M, p0, p1, res, nb, vox_size, ox,
                         oy, oz, sdf_trunc, base, base_stride, out, out_stride, nullptr, 0, 0, nullptr, 0, nullptr, 0);
}

// The scene whose environments differ: the same launch shape, the ordinals [t0, t1) of each environment's own rows.
template <bool SKIP>
__global__ __launch_bounds__(64 * MT_WAVES) void mesh_tsdf_groups_kernel(
    const float* __restrict__ fields, const int64_t* __restrict__ part_off, const int32_t* __restrict__ part_shape,
    const float* __restrict__ part_bbox_min, const float* __restrict__ part_voxel_size, const int32_t* __restrict__ grid_slot, int NG,
    int NG_shared, const int32_t* __restrict__ group_off, int G, const int32_t* __restrict__ env_group, int max_group_grids,
    const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M, int t0, int t1, int res, int nb, float vox_size,
    float ox, float oy, float oz, float sdf_trunc, const float* __restrict__ base, long base_stride, float* __restrict__ out,
    long out_stride) {
    mt_body<SKIP, true>(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, M, t0, t1, res, nb, vox_size, ox,
                        oy, oz, sdf_trunc, base, base_stride, out, out_stride, grid_slot, NG, NG_shared, group_off, G, env_group,
                        max_group_grids);
}

extern "C" int pm_mesh_tsdf_query_groups_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape,
                                             const float* part_bbox_min, const float* part_voxel_size, const int32_t* grid_slot,
                                             int NG, int NG_shared, const int32_t* group_off, int G, const int32_t* env_group,
                                             int max_group_grids, const float* pose_R, const float* pose_T, int B, int M, int t0,
                                             int t1, int res, float vox_size, float ox, float oy, float oz, float sdf_trunc,
                                             const float* base, int base_per_env, float* out, long out_stride, int brick_skip,
                                             void* stream) {
    PM_REQUIRE(fields && part_off && part_shape && part_bbox_min && part_voxel_size && grid_slot && pose_R && pose_T && base && out);
    PM_REQUIRE(B > 0 && B <= 65535 && M > 0 && NG > 0 && NG_shared >= 0 && NG_shared <= NG && G >= 0 && max_group_grids >= 0);
    PM_REQUIRE(t0 >= 0 && t0 < t1 && (long)t1 <= (long)NG_shared + max_group_grids && res > 0 && res <= 1024);
    PM_REQUIRE(G == 0 || (group_off && env_group));
    const long n = (long)res * res * res;
    PM_REQUIRE(out_stride >= n && sdf_trunc > 0.f);
    const int nb = (res + MT_BRICK - 1) / MT_BRICK;
    const long bricks = (long)nb * nb * nb;
    const dim3 grid((unsigned)((bricks + MT_WAVES - 1) / MT_WAVES), (unsigned)B), block(64 * MT_WAVES);
    const long base_stride = base_per_env ? n : 0;
    if (brick_skip)
        hipLaunchKernelGGL(mesh_tsdf_groups_kernel<true>, grid, block, 0, pm_stream(stream), fields, part_off, part_shape,
                           part_bbox_min, part_voxel_size, grid_slot, NG, NG_shared, group_off, G, env_group, max_group_grids, pose_R,
                           pose_T, M, t0, t1, res, nb, vox_size, ox, oy, oz, sdf_trunc, base, base_stride, out, out_stride);
    else
        hipLaunchKernelGGL(mesh_tsdf_groups_kernel<false>, grid, block, 0, pm_stream(stream), fields, part_off, part_shape,
                           part_bbox_min, part_voxel_size, grid_slot, NG, NG_shared, group_off, G, env_group, max_group_grids, pose_R,
                           pose_T, M, t0, t1, res, nb, vox_size, ox, oy, oz, sdf_trunc, base, base_stride, out, out_stride);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_mesh_tsdf_query_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape,
                                      const float* part_bbox_min, const float* part_voxel_size, const float* pose_R,
                                      const float* pose_T, int B, int M, int p0, int p1, int res, float vox_size, float ox,
                                      float oy, float oz, float sdf_trunc, const float* base, int base_per_env, float* out,
                                      long out_stride, int brick_skip, void* stream) {
    PM_REQUIRE(fields && part_off && part_shape && part_bbox_min && part_voxel_size && pose_R && pose_T && base && out);
    PM_REQUIRE(B > 0 && B <= 65535 && M > 0 && p0 >= 0 && p0 < p1 && p1 <= M && res > 0 && res <= 1024);
    const long n = (long)res * res * res;
    PM_REQUIRE(out_stride >= n && sdf_trunc > 0.f);
    const int nb = (res + MT_BRICK - 1) / MT_BRICK;
    const long bricks = (long)nb * nb * nb;
    const dim3 grid((unsigned)((bricks + MT_WAVES - 1) / MT_WAVES), (unsigned)B), block(64 * MT_WAVES);
    const long base_stride = base_per_env ? n : 0;
    if (brick_skip)
        hipLaunchKernelGGL(mesh_tsdf_kernel<true>, grid, block, 0, pm_stream(stream), fields, part_off, part_shape, part_bbox_min,
                           part_voxel_size, pose_R, pose_T, M, p0, p1, res, nb, vox_size, ox, oy, oz, sdf_trunc, base, base_stride,
                           out, out_stride);
    else
        hipLaunchKernelGGL(mesh_tsdf_kernel<false>, grid, block, 0, pm_stream(stream), fields, part_off, part_shape, part_bbox_min,
                           part_voxel_size, pose_R, pose_T, M, p0, p1, res, nb, vox_size, ox, oy, oz, sdf_trunc, base, base_stride,
                           out, out_stride);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
