// Signed distance of posed points to the scene's part grids (pm_mesh_sdf_points_f32 / pm_mesh_sdf_points_groups_f32): contact sensing.
//
// mesh_tsdf.hip samples the parts' baked signed-distance grids at the workspace lattice, into a clamped and normalised volume.  This
// file samples the same grids, with the same per-part arithmetic (mt_sample of mesh_sdf_sample.h: it exists once), at ARBITRARY points
// that ride on pose slots of their own -- surface samples of the hand and the fingers against the cube's grid or the cabinet's -- and
// returns metres: per point the minimum over the environment's own ordinals and the ordinal that attains it, per segment of points
// (one sensing body) the minimum and the point that attains it.
//
// Shape.  One work-group of four waves per (segment, environment), or per 256 points when there are no segments.  A wave takes the
// segment's 64-point chunks in turn (chunk c of the segment = points seg_off[s] + 64 c ...), lane = point.  The point is loaded and
// posed once, through its own carrier (vector loads, outside the sample loop); the ordinals are then walked as in mesh_tsdf.hip:
// lane l tests ordinal pb + l, the ballot is the scalar list of ordinals to sample, and an iteration's row, slot, pose and part tables
// are indexed by wave-uniform values, so they are scalar loads -- the loop's only vector loads are the four 8-byte corner gathers.
// The per-wave cull needs a bounding sphere of the chunk: chunk_sphere holds it in the frame of the chunk's carrier, built by the
// caller once (partmanip_amd/contact.py sorts the points by carrier and pads every run to whole chunks); the wave poses the centre
// with scalar loads, scales the radius by the Frobenius norm of the carrier's R (>= its largest singular value, so a non-orthonormal
// R stays conservative) and tests it against every ordinal's valid box with the inequality of mesh_tsdf.hip's brick test (that test
// stays written out over there: routing it through a shared function changed mesh_tsdf_kernel<true>'s registers, 62 -> 60 VGPRs).
// The cull is used for a chunk only when it starts on a multiple of 64 points and all its points share one carrier (checked here,
// wave-uniform); it only ever skips samples the per-point test would have called invalid (value 1, the identity of the minimum), so
// the outputs with cull on and off are bit-identical (tests/test_gpu_mesh_sdf_points.py).
//
// The segment minimum is a 64-bit minimum of (distance bits made order-preserving, NaN -> 0 so that it wins) << 32 | point id: lanes
// keep their own running key, a wave reduces with shuffles, the four waves meet in LDS.  No floating-point atomics, no dependence on
// timing: the result is bit-reproducible, ties go to the smaller id, and the first NaN wins.
//
// A non-finite pose.  Ungrouped: in any of the M slots.  Grouped: in a slot that one of the environment's own rows or any point's
// carrier names -- the work-group marks those slots in an LDS bit set (integer OR, so order does not matter) before it looks at a
// pose, and the NaN poses a scene's row table leaves past a cabinet's body count are never examined.  Such an environment is
// written as NaN / -1 and nothing else runs on it.
//
// Memory safety: segment offsets are cut to [0, NP] and made non-decreasing, carriers outside [-1, M) read no pose, group tables are
// cut as in mesh_tsdf.hip, gathers stay behind the validity test, a chunk's sphere row is (start / 64) < ceil(NP / 64).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): mesh_sdf_points_kernel: 62 VGPRs, 104 SGPRs, no scratch, 40 bytes
// of LDS, occupancy 7 waves / SIMD; mesh_sdf_points_groups_kernel: 62 VGPRs, 106 SGPRs, no scratch, 4136 bytes of LDS (the slot bit
// set), occupancy 7.  Timings: tools/time_contact.py, profiles/contact_timing.json.
#include "mesh_sdf_sample.h"

#define SP_WAVES 4                                           // waves per work-group
#define SP_MAX_M 32768                                       // grouped entry: pose slots the LDS bit set has room for

__device__ __forceinline__ unsigned sp_ordered(float v) {    // unsigned order == float order; NaN -> 0 (below -inf): NaN wins a minimum
    const unsigned u = __float_as_uint(v);
    return v != v ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float sp_unordered(unsigned k) {
    return k == 0u ? __builtin_nanf("") : __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
#define SP_KEY_NONE ((0xBF800000ull << 32) | 0xFFFFFFFFull)  // sp_ordered(1.0f), id -1: the empty segment

// The ball (centre b, radius brad, world frame) against a part's valid box: nonzero iff NO point of the ball can give a valid sample.
// |((c - b) R)_a| <= |c - b| * |column a of R|; the margin covers fp32 round-off of this evaluation and of the per-point one: 1e-5
// of the magnitudes that enter the sums (a0, a1, a2: what the centre and T were summed from, plus the radius) + 0.02 cells.
// iv = 1 / voxel_size to 1 ulp.  NaN / inf anywhere compares false: not skipped.
__device__ __forceinline__ int sp_out_of_reach(float bx, float by, float bz, float brad, float a0, float a1, float a2, float r00,
                                               float r01, float r02, float r10, float r11, float r12, float r20, float r21, float r22,
                                               float t0, float t1, float t2, float mn0, float mn1, float mn2, int rx, int ry, int rz,
                                               float iv) {
    const float d0 = bx - t0, d1 = by - t1, d2 = bz - t2;
    int skip = 0;
#define SP_AXIS(ra, rb_, rc, mn, rn)                                                                        \
    {                                                                                                        \
        const float q = d0 * ra + d1 * rb_ + d2 * rc;                                                        \
        const float rad = brad * __builtin_amdgcn_sqrtf(ra * ra + rb_ * rb_ + rc * rc) * 1.001f;             \
        const float mag = a0 * fabsf(ra) + a1 * fabsf(rb_) + a2 * fabsf(rc) + fabsf(mn);                     \
        const float uc = (q - mn) * iv, ur = fabsf(rad * iv), mg = 0.02f + 1e-5f * fabsf(mag * iv);          \
        skip |= (int)(uc + ur < 1.0f - mg) | (int)(uc - ur > (float)(rn - 2) + mg);                          \
    }
    SP_AXIS(r00, r10, r20, mn0, rx)
    SP_AXIS(r01, r11, r21, mn1, ry)
    SP_AXIS(r02, r12, r22, mn2, rz)
#undef SP_AXIS
    return skip;
}

__device__ __forceinline__ int sp_pose_finite(const float* __restrict__ R, const float* __restrict__ T) {
    int ok = 1;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok &= mt_fin(R[i]);
    return ok & mt_fin(T[0]) & mt_fin(T[1]) & mt_fin(T[2]);
}

// GROUPS = false: ordinal p is part p, placed by pose slot p.  GROUPS = true: the grid library of mesh_tsdf.hip's grouped kernel.
template <bool GROUPS>
__device__ __forceinline__ void sp_body(
    const float* __restrict__ fields, const int64_t* __restrict__ part_off, const int32_t* __restrict__ part_shape,
    const float* __restrict__ part_bbox_min, const float* __restrict__ part_voxel_size, const float* __restrict__ pose_R,
    const float* __restrict__ pose_T, int M, int p0, int p1, const float* __restrict__ pts, long pts_env_stride,
    const int32_t* __restrict__ carrier, const int32_t* __restrict__ pt_id, const float* __restrict__ chunk_sphere, int NP,
    const int32_t* __restrict__ seg_off, int NS, float* __restrict__ dist, long ld_dist, int32_t* __restrict__ arg,
    float* __restrict__ seg_min, int32_t* __restrict__ seg_arg, int cull, const int32_t* __restrict__ grid_slot, int NG, int NG_shared,
    const int32_t* __restrict__ group_off, int G, const int32_t* __restrict__ env_group, int max_group_grids) {
    __shared__ unsigned named[GROUPS ? SP_MAX_M / 32 : 1];
    __shared__ int bad_s;
    __shared__ unsigned long long red[SP_WAVES];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* Rb = pose_R + (long)b * M * 9;
    const float* Tb = pose_T + (long)b * M * 3;

    // this work-group's points [lo, hi): a segment, or 256 consecutive points
    int lo, hi;
    if (NS > 0) {
        lo = min(max(seg_off[blockIdx.x], 0), NP);
        hi = min(max(seg_off[blockIdx.x + 1], lo), NP);
    } else {
        lo = (int)blockIdx.x * (64 * SP_WAVES);
        hi = min(lo + 64 * SP_WAVES, NP);
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

    // ---- a non-finite pose in a slot that counts -> the environment is NaN
    if (tid == 0) bad_s = 0;
    if constexpr (GROUPS) {
        for (int i = tid; i < (M + 31) / 32; i += 64 * SP_WAVES) named[i] = 0u;
        __syncthreads();
        for (int t = tid; t < n_ord; t += 64 * SP_WAVES) {
            const int s = grid_slot[t < NG_shared ? t : g_lo + (t - NG_shared)];
            if (s >= 0 && s < M) atomicOr(&named[s >> 5], 1u << (s & 31));
        }
        for (int n = tid; n < NP; n += 64 * SP_WAVES) {
            const int s = carrier[n];
            if (s >= 0 && s < M) atomicOr(&named[s >> 5], 1u << (s & 31));
        }
    }
    __syncthreads();
    for (int s = tid; s < M; s += 64 * SP_WAVES) {
        bool look = true;
        if constexpr (GROUPS) look = (named[s >> 5] >> (s & 31)) & 1u;
        if (look && !sp_pose_finite(Rb + s * 9, Tb + s * 3)) bad_s = 1;
    }
    __syncthreads();
    if (bad_s) {                                             // uniform over the work-group
        for (int n = lo + tid; n < hi; n += 64 * SP_WAVES) {
            if (dist) dist[(long)b * ld_dist + n] = __builtin_nanf("");
            if (arg) arg[(long)b * ld_dist + n] = -1;
        }
        if (seg_min && tid == 0) {
            seg_min[(long)b * NS + blockIdx.x] = __builtin_nanf("");
            seg_arg[(long)b * NS + blockIdx.x] = -1;
        }
        return;
    }

    unsigned long long best = SP_KEY_NONE;
    const int nchunks = (hi - lo + 63) >> 6;
    for (int c = wave; c < nchunks; c += SP_WAVES) {
        const int start = lo + c * 64;                       // wave-uniform
        const int n = start + lane;
        const bool act = n < hi;
        const int nc = act ? n : hi - 1;                     // a lane past the end reads the last point and writes nothing
        const float* pp = pts + (long)b * pts_env_stride + 3L * nc;
        const float x0 = pp[0], x1 = pp[1], x2 = pp[2];
        const int ca = carrier[nc];
        const int id = pt_id ? pt_id[nc] : nc;
        const bool posed = ca >= 0 && ca < M;
        const bool ok = act && (posed || ca == -1);          // a carrier outside [-1, M): 1 / -1, no pose read through it
        float wx = x0, wy = x1, wz = x2;
        if (posed) {
            const float* R = Rb + ca * 9;
            const float* T = Tb + ca * 3;
            wx = posed_coord(x0, x1, x2, R[0], R[1], R[2], T[0]);
            wy = posed_coord(x0, x1, x2, R[3], R[4], R[5], T[1]);
            wz = posed_coord(x0, x1, x2, R[6], R[7], R[8], T[2]);
        }

        // the chunk's bounding sphere in the world frame (wave-uniform: scalar loads and arithmetic)
        const int c0 = __builtin_amdgcn_readfirstlane(ca);   // lane 0 is always a real point of the chunk
        const bool use_cull = cull && chunk_sphere && (start & 63) == 0 && __all(!act || ca == c0);
        float sx = 0.f, sy = 0.f, sz = 0.f, sr = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f;
        if (use_cull) {
            const float* S = chunk_sphere + (long)(start >> 6) * 4;
            const float ux = S[0], uy = S[1], uz = S[2];
            sx = ux, sy = uy, sz = uz, sr = S[3];
            e0 = fabsf(ux), e1 = fabsf(uy), e2 = fabsf(uz);
            if (c0 >= 0 && c0 < M) {
                const float* R = Rb + c0 * 9;
                const float* T = Tb + c0 * 3;
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

        // lane l looks at ordinal pb + l: is it in [p0, p1), one of the environment's own, and within the sphere's reach?
        auto ordinals = [&](int pb) -> unsigned long long {
            const int p = pb + lane;
            int pc = p < M ? p : M - 1, ps = pc;
            bool own = p < M;
            if constexpr (GROUPS) {
                own = p < n_ord;
                pc = own ? (p < NG_shared ? p : g_lo + (p - NG_shared)) : 0;
                const int s = grid_slot[pc];
                own = own && s >= 0 && s < M;
                ps = own ? s : 0;
            }
            int need = (int)(p >= p0) & (int)(p < p1) & (int)own;
            if (use_cull) {
                const float* R = Rb + ps * 9;
                const float* T = Tb + ps * 3;
                const float t0 = T[0], t1 = T[1], t2 = T[2];
                const float iv = __builtin_amdgcn_rcpf(part_voxel_size[pc]);
                need &= !sp_out_of_reach(sx, sy, sz, sr, e0 + fabsf(t0) + sr, e1 + fabsf(t1) + sr, e2 + fabsf(t2) + sr, R[0], R[1], R[2],
                                         R[3], R[4], R[5], R[6], R[7], R[8], t0, t1, t2, part_bbox_min[pc * 3], part_bbox_min[pc * 3 + 1],
                                         part_bbox_min[pc * 3 + 2], part_shape[pc * 3], part_shape[pc * 3 + 1], part_shape[pc * 3 + 2], iv);
            }
            return __ballot(need != 0);
        };

        float m = 1.0f;
        int am = -1;
        for (int pb = 0; pb < n_ord; pb += 64) {
            unsigned long long todo = ordinals(pb);
            while (todo) {
                const int t = pb + (int)__builtin_ctzll(todo);   // wave-uniform: the loads below are scalar loads
                todo &= todo - 1;
                int p = t, slot = t;
                if constexpr (GROUPS) {                      // the ordinal's row and the slot it names (in [0, M): ordinals saw to that)
                    p = t < NG_shared ? t : g_lo + (t - NG_shared);
                    slot = grid_slot[p];
                }
                const float* R = Rb + slot * 9;
                const float* T = Tb + slot * 3;
                const mt_part P = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], T[0], T[1], T[2], part_bbox_min[p * 3],
                                   part_bbox_min[p * 3 + 1], part_bbox_min[p * 3 + 2], part_voxel_size[p], part_shape[p * 3],
                                   part_shape[p * 3 + 1], part_shape[p * 3 + 2], part_off[p]};
                const float val = mt_sample(fields, P, wx, wy, wz, ok);
                if (val < m || (val != val && m == m)) am = t;   // the smallest ordinal that attains the minimum; the first NaN
                m = mt_min_nan(m, val);
            }
        }
        if (act) {
            if (dist) dist[(long)b * ld_dist + n] = m;
            if (arg) arg[(long)b * ld_dist + n] = am;
            if (id >= 0) {                                   // a negative id is a padding lane: in no segment result
                const unsigned long long key = ((unsigned long long)sp_ordered(m) << 32) | (unsigned)id;
                best = key < best ? key : best;
            }
        }
    }
    if (seg_min) {                                           // uniform; every wave of the work-group gets here
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        if (lane == 0) red[wave] = best;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < SP_WAVES; ++w) best = red[w] < best ? red[w] : best;
            seg_min[(long)b * NS + blockIdx.x] = sp_unordered((unsigned)(best >> 32));
            seg_arg[(long)b * NS + blockIdx.x] = (int)(unsigned)(best & 0xFFFFFFFFull);
        }
    }
}

__global__ __launch_bounds__(64 * SP_WAVES) void mesh_sdf_points_kernel(
    const float* __restrict__ fields, const int64_t* __restrict__ part_off, const int32_t* __restrict__ part_shape,
    const float* __restrict__ part_bbox_min, const float* __restrict__ part_voxel_size, const float* __restrict__ pose_R,
    const float* __restrict__ pose_T, int M, int p0, int p1, const float* __restrict__ pts, long pts_env_stride,
    const int32_t* __restrict__ carrier, const int32_t* __restrict__ pt_id, const float* __restrict__ chunk_sphere, int NP,
    const int32_t* __restrict__ seg_off, int NS, float* __restrict__ dist, long ld_dist, int32_t* __restrict__ arg,
    float* __restrict__ seg_min, int32_t* __restrict__ seg_arg, int cull) {
    sp_body<false>(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, M, p0, p1, pts, pts_env_stride, carrier,
                   pt_id, chunk_sphere, NP, seg_off, NS, dist, ld_dist, arg, seg_min, seg_arg, cull, nullptr, 0, 0, nullptr, 0, nullptr, 0);
}

__global__ __launch_bounds__(64 * SP_WAVES) void mesh_sdf_points_groups_kernel(
    const float* __restrict__ fields, const int64_t* __restrict__ part_off, const int32_t* __restrict__ part_shape,
    const float* __restrict__ part_bbox_min, const float* __restrict__ part_voxel_size, const int32_t* __restrict__ grid_slot, int NG,
    int NG_shared, const int32_t* __restrict__ group_off, int G, const int32_t* __restrict__ env_group, int max_group_grids,
    const float* __restrict__ pose_R, const float* __restrict__ pose_T, int M, int t0, int t1, const float* __restrict__ pts,
    long pts_env_stride, const int32_t* __restrict__ carrier, const int32_t* __restrict__ pt_id,
    const float* __restrict__ chunk_sphere, int NP, const int32_t* __restrict__ seg_off, int NS, float* __restrict__ dist,
    long ld_dist, int32_t* __restrict__ arg, float* __restrict__ seg_min, int32_t* __restrict__ seg_arg, int cull) {
    sp_body<true>(fields, part_off, part_shape, part_bbox_min, part_voxel_size, pose_R, pose_T, M, t0, t1, pts, pts_env_stride, carrier,
                  pt_id, chunk_sphere, NP, seg_off, NS, dist, ld_dist, arg, seg_min, seg_arg, cull, grid_slot, NG, NG_shared, group_off, G,
                  env_group, max_group_grids);
}

// the argument rules the two entries share
static int sp_check(const void* pts, long pts_env_stride, const void* carrier, int NP, const void* seg_off, int NS, const void* dist,
                    long ld_dist, const void* arg, const void* seg_min, const void* seg_arg) {
    PM_REQUIRE(pts && carrier && NP > 0 && NP <= (1 << 30) && NS >= 0);
    PM_REQUIRE(pts_env_stride == 0 || pts_env_stride >= 3L * NP);
    PM_REQUIRE((seg_min == nullptr) == (seg_arg == nullptr) && (dist || seg_min));
    PM_REQUIRE(NS == 0 || seg_off);
    PM_REQUIRE(!seg_min || NS > 0);
    PM_REQUIRE(!(dist || arg) || ld_dist >= NP);
    return PM_OK;
}

extern "C" int pm_mesh_sdf_points_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape, const float* part_bbox_min,
                                      const float* part_voxel_size, const float* pose_R, const float* pose_T, int B, int M, int p0, int p1,
                                      const float* pts, long pts_env_stride, const int32_t* carrier, const int32_t* pt_id,
                                      const float* chunk_sphere, int NP, const int32_t* seg_off, int NS, float* dist, long ld_dist,
                                      int32_t* arg, float* seg_min, int32_t* seg_arg, int cull, void* stream) {
    PM_REQUIRE(fields && part_off && part_shape && part_bbox_min && part_voxel_size && pose_R && pose_T);
    PM_REQUIRE(B > 0 && B <= 65535 && M > 0 && p0 >= 0 && p0 < p1 && p1 <= M);
    if (int e = sp_check(pts, pts_env_stride, carrier, NP, seg_off, NS, dist, ld_dist, arg, seg_min, seg_arg)) return e;
    const dim3 grid((unsigned)(NS > 0 ? NS : (NP + 64 * SP_WAVES - 1) / (64 * SP_WAVES)), (unsigned)B), block(64 * SP_WAVES);
    hipLaunchKernelGGL(mesh_sdf_points_kernel, grid, block, 0, pm_stream(stream), fields, part_off, part_shape, part_bbox_min,
                       part_voxel_size, pose_R, pose_T, M, p0, p1, pts, pts_env_stride, carrier, pt_id, chunk_sphere, NP, seg_off, NS, dist,
                       ld_dist, arg, seg_min, seg_arg, cull);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_mesh_sdf_points_groups_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape,
                                             const float* part_bbox_min, const float* part_voxel_size, const int32_t* grid_slot, int NG,
                                             int NG_shared, const int32_t* group_off, int G, const int32_t* env_group,
                                             int max_group_grids, const float* pose_R, const float* pose_T, int B, int M, int t0, int t1,
                                             const float* pts, long pts_env_stride, const int32_t* carrier, const int32_t* pt_id,
                                             const float* chunk_sphere, int NP, const int32_t* seg_off, int NS, float* dist, long ld_dist,
                                             int32_t* arg, float* seg_min, int32_t* seg_arg, int cull, void* stream) {
    PM_REQUIRE(fields && part_off && part_shape && part_bbox_min && part_voxel_size && grid_slot && pose_R && pose_T);
    PM_REQUIRE(B > 0 && B <= 65535 && M > 0 && M <= SP_MAX_M && NG > 0 && NG_shared >= 0 && NG_shared <= NG && G >= 0 &&
               max_group_grids >= 0);
    PM_REQUIRE(t0 >= 0 && t0 < t1 && (long)t1 <= (long)NG_shared + max_group_grids);
    PM_REQUIRE(G == 0 || (group_off && env_group));
    if (int e = sp_check(pts, pts_env_stride, carrier, NP, seg_off, NS, dist, ld_dist, arg, seg_min, seg_arg)) return e;
    const dim3 grid((unsigned)(NS > 0 ? NS : (NP + 64 * SP_WAVES - 1) / (64 * SP_WAVES)), (unsigned)B), block(64 * SP_WAVES);
    hipLaunchKernelGGL(mesh_sdf_points_groups_kernel, grid, block, 0, pm_stream(stream), fields, part_off, part_shape, part_bbox_min,
                       part_voxel_size, grid_slot, NG, NG_shared, group_off, G, env_group, max_group_grids, pose_R, pose_T, M, t0, t1, pts,
                       pts_env_stride, carrier, pt_id, chunk_sphere, NP, seg_off, NS, dist, ld_dist, arg, seg_min, seg_arg, cull);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
