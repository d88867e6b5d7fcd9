// Posed mesh point cloud (the reference's utils/mesh2pc.py: PCfromMesh.query_pc, :56-65) in one launch.
//
// The reference keeps the canonical surface points of every rigid part once per environment, multiplies all of them by the
// parts' poses (bmm over (b*m, p, 3): 12 x 1024 points per environment, 600 MB written at 4096 environments) and then gathers a
// random 1/12 of the result through a host index.  Here only the selected points are ever computed:
//     q = sel[k], p = part_of[q], x = pts[q],  out[b, k, j] = ((x0 R[b,p,j,0] + x1 R[b,p,j,1]) + x2 R[b,p,j,2]) + T[b,p,j]
// in fp32, every product and sum rounded on its own (common.h's posed_coord), so the bits are defined and repeat from call to call.
//
// Shape: a memory-bound gather whose only large stream is the output (12 B K bytes).  One lane owns one output FLOAT e = 3 k + j of
// a row, not one point: the 64 lanes of a wave then store 64 consecutive dwords (256 contiguous bytes) whatever the row's
// alignment, where a lane-per-point layout issues three stores of stride 12 bytes.  A thread owns MP_PER floats (e, e + 256, ...)
// and walks over the `eb` environments of its block (blockIdx.y): with a shared selection its (q, p, x) are fetched once
// and reused for every environment; with a per-environment selection they are fetched per row (sel, part_of and pts are a few
// hundred KB and stay in cache).  The block first lays the poses of its environments out in LDS as one 16-byte record
// (R[j,0], R[j,1], R[j,2], T[j]) per (environment, part, row j): 576 B per environment read from memory once per block with
// coalesced loads, after which an output float costs one ds_read_b128, three multiplies, three adds and one coalesced store.
// Parts beyond MP_STAGE_MAX_M do not fit that table: the same kernel then reads the four pose values from memory (STAGE = false).
//
// Stores stay dwords.  A row starts wherever the caller's out_stride puts it (4-byte aligned only), so a 16-byte store needs a
// per-row peel, and where out_stride is no multiple of 4 floats (an observation row of 3 * 1024 + 7) the floats a lane owns would
// shift from row to row and with them the reuse of (q, p, x).  Measured in its best case only (rows 16-byte aligned, 3 K a
// multiple of 4, one lane = 4 consecutive floats of two points, one 16-byte store): 0.119 ms against 0.134 ms on the 'all' cloud at
// B = 4096 (12 x the default output), 0.0289 against 0.0315 ms at B = 1024, and no change on the default 1024-point query, which
// the host's call overhead bounds.  An eleventh of the time on aligned rows only does not pay for a second store path.
//
// Memory safety.  q outside [0, Q) or p outside [0, M): the point's three floats are NaN and nothing is read through the bad
// index (part_of is not read for a bad q, no pose for a bad p).  A non-finite pose entry just propagates: no address depends on
// it.  Columns at and past 3 K of a row are never written.  No workspace, no atomics, stream-ordered, never synchronises.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), <STAGE, PER_ENV>: <true, false> (shared or no selection, the
// default) 45 VGPRs, 38 SGPRs; <true, true> 56 / 46; <false, false> 32 / 46; <false, true> 56 / 50; all without scratch, occupancy
// 8 waves / SIMD; LDS (dynamic) eb * M * 48 bytes = 9 KB at 12 parts and 16 environments per block.
// The labelled cloud (pm_mesh_pc_query_labeled_f32) is the same kernel with NF = 4 floats per point: lane e owns column e % 4 of
// point e / 4, and the lane of column 3 fetches labels[p] where the others fetch the point (no pose, no arithmetic).  The NF = 3
// instantiations compile to the figures above, unchanged; NF = 4: <true, false> 45 VGPRs, 46 SGPRs; <true, true> 45 / 52;
// <false, false> 32 / 52; <false, true> 44 / 56; no scratch, 8 waves / SIMD.
// Measured A/B on one MI355X, 12 parts x 1024 points, select = 'all' (K = 12288, 604 MB of output at B = 4096, where the floor is
// 0.096 ms at the 6.29 TB/s copy rate) / a 1024-point shared selection, ms per call at B = 4096 (tools/time_mesh_pc.py), kept = the
// last: one environment per block, one float per thread, poses read from memory per float 0.426 / 0.052 -> 16 environments per
// block reusing (q, p, x) 0.259 / 0.025 -> poses staged in LDS 0.188 / 0.019 -> four floats per thread 0.135 / 0.0175 (eight: 0.125 /
// 0.021; 32 environments per block: 0.125 / 0.019; 8 and two floats: 0.169 / 0.020).  That is 71 % of the output-bandwidth floor on
// the 'all' cloud (74 % in the run kept as profiles/mesh_pc_timing.json); the 1024-point query (50 MB, floor 0.008 ms) takes the same 0.018 ms at B = 64, 1024 and 4096: the host's
// per-call overhead, not the kernel, is what is timed there.
#include "common.h"

#ifndef MP_PER
#define MP_PER 4                                             // output floats per thread
#endif
#ifndef MP_EB
#define MP_EB 16                                             // environments per block (at most)
#endif
#ifndef MP_STAGE_MAX_M
#define MP_STAGE_MAX_M 64                                    // parts whose poses are staged in LDS: MP_EB * 64 * 48 B = 48 KB
#endif
#define MP_THREADS 256

typedef float mp_f4 __attribute__((ext_vector_type(4)));

struct mp_pt {
    float x0, x1, x2;
    int pj;                                                  // p * 3 + j; -1: NaN; MP_LABEL (NF = 4, column 3): the value is x0
};
#define MP_LABEL (-2)

// NF = floats per point: 3 (x, y, z) or 4 (x, y, z, labels[p]); n3 = NF * K
template <int NF>
__device__ __forceinline__ mp_pt mp_fetch(const float* __restrict__ pts, const int32_t* __restrict__ part_of, int Q, int M,
                                          const int32_t* __restrict__ selrow, const float* __restrict__ labels, long e, long n3) {
    mp_pt r = {0.f, 0.f, 0.f, -1};
    if (e >= n3) return r;
    const int k = (int)(e / NF), j = (int)(e - (long)NF * k);
    const int q = selrow ? selrow[k] : k;
    if (q < 0 || q >= Q) return r;
    const int p = part_of[q];
    if (p < 0 || p >= M) return r;
    if (NF == 4 && j == 3) {
        r.x0 = labels[p];
        r.pj = MP_LABEL;
        return r;
    }
    r.x0 = pts[3L * q];
    r.x1 = pts[3L * q + 1];
    r.x2 = pts[3L * q + 2];
    r.pj = p * 3 + j;
    return r;
}

template <int NF, bool STAGE, bool PER_ENV>
__global__ __launch_bounds__(MP_THREADS) void mesh_pc_kernel(const float* __restrict__ pts, const int32_t* __restrict__ part_of,
                                                              int Q, const float* __restrict__ pose_R,
                                                              const float* __restrict__ pose_T, int B, int M,
                                                              const int32_t* __restrict__ sel, long sel_stride, int K, int eb,
                                                              float* __restrict__ out, long out_stride,
                                                              const float* __restrict__ labels) {
    extern __shared__ mp_f4 mp_tab[];                        // [env in block][part][row j] = (R[j,0], R[j,1], R[j,2], T[j])
    const int b0 = blockIdx.y * eb;
    const int nb = min(eb, B - b0);
    const long n3 = (long)NF * K;
    const long e0 = (long)blockIdx.x * (MP_THREADS * MP_PER) + threadIdx.x;

    if (STAGE) {
        float* tab = (float*)mp_tab;
        const float* Rb = pose_R + (long)b0 * M * 9;
        const float* Tb = pose_T + (long)b0 * M * 3;
        for (int i = threadIdx.x; i < nb * M * 9; i += MP_THREADS) {
            const int bp = i / 9, c = i - bp * 9, j = c / 3;
            tab[(bp * 3 + j) * 4 + (c - j * 3)] = Rb[i];
        }
        for (int i = threadIdx.x; i < nb * M * 3; i += MP_THREADS) tab[i * 4 + 3] = Tb[i];
    }

    mp_pt pt[MP_PER];
    if (!PER_ENV) {
#pragma unroll
        for (int u = 0; u < MP_PER; ++u) pt[u] = mp_fetch<NF>(pts, part_of, Q, M, sel, labels, e0 + u * MP_THREADS, n3);
    }
    if (STAGE) __syncthreads();

    for (int bl = 0; bl < nb; ++bl) {
        const long b = b0 + bl;
        float* row = out + b * out_stride;
        if (PER_ENV) {
#pragma unroll
            for (int u = 0; u < MP_PER; ++u) pt[u] = mp_fetch<NF>(pts, part_of, Q, M, sel + b * sel_stride, labels, e0 + u * MP_THREADS, n3);
        }
#pragma unroll
        for (int u = 0; u < MP_PER; ++u) {
            const long e = e0 + u * MP_THREADS;
            if (e >= n3) continue;
            float v = __builtin_nanf("");
            const int pj = pt[u].pj;
            if (NF == 4 && pj == MP_LABEL) {
                v = pt[u].x0;
            } else if (pj >= 0) {
                float r0, r1, r2, t;
                if (STAGE) {
                    const mp_f4 w = mp_tab[bl * M * 3 + pj];
                    r0 = w.x, r1 = w.y, r2 = w.z, t = w.w;
                } else {
                    const float* R = pose_R + (b * M * 3 + pj) * 3;
                    r0 = R[0], r1 = R[1], r2 = R[2], t = pose_T[b * M * 3 + pj];
                }
                v = posed_coord(pt[u].x0, pt[u].x1, pt[u].x2, r0, r1, r2, t);
            }
            row[e] = v;
        }
    }
}

template <int NF>
static int mp_query(const float* pts, const int32_t* part_of, int Q, const float* pose_R, const float* pose_T, int B, int M,
                    const int32_t* sel, long sel_stride, int K, float* out, long out_stride, const float* labels, void* stream) {
    PM_REQUIRE(pts && part_of && pose_R && pose_T && out && (NF == 3 || labels));
    PM_REQUIRE(B >= 1 && M >= 1 && Q >= 1 && K >= 1 && B <= 65535 * MP_EB);
    PM_REQUIRE(out_stride >= (long)NF * K);
    PM_REQUIRE(sel || K == Q);
    PM_REQUIRE(sel_stride == 0 || sel_stride >= K);
    const long chunks = ((long)NF * K + MP_THREADS * MP_PER - 1) / (MP_THREADS * MP_PER);
    // fewer environments per block while the grid would leave most of the chip idle (same bits: the arithmetic does not change)
    int eb = MP_EB;
    while (eb > 1 && chunks * ((B + eb - 1) / eb) < 1024) eb >>= 1;
    const dim3 grid((unsigned)chunks, (unsigned)((B + eb - 1) / eb)), block(MP_THREADS);
    const bool stage = M <= MP_STAGE_MAX_M, per_env = sel && sel_stride != 0;
    const size_t lds = stage ? (size_t)eb * M * 3 * sizeof(mp_f4) : 0;
#define MP_LAUNCH(S, P)                                                                                                           \
    hipLaunchKernelGGL((mesh_pc_kernel<NF, S, P>), grid, block, lds, pm_stream(stream), pts, part_of, Q, pose_R, pose_T, B, M, sel, \
                       sel_stride, K, eb, out, out_stride, labels)
    if (stage && per_env) MP_LAUNCH(true, true);
    else if (stage) MP_LAUNCH(true, false);
    else if (per_env) MP_LAUNCH(false, true);
    else MP_LAUNCH(false, false);
#undef MP_LAUNCH
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_mesh_pc_query_f32(const float* pts, const int32_t* part_of, int Q, const float* pose_R, const float* pose_T,
                                    int B, int M, const int32_t* sel, long sel_stride, int K, float* out, long out_stride,
                                    void* stream) {
    return mp_query<3>(pts, part_of, Q, pose_R, pose_T, B, M, sel, sel_stride, K, out, out_stride, nullptr, stream);
}

extern "C" int pm_mesh_pc_query_labeled_f32(const float* pts, const int32_t* part_of, int Q, const float* pose_R,
                                            const float* pose_T, int B, int M, const int32_t* sel, long sel_stride, int K,
                                            float* out, long out_stride, const float* labels, void* stream) {
    return mp_query<4>(pts, part_of, Q, pose_R, pose_T, B, M, sel, sel_stride, K, out, out_stride, labels, stream);
}
