// Screened PointNet encoder forward (tanh, fp32 results): layers 1 and 2 are pn_fwd_kernel's, bit for bit; layer 3
// (256 -> 512, 80 % of the dense kernel's MFMA time) is only evaluated where the pooling can see it.  Included by
// pointnet_enc.hip after the dense forward, whose device pieces it reuses.
//
// Layer 3 is linear and feeds a max and a mean over the cloud's points:
//   mean_p(W3 h2[p] + b3) = W3 mean_p(h2[p]) + b3        one 256 x 512 matrix-vector product per cloud;
//   max_p                                                 only the winning point of every channel matters.
// Per 64-point tile the kernel computes an APPROXIMATE layer 3 as ONE fp16 product (h16 = fp16(h2), w16 = fp16(2^s_c W3[c]),
// both round-to-nearest-even; z~ = fmaf(sum_k w16 h16, 2^-s_c, b3) with the sum on v_mfma_f32_32x32x16_f16: 64 MFMAs of 32
// cycles per wave against 512 of 64), and with a rigorous per-channel bound eps_c >= |z~ - z^| (z^ = the fp32 dot product
// below) keeps only the points
//   !(z~ < m~ - 2 eps_c)   and   !(z~ + eps_c <= vmax)           m~ = tile maximum of z~, vmax = running exact maximum
// Both tests are written negated, so a NaN or infinite z~ / eps / vmax lands on the survivor side.  A skipped point p
// has z^_p <= z~_p + eps < m~ - eps <= z^_q for the tile's q = argmax z~ (or z^_p <= vmax): it can neither beat nor tie.
// Every survivor (p, c) is then evaluated exactly: eight lanes, lane j takes k = 4 j + 32 i + e (i = 0..7, e = 0..3) as
// one fmaf chain in that order, the eight partial sums are combined by the xor-4, -2, -1 butterfly, and b3_c is added
// last -- one fixed order, whatever the other survivors are.  A sum that is zero returns b3_c ITSELF, sign included: that
// is the IEEE sum in every case but (+0) + (-0), which would be +0, so a zero row gives its bias back bit for bit (the
// values stay numerically equal to what the plain add returns).  The running maximum takes v when
// v > vmax || (v == vmax && p < imax), so survivor order cannot change the result and ties go to the lowest point.
// A wave whose tile has more than PS_CAP survivors (degenerate clouds: all points equal, zero padding) runs the dense
// fp32 layer 3 of pn_fwd_kernel for that tile instead: such a tile costs the dense layer 3 PLUS the screen it already ran,
// at this kernel's two waves per SIMD (a batch of all-equal clouds is timed in profiles/round7_pointnet_screen.md).
//
// eps_c (ps_pack_kernel).  With |h| <= 1 under tanh, S = sum_k |w_ck| |h_k| <= ||W3[c]||_1 =: L.  Row c is scaled by the exact
// power of two 2^s (s = s_c: the row's largest finite magnitude lands in [2^14, 2^15), so no finite weight overflows fp16's
// 65504; s <= 126, which is also what an all-zero / all-non-finite row gets); x' = 2^s w below, and everything up to the
// un-scaling is in that domain.  The bound is written for a matrix unit that FLUSHES fp16 subnormal inputs; one that keeps
// them only has smaller operand errors, so it covers both.
// fp16 has 11 significant bits: round-to-nearest leaves up to 2^-11 RELATIVE (half an ulp of 2^-10), which over both operands
// would be 2^-10 L.  Both halves are taken tighter, from what is known:
//   w:      w' = w16 + r_w.  The pack step HAS the weights: R = sum_k rho_k with rho_k = |w' - w16| (exact in fp32) where w16 is
//           normal, and max(|w'|, |w' - w16|) where it is subnormal or zero (kept, or flushed to zero), is the row's own
//           rounding residual, whatever the conversion's rounding mode: |sum_k r_w h| <= R  (about 0.36 * 2^-11 2^s L for
//           weights with random mantissas).  This also holds the flushed-subnormal weights; no separate absolute term.
//   h:      h = h16 + r_h under v_cvt_pk_f16_f32, round to nearest even in the default mode (not the truncating v_cvt_pkrtz;
//           the instruction is in the .s).  |h| <= 1: in [2^-1, 1) an ulp is 2^-11, so |r_h| <= 2^-12 ABSOLUTE there and
//           less in every lower binade; 1 is exact; below 2^-14 the operand is kept or flushed, |r_h| <= 2^-14.  So
//           |r_h| <= 2^-12 everywhere (also for a tanh that overshoots 1 by a few ulp: it rounds to 1), and
//           |sum_k w16 r_h| <= 2^-12 S16,  S16 = sum_k |w16| <= (1 + 2^-11) 2^s L
//   sum:    256 products of fp16 values, each exact in fp32 (11 x 11 bits), of total magnitude <= S16, accumulated in fp32
//           from zero in the matrix unit's own order; one rounding of at most 2^-23 relative per accumulation (covers
//           round-to-nearest and truncation); no product is below 2^-48, so nothing underflows      -> 513 * 2^-24 L
//   z~:     fmaf(sum, 2^-s, b3): the product is exact, ONE rounding of |z~| <= (1 + 2^-10)(L + |b3|)  -> 2 * 2^-24 (L + |b3|)
//   tests:  m~ - 2 eps and z~ + eps each round once, |.| <= (1 + 2^-9)(L + |b3|)                    -> 4 * 2^-24 (L + |b3|)
//   z^:     256 fmaf + 3 butterfly adds + the bias add, round-to-nearest                            -> 260 * 2^-24 (L + |b3|)
//   fp32 underflow of z~ and of the 260 steps of z^ (each <= 2^-126 if flushed)                     -> 2^-116       (absolute)
//   eps_c = ((R + 2^-12 S16) 2^-s + 1024 * 2^-24 (L + |b3_c|)) (1 + 2^-10) + 2^-116, in double, rounded up to float
// 779 of the 1024 units of 2^-24 are used above; the rest and the factor 1 + 2^-10 cover the roundings of the three sums
// themselves, a 2^s w that underflows fp32 for s < 0 (<= 2^-132 L) and a tanh a few ulp above 1.  R, L, and with them eps_c,
// are inf / NaN for a row that holds an inf / NaN: every test is then false and every point of the channel survives
// (z~ = -inf, eps = inf: -inf < m~ - inf is false, -inf + inf = NaN <= vmax is false).  tests/test_pointnet_screen_bound.py
// holds the formula against an emulation of z~ (subnormals kept and flushed, random and worst-sign accumulation orders,
// operands at fp16 rounding midpoints with aligned signs).
// For default-initialised weights eps_c is about 4.8e-4 (L + |b3|), 3.5 x the three-product split-bf16 screen's this replaces,
// for a third of its MFMAs and half its LDS planes; results are the same bit for bit, since every survivor goes through the
// one exact finish above.  Measured (profiles/round10_pointnet_screen_fp16.md): 6.3 survivors per (cloud, channel) on the
// bench's cubes against 4.1 and the launch 3.35 -> 2.86 ms; posed mesh surface clouds, whose coplanar points are near-ties in
// many channels, go 9.0 -> 29.6 survivors and 4.0 -> 5.6 ms: the wider band costs there more than the MFMAs it saves.
// Since then the finish sums its lanes on DPP moves and hands each value over with one ds_max_u64 (ps_sum8, ps_best_pack
// below; profiles/round11_pointnet_screen_finish.md): a pass of eight survivors 2 k -> 0.9 k cycles, the launch 2.89 ->
// 2.53 ms, the mesh clouds 5.6 -> 3.8 ms, every output (as a number) and counter unchanged.
//
// Work-group: 8 waves own one cloud; wave w owns channels [64 w, 64 w + 64) in layer 3 and keeps their running (vmax, imax)
// in LDS, one packed 64-bit word per channel (ps_best_pack) that the finish raises with ds_max_u64 and the select pass reads
// back; lane l of it keeps pois of channel 64 w + l.  LDS: fp32 H tile 66.5 KB (H1, then H2) + fp16 plane of H2 33.8 KB +
// survivor list 8 KB + running maxima 4 KB + 4 KB = 116 864 B: one work-group per CU, two waves per SIMD.
#pragma once

typedef _Float16 ps_f16x8 __attribute__((ext_vector_type(8)));

#define PS_LDP (PN_C2 + 8)               // halfwords per plane row (528 B: 16 rows hit 16 distinct 16-B slots, as in pointnet_enc_bf3.hip)
#define PS_CAP 256                       // survivors per wave and tile before the dense fallback (~100 cycles each against 32768 dense;
                                         // the first tile of a random cloud has 85 - 115 per wave on average, C = 6 ... 3: no running
                                         // maximum prunes it yet)
#define PS_NW 8
#define PS_P3 (16 * 16 * 64 * 8)         // halfwords of the W3 plane: [nb 16][step 16][lane 64][8]
// packed buffer (bytes): W3 fp16 plane (rows scaled by 2^s_c) | W3 row-major fp32 | eps[512] | 2^-s_c [512]
#define PS_OFF_P3 0
#define PS_OFF_W3 (2 * PS_P3)
#define PS_OFF_EPS (PS_OFF_W3 + PN_C3 * PN_C2 * 4)
#define PS_OFF_INV (PS_OFF_EPS + PN_C3 * 4)
#define PS_PACKED_BYTES (PS_OFF_INV + PN_C3 * 4)
#ifndef PS_ABLATE
#define PS_ABLATE 0          // profiling only (wrong results, same launch; tools/build_ab.py): 1 = no layer 1, 2 = no layer-2 MFMAs, 4 = no tanh
                             // in the layer-2 epilogue, 8 = no plane stores after tile 0, 16 = no screen MFMAs, 32 = no select / scan (and so
                             // no finish), 64 = no survivor finish, 128 = no h2_save copy.  Every stand-in changes what the screen sees: read the
                             // survivor / fallback counters next to each timing.  Measured (profiles/round8_pointnet_screen_overlap.md): 2, 4, 32, 64
                             // and 128 keep the survivor count (3.8 - 4.1 per cloud and channel) and price their part; 1, 8 and 16 quadruple it and
                             // price nothing.
#endif
#ifndef PS_SCHED_DEFAULT
#define PS_SCHED_DEFAULT 0   // schedule of pm_pointnet_enc_fwd_screen_f32: 0 = lock-step, 1 = staggered (profiles/round8_pointnet_screen_overlap.md)
#endif

extern "C" size_t pm_pointnet_packed_screen_bytes(void) { return PS_PACKED_BYTES; }

__device__ __forceinline__ unsigned ps_cvt_pk(float a, float b) {          // {fp16(a) | fp16(b) << 16}, RNE under the default mode
    unsigned r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));        // pure: the compiler may schedule and combine it
    return r;
}

// One block per W3 row c, one thread per element k: the row's largest finite magnitude and its L1 norm (double, a fixed tree)
// give s_c and eps_c; the element goes to its slot of the fp16 plane, scaled, and to the row-major fp32 copy as it is.
__global__ __launch_bounds__(PN_C2) void ps_pack_kernel(const float* __restrict__ W3, const float* __restrict__ b3,
                                                         unsigned char* __restrict__ packed) {
    __shared__ double Ls[PN_C2], Rs[PN_C2], Ss[PN_C2];
    __shared__ float Ms[PN_C2];
    const int c = blockIdx.x, k = threadIdx.x;
    const float w = W3[c * PN_C2 + k];
    const float aw = fabsf(w);
    Ls[k] = (double)aw;
    Ms[k] = aw < INFINITY ? aw : 0.f;                                      // inf and NaN do not take part in the scale
    __syncthreads();
    for (int o = PN_C2 / 2; o > 0; o >>= 1) {
        if (k < o) {
            Ls[k] += Ls[k + o];
            Ms[k] = fmaxf(Ms[k], Ms[k + o]);
        }
        __syncthreads();
    }
    int ex = -200;                                                         // no finite non-zero weight: the clamp below decides
    if (Ms[0] > 0.f) frexpf(Ms[0], &ex);                                   // max = m 2^ex, m in [0.5, 1)
    const int s = min(15 - ex, 126);                                       // 2^s max in [2^14, 2^15); 2^s and 2^-s are normal floats (ex <= 128)
    const float ws = ldexpf(w, s);
    const _Float16 w16 = (_Float16)ws;
    const float wf = (float)w16, d = fabsf(ws - wf);                       // the difference is exact in fp32
    Rs[k] = (double)(fabsf(wf) < 0x1p-14f ? fmaxf(fabsf(ws), d) : d);      // a subnormal operand may be kept (d) or flushed (|w'|)
    Ss[k] = (double)fabsf(wf);
    __syncthreads();
    for (int o = PN_C2 / 2; o > 0; o >>= 1) {
        if (k < o) {
            Rs[k] += Rs[k + o];
            Ss[k] += Ss[k + o];
        }
        __syncthreads();
    }
    const int nb = c >> 5, li = c & 31, step = k >> 4, lq = (k >> 3) & 1, e = k & 7;
    ((_Float16*)(packed + PS_OFF_P3))[(((nb * 16 + step) * 64) + lq * 32 + li) * 8 + e] = w16;
    ((float*)(packed + PS_OFF_W3))[c * PN_C2 + k] = w;
    if (k == 0) {
        const double ed = ((Rs[0] + 0x1p-12 * Ss[0]) * ldexp(1.0, -s) + 1024.0 * 0x1p-24 * (Ls[0] + fabs((double)b3[c]))) * (1.0 + 0x1p-10) + 0x1p-116;
        float ef = (float)ed;
        if ((double)ef < ed) ef = __uint_as_float(__float_as_uint(ef) + 1);   // round up (a NaN or inf eps stays what it is: the test is false)
        ((float*)(packed + PS_OFF_EPS))[c] = ef;
        ((float*)(packed + PS_OFF_INV))[c] = ldexpf(1.f, -s);
    }
}

extern "C" int pm_pointnet_pack_weights_screen(const float* W3, const float* b3, void* packed, void* stream) {
    PM_REQUIRE(W3 && b3 && packed);
    if (((uintptr_t)packed & 15) != 0) return PM_EALIGN;
    hipLaunchKernelGGL(ps_pack_kernel, dim3(PN_C3), dim3(PN_C2), 0, pm_stream(stream), W3, b3, (unsigned char*)packed);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

#define PS_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ ps_f16x8 ps_h(const uint4& v) { return *(const ps_f16x8*)&v; }

// acc[mb][nb] += A(64 rows, the fp16 plane in LDS) * B(the packed fp16 plane), K = 256 in 16 steps of 16, one MFMA per (mb, nb)
// and step.  A step is 4 MFMAs (128 cycles a wave, 256 for the SIMD's two), far less than an L2 round trip, so B is fetched
// THREE steps ahead (four register sets in a ring) and A one step ahead, pinned with sched_barrier as in pointnet_enc_bf3.hip;
// the last three steps fetch nothing, so nothing is read past the plane.
__device__ __forceinline__ void ps_stream(const unsigned short* __restrict__ A, const uint4* __restrict__ B, f32x16 (&acc)[2][2]) {
    uint4 b0[2], b1[2], b2[2], b3[2], a0[2], a1[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        b0[nb] = B[(size_t)(nb * 16 + 0) * 64];
        b1[nb] = B[(size_t)(nb * 16 + 1) * 64];
        b2[nb] = B[(size_t)(nb * 16 + 2) * 64];
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) a0[mb] = *(const uint4*)(A + mb * 32 * PS_LDP);
#define PS_STEP(S_, AC, AN, BC, BN, PFA, PFB)                                                  \
    {                                                                                          \
        if (PFA) {                                                                             \
            _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                   \
                AN[mb] = *(const uint4*)(A + mb * 32 * PS_LDP + ((S_) + 1) * 16);              \
        }                                                                                      \
        if (PFB) {                                                                             \
            _Pragma("unroll") for (int nb = 0; nb < 2; ++nb)                                   \
                BN[nb] = B[(size_t)(nb * 16 + (S_) + 3) * 64];                                 \
        }                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        _Pragma("unroll") for (int nb = 0; nb < 2; ++nb)                                       \
            _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                   \
                acc[mb][nb] = PS_MFMA(ps_h(AC[mb]), ps_h(BC[nb]), acc[mb][nb]);                \
        __builtin_amdgcn_sched_barrier(0);                                                     \
    }
#pragma unroll 1
    for (int s = 0; s < 12; s += 4) {
        PS_STEP(s, a0, a1, b0, b3, 1, 1)
        PS_STEP(s + 1, a1, a0, b1, b0, 1, 1)
        PS_STEP(s + 2, a0, a1, b2, b1, 1, 1)
        PS_STEP(s + 3, a1, a0, b3, b2, 1, 1)
    }
    PS_STEP(12, a0, a1, b0, b3, 1, 1)
    PS_STEP(13, a1, a0, b1, b0, 1, 0)
    PS_STEP(14, a0, a1, b2, b1, 1, 0)
    PS_STEP(15, a1, a0, b3, b2, 0, 0)
#undef PS_STEP
}

// counters (optional, tests and timing only): [0] survivors evaluated, [1] (wave, tile) pairs sent to the dense
// fallback, [2] (tile, channel) pairs with at least one survivor
//
// SCHED (the order of independent work, never its arithmetic: every output is bit for bit the same under both).  A SIMD holds
// waves w and w + 4 of the one work-group.  Under SCHED 0 all eight waves run screen -> select / finish -> h2_save copy between
// the barrier after the layer-2 epilogue and the barrier at the top of the next tile, so SIMD partners reach their MFMA stream
// together and their VALU / LDS / VMEM stretches together.  Under SCHED 1 waves 4-7 run the copy FIRST: it issues under the
// partner's MFMA stream, and the partner's finish and copy issue under theirs.  Measured on MI355X this is no gain (the copy
// is 0.09 ms of a 3.5 ms launch: too short an offset; VALU / MFMA co-execution cycles rose by a quarter, the launch got
// 0.5 - 2 % longer, the all-fallback batch 2.5 %), so PS_SCHED_DEFAULT is 0 and SCHED 1 stays selectable for the next attempt
// at a longer offset.  The copy reads H (the fp32 H2 tile), which is
// complete at the barrier after the epilogue and is next written by layer 1 after the barrier at the top of the next tile;
// the screen reads only the planes and the finish only H, skey and registers, so the three may run in any order between
// those two barriers.  The branch is wave-uniform and holds no barrier: every wave executes four __syncthreads() per tile
// on every path (survivor or fallback, last tile or not, P == 64), plus the one before the kernel's epilogue.
template <int SCHED>
__device__ __forceinline__ bool ps_late_wave(int wave) { return SCHED == 1 && __builtin_amdgcn_readfirstlane(wave) >= 4; }

// training forward: the H2 tile (intact in LDS between the two barriers named above) also goes to HBM, as in pn_fwd_kernel
template <int NT>
__device__ __forceinline__ void ps_copy_h2(const float* __restrict__ H, float* __restrict__ dst, int tid) {
#pragma unroll 2
    for (int i = 0; i < PN_TM * PN_C2 / 4 / NT; ++i) {
        const int q = tid + NT * i, row = q >> 6, c4 = q & 63;
        const f32x4 v = *(const f32x4*)(H + row * PN_LD2 + 4 * c4);
        *(f32x4*)(dst + row * PN_C2 + 4 * c4) = v;
    }
}

// The next tile's points, one value per thread (PN_TM * PN_MAXC slots = PS_NW * 64 threads): the load is issued a tile ahead,
// right after the loop-top barrier, and waited for only where stage_points used to load it -- behind layer 1, the layer-2 MFMAs
// and their epilogue.  x is read once per rollout and every tile's lines are cold: the load is a full HBM miss.
static_assert(PN_TM * PN_MAXC == PS_NW * 64, "one staged slot per thread");
__device__ __forceinline__ float ps_point_load(const float* __restrict__ xb, int tile, int C, int tid) {
    const int p = tid >> 3, d = tid & 7;
    return d < C ? xb[(tile * PN_TM + p) * C + d] : 0.f;                  // slots d >= C stay zero, as in stage_points
}
__device__ __forceinline__ void ps_point_store(float v, int sub_mean, const float (&cen)[3], int tid, float* __restrict__ Xs) {
    const int d = tid & 7;
    if (sub_mean && d < 3) v -= cen[d];
    Xs[tid] = v;
}

// Lane-crossing moves of the select pass and the finish, on the VALU's DPP controls: no LDS round trip (a __shfl is a
// ds_bpermute_b32 and a full wait for it).  Every lane of the wave is active where these are called.
#define PS_DPP(old, src, ctrl, rows, banks) __builtin_amdgcn_update_dpp((old), (src), (ctrl), (rows), (banks), false)

// u = s + s[lane ^ 4];  t = u + u[lane ^ 2];  t + t[lane ^ 1]: the finish's addition tree over a group of eight lanes.
__device__ __forceinline__ float ps_sum8(float s) {
    const int si = __float_as_int(s);
    int t = PS_DPP(si, si, 0x114, 0xf, 0xa);             // row_shr:4 into banks 1 and 3: lanes 4-7 and 12-15 of a row take lane - 4
    t = PS_DPP(t, si, 0x104, 0xf, 0x5);                  // row_shl:4 into banks 0 and 2: lanes 0-3 and 8-11 take lane + 4
    s += __int_as_float(t);
    s += __int_as_float(PS_DPP(0, __float_as_int(s), 0x4e, 0xf, 0xf));       // quad_perm [2,3,0,1]: lane ^ 2
    s += __int_as_float(PS_DPP(0, __float_as_int(s), 0xb1, 0xf, 0xf));       // quad_perm [1,0,3,2]: lane ^ 1
    return s;
}

// Inclusive prefix sum over the wave's 64 lanes: row_shr 1 / 2 / 4 / 8 inside each row of 16 (a lane without a source in its
// row keeps the 0), then the row totals: row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3.
__device__ __forceinline__ int ps_prefix64(int v) {
    v += PS_DPP(0, v, 0x111, 0xf, 0xf);
    v += PS_DPP(0, v, 0x112, 0xf, 0xf);
    v += PS_DPP(0, v, 0x114, 0xf, 0xf);
    v += PS_DPP(0, v, 0x118, 0xf, 0xf);
    v += PS_DPP(0, v, 0x142, 0xa, 0xf);
    v += PS_DPP(0, v, 0x143, 0xc, 0xf);
    return v;
}

// The running maximum of a channel and its point, as ONE 64-bit integer that max() orders like the rule
// v > vmax || (v == vmax && p < imax).  High word: the order-preserving image of the fp32 value (all bits flipped if the sign
// is set, the sign bit flipped otherwise).  Low word: ((2^31 - 1 - p) << 1) | 1, so the lower point wins among equal values.
// Signed zero: the rule takes +0 and -0 as equal and keeps the lower point WITH ITS SIGN, while the image puts -0 below +0,
// and the finish can return either: its value is b3 itself where the eight-lane sum is zero (a zero row; or products that
// all underflow) and sum + b3 otherwise, so it is -0 exactly where b3 is -0 and the sum is zero, and +0 where b3 is +0 and the
// sum is zero or where a non-zero sum cancels b3: points of one channel with zeros of both signs need different b3 and so
// cannot meet, but the fallback's values of the same channel (an MFMA chain from b3) can carry the other sign.  So
// zero gets its own handling: -0 takes the image of +0 and clears bit 0 of the low word, which cannot change the order (equal
// p is the same point, the same value) and gives the sign back on decoding.  NaN is never offered (the rule never takes it).
// The dense fallback's values (an MFMA chain that starts from b3) go through the same slot, signed zeros included.
#define PS_BEST_INIT 0x007fffffffffffffull                                   // (-inf, point 0): what vmax = -inf, imax = 0 was
__device__ __forceinline__ unsigned long long ps_best_pack(float v, int p) {
    const unsigned u = __float_as_uint(v);
    const bool nz = u == 0x80000000u;
    const unsigned hi = nz ? 0x80000000u : u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
    const unsigned lo = ((0x7fffffffu - (unsigned)p) << 1) | (nz ? 0u : 1u);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ float ps_best_value(unsigned hi, unsigned lo) {   // lo = 1: a zero comes back as +0 (the select pass)
    const unsigned u = (hi & 0x80000000u) ? hi ^ 0x80000000u : ~hi;
    return __uint_as_float((lo & 1u) ? u : 0x80000000u);
}
__device__ __forceinline__ int ps_best_point(unsigned lo) { return (int)(0x7fffffffu - (lo >> 1)); }
__device__ __forceinline__ void ps_best_max(unsigned long long* slot, float v, int p) {      // ds_max_u64, no return value
    __hip_atomic_fetch_max(slot, ps_best_pack(v, p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

#ifdef PS_PROFILE   // A/B builds only (tools/ps_profile.py): cycle-counter stamps of work-groups 0-3 (one cloud each), tiles 0-15, every wave
__device__ unsigned long long ps_prof[4 * 16 * PS_NW * 16];
extern "C" int pm_debug_ps_prof_read(void* dst) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(ps_prof), sizeof(ps_prof)) == hipSuccess ? 0 : 1;
}
#define PS_STAMP(i)                                                                                         \
    if (b < 4 && tile < 16 && lane0 == 0) ps_prof[((b * 16 + tile) * PS_NW + wave) * 16 + (i)] = __builtin_readcyclecounter()
#else
#define PS_STAMP(i)
#endif

template <int CT, int SCHED>
__global__ __launch_bounds__(PS_NW * 64, 2) void pn_fwd_screen_kernel(
    const float* __restrict__ x, long ldx, int P, int C, int sub_mean, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ b2, const float* __restrict__ b3,
    const float* __restrict__ packed, const unsigned char* __restrict__ packed_s, int max_mean, float* __restrict__ feat,
    long ldf, int32_t* __restrict__ argmax, float* __restrict__ h2_save, unsigned long long* __restrict__ counters) {
    constexpr int NT = PS_NW * 64;
    __shared__ __attribute__((aligned(16))) float H[PN_TM * PN_LD2];                  // H1 [64][132], then H2 [64][260]
    __shared__ __attribute__((aligned(16))) unsigned short Hh[PN_TM * PS_LDP];        // fp16 plane of H2
    __shared__ __attribute__((aligned(16))) float Xs[PN_TM * PN_MAXC];
    __shared__ double red[16];
    __shared__ double cs[PN_C2];                                                      // column sums of h2 over the cloud
    __shared__ int skey[PS_NW][PS_CAP];                                               // survivors: (row << 6) | channel in wave
    __shared__ unsigned long long best[PS_NW][64];                                    // running (maximum, point) of channel 64 wave + l: ps_best_pack

    const int b = blockIdx.x, tid = threadIdx.x, lane0 = tid & 63, wave = tid >> 6;
    const float* xb = x + (long)b * ldx;
    const float4* P2v = (const float4*)(packed + PN_P2_OFF);
    const float4* P3v = (const float4*)(packed + PN_P3_OFF);
    const uint4* S3 = (const uint4*)(packed_s + PS_OFF_P3);
    const float* W3r = (const float*)(packed_s + PS_OFF_W3);
    const float* epsg = (const float*)(packed_s + PS_OFF_EPS);
    const float* invg = (const float*)(packed_s + PS_OFF_INV);

    float cen[3] = {0.f, 0.f, 0.f};
    if (sub_mean) cloud_centroid<NT>(xb, P, C, red, cen);

    float pois = 0.f;                        // lane l: channel 64 wave + l.  pois: sum of the non-finite exact values seen
    best[wave][lane0] = PS_BEST_INIT;        // only wave `wave` ever touches best[wave] before the epilogue: no barrier is needed for it
    double csum = 0.0;                       // lanes < 32: column 32 wave + lane of h2

    // Per-lane constants of the tile loop, loaded once per cloud (they depend on the lane and the wave only; the addresses
    // are those the loop used to recompute from the laundered lane id): 7 VGPRs, + 5 for the W1 row and b1 when C is 3 or 4.
    const int li0 = lane0 & 31;
    const float b2r = b2[wave * 32 + li0];
    const float b3r[2] = {b3[(wave * 2 + 0) * 32 + li0], b3[(wave * 2 + 1) * 32 + li0]};
    const float epsr[2] = {epsg[(wave * 2 + 0) * 32 + li0], epsg[(wave * 2 + 1) * 32 + li0]};
    const float invr[2] = {invg[(wave * 2 + 0) * 32 + li0], invg[(wave * 2 + 1) * 32 + li0]};      // 2^-s_c
    float w1r[4] = {0.f, 0.f, 0.f, 0.f}, b1r = 0.f;
    if constexpr (CT == 3 || CT == 4) layer1_row<CT>(W1, b1, w1r, b1r);

    const int ntiles = P / PN_TM;
    stage_points<PN_TM, NT>(xb, 0, C, sub_mean, cen, Xs);
    for (int tile = 0; tile < ntiles; ++tile) {
        int lane = lane0;                    // laundered per tile: see pn_fwd_kernel
        asm volatile("" : "+v"(lane));
        const int li = lane & 31, lh = lane >> 5;
        PS_STAMP(0);
        __syncthreads();                     // Xs staged; the previous tile's reads of H and the planes are done
        float xnext = 0.f;                   // tile + 1's point coordinate: in flight until the layer-2 epilogue is done
        if (tile + 1 < ntiles) xnext = ps_point_load(xb, tile + 1, C, tid);
        if (!(PS_ABLATE & 1)) {              // ablated: H1 = what the last tile left in H
            if constexpr (CT == 3 || CT == 4) layer1_tile<CT, PN_TM, NT, true>(Xs, w1r, b1r, H);
            else layer1_tile<CT, PN_TM, NT, true>(Xs, W1, b1, C, H);
        }
        PS_STAMP(1);
        __syncthreads();
        {
            f32x16 acc2[2][1];
            zero_acc<2, 1>(acc2);
            if (PS_ABLATE & 2) {             // stand-in that still differs from point to point: 32 words of H1
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc2[mb][0][r] = H[(mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * PN_LD1 + ((wave * 32 + li) & 127)];
            } else {
                layer2_mfma<2, 1>(H, P2v, wave, lane, acc2);
            }
            PS_STAMP(2);
            __syncthreads();                 // every wave has finished reading H1 (and Xs)
            PS_STAMP(3);
            // layer-2 epilogue: layer2_store's arithmetic, plus the fp16 plane and this tile's column sum
            const int col = wave * 32 + li;
            const float b2c = b2r;
            float ts = 0.f;                  // fp32 within the tile, rows in increasing order
            const bool planes = !(PS_ABLATE & 8) || tile == 0;      // ablated: the screen keeps reading tile 0's plane
            // Lanes l and l ^ 1 hold columns col and col ^ 1 of the same rows: they swap one value of every row pair (r, r + 1), so
            // the even lane holds both columns of row r and the odd lane both of row r + 1, and each converts its pair with one
            // v_cvt_pk_f16_f32 (which rounds the two halves as it rounds one) and stores it as one 32-bit word: with a single
            // plane that is one conversion and one ds_write_b32 per lane and row pair, the fewest the accumulator layout allows
            // (a lane holds ONE column; wider stores would need a four-lane exchange of three values for each one stored).
            const bool odd = (lane & 1) != 0;
            unsigned* Hh2 = (unsigned*)(Hh + (odd ? PS_LDP : 0) + (col & ~1));      // 4-byte aligned: PS_LDP and col & ~1 are even
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const float z0 = acc2[mb][0][r] + b2c, z1 = acc2[mb][0][r + 1] + b2c;
                    f32x2 v2;
                    if (PS_ABLATE & 4) {
                        v2.x = z0;
                        v2.y = z1;
                    } else {
                        v2 = pm_tanh2(z0, z1);
                    }
                    const int row0 = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;     // r is even: r + 1 is row0 + 1
                    H[row0 * PN_LD2 + col] = v2.x;
                    H[(row0 + 1) * PN_LD2 + col] = v2.y;
                    ts += v2.x;
                    ts += v2.y;
                    const float own = odd ? v2.y : v2.x, send = odd ? v2.x : v2.y;
                    const float recv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(send), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]: lane ^ 1
                    const float a = odd ? recv : own, c = odd ? own : recv;         // columns col & ~1 and col | 1 of row0 + odd
                    if (planes) Hh2[row0 * (PS_LDP / 2)] = ps_cvt_pk(a, c);         // word index of halfword row0 * PS_LDP
                }
            ts += __shfl_xor(ts, 32, 64);    // the other 32 rows; both halves hold the same sum
            csum += (double)ts;              // fp64 across tiles
            if (tile + 1 < ntiles) ps_point_store(xnext, sub_mean, cen, tid, Xs);
        }
        PS_STAMP(4);
        __syncthreads();                     // H2 and the planes are complete; nothing below writes them before the loop-top barrier
        PS_STAMP(5);

        const bool copy = h2_save && !(PS_ABLATE & 128), late = ps_late_wave<SCHED>(wave);
        float* h2dst = copy ? h2_save + ((long)b * P + (long)tile * PN_TM) * PN_C2 : nullptr;
        if (copy && late) ps_copy_h2<NT>(H, h2dst, tid);     // waves 4-7, SCHED 1: under the SIMD partner's screen MFMAs

        // ---- screen: z~ for 64 points x this wave's 64 channels ---------------------------------------------
        f32x16 acc[2][2];
        if (PS_ABLATE & 16) {                // stand-in that still differs from point to point: b3 + 64 words of H2
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[mb][nb][r] = b3r[nb] + H[(mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * PN_LD2 + ((wave * 64 + nb * 32 + li) & 255)];
        } else {
            zero_acc<2, 2>(acc);
            ps_stream(Hh + li * PS_LDP + lh * 8, S3 + (size_t)(wave * 2 * 16) * 64 + lane, acc);
        }
        PS_STAMP(6);

        unsigned msk[2];
        float tmax[2];                       // PS_ABLATE & 64 only
        // the running maxima of this lane's two channels: last written by this wave's finish of the tile before, two barriers ago
        const unsigned bhi[2] = {(unsigned)(best[wave][li] >> 32), (unsigned)(best[wave][32 + li] >> 32)};
#if (PS_ABLATE & 32) && defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {     // timing probe: the screen's results stay live without the compare / scan pass
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) asm volatile("" ::"v"(acc[mb][nb]));
            msk[nb] = 0;
            tmax[nb] = 0.f;
        }
#else
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            float m = -INFINITY;
            const float iv = invr[nb], b3c = b3r[nb];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!(PS_ABLATE & 16)) acc[mb][nb][r] = fmaf(acc[mb][nb][r], iv, b3c);      // z~: un-scaled, one rounding (in eps)
                    m = fmaxf(m, acc[mb][nb][r]);
                }
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            const float e = epsr[nb];
            const float vm = ps_best_value(bhi[nb], 1u);
            const float thr = m - 2.f * e;
            unsigned k = 0;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float z = acc[mb][nb][r];
                    const bool s = !(z < thr) && !(z + e <= vm);
                    k |= (s ? 1u : 0u) << (mb * 16 + r);
                }
            msk[nb] = k;
            tmax[nb] = m;
        }
#endif
        const int n = __popc(msk[0]) + __popc(msk[1]);
        const int incl = ps_prefix64(n);
        const int total = __builtin_amdgcn_readlane(incl, 63);
        PS_STAMP(7);

        if (PS_ABLATE & 64) {
            // no finish: the running maximum follows the tile maxima of z~ instead, so that the second test keeps pruning
            const float tm = lh ? tmax[1] : tmax[0];
            if (tm == tm) ps_best_max(&best[wave][lane], tm, 0);
            if (counters && lane == 0) atomicAdd(counters + 0, (unsigned long long)total);
        } else if (total <= PS_CAP) {
            // ---- survivors -> list -> exact fp32 values -> running maximum ------------------------------------
            int off = incl - n;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                unsigned m = msk[nb];
                while (m) {
                    const int bit = __ffs(m) - 1;
                    m &= m - 1;
                    const int row = (bit >> 4) * 32 + (bit & 3) + 8 * ((bit & 15) >> 2) + 4 * lh;
                    skey[wave][off++] = (row << 6) | (nb * 32 + li);
                }
            }
            __builtin_amdgcn_wave_barrier();
            const int j = lane & 7, g = lane >> 3;
            for (int e0 = 0; e0 < total; e0 += 8) {
                const int e = e0 + g;
                const int key = (e < total) ? skey[wave][e] : 0;
                const int row = key >> 6, cl = key & 63;
                const float* hp = H + row * PN_LD2 + 4 * j;
                const float* wp = W3r + (size_t)(wave * 64 + cl) * PN_C2 + 4 * j;
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float4 w = *(const float4*)(wp + 32 * i);
                    const float4 h = *(const float4*)(hp + 32 * i);
                    s = fmaf(w.x, h.x, s);
                    s = fmaf(w.y, h.y, s);
                    s = fmaf(w.z, h.z, s);
                    s = fmaf(w.w, h.w, s);
                }
                s = ps_sum8(s);
                const float b3s = b3[wave * 64 + cl];
                s = s == 0.f ? b3s : s + b3s;                 // a zero sum of either sign: the bias itself (header)
                // All eight lanes of a group hold the same s (the butterfly's adds commute); its first lane offers (s, point) to
                // the channel's slot.  Two survivors of one channel in one pass meet in the atomic; max() does not depend on order.
                const bool live = e < total;
                if (live && j == 0 && s == s) ps_best_max(&best[wave][cl], s, tile * PN_TM + row);
                // pois sums a channel's non-finite values in list order, in its owner lane: a pass that holds one (rare) hands
                // its values over through scalar registers, as every pass used to.
                if (__any(live && !(fabsf(s) < INFINITY))) {
#pragma unroll
                    for (int gg = 0; gg < 8; ++gg)
                        if (e0 + gg < total) {                // wave-uniform
                            const int kk = __builtin_amdgcn_readlane(key, gg * 8);
                            const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), gg * 8));
                            if ((kk & 63) == lane && !(fabsf(v) < INFINITY)) pois += v;
                        }
                }
            }
            if (counters) {
                const unsigned long long h0 = __ballot(msk[0] != 0), h1 = __ballot(msk[1] != 0);
                if (lane == 0) {
                    atomicAdd(counters + 0, (unsigned long long)total);
                    atomicAdd(counters + 2, (unsigned long long)(__popc((unsigned)(h0 | (h0 >> 32))) + __popc((unsigned)(h1 | (h1 >> 32)))));
                }
            }
        } else {
            // ---- too many survivors: the dense fp32 layer 3 of pn_fwd_kernel for this wave and tile ----------
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const float b3c = b3r[nb];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][nb][r] = acc[1][nb][r] = b3c;
            }
            mfma_stream<2, 2, 32>(H + li * PN_LD2 + lh * 128, PN_LD2, P3v + (size_t)(wave * 2) * 32 * 64 + lane, acc);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                float bv = -INFINITY, ps = 0.f;
                int bp = 0;
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {            // increasing point order: strict > keeps the lowest index
                        const float v = acc[mb][nb][r];
                        if (!(fabsf(v) < INFINITY)) ps += v;
                        if (v > bv) {
                            bv = v;
                            bp = tile * PN_TM + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        }
                    }
                const float ov = __shfl_xor(bv, 32, 64), os = __shfl_xor(ps, 32, 64);
                const int op = __shfl_xor(bp, 32, 64);
                if (ov > bv || (ov == bv && op < bp)) {
                    bv = ov;
                    bp = op;
                }
                if (lh == nb) {                               // the lane that owns channel 64 wave + 32 nb + li
                    pois += ps + os;
                    ps_best_max(&best[wave][lane], bv, bp);   // bv is never NaN: it starts at -inf and only v > bv replaces it
                }
            }
            if (counters && lane == 0) atomicAdd(counters + 1, 1ull);
        }
        PS_STAMP(8);
        if (copy && !late) ps_copy_h2<NT>(H, h2dst, tid);    // SCHED 1, waves 0-3: under the SIMD partner's screen MFMAs
        PS_STAMP(9);
    }
    // ---- epilogue: thread tid owns channel tid --------------------------------------------------------------
    if ((lane0 >> 5) == 0) cs[wave * 32 + lane0] = csum;
    __syncthreads();
    const int ch = tid;
    // A non-finite layer-3 value always survives the screen (its z~ is NaN or infinite), so pois is the sum of ALL of this
    // channel's non-finite values: NaN exactly when the dense kernel's column sum is (a NaN, or infinities of both signs),
    // which is when that kernel, like torch.max on a NaN, returns NaN.
    const unsigned long long bq = best[ch >> 6][ch & 63];
    float v = ps_best_value((unsigned)(bq >> 32), (unsigned)bq);
    const int imax = ps_best_point((unsigned)bq);
    if (pois != pois) v = pois;
    feat[(long)b * ldf + ch] = v;
    argmax[(long)b * PN_C3 + ch] = imax;
    if (max_mean) {
        // mean_p z3[p] = W3 (sum_p h2[p]) / P + b3 in fp64 (k increasing), rounded to fp32 once
        const float* wr = W3r + (size_t)ch * PN_C2;
        double s = 0.0;
#pragma unroll 4
        for (int k = 0; k < PN_C2; k += 4) {
            const float4 w = *(const float4*)(wr + k);
            s = fma((double)w.x, cs[k], s);
            s = fma((double)w.y, cs[k + 1], s);
            s = fma((double)w.z, cs[k + 2], s);
            s = fma((double)w.w, cs[k + 3], s);
        }
        float mv = (float)(s / (double)P + (double)b3[ch]);
        if (pois != pois) mv = pois;
        feat[(long)b * ldf + PN_C3 + ch] = mv;
    }
}

extern "C" int pm_pointnet_enc_fwd_screen_sched_f32(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                                                    const float* b1, const float* b2, const float* b3, const float* packed,
                                                    const void* packed_screen, int max_mean, float* feat, long ldf,
                                                    int32_t* argmax, float* h2_save, unsigned long long* counters, int schedule,
                                                    void* stream) {
    PM_REQUIRE(x && W1 && b1 && b2 && b3 && packed && packed_screen && feat && argmax);
    PM_REQUIRE(schedule == 0 || schedule == 1);
    if (h2_save && ((uintptr_t)h2_save & 15) != 0) return PM_EALIGN;
    PM_REQUIRE(B > 0 && P > 0 && P % PN_TM == 0 && C >= 1 && C <= PN_MAXC && ldx >= (long)P * C);
    PM_REQUIRE(ldf >= PN_C3 * (max_mean ? 2 : 1));
    PM_REQUIRE(!sub_mean || C >= 3);
    if (((uintptr_t)packed & 15) != 0 || ((uintptr_t)packed_screen & 15) != 0 || ((uintptr_t)counters & 7) != 0) return PM_EALIGN;
#define PS_LAUNCH(CT, S)                                                                                              \
    hipLaunchKernelGGL((pn_fwd_screen_kernel<CT, S>), dim3(B), dim3(PS_NW * 64), 0, pm_stream(stream), x, ldx, P, C, sub_mean, \
                       W1, b1, b2, b3, packed, (const unsigned char*)packed_screen, max_mean, feat, ldf, argmax, h2_save,   \
                       counters)
    if (schedule == 0) {
        if (C == 3) PS_LAUNCH(3, 0);
        else if (C == 4) PS_LAUNCH(4, 0);
        else PS_LAUNCH(0, 0);
    } else {
        if (C == 3) PS_LAUNCH(3, 1);
        else if (C == 4) PS_LAUNCH(4, 1);
        else PS_LAUNCH(0, 1);
    }
#undef PS_LAUNCH
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_pointnet_enc_fwd_screen_f32(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                                              const float* b1, const float* b2, const float* b3, const float* packed,
                                              const void* packed_screen, int max_mean, float* feat, long ldf,
                                              int32_t* argmax, float* h2_save, unsigned long long* counters, void* stream) {
    return pm_pointnet_enc_fwd_screen_sched_f32(x, ldx, B, P, C, sub_mean, W1, b1, b2, b3, packed, packed_screen, max_mean, feat,
                                                ldf, argmax, h2_save, counters, PS_SCHED_DEFAULT, stream);
}
