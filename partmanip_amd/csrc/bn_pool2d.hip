// Batch normalisation, 3x3/2 max pool and global average pool over channels-last activations: what a 2-D residual network needs
// beside its convolutions (`network.name: depthResNet` and `ResNet`; the convolutions are the gathered GEMMs of gemm_f32.hip), the
// stems' patch matrices, and the colour frame's way into an observation row.
//
// Every activation is a matrix (rows = b*H*W, C) with a row stride ld >= C, C % 4 == 0, 16-byte aligned: a lane owns FOUR
// consecutive channels (one 16-byte access) and the lanes of a work-group that share a channel quad walk rows.  All kernels are
// bandwidth-bound.  Determinism: no atomics; every per-channel sum is taken in a fixed order that depends on (rows, C) only --
// rows strided over work-groups and over the row slots of a work-group, row slots combined in LDS in ascending order, work-groups
// combined by the finishing kernel (one wave per channel: lane sums in ascending order, then a fixed butterfly).
//
// Accuracy of the statistics: a depth image holds 100.0 (the far plane) beside values near 1, so E[x^2] - E[x]^2 in fp32 would lose
// the variance.  The sums are taken in fp64 over x - K, K = the channel's first row (a constant channel has variance exactly 0 and
// its mean is exact); the weight-gradient sums of the backward are fp64 as well.
#include "common.h"

#define BP_NT 256
#define BP_MAX_BLOCKS 512

static inline bool bp_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// row slots of a work-group: BP_NT / (C/4) rows are in flight at once (C/4 <= BP_NT)
static inline int bp_rows_per_pass(int C) { return BP_NT / (C / 4); }
static inline int bp_blocks(long rows, int C) {
    const long rpp = bp_rows_per_pass(C);
    const long b = (rows + rpp * 4 - 1) / (rpp * 4);          // >= 4 passes per work-group before another one is worth its partial
    return (int)(b < 1 ? 1 : (b > BP_MAX_BLOCKS ? BP_MAX_BLOCKS : b));
}

__device__ __forceinline__ float4 bp_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void bp_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// The two per-channel totals of the work-groups' partials, by one wave: lane l adds the partials of work-groups l, l + 64, ... in
// ascending order, then the 64 lane sums meet in the fixed butterfly of wave_sum.  Every lane gets the totals.
__device__ __forceinline__ void bp_partial_total(const double* __restrict__ partial, int nblk, int C, int c, int lane, double& s1,
                                                 double& s2) {
    double a = 0.0, b = 0.0;
    for (int k = lane; k < nblk; k += 64) {
        a += partial[(long)k * 2 * C + c];
        b += partial[(long)k * 2 * C + C + c];
    }
    s1 = wave_sum(a);
    s2 = wave_sum(b);
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
// partial[blk][0][c] = sum_r (x[r][c] - K[c]), partial[blk][1][c] = sum_r (x[r][c] - K[c])^2 over the rows of the work-group
__global__ __launch_bounds__(BP_NT) void bn_stats_partial_kernel(const float* __restrict__ x, long ldx, long rows, int C,
                                                                  double* __restrict__ partial) {
    __shared__ double lds[8 * BP_NT];
    const int C4 = C >> 2, nslot = BP_NT / C4;
    const int c4 = threadIdx.x % C4, slot = threadIdx.x / C4;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (slot < nslot) {
        const float4 k = bp_ld4(x + c4 * 4);
        for (long r = (long)blockIdx.x * nslot + slot; r < rows; r += (long)gridDim.x * nslot) {
            const float4 v = bp_ld4(x + r * ldx + c4 * 4);
            const double d0 = (double)v.x - (double)k.x, d1 = (double)v.y - (double)k.y, d2 = (double)v.z - (double)k.z,
                         d3 = (double)v.w - (double)k.w;
            a[0] += d0; a[1] += d1; a[2] += d2; a[3] += d3;
            a[4] += d0 * d0; a[5] += d1 * d1; a[6] += d2 * d2; a[7] += d3 * d3;
        }
    }
    const bool live = slot < nslot;
    // (threads past the last whole slot hold zeros and stay out of the LDS exchange)
    if (live) {
        for (int i = 0; i < 8; ++i) lds[((long)i * nslot + slot) * C4 + c4] = a[i];
    }
    __syncthreads();
    if (live && slot == 0) {
        double* p = partial + (long)blockIdx.x * 2 * C;
        for (int i = 0; i < 8; ++i) {
            double t = 0.0;
            for (int s = 0; s < nslot; ++s) t += lds[((long)i * nslot + s) * C4 + c4];
            p[(i >> 2) * C + c4 * 4 + (i & 3)] = t;
        }
    }
}

// mean, biased variance, invstd; running statistics when asked ((1 - m) running + m batch, unbiased variance n / (n - 1))
__global__ __launch_bounds__(BP_NT) void bn_stats_finish_kernel(const float* __restrict__ x, const double* __restrict__ partial, int nblk,
                                                                 long rows, int C, float eps, float* __restrict__ mean,
                                                                 float* __restrict__ var, float* __restrict__ invstd,
                                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                 long long* __restrict__ num_batches_tracked, float momentum) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * (BP_NT / 64) + (threadIdx.x >> 6);      // one wave per channel
    if (blockIdx.x == 0 && threadIdx.x == 0 && num_batches_tracked) num_batches_tracked[0] += 1;
    if (c >= C) return;
    double s1, s2;
    bp_partial_total(partial, nblk, C, c, lane, s1, s2);
    if (lane != 0) return;
    const double n = (double)rows;
    const double m1 = s1 / n;
    double v = s2 / n - m1 * m1;
    v = v != v ? v : (v < 0.0 ? 0.0 : v);
    const double mu = (double)x[c] + m1;
    const float muf = (float)mu, vf = (float)v;
    mean[c] = muf;
    if (var) var[c] = vf;
    invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
    if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * muf;
    if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)(v * (n / (n - 1.0)));
}

// ---- apply: y = gamma (x - mean) invstd + beta [+ residual] [relu] ------------------------------------------------------------
__device__ __forceinline__ float bp_relu(float v) { return v != v ? v : fmaxf(v, 0.0f); }      // a NaN stays a NaN, as torch.relu

__global__ __launch_bounds__(BP_NT) void bn_apply_kernel(const float* __restrict__ x, long ldx, long rows, int C,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ res, long ldr, int relu, float* __restrict__ y,
                                                          long ldy) {
    const int C4 = C >> 2;
    const long total = rows * C4;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long r = e / C4;
        const int c = (int)(e - r * C4) * 4;
        const float4 v = bp_ld4(x + r * ldx + c), mu = bp_ld4(mean + c), is = bp_ld4(invstd + c), g = bp_ld4(gamma + c),
                     b = bp_ld4(beta + c);
        float4 o;
        o.x = (v.x - mu.x) * (g.x * is.x) + b.x;
        o.y = (v.y - mu.y) * (g.y * is.y) + b.y;
        o.z = (v.z - mu.z) * (g.z * is.z) + b.z;
        o.w = (v.w - mu.w) * (g.w * is.w) + b.w;
        if (res) {
            const float4 q = bp_ld4(res + r * ldr + c);
            o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
        }
        if (relu) { o.x = bp_relu(o.x); o.y = bp_relu(o.y); o.z = bp_relu(o.z); o.w = bp_relu(o.w); }
        bp_st4(y + r * ldy + c, o);
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// dy_m = (dy [+ dy2]) masked by y > 0 when the layer ends in a ReLU
__device__ __forceinline__ float4 bp_masked_dy(const float* dy, long lddy, const float* dy2, long lddy2, const float* y, long ldy,
                                               int relu, long r, int c) {
    float4 d = bp_ld4(dy + r * lddy + c);
    if (dy2) {
        const float4 e = bp_ld4(dy2 + r * lddy2 + c);
        d.x += e.x; d.y += e.y; d.z += e.z; d.w += e.w;
    }
    if (relu) {
        const float4 o = bp_ld4(y + r * ldy + c);
        d.x = o.x > 0.0f ? d.x : 0.0f; d.y = o.y > 0.0f ? d.y : 0.0f; d.z = o.z > 0.0f ? d.z : 0.0f; d.w = o.w > 0.0f ? d.w : 0.0f;
    }
    return d;
}

// partial[blk][0][c] = sum_r dy_m, partial[blk][1][c] = sum_r dy_m * xhat
__global__ __launch_bounds__(BP_NT) void bn_bwd_partial_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ dy2,
                                                                long lddy2, const float* __restrict__ x, long ldx,
                                                                const float* __restrict__ y, long ldy, int relu, long rows, int C,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                double* __restrict__ partial) {
    __shared__ double lds[8 * BP_NT];
    const int C4 = C >> 2, nslot = BP_NT / C4;
    const int c4 = threadIdx.x % C4, slot = threadIdx.x / C4;
    const bool live = slot < nslot;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        const int c = c4 * 4;
        const float4 mu = bp_ld4(mean + c), is = bp_ld4(invstd + c);
        for (long r = (long)blockIdx.x * nslot + slot; r < rows; r += (long)gridDim.x * nslot) {
            const float4 d = bp_masked_dy(dy, lddy, dy2, lddy2, y, ldy, relu, r, c);
            const float4 v = bp_ld4(x + r * ldx + c);
            a[0] += (double)d.x; a[1] += (double)d.y; a[2] += (double)d.z; a[3] += (double)d.w;
            a[4] += (double)d.x * (double)((v.x - mu.x) * is.x);
            a[5] += (double)d.y * (double)((v.y - mu.y) * is.y);
            a[6] += (double)d.z * (double)((v.z - mu.z) * is.z);
            a[7] += (double)d.w * (double)((v.w - mu.w) * is.w);
        }
        for (int i = 0; i < 8; ++i) lds[((long)i * nslot + slot) * C4 + c4] = a[i];
    }
    __syncthreads();
    if (live && slot == 0) {
        double* p = partial + (long)blockIdx.x * 2 * C;
        for (int i = 0; i < 8; ++i) {
            double t = 0.0;
            for (int s = 0; s < nslot; ++s) t += lds[((long)i * nslot + s) * C4 + c4];
            p[(i >> 2) * C + c4 * 4 + (i & 3)] = t;
        }
    }
}

__global__ __launch_bounds__(BP_NT) void bn_bwd_finish_kernel(const double* __restrict__ partial, int nblk, int C,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * (BP_NT / 64) + (threadIdx.x >> 6);      // one wave per channel
    if (c >= C) return;
    double s1, s2;
    bp_partial_total(partial, nblk, C, c, lane, s1, s2);
    if (lane != 0) return;
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
}

// dx = gamma invstd (dy_m - dbeta / n - xhat dgamma / n); dy_m is written too when the residual branch wants it
__global__ __launch_bounds__(BP_NT) void bn_bwd_apply_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ dy2,
                                                              long lddy2, const float* __restrict__ x, long ldx,
                                                              const float* __restrict__ y, long ldy, int relu, long rows, int C,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                              const float* __restrict__ dbeta, float* __restrict__ dx, long lddx,
                                                              float* __restrict__ dym, long lddym) {
    const int C4 = C >> 2;
    const long total = rows * C4;
    const float inv_n = 1.0f / (float)rows;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long r = e / C4;
        const int c = (int)(e - r * C4) * 4;
        const float4 d = bp_masked_dy(dy, lddy, dy2, lddy2, y, ldy, relu, r, c);
        const float4 v = bp_ld4(x + r * ldx + c), mu = bp_ld4(mean + c), is = bp_ld4(invstd + c), g = bp_ld4(gamma + c),
                     dg = bp_ld4(dgamma + c), db = bp_ld4(dbeta + c);
        float4 o;
        o.x = (g.x * is.x) * ((d.x - db.x * inv_n) - ((v.x - mu.x) * is.x) * (dg.x * inv_n));
        o.y = (g.y * is.y) * ((d.y - db.y * inv_n) - ((v.y - mu.y) * is.y) * (dg.y * inv_n));
        o.z = (g.z * is.z) * ((d.z - db.z * inv_n) - ((v.z - mu.z) * is.z) * (dg.z * inv_n));
        o.w = (g.w * is.w) * ((d.w - db.w * inv_n) - ((v.w - mu.w) * is.w) * (dg.w * inv_n));
        bp_st4(dx + r * lddx + c, o);
        if (dym) bp_st4(dym + r * lddym + c, d);
    }
}

// ---- max pool 3x3, stride 2, padding 1 ------------------------------------------------------------------------------------------
// One thread per (output pixel, channel quad).  The winner is the first tap in row-major window order whose value is greater than
// all before it; a NaN replaces whatever stands (so the last NaN of a window wins); the padding is never looked at.  idx = ih*W + iw
// of the winner inside its sample's plane: torch's return_indices.
__global__ __launch_bounds__(BP_NT) void maxpool3s2_fwd_kernel(const float* __restrict__ x, long ldx, int B, int H, int W, int C,
                                                                int Ho, int Wo, float* __restrict__ y, long ldy,
                                                                int32_t* __restrict__ idx) {
    const int C4 = C >> 2;
    const long total = (long)B * Ho * Wo * C4;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long o = e / C4;
        const int c = (int)(e - o * C4) * 4;
        const int ow = (int)(o % Wo), oh = (int)((o / Wo) % Ho), b = (int)(o / ((long)Wo * Ho));
        const int h0 = max(oh * 2 - 1, 0), h1 = min(oh * 2 + 2, H), w0 = max(ow * 2 - 1, 0), w1 = min(ow * 2 + 2, W);
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {h0 * W + w0, h0 * W + w0, h0 * W + w0, h0 * W + w0};
        for (int ih = h0; ih < h1; ++ih) {
            for (int iw = w0; iw < w1; ++iw) {
                const float4 v = bp_ld4(x + ((long)b * H * W + (long)ih * W + iw) * ldx + c);
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (vv[k] > best[k] || vv[k] != vv[k]) { best[k] = vv[k]; bi[k] = ih * W + iw; }
                }
            }
        }
        bp_st4(y + o * ldy + c, make_float4(best[0], best[1], best[2], best[3]));
        *reinterpret_cast<int4*>(idx + o * C + c) = make_int4(bi[0], bi[1], bi[2], bi[3]);
    }
}

// Backward as a gather: input pixel (ih, iw) sums the (at most four) windows that contain it and whose winner it is, in ascending
// window order.  dx is written everywhere (zeros where the pixel won nothing).
__global__ __launch_bounds__(BP_NT) void maxpool3s2_bwd_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ dy2,
                                                                long lddy2, const int32_t* __restrict__ idx, int B, int H, int W, int C,
                                                                int Ho, int Wo, float* __restrict__ dx, long lddx) {
    const int C4 = C >> 2;
    const long total = (long)B * H * W * C4;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long p = e / C4;
        const int c = (int)(e - p * C4) * 4;
        const int iw = (int)(p % W), ih = (int)((p / W) % H), b = (int)(p / ((long)W * H));
        const int me = ih * W + iw;
        // windows oh with 2 oh - 1 <= ih <= 2 oh + 1
        const int oh0 = ih >> 1, oh1 = min((ih + 1) >> 1, Ho - 1), ow0 = iw >> 1, ow1 = min((iw + 1) >> 1, Wo - 1);
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int oh = oh0; oh <= oh1; ++oh) {
            for (int ow = ow0; ow <= ow1; ++ow) {
                const long o = ((long)b * Ho + oh) * Wo + ow;
                const int4 w = *reinterpret_cast<const int4*>(idx + o * C + c);
                float4 d = bp_ld4(dy + o * lddy + c);
                if (dy2) {
                    const float4 q = bp_ld4(dy2 + o * lddy2 + c);
                    d.x += q.x; d.y += q.y; d.z += q.z; d.w += q.w;
                }
                s.x += w.x == me ? d.x : 0.0f;
                s.y += w.y == me ? d.y : 0.0f;
                s.z += w.z == me ? d.z : 0.0f;
                s.w += w.w == me ? d.w : 0.0f;
            }
        }
        bp_st4(dx + p * lddx + c, s);
    }
}

// ---- global average pool: y[b][c] = mean over the HW rows of sample b (ascending order); y's rows may have any stride ---------------
__global__ __launch_bounds__(BP_NT) void avgpool_fwd_kernel(const float* __restrict__ x, long ldx, int B, int HW, int C,
                                                             float* __restrict__ y, long ldy) {
    const int C4 = C >> 2;
    const float n = (float)HW;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < (long)B * C4; e += (long)gridDim.x * BP_NT) {
        const long b = e / C4;
        const int c = (int)(e - b * C4) * 4;
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int r = 0; r < HW; ++r) {
            const float4 v = bp_ld4(x + (b * HW + r) * ldx + c);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        float* o = y + b * ldy + c;
        o[0] = s.x / n; o[1] = s.y / n; o[2] = s.z / n; o[3] = s.w / n;
    }
}

__global__ __launch_bounds__(BP_NT) void avgpool_bwd_kernel(const float* __restrict__ dy, long lddy, int B, int HW, int C,
                                                             float* __restrict__ dx, long lddx) {
    const int C4 = C >> 2;
    const long total = (long)B * HW * C4;
    const float n = (float)HW;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long r = e / C4;
        const int c = (int)(e - r * C4) * 4;
        const float* d = dy + (r / HW) * lddy + c;
        bp_st4(dx + r * lddx + c, make_float4(d[0] / n, d[1] / n, d[2] / n, d[3] / n));
    }
}

// ---- patch matrix of a single-channel image (the stem: K = k*k is no multiple of 4, so it cannot be a gathered GEMM operand) -------
// dst[(b, oh, ow)][kh*k + kw] = x[b][oh*stride - pad + kh][ow*stride - pad + kw] (0 in the padding); columns k*k .. ldd-1 are zeros
__global__ __launch_bounds__(BP_NT) void im2col2d_c1_kernel(const float* __restrict__ x, long ldx, int B, int H, int W, int k, int stride,
                                                             int pad, int Ho, int Wo, float* __restrict__ dst, int ldd) {
    const long total = (long)B * Ho * Wo * ldd;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long o = e / ldd;
        const int j = (int)(e - o * ldd);
        float v = 0.0f;
        if (j < k * k) {
            const int ow = (int)(o % Wo), oh = (int)((o / Wo) % Ho), b = (int)(o / ((long)Wo * Ho));
            const int ih = oh * stride - pad + j / k, iw = ow * stride - pad + j % k;
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = x[(long)b * ldx + (long)ih * W + iw];
        }
        dst[e] = v;
    }
}

// ---- patch matrix of a C-channel planar image (the RGB stem: K = 3*7*7 = 147) ------------------------------------------------------
// dst[(b, oh, ow)][c*k*k + kh*k + kw] = x[b][c][oh*stride - pad + kh][ow*stride - pad + kw] (0 in the padding); columns C*k*k .. ldd-1
// are zeros.  The column order (c, kh, kw) is that of conv.weight.view(Cout, C*k*k): the weight and its gradient are used as they lie.
// One thread per (patch row, c, kh), as conv3d.hip's im2col3d_kernel: it decodes its indices once and copies the k taps along w
// (contiguous in the image and in the patch row); one extra group per row zero-fills the pad columns.  ldd: the Linear kernels take
// their fast path with whole K-steps of 32 (G2_TK, gemm2_f32.hip), so the caller rounds 147 up to 160 (the depth stem's 49 to 64).
__global__ __launch_bounds__(BP_NT) void im2col2d_kernel(const float* __restrict__ x, long ldx, int C, int H, int W, int k, int stride,
                                                          int pad, int Ho, int Wo, long total, float* __restrict__ dst, int ldd) {
    const int kk = k * k, ncol = C * kk, gpr = C * k + 1;                                       // groups per row
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long row = e / gpr;
        const int grp = (int)(e - row * gpr);
        float* d = dst + row * ldd;
        if (grp == C * k) {
            for (int col = ncol; col < ldd; ++col) d[col] = 0.0f;
            continue;
        }
        const int c = grp / k, kh = grp - c * k;
        const int ow = (int)(row % Wo), oh = (int)((row / Wo) % Ho);
        const long b = row / ((long)Wo * Ho);
        const int ih = oh * stride - pad + kh, w0 = ow * stride - pad;
        const bool ok = ih >= 0 && ih < H;
        const float* src = x + b * ldx + ((long)c * H + (ok ? ih : 0)) * W;
        d += c * kk + kh * k;
        for (int kw = 0; kw < k; ++kw) {
            const int iw = w0 + kw;
            d[kw] = (ok && iw >= 0 && iw < W) ? src[iw] : 0.0f;
        }
    }
}

// ---- colour frame -> observation rows (the `rgb_img` mode: hand_base.py:344-353 puts camera v's image, permuted to (3, h, w), raw
// 0..255, at the head of the row) -----------------------------------------------------------------------------------------------------
// out[b*ldo + c*h*w + p] = (float) rgb[b][v][p][c], p = y*w + x; columns >= 3*h*w of a row are not touched.  Pure data movement.
// Vector path: one thread converts four consecutive pixels -- three aligned dwords in (12 bytes = R0 G0 B0 R1 | G1 B1 R2 G2 |
// B2 R3 G3 B3), one 16-byte store to each of the three planes.  It needs h*w % 4 == 0 (then every image starts on a dword and every
// plane on 16 bytes), ldo % 4 == 0 and 16-byte aligned bases; the host picks the scalar kernel otherwise.
__global__ __launch_bounds__(BP_NT) void rgb_planes_vec4_kernel(const uint8_t* __restrict__ rgb, int B, int V, int hw, int v,
                                                                 float* __restrict__ out, long ldo) {
    const int q4 = hw >> 2;
    const long total = (long)B * q4;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long b = e / q4;
        const int p = (int)(e - b * q4) * 4;
        const uint32_t* s = reinterpret_cast<const uint32_t*>(rgb + ((b * V + v) * hw + p) * 3);
        const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
        float* o = out + b * ldo + p;
        bp_st4(o, make_float4((float)(d0 & 255u), (float)(d0 >> 24), (float)((d1 >> 16) & 255u), (float)((d2 >> 8) & 255u)));
        bp_st4(o + hw, make_float4((float)((d0 >> 8) & 255u), (float)(d1 & 255u), (float)(d1 >> 24), (float)((d2 >> 16) & 255u)));
        bp_st4(o + 2 * (long)hw, make_float4((float)((d0 >> 16) & 255u), (float)((d1 >> 8) & 255u), (float)(d2 & 255u), (float)(d2 >> 24)));
    }
}

// the same definition, one thread per pixel: any h*w, any row stride, any alignment
__global__ __launch_bounds__(BP_NT) void rgb_planes_scalar_kernel(const uint8_t* __restrict__ rgb, int B, int V, int hw, int v,
                                                                   float* __restrict__ out, long ldo) {
    const long total = (long)B * hw;
    for (long e = (long)blockIdx.x * BP_NT + threadIdx.x; e < total; e += (long)gridDim.x * BP_NT) {
        const long b = e / hw;
        const int p = (int)(e - b * hw);
        const uint8_t* s = rgb + ((b * V + v) * hw + p) * 3;
        float* o = out + b * ldo + p;
        o[0] = (float)s[0];
        o[hw] = (float)s[1];
        o[2 * (long)hw] = (float)s[2];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static inline unsigned bp_grid(long total) {
    const long g = (total + BP_NT - 1) / BP_NT;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
static inline bool bp_shape_ok(long rows, int C) { return rows > 0 && rows < 0x7fffffffL && C > 0 && C % 4 == 0 && C / 4 <= BP_NT; }

extern "C" size_t pm_bn2d_workspace_bytes(long rows, int C) {
    if (!bp_shape_ok(rows, C)) return 0;
    return (size_t)bp_blocks(rows, C) * 2 * C * sizeof(double);
}

extern "C" int pm_bn2d_stats_f32(const float* x, long ldx, long rows, int C, float eps, float* mean, float* var, float* invstd,
                                 float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    PM_REQUIRE(x && mean && invstd && bp_shape_ok(rows, C) && ldx >= C && eps >= 0.0f);
    PM_REQUIRE(rows >= 2);                                  // torch: "Expected more than 1 value per channel when training"
    if (!bp_aligned16(x) || ldx % 4 != 0) return PM_EALIGN;
    if (!workspace || workspace_bytes < pm_bn2d_workspace_bytes(rows, C)) return PM_EWORKSPACE;
    if ((((uintptr_t)workspace) & 7) != 0) return PM_EALIGN;
    const int nblk = bp_blocks(rows, C);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(nblk), dim3(BP_NT), 0, pm_stream(stream), x, ldx, rows, C, (double*)workspace);
    PM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + BP_NT / 64 - 1) / (BP_NT / 64)), dim3(BP_NT), 0, pm_stream(stream), x,
                       (const double*)workspace, nblk, rows, C, eps, mean, var, invstd, running_mean, running_var,
                       (long long*)num_batches_tracked, momentum);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

__global__ __launch_bounds__(BP_NT) void bn_invstd_kernel(const float* __restrict__ var, int C, float eps, float* __restrict__ invstd) {
    const int c = blockIdx.x * BP_NT + threadIdx.x;
    if (c < C) invstd[c] = (float)(1.0 / sqrt((double)var[c] + (double)eps));
}

extern "C" int pm_bn2d_invstd_f32(const float* var, int C, float eps, float* invstd, void* stream) {
    PM_REQUIRE(var && invstd && C > 0 && eps >= 0.0f);
    hipLaunchKernelGGL(bn_invstd_kernel, dim3((C + BP_NT - 1) / BP_NT), dim3(BP_NT), 0, pm_stream(stream), var, C, eps, invstd);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_bn2d_apply_f32(const float* x, long ldx, long rows, int C, const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, const float* residual, long ldr, int relu, float* y, long ldy, void* stream) {
    PM_REQUIRE(x && mean && invstd && gamma && beta && y && bp_shape_ok(rows, C) && ldx >= C && ldy >= C && (!residual || ldr >= C));
    if (!bp_aligned16(x) || !bp_aligned16(y) || !bp_aligned16(mean) || !bp_aligned16(invstd) || !bp_aligned16(gamma) ||
        !bp_aligned16(beta) || !bp_aligned16(residual) || ldx % 4 != 0 || ldy % 4 != 0 || (residual && ldr % 4 != 0))
        return PM_EALIGN;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(bp_grid(rows * (C / 4))), dim3(BP_NT), 0, pm_stream(stream), x, ldx, rows, C, mean, invstd,
                       gamma, beta, residual, ldr, relu, y, ldy);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_bn2d_bwd_f32(const float* dy, long lddy, const float* dy2, long lddy2, const float* x, long ldx, const float* y,
                               long ldy, int relu, long rows, int C, const float* mean, const float* invstd, const float* gamma,
                               float* dgamma, float* dbeta, float* dx, long lddx, float* dy_masked, long lddym, void* workspace,
                               size_t workspace_bytes, void* stream) {
    PM_REQUIRE(dy && x && mean && invstd && gamma && dgamma && dbeta && dx && bp_shape_ok(rows, C) && lddy >= C && ldx >= C &&
               lddx >= C && (!dy2 || lddy2 >= C) && (!relu || (y && ldy >= C)) && (!dy_masked || lddym >= C));
    if (!bp_aligned16(dy) || !bp_aligned16(dy2) || !bp_aligned16(x) || (relu && !bp_aligned16(y)) || !bp_aligned16(mean) ||
        !bp_aligned16(invstd) || !bp_aligned16(gamma) || !bp_aligned16(dgamma) || !bp_aligned16(dbeta) || !bp_aligned16(dx) ||
        !bp_aligned16(dy_masked) || lddy % 4 != 0 || ldx % 4 != 0 || lddx % 4 != 0 || (dy2 && lddy2 % 4 != 0) ||
        (relu && ldy % 4 != 0) || (dy_masked && lddym % 4 != 0))
        return PM_EALIGN;
    if (!workspace || workspace_bytes < pm_bn2d_workspace_bytes(rows, C)) return PM_EWORKSPACE;
    if ((((uintptr_t)workspace) & 7) != 0) return PM_EALIGN;
    const int nblk = bp_blocks(rows, C);
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(nblk), dim3(BP_NT), 0, pm_stream(stream), dy, lddy, dy2, lddy2, x, ldx, y, ldy, relu,
                       rows, C, mean, invstd, (double*)workspace);
    PM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + BP_NT / 64 - 1) / (BP_NT / 64)), dim3(BP_NT), 0, pm_stream(stream), (const double*)workspace,
                       nblk, C, dgamma, dbeta);
    PM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(bp_grid(rows * (C / 4))), dim3(BP_NT), 0, pm_stream(stream), dy, lddy, dy2, lddy2, x, ldx,
                       y, ldy, relu, rows, C, mean, invstd, gamma, (const float*)dgamma, (const float*)dbeta, dx, lddx, dy_masked, lddym);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_pool2d_out(int n) { return n > 0 ? (n - 1) / 2 + 1 : 0; }      // floor((n + 2*1 - 3) / 2) + 1

extern "C" int pm_pool2d_max3s2_fwd_f32(const float* x, long ldx, int B, int H, int W, int C, float* y, long ldy, int32_t* idx,
                                        void* stream) {
    PM_REQUIRE(x && y && idx && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && (long)H * W < 0x7fffffffL);
    if (!bp_aligned16(x) || !bp_aligned16(y) || !bp_aligned16(idx) || ldx % 4 != 0 || ldy % 4 != 0) return PM_EALIGN;
    const int Ho = pm_pool2d_out(H), Wo = pm_pool2d_out(W);
    hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3(bp_grid((long)B * Ho * Wo * (C / 4))), dim3(BP_NT), 0, pm_stream(stream), x, ldx, B, H, W,
                       C, Ho, Wo, y, ldy, idx);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_pool2d_max3s2_bwd_f32(const float* dy, long lddy, const float* dy2, long lddy2, const int32_t* idx, int B, int H, int W,
                                        int C, float* dx, long lddx, void* stream) {
    PM_REQUIRE(dy && idx && dx && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && lddy >= C && lddx >= C && (!dy2 || lddy2 >= C) &&
               (long)H * W < 0x7fffffffL);
    if (!bp_aligned16(dy) || !bp_aligned16(dy2) || !bp_aligned16(dx) || !bp_aligned16(idx) || lddy % 4 != 0 || lddx % 4 != 0 ||
        (dy2 && lddy2 % 4 != 0))
        return PM_EALIGN;
    const int Ho = pm_pool2d_out(H), Wo = pm_pool2d_out(W);
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3(bp_grid((long)B * H * W * (C / 4))), dim3(BP_NT), 0, pm_stream(stream), dy, lddy, dy2,
                       lddy2, idx, B, H, W, C, Ho, Wo, dx, lddx);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_pool2d_avg_fwd_f32(const float* x, long ldx, int B, int HW, int C, float* y, long ldy, void* stream) {
    PM_REQUIRE(x && y && B > 0 && HW > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C);
    if (!bp_aligned16(x) || ldx % 4 != 0) return PM_EALIGN;
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(bp_grid((long)B * (C / 4))), dim3(BP_NT), 0, pm_stream(stream), x, ldx, B, HW, C, y, ldy);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_pool2d_avg_bwd_f32(const float* dy, long lddy, int B, int HW, int C, float* dx, long lddx, void* stream) {
    PM_REQUIRE(dy && dx && B > 0 && HW > 0 && C > 0 && C % 4 == 0 && lddy >= C && lddx >= C);
    if (!bp_aligned16(dx) || lddx % 4 != 0) return PM_EALIGN;
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(bp_grid((long)B * HW * (C / 4))), dim3(BP_NT), 0, pm_stream(stream), dy, lddy, B, HW, C, dx,
                       lddx);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_im2col2d_c1_f32(const float* x, long ldx, int B, int H, int W, int k, int stride, int pad, float* dst, int ldd,
                                  void* stream) {
    PM_REQUIRE(x && dst && B > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0 && ldd >= k * k && ldx >= (long)H * W &&
               H + 2 * pad >= k && W + 2 * pad >= k);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    hipLaunchKernelGGL(im2col2d_c1_kernel, dim3(bp_grid((long)B * Ho * Wo * ldd)), dim3(BP_NT), 0, pm_stream(stream), x, ldx, B, H, W, k,
                       stride, pad, Ho, Wo, dst, ldd);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_im2col2d_f32(const float* x, long ldx, int B, int C, int H, int W, int k, int stride, int pad, float* dst, int ldd,
                               void* stream) {
    PM_REQUIRE(x && dst && B > 0 && C > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0 && H + 2 * pad >= k && W + 2 * pad >= k);
    PM_REQUIRE((long)C * k * k < 0x7fffffffL && ldd >= C * k * k && (long)C * H * W < 0x7fffffffL && ldx >= (long)C * H * W);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const long total = (long)B * Ho * Wo * (C * k + 1);
    hipLaunchKernelGGL(im2col2d_kernel, dim3(bp_grid(total)), dim3(BP_NT), 0, pm_stream(stream), x, ldx, C, H, W, k, stride, pad, Ho, Wo,
                       total, dst, ldd);
    PM_CHECK_LAUNCH();
    return PM_OK;
}

extern "C" int pm_rgb_planes_f32(const uint8_t* rgb, int B, int V, int h, int w, int v, float* out, long ldo, void* stream) {
    PM_REQUIRE(rgb && out && B > 0 && V > 0 && h > 0 && w > 0 && v >= 0 && v < V && (long)h * w < 0x7fffffffL / 3 && ldo >= 3L * h * w);
    const int hw = h * w;
    const bool vec = hw % 4 == 0 && ldo % 4 == 0 && bp_aligned16(rgb) && bp_aligned16(out);
    if (vec)
        hipLaunchKernelGGL(rgb_planes_vec4_kernel, dim3(bp_grid((long)B * (hw / 4))), dim3(BP_NT), 0, pm_stream(stream), rgb, B, V, hw, v,
                           out, ldo);
    else
        hipLaunchKernelGGL(rgb_planes_scalar_kernel, dim3(bp_grid((long)B * hw)), dim3(BP_NT), 0, pm_stream(stream), rgb, B, V, hw, v, out,
                           ldo);
    PM_CHECK_LAUNCH();
    return PM_OK;
}
