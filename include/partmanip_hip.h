/*
 * partmanip_hip.h -- C ABI of libpartmanip_hip.so (MI355X / gfx950 only).
 *
 * The reference (PKU-EPIC/PartManip) is 100 % Python on PyTorch and has no FFI
 * of its own; the boundary it offers is the Python API of
 * algorithms/ppo.py, algorithms/dagger.py and the algorithms/algo_utils package.
 * This header is the NEW native boundary underneath that API: every entry
 * point replaces the ATen work one reference call site dispatches (cited per
 * function as file:line under /root/reference).  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless
 *     the name ends in _host; no torch types; no hidden allocations.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*,
 *     NULL = the null stream), never synchronises, keeps no global state and
 *     is re-entrant.  Scratch memory is supplied by the caller
 *     (pm_*_workspace_bytes tells how much).
 *   - return value: PM_OK (0) or a negative PM_E* code; a HIP launch error is
 *     returned as -(1000 + hipError_t).
 *   - matrices are row-major fp32 with an explicit row stride in ELEMENTS
 *     (ld*), weights use torch.nn.Linear layout (out_features, in_features).
 */
#ifndef PARTMANIP_HIP_H
#define PARTMANIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_OK 0
#define PM_EINVAL (-1)     /* bad argument (null pointer, non-positive size, unsupported shape) */
#define PM_EWORKSPACE (-2) /* workspace too small                                                */
#define PM_EALIGN (-3)     /* pointer / stride not aligned as required                           */
#define PM_EUNSUPPORTED (-4) /* shape has no fused instantiation: use the generic kernels instead  */

#define PM_ACT_NONE 0
#define PM_ACT_TANH 1
/* network.py:7-24 `get_activation`: the other activations a cfg may name (Linear epilogues only: the fused point-cloud /
 * voxel encoders are tanh kernels).  Each derivative is a function of the activation OUTPUT h, which is what the
 * backward kernels are handed: relu 1[h>0]; lrelu (slope 0.01) h>0 ? 1 : 0.01; elu (alpha 1) h>0 ? 1 : h+1;
 * selu h>0 ? lambda : h + lambda*alpha; sigmoid h(1-h). */
#define PM_ACT_RELU 2
#define PM_ACT_LRELU 3
#define PM_ACT_ELU 4
#define PM_ACT_SELU 5
#define PM_ACT_SIGMOID 6
#define PM_ACT_MAX 6

/* ABI version: major*10000 + minor*100 + patch */
#define PM_ABI_VERSION 163 /* bumped whenever a signature changes; additions that change none keep it */
int pm_version(void);      /* returns PM_ABI_VERSION of the built library: loaders compare it with their header */

/* ------------------------------------------------------------------ K1  GAE return scan
 * Replaces RolloutStorage.compute_returns, algorithms/algo_utils/storage.py:96-112.
 * rewards/values/returns/advantages: (T,N) fp32, N contiguous; dones/succs: (T,N) bytes
 * (torch.bool storage); last_values: (N).  gamma_lam = (float)(gamma*lam) computed in
 * double by the caller exactly as Python does.  use_succ==0 reproduces
 * `default_succ_value is None`.  Bit-exact with the reference (no FMA contraction).
 * Algorithmic HBM traffic: 18 B per env-step (8 B r,V + 2 B masks in, 8 B ret,adv out). */
int pm_gae_scan_f32(const float* rewards, const float* values, const uint8_t* dones, const uint8_t* succs,
                    const float* last_values, float* returns, float* advantages, int T, int N, float gamma,
                    float gamma_lam, int use_succ, float succ_value, void* stream);

/* ------------------------------------------------------------------ K2  advantage normalisation
 * storage.py:113-114 (whole batch) and ppo.py:329 (mini-batch): (x-mean)/(std_unbiased+eps).
 * pm_moments_f64 writes {sum, sum of squares} (fp64, deterministic two-stage reduction) to
 * moments[0..1]; data-parallel callers all-reduce those two doubles (and the count) before
 * pm_normalize_apply_f32.  Workspace: pm_moments_workspace_bytes(n). */
size_t pm_moments_workspace_bytes(long n);
int pm_moments_f64(const float* x, long n, double* moments, void* workspace, size_t workspace_bytes, void* stream);
int pm_normalize_apply_f32(float* x, long n, const double* moments, double count, float eps, void* stream);
/* The single-process form in ONE call (the name SURVEY.md 8b lists): x <- (x - mean) / (std_unbiased + eps) over x's n
 * elements = pm_moments_f64 + pm_normalize_apply_f32 with count = n.  Workspace (8-byte aligned): pm_adv_normalize_workspace_bytes. */
size_t pm_adv_normalize_workspace_bytes(long n);
int pm_adv_normalize_f32(float* x, long n, float eps, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ K3  mini-batch gather
 * ppo.py:317-324,361-364 / dagger.py:307-308: dst[i,:] = src[idx[i],:] for `sampler: random`
 * (sequential mini-batches are contiguous slices and need no copy). idx: int64 device. */
int pm_gather_rows_f32(const float* src, const int64_t* idx, float* dst, long n_rows, long row_elems,
                       long src_ld, long dst_ld, void* stream);

/* ------------------------------------------------------------------ K4/K5  Linear layers (fp32 MFMA)
 * network.py:53-54 (MLP) and network.py:154-160,196 (PointNet.final_mlp) forward, and the
 * autograd backward ppo.py:348,378 / dagger.py:318 triggers for them.
 *   fwd : Y[M,N]  = act(X[M,K] * W[N,K]^T + b[N])
 *   bwd_data  : dX[M,K] = (dY[M,N] * W[N,K]) .* act'(H[M,K])   (H = the layer input, i.e. the previous
 *               layer's activation OUTPUT; act' for tanh is 1-H^2, the others as listed at PM_ACT_*; H may be NULL with
 *               PM_ACT_NONE)
 *   bwd_weight: dW[N,K] = dY^T * X ; db[N] = column sums of dY (db may be NULL)
 * v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate. */
int pm_linear_fwd_f32(const float* X, long ldx, const float* W, long ldw, const float* b, float* Y, long ldy,
                      int M, int N, int K, int act, void* stream);
int pm_linear_bwd_data_f32(const float* dY, long lddy, const float* W, long ldw, const float* H, long ldh,
                           float* dX, long lddx, int M, int N, int K, int act, void* stream);
size_t pm_linear_bwd_weight_workspace_bytes(int M, int N, int K);
int pm_linear_bwd_weight_f32(const float* dY, long lddy, const float* X, long ldx, float* dW, long lddw,
                             float* db, int M, int N, int K, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Whole-MLP forms (the names SURVEY.md 8b lists; network.py:27-54 `MLP`: activation after every layer but the last).  dims[0..
 * n_layers] = layer widths; W, b, H, dW, db = HOST arrays of n_layers DEVICE pointers; H[l] (M, dims[l+1]) = output of layer l.
 * They issue the per-layer entry points above in order on `stream` (same kernels, same bits); pm_mlp_bwd_f32 returns dW[l],
 * db[l] (db or db[l] may be NULL) and, when dX != NULL, the input gradient (M, dims[0]).  Workspace 16-byte aligned. */
int pm_mlp_fwd_f32(const float* X, long ldx, int M, int n_layers, const int* dims, const float* const* W, const float* const* b,
                   int act, float* const* H, void* stream);
size_t pm_mlp_bwd_workspace_bytes(int M, int n_layers, const int* dims);
int pm_mlp_bwd_f32(const float* X, long ldx, int M, int n_layers, const int* dims, const float* const* W, const float* const* H,
                   int act, const float* dY, float* const* dW, float* const* db, float* dX, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Grouped forms (new; the reference runs one ATen GEMM per layer per network): up to PM_LINEAR_GROUP_MAX independent
 * problems of the SAME kind in ONE launch.  The small-step regime (state PPO, ppo.py:315-384: 2560 dependent optimiser
 * steps per iteration on 2048 x 512 matrices = one MFMA block per SIMD) is bound by per-launch ramp / drain and by
 * single-wave stalls; the actor's and the critic's layer l are independent (ppo.py:73-74: disjoint parameters), and so
 * are all weight gradients of a backward pass, so they share a grid.  Each desc has exactly the meaning of the
 * corresponding single-problem call.
 * pm_linear_bwd_weight_group_f32 with splits > 1 does NOT reduce: slab z (z = 0..splits-1) of problem i's dW / db is
 * written at dW + z * slab_stride / db + z * slab_stride (the reduction over M is cut into `splits` equal ranges of
 * whole 32-row steps); the caller sums the slabs in fixed order -- pm_clip_adam_group_f32 does it while it computes the
 * gradient norm.  With splits == 1 dW / db are final. */
#define PM_LINEAR_GROUP_MAX 8
typedef struct pm_linear_fwd_desc {
    const float* X; long ldx; const float* W; long ldw; const float* b; float* Y; long ldy; int M, N, K, act;
} pm_linear_fwd_desc;
typedef struct pm_linear_bwd_data_desc {
    const float* dY; long lddy; const float* W; long ldw; const float* H; long ldh; float* dX; long lddx; int M, N, K, act;
} pm_linear_bwd_data_desc;
typedef struct pm_linear_bwd_weight_desc {
    const float* dY; long lddy; const float* X; long ldx; float* dW; long lddw; float* db; long slab_stride; int M, N, K;
    int dy_cols, x_cols; /* 0, or the number of columns of a dY / X row that may be READ (>= N / K, <= the row stride): rows of 10 or 53
                          * floats inside 16- / 56-float strides take the 16-byte loaders with dy_cols = 16 / x_cols = 56; the extra
                          * columns' contents do not reach dW / db */
    int pad_;
} pm_linear_bwd_weight_desc;
int pm_linear_fwd_group_f32(int n, const pm_linear_fwd_desc* d, void* stream);
int pm_linear_bwd_data_group_f32(int n, const pm_linear_bwd_data_desc* d, void* stream);
int pm_linear_bwd_weight_group_f32(int n, const pm_linear_bwd_weight_desc* d, int splits, void* stream);
/* Which kernel would this call run on?  Each query takes the arguments of its launch entry point without the stream (and
 * without workspace_bytes), runs the SAME host selection the launch consumes and fills `out`; it launches nothing, makes no HIP
 * call and needs no device.  Pointers are looked at for alignment only (made-up addresses are fine; the weight-gradient
 * workspace may be NULL = 16-byte aligned).  Returns what the launch would return for bad arguments.  Tests use it to pin which
 * member of the kernel family a shape exercises.  The gathered / scattered sparse-convolution problems have the same query
 * (pm_sparse_conv_*_variant_f32, below).  Not covered: the chain launches (pm_linear_*_chain_f32), which have their own tests. */
#define PM_LINEAR_PATH_SKINNY 0 /* row-wise VALU kernels, N <= 16 outputs and M >= 256 (forward, data gradient) */
#define PM_LINEAR_PATH_REG 1    /* MFMA GEMM, operands staged through registers */
#define PM_LINEAR_PATH_DMA 2    /* MFMA GEMM, operands by LDS-DMA (16-byte loadable, reduction a multiple of 32) */
typedef struct pm_linear_variant {
    int path;                          /* PM_LINEAR_PATH_* */
    int tm, tn;                        /* work-group tile in output rows x columns of the GEMM (0 for the skinny kernels) */
    int lay;                           /* 0, 1 = the 32 x 128 weight-gradient tile, 2 = the 128 x 32 forward tile */
    int stages;                        /* LDS ring stages of the LDS-DMA kernels, else 0 */
    int vec;                           /* 16-byte operand loads (all problems of a group, or none) */
    int big;                           /* >= 512 tiles of 128 x 128, split-K slabs counted, over the whole group */
    int grid;                          /* work-groups launched (a group pads every problem's range to a multiple of 8) */
    int n;                             /* problems */
    int vecC[PM_LINEAR_GROUP_MAX];     /* per problem: 16-byte epilogue stores (and bias / H loads) */
    int splits[PM_LINEAR_GROUP_MAX];   /* per problem: split-K slabs */
    int kchunk[PM_LINEAR_GROUP_MAX];   /* per problem: reduction range of one slab (a multiple of 32; 0 for the skinny kernels) */
} pm_linear_variant;
int pm_linear_fwd_variant_f32(const float* X, long ldx, const float* W, long ldw, const float* b, const float* Y, long ldy,
                              int M, int N, int K, int act, pm_linear_variant* out);
int pm_linear_bwd_data_variant_f32(const float* dY, long lddy, const float* W, long ldw, const float* H, long ldh,
                                   const float* dX, long lddx, int M, int N, int K, int act, pm_linear_variant* out);
int pm_linear_bwd_weight_variant_f32(const float* dY, long lddy, const float* X, long ldx, const float* dW, long lddw,
                                     const float* db, int M, int N, int K, const void* workspace, pm_linear_variant* out);
int pm_linear_fwd_group_variant_f32(int n, const pm_linear_fwd_desc* d, pm_linear_variant* out);
int pm_linear_bwd_data_group_variant_f32(int n, const pm_linear_bwd_data_desc* d, pm_linear_variant* out);
int pm_linear_bwd_weight_group_variant_f32(int n, const pm_linear_bwd_weight_desc* d, int splits, pm_linear_variant* out);
/* Chains: n (2..4) CONSECUTIVE layers of one network in one launch -- d[i + 1].X must be d[i].Y (forward: network.py:53-54
 * `self.model(x)`), resp. d[i + 1].dY must be d[i].dX (data gradient, top layer first) -- for the small-step regime, where a
 * kernel boundary between two 15 us layers costs a third of a layer.  A 64-row stripe of layer l + 1 depends on the same 64
 * rows of layer l only, so the work-groups of a stripe hand their tiles over inside the launch (write-through stores, one
 * arrival counter per stripe in `workspace`, bounded spins).  Same arithmetic per layer as the single-problem entry points.
 * Needs equal layer widths N (a multiple of 64), 16-byte-loadable operands with K % 32 == 0 (the FIRST forward layer may
 * instead have K <= 64 and unaligned rows: the input layer), and ceil(M / 64) * N / 64 <= 256 work-groups; otherwise returns
 * PM_EUNSUPPORTED (-4) and the caller issues the layers one by one.  workspace: pm_linear_chain_workspace_bytes(M) bytes,
 * 8-byte aligned, ZEROED ONCE by the caller and then handed only to chains of the same (M, N, n): the arrival counters in it
 * are monotonic (no memset per launch, graph-replay safe); its LAST 8-byte word is non-zero once a spin has given up
 * (results of that launch are invalid). */
size_t pm_linear_chain_workspace_bytes(int M);
int pm_linear_fwd_chain_f32(int n, const pm_linear_fwd_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int pm_linear_bwd_data_chain_f32(int n, const pm_linear_bwd_data_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ K6/K7  PointNet encoder
 * network.py:147-153,172-181: per-point shared MLP C->128->256->512 (act,act,none) over
 * (B, P, C) clouds fused with the symmetric max(/mean) pooling; the (B,P,512) activation
 * is never materialised.  feat (B, ldf) receives [max(512) | mean(512) if max_mean];
 * argmax (B,512) int32 is the pooling index (lowest index on ties, as torch.max).
 * x points are read at x + b*ldx + p*C (the reference's flat (B, P*C [+proprio]) rows).
 * Weights in torch layout: W1 (128,C), W2 (256,128), W3 (512,256).
 * pm_pointnet_pack_weights_f32 re-lays W2/W3 into the MFMA-operand order the kernels
 * stream (call after every optimiser step); packed size = pm_pointnet_packed_elems(). */
size_t pm_pointnet_packed_elems(void);
int pm_pointnet_pack_weights_f32(const float* W2, const float* W3, float* packed, void* stream);
int pm_pointnet_enc_fwd_f32(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                            const float* b1, const float* b2, const float* b3, const float* packed,
                            int max_mean, float* feat, long ldf, int32_t* argmax,
                            float* h2_save /* NULL, or (B, P, 256): the layer-2 activations for the backward */,
                            int act /* PM_ACT_* of the two hidden layers (network.py:147-153 takes any of get_activation's
                                       seven; PM_ACT_TANH -- every shipped cfg -- runs the tuned packed-tanh kernels) */,
                            void* stream);
/* Screened tanh forward (csrc/pointnet_enc_screen.h): same contract as pm_pointnet_enc_fwd_f32 with act = PM_ACT_TANH and the
 * same fp32 result class.  Layers 1-2 are the dense kernel's (h2_save bit-identical); layer 3 is screened per 64-point tile on
 * one fp16 MFMA product with a rigorous per-channel error bound, and only the points that can still be a channel's maximum get
 * their exact fp32 dot product; the mean is W3 * mean(h2) + b3.  `packed` as above (layer 2, and layer 3 of the dense
 * fallback); `packed_screen` = pm_pointnet_packed_screen_bytes() bytes written by pm_pointnet_pack_weights_screen from the
 * current W3 / b3 (16-byte aligned).  counters: NULL, or three device uint64 the kernel ADDS to (survivors evaluated, (wave,
 * tile) pairs sent to the dense fallback, (tile, channel) pairs with a survivor) -- tests and timing only. */
size_t pm_pointnet_packed_screen_bytes(void);
int pm_pointnet_pack_weights_screen(const float* W3, const float* b3, void* packed, void* stream);
int pm_pointnet_enc_fwd_screen_f32(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                                   const float* b1, const float* b2, const float* b3, const float* packed,
                                   const void* packed_screen, int max_mean, float* feat, long ldf, int32_t* argmax,
                                   float* h2_save, unsigned long long* counters, void* stream);
/* The same kernel with the order of its independent per-tile work chosen by the caller: schedule 0 = all eight waves in lock-step,
 * 1 = waves 4-7 staggered against their SIMD partners (csrc/pointnet_enc_screen.h, SCHED).  Every output is bit-identical under
 * both; pm_pointnet_enc_fwd_screen_f32 runs the measured default.  Any other schedule is refused (-1) before a launch.
 * PM_ABI_VERSION stays 163 with this addition (no existing signature changed): a loader that wants it looks the symbol up. */
int pm_pointnet_enc_fwd_screen_sched_f32(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                                         const float* b1, const float* b2, const float* b3, const float* packed,
                                         const void* packed_screen, int max_mean, float* feat, long ldf, int32_t* argmax,
                                         float* h2_save, unsigned long long* counters, int schedule, void* stream);
/* OPT-IN split-bf16 forward: same contract as pm_pointnet_enc_fwd_f32, but the two big per-point GEMMs run as
 * a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on bf16 MFMAs with fp32 accumulation (~1e-5 relative instead of ~1e-7;
 * 5.3x less matrix-pipe time).  P must be a multiple of 128.  `packed` = pm_pointnet_packed_bf3_bytes() bytes
 * written by pm_pointnet_pack_weights_bf3 (hi/lo bf16 planes of W2, W3 in MFMA B-operand order). */
size_t pm_pointnet_packed_bf3_bytes(void);
int pm_pointnet_pack_weights_bf3(const float* W2, const float* W3, void* packed, void* stream);
int pm_pointnet_enc_fwd_bf3(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                            const float* b1, const float* b2, const float* b3, const void* packed, int max_mean,
                            float* feat, long ldf, int32_t* argmax, float* h2_save /* as pm_pointnet_enc_fwd_f32 */,
                            void* stream);
/* OPT-IN fp32-class split-bf16 forward: same contract again, with every operand split into THREE bf16 planes and the
 * six products a0b0, a0b1, a1b0, a0b2, a1b1, a2b0 accumulated in fp32 (dropped terms <= 2^-24 relative: the error
 * against fp64 is that of the fp32 MFMA kernel, at 2.7x less matrix-pipe time).  P must be a multiple of 64.
 * `packed` = pm_pointnet_packed_bf6_bytes() bytes written by pm_pointnet_pack_weights_bf6. */
size_t pm_pointnet_packed_bf6_bytes(void);
int pm_pointnet_pack_weights_bf6(const float* W2, const float* W3, void* packed, void* stream);
int pm_pointnet_enc_fwd_bf6(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                            const float* b1, const float* b2, const float* b3, const void* packed, int max_mean,
                            float* feat, long ldf, int32_t* argmax, float* h2_save /* as pm_pointnet_enc_fwd_f32 */,
                            void* stream);
/* Backward of the above w.r.t. the six encoder parameters given dfeat (B, ldf) =
 * [d max(512) | d mean(512)].  Uses the pooling structure: the gradient of the 512-wide
 * layer-3 output is (d mean)/P on every point plus (d max) on the argmax point only, so
 * layers 1-2 are recomputed per tile and only the 256->128 GEMMs run dense.
 * Workspace: pm_pointnet_enc_bwd_workspace_bytes(B). Gradients are WRITTEN (not accumulated). */
size_t pm_pointnet_enc_bwd_workspace_bytes(int B, int P, int C);
int pm_pointnet_enc_bwd_f32(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                            const float* b1, const float* b2, const float* W3, const float* packed,
                            int max_mean, const float* dfeat, long ldf, const int32_t* argmax, float* dW1,
                            float* db1, float* dW2, float* db2, float* dW3, float* db3,
                            const float* h2_saved /* NULL = recompute layer 2; else what the forward saved */,
                            int act /* as the forward's */, void* workspace, size_t workspace_bytes, void* stream);
/* The same call pinned to the 4-wave kernel: pm_pointnet_enc_bwd_f32 runs a saved layer 2 on the 16-wave kernel and only the
 * recomputing backward on the 4-wave one; this entry runs the 4-wave kernel for both (same arguments, same results class), so its
 * saved-layer-2 form stays tested.  PM_ABI_VERSION stays 163 with this addition (no existing signature changed). */
int pm_pointnet_enc_bwd_w4_f32(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                               const float* b1, const float* b2, const float* W3, const float* packed,
                               int max_mean, const float* dfeat, long ldf, const int32_t* argmax, float* dW1,
                               float* db1, float* dW2, float* db2, float* dW3, float* db3, const float* h2_saved,
                               int act, void* workspace, size_t workspace_bytes, void* stream);
/* OPT-IN fp32-class split-bf16 form of the same call (csrc/pointnet_enc_bwd_bf6.h): the two dense GEMMs of the backward
 * (dW2 = dz2^T h1, dh1 = dz2 W2) run on bf16 MFMAs with every operand split into three bf16 planes and six products summed in
 * the fp32 accumulator -- the fp32 kernel's error level at 2.7x less matrix-pipe time; everything else is the fp32 code.  tanh
 * encoders with the forward's saved layer 2 only (h2_saved != NULL).  packed_w2_bf6 = pm_pointnet_packed_bwd_bf6_bytes()
 * bytes written by pm_pointnet_pack_weights_bwd_bf6 from the current W2 (16-byte aligned); same workspace as the fp32 call. */
size_t pm_pointnet_packed_bwd_bf6_bytes(void);
int pm_pointnet_pack_weights_bwd_bf6(const float* W2, void* packed, void* stream);
int pm_pointnet_enc_bwd_bf6(const float* x, long ldx, int B, int P, int C, int sub_mean, const float* W1,
                            const float* b1, const float* b2, const float* W3, const float* packed,
                            const void* packed_w2_bf6, int max_mean, const float* dfeat, long ldf, const int32_t* argmax,
                            float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3, const float* h2_saved,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ K8  PPO actor loss
 * actor_critic.py:74-78,93-100 + ppo.py:327-344 in one pass over a mini-batch of B rows:
 * atanh(clamp(a/max_a)), Gaussian log-prob with std = exp(log_std)^2, analytic KL to the
 * stored (mu_old, log_std_old), ratio, clipped surrogate; and its backward.
 * scal_out[0]=surrogate loss, [1]=kl mean, [2]=skip flag (kl_mean > desired_kl, as 0/1 float),
 * [3]=entropy (identical for every row; unused by the loss, ppo.py:326).  dmu (B,A) and
 * dlog_std (A) are d(loss)/d(.) and are ALWAYS written: the reference's `continue`
 * (ppo.py:337-338) is realised by handing &scal_out[2] to pm_clip_adam_step_f32 as its
 * skip flag, so no host sync sits between loss and optimiser.  adv_moments: NULL, or
 * {sum,sumsq} of the mini-batch advantages (count adv_count) for ppo.py:329's
 * mini_adv_norm (data-parallel callers all-reduce them first).  Two launches: <= 64 work-groups
 * of 256 rows, then a one-wave fixed-order reduction of their partials (deterministic). */
int pm_ppo_actor_loss_fwd_bwd_f32(const float* mu, long ldmu, const float* log_std, const float* actions,
                                  long lda, const float* old_logp, const float* adv, const float* old_mu,
                                  long ldom, const float* old_sigma, long ldos, int B, int A, float max_action,
                                  int act_tanh, float eps_clip, float desired_kl, const double* adv_moments,
                                  double adv_count, float* scal_out, float* dmu, long lddmu, float* dlog_std,
                                  void* workspace, size_t workspace_bytes, void* stream);
size_t pm_ppo_actor_loss_workspace_bytes(int B);
/* The policy head and its loss as ONE launch (small-step regime; ppo.py:322-347 from the last hidden activation on):
 * mu = H W^T + bias (H: B x K last hidden activations, W: A x K, the head of network.py:40) -> the loss rows of
 * pm_ppo_actor_loss_fwd_bwd_f32 -> dmu -> dH = (dmu W) .* act'(H) (hidden_act: PM_ACT_* of the hidden layers) -> the last
 * work-group to finish reduces the partials.  Same arithmetic and summation order as pm_linear_fwd_f32 (row-wise form) +
 * pm_ppo_actor_loss_fwd_bwd_f32 + pm_linear_bwd_data_f32: bit-identical outputs.  mu_out: NULL or B x A.  counter: one
 * device uint32, zero before the first launch (the kernel leaves it zero).  Shapes: A <= 16, K % 4 == 0, A * K * 4 <= 64 KiB,
 * 16-byte aligned rows (pm_ppo_actor_head_supported); otherwise PM_EUNSUPPORTED: use the three entry points separately. */
int pm_ppo_actor_head_supported(const float* H, long ldh, const float* W, long ldw, int A, int K, const float* dH, long lddh);
int pm_ppo_actor_head_f32(const float* H, long ldh, const float* W, long ldw, const float* bias, int K, int hidden_act,
                          const float* log_std, const float* actions, long lda, const float* old_logp, const float* adv,
                          const float* old_mu, long ldom, const float* old_sigma, long ldos, int B, int A, float max_action,
                          int act_tanh, float eps_clip, float desired_kl, const double* adv_moments, double adv_count,
                          float* scal_out, float* mu_out, long ldmu, float* dmu, long lddmu, float* dH, long lddh,
                          float* dlog_std, void* workspace, size_t workspace_bytes, unsigned int* counter, void* stream);
/* forward-only: log-prob/entropy rows, actor_critic.py:71-82 (used by rollout + tests). */
int pm_gaussian_logp_f32(const float* mu, long ldmu, const float* log_std, const float* actions, long lda,
                         int B, int A, float max_action, int act_tanh, float* logp, float* entropy,
                         void* stream);

/* ------------------------------------------------------------------ K9  value loss
 * ppo.py:368-374: mean((ret-V)^2), or the clipped variant with the batch-mean clip width.
 * clip_mean_extern: NULL or device float = all-reduced mean(|eps*V_old|) (data parallel).
 * scal_out[0] = loss.  dV (B rows of stride lddv >= 1) = d loss / dV * grad_scale. */
int pm_value_loss_fwd_bwd_f32(const float* V, const float* returns, const float* old_values, int B,
                              int clipped, float eps_clip, const float* clip_mean_extern, float grad_scale,
                              float* scal_out, float* dV, long lddv, void* stream);

/* The value head and its loss as ONE launch (small-step regime; ppo.py:362-377 from the last hidden activation on):
 * V = H w + bias (H: B x K, w: the (1 x K) head of network.py:40) -> the loss above -> dV (rows of stride lddv) ->
 * dH = (dV w) .* act'(H) -> the last work-group to finish sums the loss partials.  V, dV, dH: the bits of pm_linear_fwd_f32
 * (row-wise form) + pm_value_loss_fwd_bwd_f32 + pm_linear_bwd_data_f32; scal_out[0]: the same sum in another association
 * (double precision).  V_out: NULL or B.  counter: one device uint32, zero before the first launch (left zero).  K % 4 == 0,
 * K * 4 <= 64 KiB, 16-byte aligned rows (pm_value_head_supported), otherwise PM_EUNSUPPORTED. */
size_t pm_value_head_workspace_bytes(void);
int pm_value_head_supported(const float* H, long ldh, const float* W, int K, const float* dH, long lddh);
int pm_value_head_f32(const float* H, long ldh, const float* W, const float* bias, int K, int hidden_act, const float* returns,
                      const float* old_values, int B, int clipped, float eps_clip, const float* clip_mean_extern,
                      float grad_scale, float* scal_out, float* V_out, float* dV, long lddv, float* dH, long lddh,
                      void* workspace, size_t workspace_bytes, unsigned int* counter, void* stream);

/* ------------------------------------------------------------------ K11 DAgger loss
 * dagger.py:310-314: mean((tanh(tea_mu)*max_a - tanh(stu_mu)*max_a)^2) over B*A and
 * d/d stu_mu.  act_tanh==0 -> identity squashing (actor_critic.py:87-88).  act_tanh==3: the student is
 * squashed but `tea_mu` already holds recorded ACTIONS -- bc.py:139 `(actions - stu_act).pow(2).mean()`. */
int pm_mse_tanh_loss_fwd_bwd_f32(const float* stu_mu, long lds, const float* tea_mu, long ldt, int B, int A,
                                 float max_action, int act_tanh, float grad_scale, float* scal_out,
                                 float* dstu_mu, long ldd, void* stream);
/* actor_critic.py:84-91 */
int pm_action_activation_f32(const float* mu, float* out, long n, float max_action, int act_tanh, void* stream);
/* Backward halves of pm_gaussian_logp_f32 / pm_action_activation_f32 for callers that differentiate through
 * ActorCritic.update_act_cri / update_act with torch autograd, the way the reference's own update() does
 * (ppo.py:326,347-348; dagger.py:312-318; partmanip_amd/autograd.py wraps them in torch.autograd.Function):
 * dmu (B, A) = dlogp[i] * (x - mu) / s^2 and dlog_std (A) = sum_i dlogp[i] (2 z^2 - 2) + 2 dent[i], with s = exp(log_std)^2,
 * z = (x - mu) / s, x = atanh(clamp(a / max_action)) -- dlogp / dent (B) are the incoming gradients (either may be NULL). */
int pm_gaussian_logp_bwd_f32(const float* mu, long ldmu, const float* log_std, const float* actions, long lda, int B, int A,
                             float max_action, int act_tanh, const float* dlogp, const float* dent, float* dmu, long lddm,
                             float* dlog_std, void* stream);
int pm_action_activation_bwd_f32(const float* out, const float* dout, float* dmu, long n, float max_action, int act_tanh,
                                 void* stream);

/* ------------------------------------------------------------------ K10 clip + Adam
 * nn.utils.clip_grad_norm_ (ppo.py:351,381) fused with torch.optim.Adam.step (ppo.py:353,382,
 * dagger.py:319) over ONE flat fp32 parameter buffer: the L2 norm / clip coefficient
 * min(1, max_norm/(norm+1e-6)) covers the first n_clip elements only (the actor optimiser
 * also owns log_std, which the reference does not clip); max_norm<=0 disables clipping.
 * state (device, 4 x int32): [0]=step count t (incremented here unless skipped).
 * skip_flag: NULL or device float; non-zero -> the whole step is a no-op (ppo.py:337-338).
 * Adam: betas (b1,b2), eps, bias-corrected exactly as torch (denom = sqrt(v)/sqrt(1-b2^t)+eps,
 * step = lr/(1-b1^t)).  Workspace: pm_clip_adam_workspace_bytes(n). */
size_t pm_clip_adam_workspace_bytes(long n);
/* The same step for several optimisers in two launches (ppo.py:353 and :382 are independent: optimizer_actor and
 * optimizer_critic), each optionally summing split-K gradient slabs first: grads[i] += sum_{s=1..n_extra} extra[(s-1) *
 * extra_stride + i] for i < n_sum (fixed order; grads is slab 0 of pm_linear_bwd_weight_group_f32), then exactly
 * pm_clip_adam_step_f32.  workspace: pm_clip_adam_workspace_bytes(n) doubles per desc, 8-byte aligned. */
typedef struct pm_clip_adam_desc {
    float* params; float* grads; float* exp_avg; float* exp_avg_sq; long n, n_clip; const float* extra; long extra_stride;
    long n_sum; int n_extra; float max_norm; double lr, b1, b2, eps; int32_t* state; const float* skip_flag;
    float* gnorm_out; void* workspace;
    /* optional (stats_acc != NULL): pm_ppo_accumulate_stats_f32(stats_acc, stats_scal, stats_which) folded into the norm pass */
    float* stats_acc; const float* stats_scal; int stats_which;
    /* data-parallel step (new: the reference has no collective): `grads` and the step's scalars arrive as the
     * all-reduce SUM over W ranks.  The form is on when dp_scal != NULL or grad_scale is neither 0 nor 1; it requires n_extra == 0
     * (fold the slabs with pm_grad_slab_sum_f32 BEFORE the reduce).  grad_scale = 1/W: the norm pass first rewrites grads[0..n) *= grad_scale
     * (mean gradient; clip + Adam then see exactly what a single process with the W-fold mini-batch computes).  dp_scal
     * (NULL = off): the step's scalar record {loss, kl, skip}: [0], [1] *= grad_scale, and when dp_kl_desired > 0 the KL
     * early-stop predicate of ppo.py:337-338 is re-taken from the REDUCED kl ([2] = kl > dp_kl_desired) before skip_flag /
     * stats are read -- every rank takes the same branch without a host round trip or an extra launch. */
    float grad_scale; float dp_kl_desired; float* dp_scal;
} pm_clip_adam_desc;
int pm_clip_adam_group_f32(int n, const pm_clip_adam_desc* d, void* stream);
/* grads[i] += sum_{s=1..n_extra} extra[(s-1) * extra_stride + i] for i < n_sum, in the order pm_clip_adam_group_f32's norm
 * pass uses (bit-identical): the split-K slabs of pm_linear_bwd_weight_group_f32 folded BEFORE a gradient all-reduce, so
 * that the message is one slab and not n_extra + 1. */
int pm_grad_slab_sum_f32(float* grads, const float* extra, long extra_stride, long n_sum, int n_extra, void* stream);
int pm_clip_adam_step_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n,
                          long n_clip, float max_norm, double lr, double b1, double b2, double eps,
                          int32_t* state, const float* skip_flag, float* gnorm_out, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ scalar bookkeeping of ppo.update
 * ppo.py:335-336,355-357,384: device-side running sums so the host never syncs per
 * mini-batch. acc (device, 8 floats): [0]=sum surrogate,[1]=sum kl,[2]=kl max,[3]=count,
 * [4]=sum value loss,[5]=n value steps.  which: 0 = actor step (reads scal[0..2]), 1 = critic. */
int pm_ppo_accumulate_stats_f32(float* acc, const float* scal, int which, void* stream);

/* ------------------------------------------------------------------ K12-K14 point-set operators
 * K12: utils/depth2tsdf.py:113,160 call pytorch3d.ops.sample_farthest_points(points, K)
 * (un-vendored; defaults: start index 0, no lengths).  idx_out (B,K) int32; squared-L2
 * running-min distance; next = argmax, lowest index on ties.  PARITY UNPINNED (no reference
 * implementation in tree) -- checked against the restatement `oracle/ref_cpu.py::fps` / `ball_query` / `group_points`
 * (tests/test_gpu_kernels.py, tests/test_gpu_fuzz.py: indices bit-exact).
 * K13/K14: PointNet++ ball query / grouping -- absent from the reference (README.md:23,30),
 * mandated by BASELINE.json.north_star; first `nsample` in-radius indices in ascending
 * order, padded with the first hit, all-zero row when the ball is empty. */
size_t pm_fps_workspace_bytes(int B, int P);   /* 0 when the cloud fits in registers (P <= 8192) */
int pm_fps_f32(const float* xyz, int B, int P, int D, int K, int32_t* idx_out, void* workspace,
               size_t workspace_bytes, void* stream);
int pm_ball_query_f32(const float* xyz, const float* centers, int B, int P, int S, float radius, int nsample,
                      int32_t* idx_out, void* stream);
int pm_group_points_f32(const float* feat, const int32_t* idx, int B, int P, int C, int S, int nsample,
                        float* out, void* stream);
/* (the gradient of the gather: per source point the sum of its rows of dout in ASCENDING row order -- one work-group per cloud inverts
 * the index table in LDS, no floating-point atomics, every element of dfeat written -- when 2 P + S nsample <= ~15.7 k; larger
 * tables: fp32 atomics into the zero-filled dfeat, summation order not fixed.  pm_group_concat_bwd_f32 alike.) */
int pm_group_points_bwd_f32(const float* dout, const int32_t* idx, int B, int P, int C, int S, int nsample,
                            float* dfeat, void* stream);

/* ------------------------------------------------------------------ K15 PointNet++ set-abstraction glue
 * (absent from the reference; north-star mandated; parity unpinned, own oracle).
 * group_concat: out[b,s,j,:] = [xyz[b,idx]-centers[b,s] (3) | feat[b,idx,:] (Cf) | zero pad to ldo]
 * (the rows the shared per-point MLP consumes); its backward scatter-adds the feature columns
 * (fixed-order sums like pm_group_points_bwd_f32; fp32 atomics into the zero-filled dfeat only beyond its size limit).  maxpool_rows: max over the nsample axis of
 * (G, nsample, C) with the lowest arg-max index; its backward writes every element of dx. */
int pm_group_concat_f32(const float* xyz, const float* feat, const float* centers, const int32_t* idx, int B, int P,
                        int Cf, int S, int nsample, int ldo, float* out, void* stream);
/* Column-block copy: dst[r][d_b .. d_b + e_b - s_b) = src[r][s_b .. e_b) for two blocks b (an empty block: s == e); the other
 * columns of dst in [col0, dst_cols) are zeroed when zero_other != 0; columns below col0 are left alone.  A non-empty block must land
 * inside [col0, dst_cols), the two blocks must not overlap, src may be NULL when both blocks are empty (zero-only), and dst == src is
 * allowed only with blocks that read below col0 (PM_EINVAL otherwise -- never a silently skipped block).  The PointNet++ plug-in's
 * glue around its GEMMs in one launch each (weights in operand column order padded to the K-step, gradients back, [xyz | 0] behind the
 * group-all rows' features). */
int pm_col_blocks_f32(float* dst, long ldd, const float* src, long lds, long rows, int dst_cols, int col0, int s0, int e0, int d0,
                      int s1, int e1, int d1, int zero_other, void* stream);
/* dst[q] = table[q] >= 0 ? src[table[q]] : 0 for q < n.  Every weight-derived operand copy of a network (the pack entry points'
 * outputs, aligned / padded column blocks) is such a gather of the flat parameter buffer with a table fixed by the layouts: the host
 * records the table once (by running the pack entry points on index-valued weights) and refreshes all copies with this ONE launch per
 * forward instead of one tiny launch per copy. */
int pm_gather_copy_f32(float* dst, const float* src, const int32_t* table, long n, void* stream);
int pm_group_concat_bwd_f32(const float* dout, const int32_t* idx, int B, int P, int Cf, int S, int nsample, int ldo,
                            float* dfeat, void* stream);
int pm_maxpool_rows_f32(const float* x, long G, int nsample, int C, float* out, long ldo, int32_t* arg, void* stream);
int pm_maxpool_rows_bwd_f32(const float* dout, long lddo, const int32_t* arg, long G, int nsample, int C,
                            const float* y_tanh /* NULL, or the pooled tanh outputs: dx *= 1-y^2 */, float* dx,
                            void* stream);

/* ------------------------------------------------------------------ depth images -> world-frame cloud
 * utils/depth2tsdf.py:142-157 (TSDFVolume.depth2pc before the sampling at :160): pinhole back-projection of
 * depth (B, M, H, W), rigid transform with cam_pose (M, 4, 4 row-major, camera -> world), points outside the
 * OPEN box (lo, hi) zeroed.  out (B, M*H*W, 3).  lo / hi are HOST pointers to 3 floats.  K12 then samples it. */
int pm_depth_backproject_f32(const float* depth, int B, int M, int H, int W, const float* cam_pose, float fx,
                             float fy, float cx, float cy, const float* lo, const float* hi, float* out,
                             void* stream);

/* Crop compaction + variable-length FPS for the step above.  pm_depth_compact_f32: out (B, P, 3) receives, per
 * env and in the original order, every non-zero point plus the FIRST zero point; lengths[b] = how many.  FPS over
 * that prefix selects the same sequence of POINTS as FPS over the full cropped cloud (the zeroed points are one
 * candidate).  pm_fps_varlen_f32: clouds are the first lengths[b] rows of a (B, ld, D) buffer; K rounds always
 * (no -1 padding: once every point is taken the lowest index repeats, as on the full cloud); workspace
 * B*ld floats when ld > 8192. */
int pm_depth_compact_f32(const float* xyz, int B, int P, float* out, int32_t* lengths, void* stream);
/* Workspace: 0 when every cloud fits in registers (ld <= 8192).  With the full reservation (8-byte aligned) camera-sized xyz
 * clouds run on pm_fps_varlen_groups(B, ld, D) >= 2 work-groups per cloud, each keeping its chunk on chip; the partners of a
 * cloud wait for each other INSIDE the launch, with ONE bounded poll budget per work-group and launch (~1 s; pm_fps_config.spin_limit).
 * A work-group that exhausts it gives up ONCE: it latches the flag, sets the reservation's last 8 bytes (which every other
 * work-group of the launch watches and follows) and returns; the call then DEGRADES on the device: a launch queued behind it
 * re-samples the batch's big clouds on one work-group each when -- and only when -- that word is set (no host round trip, the
 * indices are valid either way; the word stays set for diagnostics until the next multi-work-group call clears it).  Other
 * kernels on the device only delay the hand-offs (their work-groups drain); two such launches running concurrently on two
 * streams can hold each other's CUs until the budget trips -- issue them from one stream, or cap the group count (pm_fps_config.max_groups,
 * 0 / 1 = one work-group per cloud) when CUs are masked or shared. */
/* Launch policy of the multi-work-group sampler, PASSED by the caller (the library reads no environment variable and keeps no
 * state between calls); NULL = the defaults.  max_groups: cap on the work-groups per cloud (< 0: none; 0 / 1: one work-group per
 * cloud -- when CUs are masked or shared); resident_cus: the CUs the caller knows the launch can occupy (0: all the device
 * reports -- wrong under a CU mask or beside a long-running kernel, which is why it is the caller's to say); spin_limit (when
 * spin_limit_set): the poll budget of a hand-off; legacy_shape: the 1024-thread x 16-point launch shape (A/B). */
typedef struct pm_fps_config {
    int max_groups;
    int resident_cus;
    unsigned spin_limit;
    int spin_limit_set;
    int legacy_shape;
} pm_fps_config;
size_t pm_fps_varlen_workspace_bytes(int B, int ld);
int pm_fps_varlen_groups(int B, int ld, int D);                                  /* = _cfg(..., NULL) */
int pm_fps_varlen_groups_cfg(int B, int ld, int D, const pm_fps_config* cfg);
int pm_fps_varlen_cfg_f32(const float* xyz, int B, int ld, int D, int K, const int32_t* lengths, int pad, int32_t* idx_out,
                          const pm_fps_config* cfg, void* workspace, size_t workspace_bytes, void* stream);
int pm_fps_varlen_f32(const float* xyz, int B, int ld, int D, int K, const int32_t* lengths,
                      int pad /* 1: pytorch3d semantics, -1 once a cloud is exhausted; 0: keep sampling (see above) */,
                      int32_t* idx_out, void* workspace, size_t workspace_bytes, void* stream);
/* utils/depth2tsdf.py:103-119 (`TSDFVolume.sparse_voxel` after pm_tsdf_integrate_f32): pm_tsdf_select_f32 writes, per
 * env and in row-major voxel order (= torch.where), the integer coordinates (as floats) of the voxels with
 * lo < tsdf < hi into coords (B, res^3, 3) and their count into lengths; pm_fps_varlen_f32 (pad = 1) samples them;
 * pm_tsdf_sparse_gather_f32 emits out (B, K, 4) = (x, y, z, tsdf), padding indices reading voxel (0,0,0). */
int pm_tsdf_select_f32(const float* vol, int B, int res, float lo, float hi, float* coords, int32_t* lengths,
                       void* stream);
int pm_tsdf_sparse_gather_f32(const float* coords, const int32_t* idx, const float* vol, int B, int res, int K,
                              float* out, void* stream);

/* ------------------------------------------------------------------ depth images -> compact cloud with source pixels, part labels
 * pm_depth_cloud_f32 = pm_depth_compact_f32(pm_depth_backproject_f32(...)) in one kernel that never writes the (B, P, 3) world cloud
 * and records the pixel every kept point came from.  P = M H W; pixel r = view * H W + row * W + col; w(r) is what
 * pm_depth_backproject_f32 writes for that pixel (the same device function computes it: same arithmetic, same zeroing outside the
 * OPEN box (lo, hi); lo / hi are HOST pointers to 3 floats).  Kept pixels: every r with w(r) != (0, 0, 0) by value, plus the
 * smallest r with w(r) == (0, 0, 0) if there is one (a pixel whose world point lies inside the box but exactly at the origin counts
 * as zero, as in the composition).  The j-th kept pixel in ascending r goes to xyz[b, j] = w(r) and src[b, j] = r, for j < cap;
 * lengths[b] = min(count, cap); rows at and past lengths[b] are NOT written.  xyz (B, cap, 3), src (B, cap) int32 or NULL (not
 * wanted), lengths (B) int32.  With cap >= count, xyz[b, :lengths[b]] and lengths equal the composition bit for bit; with
 * cap < count the first cap kept points survive (a truncation the caller chose, to bound memory).  One work-group per environment,
 * no atomics on global memory, no workspace, stream-ordered, never synchronises.
 * PM_EINVAL: a NULL depth / cam_pose / lo / hi / xyz / lengths, B, M, H, W or cap < 1, M H W > INT_MAX. */
int pm_depth_cloud_f32(const float* depth, int B, int M, int H, int W, const float* cam_pose, float fx, float fy, float cx,
                       float cy, const float* lo, const float* hi, int cap, float* xyz, int32_t* src, int32_t* lengths,
                       void* stream);
/* Rows (x, y, z, label) of sampled points of such a cloud.  xyz (B, ld, 3) and src (B, ld) as written above (ld = cap), idx (B, K)
 * int32 (pm_fps_varlen_f32's), seg: int32 labels per pixel, row b at seg + b * seg_stride, P pixels per row.  With i = idx[b, k]:
 *   out[b * out_stride + 4 k + 0..2] = xyz[b, i, :]
 *   out[b * out_stride + 4 k + 3]    = zero_label if xyz[b, i] == (0, 0, 0) by value -- the one point that stands for everything
 *                                      cropped away or missed: its pixel is whichever came first, so its label would mean nothing;
 *                                      otherwise (float) seg[b * seg_stride + src[b, i]]
 * i outside [0, ld): all four floats are NaN and nothing is read through i.  src[b, i] outside [0, P): the label is NaN and seg is
 * not read.  Columns at and past 4 K of a row are never written (the proprio tail of an observation row); rows need 4-byte
 * alignment only.  No workspace, no atomics, stream-ordered.
 * PM_EINVAL: a NULL xyz / src / idx / seg / out, B, ld, K or P < 1, out_stride < 4 K, seg_stride < P. */
int pm_cloud_gather_labeled_f32(const float* xyz, const int32_t* src, int B, int ld, const int32_t* idx, int K, const int32_t* seg,
                                long seg_stride, int P, float zero_label, float* out, long out_stride, void* stream);
/* PM_ABI_VERSION stays 163 with these additions and with pm_mesh_pc_query_labeled_f32 below (no existing signature changed). */

/* algorithms/algo_utils/network.py:72,119 -- Conv3DNet's INPUT layer, Conv3d(1, Cout, k, stride, padding k/2), as a direct
 * stencil over the single-channel volume (no patch matrix): x (B, D, H, W) through element strides (sb, sd, sh, sw);
 * wt = conv.weight viewed (Cout, k^3) TRANSPOSED to (k^3, Cout); y (B*Do*Ho*Wo, ldy) rows of Cout = act(conv + bias)
 * (channels-last, what the next layer's pm_im2col3d_f32 reads through strides).  pm_conv3d_c1_wgrad_f32: dW (Cout, lddw
 * >= k^3) and db (Cout, may be NULL) from dz (rows, lddz) = the gradient at this layer's pre-activation.  Instantiated
 * for k = 5, Cout = 16 (pm_conv3d_c1_supported); other shapes return PM_EUNSUPPORTED: use im2col + the Linear kernels.
 * batch_index (may be NULL): volume b of the batch is row batch_index[b] (stride sb) of a larger store -- DAgger's
 * mini-batches are random rows of the ring (dagger.py:305-306): the 0.8 GB gathered copy of 1600 volumes is not made. */
int pm_conv3d_c1_supported(int k, int Cout);
size_t pm_conv3d_c1_wgrad_workspace_bytes(int Cout);
int pm_conv3d_c1_fwd_f32(const float* x, int B, int D, int H, int W, int k, int stride, int pad, long sb, long sd, long sh,
                         long sw, const float* wt, const float* bias, int Cout, int act, float* y, long ldy,
                         const int64_t* batch_index, void* stream);
int pm_conv3d_c1_wgrad_f32(const float* dz, long lddz, const float* x, int B, int D, int H, int W, int k, int stride,
                           int pad, long sb, long sd, long sh, long sw, int Cout, float* dW, long lddw, float* db,
                           const int64_t* batch_index, void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------ Conv3D students: patch gather / scatter
 * network.py:56-94 (`Conv3DNet` / `Encoder`: nn.Conv3d(k, stride, padding = k/2)).  A convolution runs as
 * cols = im2col(x) -> pm_linear_fwd_f32 with conv.weight viewed (Cout, Cin*k^3) -> rows (b, od, oh, ow) x Cout;
 * its backward as pm_linear_bwd_weight_f32 / pm_linear_bwd_data_f32 on the same cols and dx = col2im(dcols).
 * x / dx are addressed by ELEMENT strides (sb, sc, sd, sh, sw): channels-first inputs and channels-last layer
 * outputs both work.  cols / dcols: (B*Do*Ho*Wo, ldc), column (c, kd, kh, kw) with c slowest; im2col zero-fills
 * columns [C*k^3, ldc).  Do = (D + 2*pad - k)/stride + 1 etc.  col2im overwrites every dx element. */
int pm_im2col3d_f32(const float* x, int B, int C, int D, int H, int W, int k, int stride, int pad, long sb, long sc,
                    long sd, long sh, long sw, float* cols, int ldc, void* stream);
int pm_col2im3d_f32(const float* dcols, int B, int C, int D, int H, int W, int k, int stride, int pad, long sb,
                    long sc, long sd, long sh, long sw, const float* y_tanh /* NULL, or x itself when it is an activation
                    output laid out like dx: dx *= act'(x), 1 - x^2 for tanh */, int act /* PM_ACT_* of that layer */,
                    float* dx, int ldc, void* stream);

/* ------------------------------------------------------------------ TSDF integration (observation side)
 * utils/depth2tsdf.py:68-86 `TSDFVolume.integrate`: depth (B, M, H*W) -> out (B, V) truncated signed distances
 * averaged over the views that see each voxel.  pix_idx (M, V) int32 = row*W + col of the voxel's pixel in view m,
 * or -1 outside the frustum; pix_z (M, V) = its camera-frame depth (both built at register_camera time,
 * depth2tsdf.py:41-60).  trunc = 4 voxels; default_tsdf for voxels no view sees. */
int pm_tsdf_integrate_f32(const float* depth, const int32_t* pix_idx, const float* pix_z, int B, int M, long HW,
                          long V, float trunc, float default_tsdf, float* out, void* stream);

/* ------------------------------------------------------------------ mesh-TSDF observation (observation side)
 * utils/mesh2sdf.py:119-132, 239-272 `TSDFfromMesh.query_tsdf_parallel` in one launch: for every environment b and workspace
 * voxel v (centre (i, j, k) * vox_size + origin, k fastest) the signed-distance grids of the parts [p0, p1) are sampled
 * trilinearly under the parts' poses (q = (c_v - T[b,p]) R[b,p]; valid iff 1 <= (q - bbox_min[p]) / voxel_size[p] <= shape[p] - 2
 * on all three axes, else the sample is 1), out[b * out_stride + v] = clamp(min(min_p sample, base) / sdf_trunc, -1, 1).
 * fields: the parts' grids (X, Y, Z row-major, un-padded) concatenated; part_off (M) int64 element offsets into it; part_shape
 * (M, 3) int32 (every grid < 2^31 cells); part_bbox_min (M, 3); part_voxel_size (M); pose_R (B, M, 3, 3); pose_T (B, M, 3).
 * base: (res^3) shared by all environments (base_per_env = 0: the ground plane) or (B, res^3) (base_per_env = 1: after
 * initialize_sdf).  out_stride >= res^3 in elements: the volume can land in the left part of an observation row.  brick_skip != 0
 * drops a part for a whole 4^3 brick of voxels when the brick cannot reach the part's valid box (bit-identical output, faster).
 * An environment with a non-finite pose entry (any of its M parts) comes out all-NaN; nothing is ever read out of bounds.
 * PM_EINVAL: a NULL pointer, B outside [1, 65535], p0 >= p1, p1 > M, res <= 0, out_stride < res^3, sdf_trunc <= 0. */
int pm_mesh_tsdf_query_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape, const float* part_bbox_min,
                           const float* part_voxel_size, const float* pose_R, const float* pose_T, int B, int M, int p0, int p1,
                           int res, float vox_size, float ox, float oy, float oz, float sdf_trunc, const float* base,
                           int base_per_env, float* out, long out_stride, int brick_skip, void* stream);

/* ------------------------------------------------------------------ mesh-TSDF observation of a scene whose environments differ
 * pm_mesh_tsdf_query_groups_f32: the arguments of the entry above with the part tables read as a GRID LIBRARY of NG rows (fields,
 * part_off, part_shape, part_bbox_min, part_voxel_size: one row per grid) plus
 *   grid_slot (NG) int32     the pose slot in [0, M) that row's grid is placed by: its pose in environment b is pose[b, grid_slot[row]]
 *   NG_shared                rows [0, NG_shared) are sampled by every environment
 *   group_off (G + 1) int32  rows relative to NG_shared, non-decreasing, group_off[0] = 0, group_off[G] = NG - NG_shared
 *   env_group (B) int32      g = env_group[b] in [0, G): environment b also owns the rows of group g; g = -1: the shared rows only
 *   max_group_grids          an upper bound of the rows of a group, max_g (group_off[g + 1] - group_off[g])
 *   t0, t1                   an ordinal range in place of p0, p1
 * Definition: environment b owns the ordinals t < NG_shared (row t) and t = NG_shared + i for i < group_off[g + 1] - group_off[g]
 * (row NG_shared + group_off[g] + i).  Take its own rows, in ordinal order, as the parts of pm_mesh_tsdf_query_f32, each with the
 * pose of the slot its row names, and p0, p1 = its own ordinals inside [t0, t1): the volume of environment b is exactly that result
 * -- the same fp32 association, the same validity rule against the row's own shape, the same min with the base, the same division
 * and clamp -- bit for bit, with brick_skip on and off.  No own ordinal inside [t0, t1): clamp(base / sdf_trunc, -1, 1).
 * Environment b comes out all-NaN iff a pose of a slot named by one of its OWN rows has a non-finite entry, whatever t0 and t1 are;
 * slots no own row names are never examined (the NaN poses a scene's row table leaves past a cabinet's body count do nothing).
 * Launch shape: that of the entry above (one wave per 4^3 brick, four bricks per work-group, grid row = environment); lane l tests
 * ordinal pb + l; group, row and slot of an iteration are wave-uniform, so table and pose reads stay scalar loads.
 * Memory safety: g outside [-1, G) counts as -1; group_off is cut to [0, NG - NG_shared], so rows stay in [NG_shared, NG); at most
 * max_group_grids rows of a group are sampled (a bound that is too small drops the group's last rows); a grid_slot outside [0, M)
 * makes its row unsampled and no pose is read through it; gathers stay behind the validity test.
 * PM_EINVAL (before any launch): every condition of the entry above (p0, p1 read as t0, t1), NG <= 0, NG_shared outside [0, NG],
 * G < 0, max_group_grids < 0, t0 < 0, t0 >= t1, t1 > NG_shared + max_group_grids, a NULL grid_slot, a NULL group_off or env_group
 * with G > 0.  PM_ABI_VERSION stays 163 with this addition (no existing signature changed). */
int pm_mesh_tsdf_query_groups_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape, const float* part_bbox_min,
                                  const float* part_voxel_size, const int32_t* grid_slot, int NG, int NG_shared,
                                  const int32_t* group_off, int G, const int32_t* env_group, int max_group_grids, const float* pose_R,
                                  const float* pose_T, int B, int M, int t0, int t1, int res, float vox_size, float ox, float oy,
                                  float oz, float sdf_trunc, const float* base, int base_per_env, float* out, long out_stride,
                                  int brick_skip, void* stream);

/* ------------------------------------------------------------------ contact sensing: posed points against the part grids
 * pm_mesh_sdf_points_f32 / pm_mesh_sdf_points_groups_f32: the signed distance, in metres, of NP points per environment to the grids
 * that pm_mesh_tsdf_query_f32 / pm_mesh_tsdf_query_groups_f32 sample at the workspace lattice.  The part tables, pose_R, pose_T, B, M,
 * p0, p1 and the group tables, t0, t1 mean what they mean there, with the same clamping and memory-safety rules.
 *   pts               point n of environment b is the three floats at pts + b * pts_env_stride + 3 n; pts_env_stride = 0: one set
 *                     of points shared by all environments
 *   carrier (NP) int32         the pose slot in [0, M) whose body carries the point; -1: the point is given in the world frame
 *   pt_id (NP) int32 or NULL   the id the point is reported under in seg_arg and that settles ties there (NULL: n itself); a
 *                     negative id marks a padding point, which enters no segment result (its dist / arg are written like any other)
 *   chunk_sphere (ceil(NP / 64), 4) float32 or NULL   (centre, radius), in the carrier's frame, of a ball that holds the points
 *                     [64 c, 64 c + 64) of row c; read for a row only when cull != 0, a segment's 64-point run starts at 64 c and all
 *                     its points share one carrier, so a caller that wants the cull sorts by carrier and pads runs to whole chunks
 *   seg_off (NS + 1) int32     non-decreasing, seg_off[0] = 0, seg_off[NS] = NP: NS segments of points, one per sensing body; NS = 0
 *                     (seg_off may be NULL): no segments
 * Definition, every operation one correctly rounded fp32 operation, no contraction:
 *   1. w_a = ((R[c,a,0] x_0 + R[c,a,1] x_1) + R[c,a,2] x_2) + T[c,a] with c the carrier; carrier -1: w = x.
 *   2. every own ordinal of the environment inside [p0, p1) / [t0, t1) is sampled at w exactly as the TSDF entries sample it at a voxel
 *      centre (d = w - T_p, q = ((d0 R0j + d1 R1j) + d2 R2j), u = (q - bbox_min) / voxel_size, valid iff u_a >= 1 and u_a - shape_a
 *      <= -2 on all axes, the same trilinear association); an invalid sample is 1.
 *   3. dist[b * ld_dist + n] = the minimum of the samples, NaN wins, starting from 1: metres, neither divided by a truncation nor
 *      clamped.  arg[b * ld_dist + n] = the smallest ordinal that attains it, -1 if no sample was below 1.  arg may be NULL.
 *   4. seg_min[b * NS + s] = the minimum of dist over the segment's points with id >= 0, NaN wins; seg_arg[b * NS + s] = the smallest
 *      id that attains it (of the NaNs if there is one); an empty segment: 1 and -1.  Both may be NULL together; dist may be NULL
 *      when they are not.
 *   5. environment b comes out all-NaN (dist, seg_min) with arg = seg_arg = -1 iff a pose has a non-finite entry -- ungrouped: in any
 *      of the M slots; grouped: in a slot that one of its own rows or a carrier names.  Other environments are untouched.
 *   6. a carrier outside [-1, M) makes its point 1 / -1, and no pose is read through it.
 *   7. cull != 0 lets a wave drop an ordinal for a whole chunk that its sphere cannot bring into the ordinal's valid box.  The output
 *      with cull on and off is bit-identical, and so are two runs: no floating-point atomics, ordinary vector stores only.
 * Memory safety: seg_off is cut to [0, NP] and made non-decreasing in the kernel (points that then lie in no segment are not
 * written); everything else as the TSDF entries state.  Launch: one work-group of four waves per (segment, environment), or per 256
 * points with NS = 0; lane = point; the sample loop's table and pose reads are scalar loads.
 * PM_EINVAL (before any launch): a NULL table, pose, pts or carrier; B outside [1, 65535]; M <= 0 (grouped: M > 32768); p0 >= p1,
 * p1 > M (grouped: the t0, t1, NG, NG_shared, G, max_group_grids and group-table conditions of pm_mesh_tsdf_query_groups_f32); NP
 * outside [1, 2^30]; NS < 0; NS > 0 with a NULL seg_off; pts_env_stride neither 0 nor >= 3 NP; only one of seg_min, seg_arg; seg_min
 * with NS = 0; neither dist nor seg_min; ld_dist < NP with dist or arg.  PM_ABI_VERSION stays 163 (no existing signature changed). */
int pm_mesh_sdf_points_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape, const float* part_bbox_min,
                           const float* part_voxel_size, const float* pose_R, const float* pose_T, int B, int M, int p0, int p1,
                           const float* pts, long pts_env_stride, const int32_t* carrier, const int32_t* pt_id,
                           const float* chunk_sphere, int NP, const int32_t* seg_off, int NS, float* dist, long ld_dist, int32_t* arg,
                           float* seg_min, int32_t* seg_arg, int cull, void* stream);
int pm_mesh_sdf_points_groups_f32(const float* fields, const int64_t* part_off, const int32_t* part_shape, const float* part_bbox_min,
                                  const float* part_voxel_size, const int32_t* grid_slot, int NG, int NG_shared,
                                  const int32_t* group_off, int G, const int32_t* env_group, int max_group_grids, const float* pose_R,
                                  const float* pose_T, int B, int M, int t0, int t1, const float* pts, long pts_env_stride,
                                  const int32_t* carrier, const int32_t* pt_id, const float* chunk_sphere, int NP,
                                  const int32_t* seg_off, int NS, float* dist, long ld_dist, int32_t* arg, float* seg_min,
                                  int32_t* seg_arg, int cull, void* stream);

/* ------------------------------------------------------------------ mesh bake (producer of the mesh-TSDF part grids)
 * utils/mesh2sdf.py:201-237 `TSDFfromMesh.mesh2sdf` without kaolin / ManifoldPlus: the signed-distance grid of one triangle mesh.
 * tri: (F, 3, 3) float32 corner positions (faces with two equal corners already dropped by the caller; a remaining zero-area
 * triangle counts as its longest edge for the distance and as nothing for the sign).  Voxel (i, j, k) of the (X, Y, Z) grid sits at
 * (idx - shape / 2) * voxel_size + (cx, cy, cz), multiply and add rounded separately.  sdf[(i * Y + j) * Z + k] =
 * clamp(s * sqrt(min_f squared distance to triangle f), -trunc, trunc), s = -1 iff |generalised winding number| >= 0.5 (sum of the
 * van Oosterom-Strackee solid angles / 4 pi), else +1.  tri_cull != 0 skips the distance part of a triangle for a whole 4^3 brick
 * whose voxels it cannot bring below trunc (bit-identical output, faster).  workspace: pm_mesh_sdf_bake_workspace_bytes(F) bytes of
 * device memory (per-triangle records; contents undefined afterwards).  Deterministic: no atomics, fixed summation order.
 * PM_EINVAL: a NULL pointer, F <= 0, a non-positive shape, voxel_size or trunc, X * Y * Z >= 2^31, a workspace that is too small. */
size_t pm_mesh_sdf_bake_workspace_bytes(int F);
int pm_mesh_sdf_bake_f32(const float* tri, int F, int X, int Y, int Z, float voxel_size, float cx, float cy, float cz, float trunc,
                         int tri_cull, float* sdf, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ posed mesh point cloud (observation side)
 * utils/mesh2pc.py:56-65 `PCfromMesh.query_pc` in one launch, computing only the selected points.  pts (Q, 3): the canonical
 * surface points of all parts, concatenated; part_of (Q) int32: each point's part; pose_R (B, M, 3, 3), pose_T (B, M, 3).
 * sel: NULL = identity (requires K == Q); (K) int32 with sel_stride == 0 = one selection shared by all environments; (B, K) with
 * sel_stride >= K (in elements) = one selection per environment.  With q = sel[.. k], p = part_of[q], x = pts[q]:
 *   out[b * out_stride + 3 k + j] = ((x0 R[b,p,j,0] + x1 R[b,p,j,1]) + x2 R[b,p,j,2]) + T[b,p,j]
 * (the reference's bmm(all_pc, R^T) + T) in fp32, in exactly that association, every operation rounded on its own: the bits are
 * defined and repeat.  out_stride >= 3 K in elements; columns at and past 3 K of a row are not touched (the proprio tail of an
 * observation row); rows need 4-byte alignment only.  q outside [0, Q) or p outside [0, M): the point's three outputs are NaN and
 * nothing is read through that index.  A non-finite pose propagates; no address depends on it.  No workspace, no atomics,
 * stream-ordered, never synchronises.
 * PM_EINVAL: a NULL pts / part_of / pose_R / pose_T / out, B, M, Q or K < 1, B > 1048560 (65535 grid rows of 16 environments),
 * out_stride < 3 K, sel == NULL with K != Q, a non-zero sel_stride < K. */
int pm_mesh_pc_query_f32(const float* pts, const int32_t* part_of, int Q, const float* pose_R, const float* pose_T, int B, int M,
                         const int32_t* sel, long sel_stride, int K, float* out, long out_stride, void* stream);
/* The same cloud with a fourth column, the label of the point's part: labels (M) float32, one number per pose slot.
 *   out[b * out_stride + 4 k + j], j < 3: exactly what pm_mesh_pc_query_f32 defines for out[b * out_stride + 3 k + j]
 *   out[b * out_stride + 4 k + 3] = labels[p]
 * (the same kernel with four floats per point instead of three).  q outside [0, Q) or p outside [0, M): the point's FOUR outputs
 * are NaN and nothing is read through that index, labels included.  out_stride >= 4 K; columns at and past 4 K are not touched.
 * PM_EINVAL: as above with 4 K for 3 K, and a NULL labels. */
int pm_mesh_pc_query_labeled_f32(const float* pts, const int32_t* part_of, int Q, const float* pose_R, const float* pose_T, int B,
                                 int M, const int32_t* sel, long sel_stride, int K, float* out, long out_stride,
                                 const float* labels, void* stream);

/* ------------------------------------------------------------------ depth camera over the posed part meshes (observation side)
 * The producer of the depth observations of tasks/hand_base.py:312-343 (there: the simulator's camera sensors): out (B, V, H, W) =
 * z-depth (not ray length) of the nearest surface along the ray through each pixel centre, `far` where nothing is hit -- with
 * far = 100 the tensor that TSDFVolume.depth2pc / integrate / sparse_voxel take.  verts (NV, 3): canonical vertices of all parts,
 * concatenated; vert_part (NV) int32: each vertex's part; faces (F, 3) int32 into verts; pose_R (B, M, 3, 3), pose_T (B, M, 3) as
 * in pm_mesh_pc_query_f32; cam_pose (V, 4, 4) camera->world, the camera looking along +z with x right and y down (what
 * TSDFVolume.register_camera takes).  All arithmetic fp32, every product, sum and difference rounded on its own, divisions IEEE:
 *   world vertex of part j   xw = ((x0 R[j,0] + x1 R[j,1]) + x2 R[j,2]) + T[j]
 *   camera vertex            d = xw - C[:,3],  p_k = (d0 C[0,k] + d1 C[1,k]) + d2 C[2,k]
 *   triangle (p0, p1, p2)    n0 = p1 x p2, n1 = p2 x p0, n2 = p0 x p1, each component a b - c d in the usual order
 *   pixel (row r, column c)  dx = (float(c) - cx) / fx, dy = (float(r) - cy) / fy, w_i = (dx n_i.x + dy n_i.y) + n_i.z,
 *                            s = (w0 + w1) + w2
 *   hit                      iff w0, w1, w2 are all >= 0 or all <= 0 (both faces count, inclusive), s != 0 and
 *                            z = ((w0 p0.z + w1 p1.z) + w2 p2.z) / s satisfies near < z < far
 *   out[b * out_stride + (v H + r) W + c] = min z over the triangles that hit, else far.
 * The bits are defined and repeat: the minimum is order-free (integer min on the bits of the positive z, no float atomics), and
 * two triangles sharing an edge see exactly opposite edge values, so no crack opens between them.  A triangle is skipped when a
 * face index is outside [0, NV), a part outside [0, M) or a camera-space coordinate non-finite; nothing is read through a bad
 * index.  A triangle with a corner at z <= near is tested against the whole image.  out_stride >= V H W in elements; floats of a
 * row past V H W are not touched.  Two launches (fill, raster), no workspace, stream-ordered, never synchronises.
 * PM_EINVAL (before any launch): a NULL pointer, NV, F, B, M, V, H or W < 1, near <= 0, far <= near, out_stride < V H W,
 * W + H > 12288 (the per-block table of dx and dy), ceil(F / 256) V B >= 2^31. */
int pm_mesh_depth_render_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F,
                             const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V, float fx,
                             float fy, float cx, float cy, int H, int W, float near, float far, float* out, long out_stride,
                             void* stream);

/* ------------------------------------------------------------------ frame camera over the posed part meshes (depth, part label, colour)
 * The colour image and the IMAGE_SEGMENTATION image of the reference's camera sensors (tasks/hand_base.py:222-227, 355-357; the
 * robot's bodies carry id 1, load_robot.py:83), rendered from the posed part meshes.  Geometry, pose and camera arguments, the
 * arithmetic, the hit rule and z are those of pm_mesh_depth_render_f32 above, formula for formula.  Per pixel:
 *   winner                   the triangle f (its row in faces) of the smallest key (bits(z) << 32) | f over the triangles that hit:
 *                            nearer first, then the smaller face index -- the tie-break of coincident triangles and of pixel
 *                            centres exactly on a shared edge.  z > 0, so the unsigned order of the key is that order.
 *   miss (no triangle hits)  depth = far, seg = miss_label, rgb = (bg_r, bg_g, bg_b)
 *   hit                      depth = the winner's z: the bits pm_mesh_depth_render_f32 writes
 *                            p = vert_part[faces[3 f]];  seg = part_label[p], or p when part_label is NULL
 *   shade (p0, p1, p2 the winner's camera vertices as above; every product, sum and difference rounded on its own, sqrt and / IEEE)
 *                            e1 = p1 - p0,  e2 = p2 - p0,  g = e1 x e2 (each component a b - c d in the usual order)
 *                            q = (gx gx + gy gy) + gz gz
 *                            l = |gz| / sqrt(q) if q > 0 and q is finite, else 0     (a headlight along the optical axis, two-sided)
 *                            k = ambient + one_minus_ambient l
 *                            rgb[c] = (uint8)(int)(palette[p][c] k + 0.5f)            palette (M, 3) float32 in [0, 255]
 *   depth[b * depth_stride + (v H + r) W + c], seg[b * seg_stride + (v H + r) W + c], rgb[b * rgb_stride + 3 ((v H + r) W + c) + ch]
 * Every output is a function of (triangles, pixel) alone: the bits of all three are defined and repeat; a numpy float32 evaluation
 * of these lines gives the same bytes.  The headlight and the palette are this project's choices, not Isaac Gym's renderer.
 * Each of depth, seg and rgb may be NULL (not all three); palette may be NULL only when rgb is.  Strides are per environment, in
 * elements (depth, seg: >= V H W) or bytes (rgb: >= 3 V H W); nothing past those columns of a row is written.  Skipped triangles
 * as in pm_mesh_depth_render_f32: they never win a pixel.  workspace: pm_mesh_frame_workspace_bytes(B, V, H, W) = 8 B V H W bytes
 * of 64-bit keys, 8-byte aligned, caller-owned; its content before and after the call is unspecified.  Three launches (fill,
 * raster, resolve) on `stream`; 64-bit integer atomicMin, no float atomics; never synchronises.
 * Before any launch -- PM_EINVAL: the conditions of pm_mesh_depth_render_f32 (with "out" read as: depth, seg and rgb all NULL, or
 * a given output's stride too short), rgb without palette, ambient or one_minus_ambient < 0 or their sum > 1 (or NaN), a
 * background component outside [0, 255]; PM_EWORKSPACE: workspace NULL or workspace_bytes too small; PM_EALIGN: workspace not
 * 8-byte aligned. */
size_t pm_mesh_frame_workspace_bytes(int B, int V, int H, int W);
int pm_mesh_frame_render_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F,
                             const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V, float fx,
                             float fy, float cx, float cy, int H, int W, float near, float far, const int32_t* part_label,
                             int miss_label, const float* palette, float ambient, float one_minus_ambient, int bg_r, int bg_g,
                             int bg_b, float* depth, long depth_stride, int32_t* seg, long seg_stride, uint8_t* rgb,
                             long rgb_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ the two cameras over a scene whose environments differ
 * pm_mesh_depth_render_groups_f32 / pm_mesh_frame_render_groups_f32: the arguments of the two entries above plus a partition of the
 * rows of `faces` into a shared range and G groups, and one group per environment (open_drawer: env % num_objs is its cabinet).
 *   F_shared                 rows [0, F_shared) of faces are drawn by every environment
 *   group_off (G + 1) int32  rows relative to F_shared, non-decreasing, group_off[0] = 0, group_off[G] = F - F_shared
 *   env_group (B) int32      g = env_group[b] in [0, G): environment b also draws rows [F_shared + group_off[g],
 *                            F_shared + group_off[g + 1]); g = -1: the shared rows only
 *   max_group_faces          an upper bound of the rows of a group, max_g (group_off[g + 1] - group_off[g]); it sizes the grid
 * Definition: the image of environment b is the definition of the ungrouped entry applied to that subset of faces -- the same fp32
 * association, hit rule, near / far; the frame's winner is the nearest triangle, a tie goes to the smaller row of faces (the key
 * keeps the row in faces, so depth, seg and rgb are those of the ungrouped entry called with the subset in row order, and the
 * resolve launch is unchanged).  vert_part keeps its meaning: a vertex names its pose slot, a static property of the vertex, equal
 * in every environment that draws it; what differs between environments is which rows are drawn and the poses in the slots.
 * Launch shape: one lane per (environment, view, face ordinal t < F_shared + max_group_faces); t < F_shared is row t, else row
 * F_shared + group_off[g] + (t - F_shared) while that lies in the group.  An environment pays the set-up of its own triangles only.
 * Memory safety: g outside [-1, G) counts as -1; a group's rows are clamped to [F_shared, F); at most max_group_faces rows of a
 * group are drawn (a bound that is too small drops the group's last rows, it reads nothing out of range); nothing is read through
 * a bad index.  No float atomics, no workspace beyond the frame camera's keys, stream-ordered, never synchronises.
 * Before any launch -- PM_EINVAL: every condition of the ungrouped entry (its grid condition read with F_shared + max_group_faces in
 * place of F), F_shared outside [0, F], G < 0, max_group_faces < 0, a NULL group_off or env_group with G > 0; PM_EWORKSPACE and
 * PM_EALIGN as above.  PM_ABI_VERSION stays 163 with these additions (no existing signature changed). */
int pm_mesh_depth_render_groups_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F, int F_shared,
                                    const int32_t* group_off, int G, const int32_t* env_group, int max_group_faces,
                                    const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V, float fx,
                                    float fy, float cx, float cy, int H, int W, float near, float far, float* out, long out_stride,
                                    void* stream);
int pm_mesh_frame_render_groups_f32(const float* verts, const int32_t* vert_part, int NV, const int32_t* faces, int F, int F_shared,
                                    const int32_t* group_off, int G, const int32_t* env_group, int max_group_faces,
                                    const float* pose_R, const float* pose_T, int B, int M, const float* cam_pose, int V, float fx,
                                    float fy, float cx, float cy, int H, int W, float near, float far, const int32_t* part_label,
                                    int miss_label, const float* palette, float ambient, float one_minus_ambient, int bg_r, int bg_g,
                                    int bg_b, float* depth, long depth_stride, int32_t* seg, long seg_stride, uint8_t* rgb,
                                    long rgb_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ body poses of a whole scene (the cameras' pose input)
 * rigid_body (nrows, 13) flat rows (position, quaternion (i, j, k, r), velocities); rows (B, M) int32: slot m of environment b is
 * row rows[b, m]; part_C (MC, 3, 3) or NULL with MC = 0: the mesh-frame matrices of the first MC slots.
 *   pose_T[b, m] = the row's position
 *   pose_R[b, m] = quat_to_mat(q) for m >= MC, and for m < MC
 *   pose_R[b, m][i][j] = (Q[i][0] C_m[0][j] + Q[i][1] C_m[1][j]) + Q[i][2] C_m[2][j]
 * with quat_to_mat and the product exactly as the task kernels compute them (pm_grasp_cube_post_f32), so a slot both produce carries
 * the same bits.  A row index outside [0, nrows) gives a NaN pose and its address is never formed (the cameras skip a triangle
 * with a non-finite corner).  One launch, no workspace, no atomics, stream-ordered, never synchronises.
 * PM_EINVAL: a NULL rigid_body / rows / pose_R / pose_T, nrows, B or M < 1, MC outside [0, M], MC > 0 with a NULL part_C.
 * PM_ABI_VERSION stays 163 with this addition. */
int pm_body_pose_gather_f32(const float* rigid_body, long nrows, const int32_t* rows, int B, int M, const float* part_C, int MC,
                            float* pose_R, float* pose_T, void* stream);

/* ------------------------------------------------------------------ grasp_cube task step (simulator side of the learner)
 * The tensor program of the reference's task layer (tasks/grasp_cube.py, tasks/load_robot.py, tasks/hand_base.py:363-392, 431-441)
 * as one launch after physics and one before it.  Neither synchronises, allocates or uses float atomics; both are stream-ordered.
 *
 * pm_grasp_cube_post_f32 = grasp_cube.compute_observations + franka.update_state + grasp_cube.compute_reward + compute_scene_pose.
 * Inputs (contiguous): rigid_body (N, nb, 13), dof_state (N, nd, 2), root (N, na, 13) whose actor obj_actor is the object;
 * ltip / rtip: the two finger-tip bodies; dof_lo / dof_hi (nd); pose_lo / pose_hi (7); goal (3); obj_default_pos (3);
 * part_body (M) int32 and part_C (M, 3, 3) or NULL (identity) for the pose outputs.  With tip = (rb[ltip] + rb[rtip]) / 2 over all
 * 7 pose entries, scale(x) = 2 (x - lo) / (hi - lo) - 1, quat_to_mat in the order (i, j, k, r) with two_s = 2 / sum q^2 and no
 * normalisation, D(q) = the candidate of largest trace among the 24 signed column pairs of quat_to_mat(q) (lowest index on ties):
 *   normal_state (N, 19 + 2 nd) = [scale(tip[:7]) | scale(obj_pos) | D(obj_quat) row-major | qpos_normalized | qvel]
 *   proprio (N, 7 + 2 nd)       = [scale(tip[:7]) | qpos_normalized | qvel]
 *   rew (N) = reaching + 0.5 rot + 5 close + 20 reaching_goal + 3 success;  success, is_reached (N) bytes
 *   extras (N, 8) = reaching_reward, close_reward, rot_reward, reaching_goal_reward, obj_movement, raw_reward, obj_height, obj_up_flag
 *   pose_T (N, M, 3) = rb[b, part_body[p], :3];  pose_R (N, M, 3, 3) = quat_to_mat(rb[b, part_body[p], 3:7]) C_p
 * Every output may be NULL (skipped).  normal_state, proprio and extras take a row stride in elements (column views of a wider
 * observation buffer; 4-byte alignment only); nothing outside the named columns is written.  A part_body entry outside [0, nb) gives
 * NaN poses for that part and is never dereferenced.  An environment's outputs depend on its own rows only and do not depend on N.
 * PM_EINVAL: a NULL input, N, nb, nd, na < 1, an index outside its range, a row stride below the row width, pose outputs without
 * part_body or with M < 1, nb or nd too large for the kernel's staging (nb * 13 + nd * 2 > 12000).
 *
 * pm_franka_control_f32 = franka.control + solve_ik + hand_base.pre_physics_step:365-375 + the buffer part of grasp_cube.reset_idx.
 * actions (N, A) with a row stride; jac (N, nl, 6, nd), link rows jl and jr (NULL allowed with drive_mode 1).  drive_mode 0 = 'ik'
 * (A == 7): dpose = 0.005 a[:6], J = (jac[jl] + jac[jr]) / 2 over DOFs [0, nd - 2), arm = qpos + J^T (J J^T + 0.05^2 I)^-1 dpose
 * (Cholesky, fp32), both fingers = qpos + a[6] dt / 5; drive_mode 1 = 'pos' (A == nd - 1): arm = qpos + a[:nd-2] dt 20, fingers =
 * qpos + a[nd-2] dt; clamped to [dof_lo, dof_hi] (NaN propagates).  Then, in the reference's order, with rew / success of the
 * previous post step: train != 0: epis_max_step = rew < epis_max_rew ? epis_max_step : progress; epis_max_rew = max(rew,
 * epis_max_rew); reset = progress >= epis_max_step + explore_step | success; reset_succ = success.  train == 0: reset = progress >=
 * max_episode_length.  Environments being reset: pos_act = default_dof_pos, progress = 0, success = 0, epis_max_rew = -100,
 * epis_max_step = 0.  counters: 4 int32; this call ADDS the number of set success bytes (before the reset) to counters[2 slot] and
 * the number of resets to counters[2 slot + 1] and ZEROES the other pair, so a caller that starts from zeros and alternates slot =
 * 0, 1, 0, ... reads this step's two sums from its own pair without a clearing launch.
 * PM_EINVAL: a NULL pointer (jac with drive_mode 0), N < 1, nd < 3 or > 64, A not as stated, jl / jr outside [0, nl), slot not 0 / 1,
 * an unknown drive_mode, act_stride < A.
 *
 * pm_franka_control_mobile_f32 = the same launch for the mobile Franka (load_robot.py:97-101, 112-113 with `mobile`): nbase = 3
 * virtual prismatic base joints in front of the arm, so the arm is DOFs [nbase, nd - 2) and the action row is [base 3 | arm | gripper].
 * base_R (3, 3) row-major in device memory = quat_to_mat of the robot's default root quaternion.  Per environment that is not
 * resetting, a = its action row, q = its DOF positions, db = 0.005 a[0:3]:
 *   base: target[i] = q[i] + sum_j base_R[j][i] db[j], i < 3 (base_R transposed times db, summed left to right)
 *   drive_mode 1 = 'pos' (A == nd - 1): arm k in [nbase, nd - 2): q[k] + a[k] dt 20; fingers = q + a[A - 1] dt
 *   drive_mode 0 = 'ik' (A == 7 + nbase), b = a[nbase:]: dpose = 0.005 b[0:6], dpose[0:3] -= db; J = (jac[jl] + jac[jr]) / 2 over the
 *   columns [nbase, nd - 2) only (the base's columns are never read); arm = q[nbase:nd-2] + J^T (J J^T + 0.05^2 I)^-1 dpose;
 *   fingers = q + b[6] dt / 5
 * every target clamped to [dof_lo, dof_hi] (NaN propagates); resetting environments get default_dof_pos over all nd DOFs.  The
 * bookkeeping, the counter slots and the stream ordering are those of pm_franka_control_f32: one launch, no synchronisation, no
 * allocation.  PM_EINVAL: nbase != 3 (nbase == 0 is pm_franka_control_f32), base_R NULL, nd < nbase + 3 or > 64, A not as stated, and
 * everything pm_franka_control_f32 refuses. */
int pm_grasp_cube_post_f32(const float* rigid_body, const float* dof_state, const float* root, int N, int nb, int nd, int na,
                           int obj_actor, int ltip, int rtip, const float* dof_lo, const float* dof_hi, const float* pose_lo,
                           const float* pose_hi, const float* goal, float goal_thresh, const float* obj_default_pos,
                           const int32_t* part_body, const float* part_C, int M, float* normal_state, long ns_stride,
                           float* proprio, long pr_stride, float* rew, uint8_t* success, uint8_t* is_reached, float* extras,
                           long ex_stride, float* pose_R, float* pose_T, void* stream);
int pm_franka_control_f32(const float* actions, long act_stride, int A, const float* dof_state, const float* jac, int N, int nd,
                          int nl, int jl, int jr, const float* dof_lo, const float* dof_hi, const float* default_dof_pos, float dt,
                          int drive_mode, const float* rew, uint8_t* success, int64_t* progress, int explore_step,
                          int max_episode_length, int train, float* pos_act, float* epis_max_rew, int64_t* epis_max_step,
                          uint8_t* reset, uint8_t* reset_succ, int32_t* counters, int slot, void* stream);
int pm_franka_control_mobile_f32(const float* actions, long act_stride, int A, const float* dof_state, const float* jac, int N,
                                 int nd, int nl, int jl, int jr, const float* dof_lo, const float* dof_hi,
                                 const float* default_dof_pos, float dt, int drive_mode, int nbase, const float* base_R,
                                 const float* rew, uint8_t* success, int64_t* progress, int explore_step, int max_episode_length,
                                 int train, float* pos_act, float* epis_max_rew, int64_t* epis_max_step, uint8_t* reset,
                                 uint8_t* reset_succ, int32_t* counters, int slot, void* stream);

/* ------------------------------------------------------------------ open_drawer task step (heterogeneous environments)
 * The tensor program of the reference's tasks/open_drawer.py (compute_observations, compute_reward, reset_idx) with
 * load_robot.update_state: one launch after physics, one before it next to pm_franka_control_f32.  Neither synchronises, allocates
 * or uses atomics; both are stream-ordered.
 *
 * Every environment holds another cabinet, so the simulator's tensors are flat: rigid_body_all (B, 13), dof_state_all (D, 2), root
 * (N, na, 13), contiguous.  rigid_body_mask (N, nrb + 2) and dof_state_mask (N, nd + 1) int32 are row indices into them: the robot's
 * nrb bodies, then the target link and the handle; the robot's nd DOFs, then the target joint.  Per environment: part_bbox_init
 * (N, 8, 3), part_axis_dir_init (N, 3), joint_lo / joint_hi (N), obj_id (N) int32 in [0, num_objs).
 *
 * pm_open_drawer_post_f32.  Row g[s] = rigid_body_all[rigid_body_mask[e, s]], d[k] = dof_state_all[dof_state_mask[e, k]], q = d[nd][0]:
 *   tip (13) = (g[ltip] + g[rtip]) / 2 (quaternion included: not unit);  gripper_length = |g[ltip][:3] - g[rtip][:3]|
 *   part_bbox (N, 8, 3) = (part_bbox_init + q axis) R(obj quat)^T + obj pos, R = quat_to_mat of the object's root quaternion
 *   out = b0 - b4, long = b1 - b0, short = b3 - b0 (each normalised, lengths kept), mid = (b0 + b6) / 2
 *   normal_state (N, 29 + 2 nd) = [tip 13 | mid 3 | out 3 | short 3 | long 3 | |out| |long| |short| | qpos_normalized nd | qvel nd | q]
 *   delta = tip[:3] - mid;  reached_out = |delta . out| < |out| / 2;  reached_long likewise;  reached_short = ((g[ltip][:3] - mid) .
 *   short) ((g[rtip][:3] - mid) . short) < 0;  is_reached = all three;  reaching = -|delta| + 0.1 (any of the three)
 *   axes by quat_rotate(tip[3:7], e) = e (2 w^2 - 1) + 2 w (q x e) + 2 q (q . e): grip = e_z, sep = e_y, down = e_x
 *   rot = -grip . out + max(sep . short, -sep . short) + max(down . long, -down . long) - 3
 *   close = (0.1 - gripper_length) is_reached + 0.1 (gripper_length - 0.1) (not is_reached)
 *   is_grasped = is_reached and gripper_length < |short| + 0.01 and rot > -0.2;  frac = (q - joint_lo) / joint_hi
 *   joint_state = is_grasped (0.1 + min(frac, suc_prop));  is_open_notgrasp = frac > 0.1;  is_open = is_grasped and is_open_notgrasp
 *   base = reaching + 0.5 rot + 5 close + 5 joint_state;  success = is_grasped and q - joint_lo >= suc_prop joint_hi
 *   rew = base + |base| rot + 2 success;  min / max propagate NaN, comparisons with NaN are false
 *   extras (N, 8) = is_open, is_open_notgrasp, reaching_reward, close_reward, rot_reward, joint_state_reward, raw_reward, is_grasped
 *   succ_objid (num_objs) bytes: succ_objid[obj_id[e]] = 1 where success (sticky: never cleared here)
 *   robot_dof_state (N, nd, 2) = d[:nd], part_dof_state (N, 2) = d[nd]: the gathered rows, bit for bit
 *   pose_T (N, M, 3) = g[part_slot[p]][:3];  pose_R (N, M, 3, 3) = quat_to_mat(g[part_slot[p]][3:7]) C_p (part_C NULL: identity)
 * Every output may be NULL (skipped).  normal_state and extras take a row stride in elements; nothing outside the named columns is
 * written.  A mask entry outside its tensor reads as NaN and a part_slot entry outside [0, nrb + 2) gives NaN poses; neither is
 * dereferenced; an obj_id outside [0, num_objs) sets no flag.  An environment's outputs depend on its own rows only.
 * PM_EINVAL: a NULL input, N, nrb, nd, na, B, D < 1, B or D >= 2^31, an index outside its range, a row stride below the row width,
 * succ_objid without obj_id or with num_objs < 1, pose outputs without part_slot or with M < 1, rows too large for the staging.
 *
 * pm_open_drawer_reset_f32 = the state half of open_drawer.reset_idx, after pm_franka_control_f32 wrote pos_act (N, nd) and reset (N).
 * Every environment: pos_act_all[dof_state_mask[e, k]] = pos_act[e, k], k < nd.  Environments with reset[e] != 0, in place:
 *   root[e, robot_actor, :7] = robot_default_root;  root[e, obj_actor, :7] = obj_default_root;  root[e, :, 7:] = 0
 *   random_reset != 0, u (N, 4) in [0, 1): position += u[:3] t_range 2 - t_range;  quaternion = quat_mul(default, (0, 0, sin a, cos a)),
 *   a = u[3] r_range 2 - r_range, quat_mul in Isaac Gym's association
 *   dof_state_all[dof_state_mask[e, k]] = (default_dof_pos[k], 0), k < nd;  dof_state_all[dof_state_mask[e, nd]] = (joint_lo[e], 0)
 *   robot_dof_state[e] and part_dof_state[e] (either may be NULL) receive the same values
 * Nothing else is written: other environments' rows and a cabinet's other joints stay as they are.  dof_state_mask must not name a
 * row twice (the writes would race); entries outside [0, D) are skipped.
 * PM_EINVAL: a NULL pointer (u with random_reset), N, nd, na, D < 1, D >= 2^31, an actor outside [0, na), robot_actor == obj_actor. */
int pm_open_drawer_post_f32(const float* rigid_body_all, long B, const float* dof_state_all, long D, const float* root, int N, int nrb,
                            int nd, int na, int obj_actor, int ltip, int rtip, const int32_t* rigid_body_mask,
                            const int32_t* dof_state_mask, const int32_t* obj_id, int num_objs, const float* part_bbox_init,
                            const float* part_axis_dir_init, const float* joint_lo, const float* joint_hi, const float* dof_lo,
                            const float* dof_hi, float suc_prop, const int32_t* part_slot, const float* part_C, int M,
                            float* normal_state, long ns_stride, float* rew, uint8_t* success, uint8_t* is_reached, float* part_bbox,
                            float* extras, long ex_stride, uint8_t* succ_objid, float* robot_dof_state, float* part_dof_state,
                            float* pose_R, float* pose_T, void* stream);
int pm_open_drawer_reset_f32(const uint8_t* reset, const float* pos_act, const int32_t* dof_state_mask, int N, int nd, int na,
                             int robot_actor, int obj_actor, const float* robot_default_root, const float* obj_default_root,
                             int random_reset, const float* u, float t_range, float r_range, const float* default_dof_pos,
                             const float* joint_lo, float* root, float* dof_state_all, long D, float* pos_act_all,
                             float* robot_dof_state, float* part_dof_state, void* stream);

/* ------------------------------------------------------------------ kinematic articulation (a stand-in for the simulator's robot)
 * The producer of the three tensors the task steps start from, for one robot per environment: position targets in, dof_state,
 * rigid-body rows and the Jacobian out, in one launch (csrc/articulation.hip).  Kinematics only: no dynamics, contact or gravity.
 * The tree (partmanip_amd/urdf.py; bodies ordered so that a parent precedes its children, DOFs numbered in body order):
 *   parent, jtype, dof (nb) int32: the parent body (-1: the root, which hangs off base_pose), 0 fixed / 1 revolute / 2 prismatic,
 *   the joint's DOF (-1 for a fixed joint);  origin_q (nb, 4) unit (x, y, z, w), origin_t (nb, 3): the joint origin in the parent's
 *   frame;  axis (nb, 3) unit, in the joint's frame;  anc_mask (nb) 64-bit: bit d set where DOF d lies on the body's path to the root.
 * dof_lo, dof_hi (nd);  vmax (nd) or NULL (exact tracking);  base_pose: 7 floats per environment, position and quaternion (x, y, z, w),
 * base_stride floats apart (0: one pose for all); the quaternion is divided by its norm.
 * dof_state: rows of (q, qd), dof_rows rows in all; environment e's nd rows start at row dof_row0[e], or at e * dof_stride with
 * dof_row0 NULL.  rigid_body: rows of 13, rb_rows in all, environment e's nb rows from rb_row0[e] or e * rb_stride.  So the robot may
 * sit inside a wider (N, nb_total, 13) tensor or inside flat (B, 13) / (D, 2) tensors; no other row is touched.  An environment whose
 * rows would not lie inside [0, rows) is computed as NaN and stores no dof_state / rigid_body row.
 * Per environment, with targets (N, nd) (row stride tgt_stride) given, dof_state is updated in place:
 *   q' = q + clamp(t - q, -vmax dt, vmax dt) (vmax NULL: q' = t), then q' = clamp(q', dof_lo, dof_hi);  qd' = (q' - q) / dt
 *   reset (N) bytes, where given and set: q' = clamp(t, dof_lo, dof_hi), qd' = 0, whatever vmax is
 *   clamp passes a NaN through.  targets NULL: dof_state is only read (q' = q, qd' = qd): pure forward kinematics.
 * Body frame = parent o origin o joint, in quaternion arithmetic (the chain of frames in float64, rounded to float32 once per body),
 * each body's quaternion divided by its norm; the joint is a
 * rotation by q' about axis (revolute) or a translation by q' axis (prismatic).
 * jac (N, nb - 1, 6, nd): the world-frame geometric Jacobian at the body origin, row l = body l + 1, rows 0-2 linear, 3-5 angular;
 * column d is exactly 0 unless bit d of the body's anc_mask is set, else (a x (p_body - p_joint), a) for a revolute DOF and (a, 0)
 * for a prismatic one, a = the joint axis in the world.  rigid_body row = position 3, quaternion 4, linear velocity 3 = J[:3] qd',
 * angular velocity 3 = J[3:] qd' (the root body: 0).  rigid_body and jac may each be NULL (skipped).
 * An environment's outputs depend on its own rows only and do not depend on N.  No synchronisation, allocation or atomics;
 * stream-ordered.  PM_EINVAL: a NULL required pointer (every table, the limits, base_pose, dof_state), N < 1, nb or nd outside
 * [1, 64], a stride below its row width (base_stride other than 0 below 7, tgt_stride < nd, rb_stride < nb, dof_stride < nd), rows
 * that N environments at the given stride would not fit, dt <= 0 with targets.  The tables' contents are the caller's to validate. */
int pm_articulation_step_f32(const int32_t* parent, const int32_t* jtype, const int32_t* dof, const float* origin_q,
                             const float* origin_t, const float* axis, const uint64_t* anc_mask, const float* dof_lo,
                             const float* dof_hi, const float* vmax, float dt, const float* base_pose, long base_stride,
                             float* dof_state, long dof_rows, const float* targets, long tgt_stride, const uint8_t* reset,
                             const int32_t* rb_row0, long rb_stride, long rb_rows, const int32_t* dof_row0, long dof_stride, int N,
                             int nb, int nd, float* rigid_body, float* jac, void* stream);

/* ------------------------------------------------------------------ contact blocking: a swept test of one kinematic step
 * pm_articulation_sweep_f32 / pm_articulation_sweep_groups_f32 (csrc/articulation_sweep.hip): how far along this step can the robot
 * go before one of its sensing points enters a target grid.  One launch, one work-group per environment; it writes no state.  A
 * stated rule, not physics: nothing slides, bounces or is pushed -- the robot stops short of contact.
 * Arguments, each meaning what it means in the entry it comes from:
 *   pm_articulation_step_f32: the tree tables (anc_mask is not needed), dof_lo, dof_hi, vmax or NULL, dt, base_pose / base_stride,
 *     dof_state / dof_rows / dof_row0 / dof_stride (ONLY READ here), targets / tgt_stride (required), reset or NULL, N, nb, nd;
 *   pm_mesh_sdf_points(_groups)_f32: the part tables, (the group tables and max_group_grids,) pose_R, pose_T (the caller's scene
 *     pose table, N x M slots), M, p0, p1 (t0, t1), pts, pts_env_stride, carrier, pt_id, chunk_sphere, NP, seg_off, NS >= 1, cull;
 *   slot_body (M) int32   the robot-local body in [0, nb) whose frame places pose slot m; -1: the slot's pose is the table's;
 *                         any other value: the slot's pose is NaN (what a row outside the rigid-body tensor gives the gather)
 *   slot_C (MC <= M, 3, 3) or NULL with MC = 0   the part_C of pm_body_pose_gather_f32
 *   S in [1, 63]          the number of parts the step is cut into
 *   block_margin          the distance at or below which a candidate counts as contact
 *   free_env (N) bytes or NULL   environments that are not guarded
 * Outputs: sweep_dist (N, S + 1) float32, steps (N) int32, targets_out (N, nd) float32 (contiguous).
 * Definition.  Every fp32 operation is one correctly rounded operation, no contraction.
 *   1. q' = the drive rule of pm_articulation_step_f32, operation for operation: reset[b] set: clamp(t, lo, hi); else
 *      clamp(q + clamp(t - q, -vmax dt, vmax dt), lo, hi), or clamp(t, lo, hi) with vmax NULL.  clamp passes a NaN through.
 *   2. candidates k = 0 .. S:  a_k = (float)k / (float)S;  q_0 = clamp(q, lo, hi);  q_S = q';
 *      q_k = clamp(q + a_k (q' - q), lo, hi) for 0 < k < S.
 *   3. the candidate's pose table P_k = the caller's table, except that a slot m with slot_body[m] >= 0 takes the pose that
 *      pm_body_pose_gather_f32 computes (part_C = slot_C) from the rigid-body row that pm_articulation_step_f32 writes for the joint
 *      state q_k: the same float64 chain rounded once, quat_to_mat, the C product in the same association.
 *   4. sweep_dist[b, k] = the minimum over the NS segments, NaN wins, of the seg_min that pm_mesh_sdf_points(_groups)_f32 returns on
 *      P_k, by its rules 1 to 7 (the NaN-pose rule, padding ids, carriers outside [-1, M), cull on = cull off).
 *   5. candidate k >= 1 is admissible iff D_k > block_margin or D_k >= D_{k-1} (D = sweep_dist[b]): a robot already in contact
 *      may move away or along, never deeper.  A NaN is not admissible.
 *   6. steps[b] = the largest K such that candidates 1 .. K are all admissible (0 if candidate 1 is not); forced to S where
 *      reset[b] or free_env[b] is set (sweep_dist is written for those environments all the same).
 *   7. targets_out[b] = q_steps[b].  Passed as the targets of pm_articulation_step_f32 with vmax NULL and the same reset, the
 *      executed joint state is that candidate bit for bit (clamp is idempotent).
 * So sweep_dist[:, k] has the bits of the three existing entries run one after the other on q_k, two runs give the same bits (no
 * floating-point atomics, ordinary vector stores only), and an environment's outputs depend on its own rows only: not on N or on
 * the block it lands in; a NaN target, joint or pose stays in its environment (a NaN candidate is not admissible: steps = 0 from
 * a NaN target).  An environment whose DOF rows would not lie inside [0, dof_rows) reads none and is NaN throughout.
 * Memory safety as in the two entries; no address is formed from an unchecked slot_body.  No synchronisation or allocation.
 * PM_EINVAL (before any launch): what pm_articulation_step_f32 refuses of its arguments (with targets required and dt > 0), what
 * pm_mesh_sdf_points(_groups)_f32 refuses of theirs (with NS >= 1 required), a NULL slot_body or output, MC outside [0, M], MC > 0
 * with a NULL slot_C, S outside [1, 63], a NaN block_margin, or (S + 1) ((7 nb | 1) 8 + 4 nd) bytes of LDS above 57344 (the Franka's
 * 13 bodies fit S = 63; 64 bodies and DOFs fit S = 13).  PM_ABI_VERSION stays 163 with these additions (no existing signature changed). */
int pm_articulation_sweep_f32(const int32_t* parent, const int32_t* jtype, const int32_t* dof, const float* origin_q,
                              const float* origin_t, const float* axis, const float* dof_lo, const float* dof_hi, const float* vmax,
                              float dt, const float* base_pose, long base_stride, const float* dof_state, long dof_rows,
                              const float* targets, long tgt_stride, const uint8_t* reset, const int32_t* dof_row0, long dof_stride,
                              int N, int nb, int nd, const float* fields, const int64_t* part_off, const int32_t* part_shape,
                              const float* part_bbox_min, const float* part_voxel_size, const float* pose_R, const float* pose_T, int M,
                              int p0, int p1, const float* pts, long pts_env_stride, const int32_t* carrier, const int32_t* pt_id,
                              const float* chunk_sphere, int NP, const int32_t* seg_off, int NS, int cull, const int32_t* slot_body,
                              const float* slot_C, int MC, int S, float block_margin, const uint8_t* free_env, float* sweep_dist,
                              int32_t* steps, float* targets_out, void* stream);
int pm_articulation_sweep_groups_f32(const int32_t* parent, const int32_t* jtype, const int32_t* dof, const float* origin_q,
                                     const float* origin_t, const float* axis, const float* dof_lo, const float* dof_hi,
                                     const float* vmax, float dt, const float* base_pose, long base_stride, const float* dof_state,
                                     long dof_rows, const float* targets, long tgt_stride, const uint8_t* reset,
                                     const int32_t* dof_row0, long dof_stride, int N, int nb, int nd, const float* fields,
                                     const int64_t* part_off, const int32_t* part_shape, const float* part_bbox_min,
                                     const float* part_voxel_size, const int32_t* grid_slot, int NG, int NG_shared,
                                     const int32_t* group_off, int G, const int32_t* env_group, int max_group_grids,
                                     const float* pose_R, const float* pose_T, int M, int t0, int t1, const float* pts,
                                     long pts_env_stride, const int32_t* carrier, const int32_t* pt_id, const float* chunk_sphere,
                                     int NP, const int32_t* seg_off, int NS, int cull, const int32_t* slot_body, const float* slot_C,
                                     int MC, int S, float block_margin, const uint8_t* free_env, float* sweep_dist, int32_t* steps,
                                     float* targets_out, void* stream);

/* ------------------------------------------------------------------ kinematic objects (a stand-in for the simulator's cabinets)
 * One articulated object per environment, each environment a tree of its own out of a library of K, posed into the flat
 * rigid_body (rb_rows, 13) and dof_state (dof_rows, 2) in one launch (csrc/articulation_objects.hip).  Kinematics only: no dynamics,
 * contact, gravity or friction.  The library is K trees of pm_articulation_step_f32 laid end to end:
 *   body_off, dof_off (K + 1) int32: tree k owns bodies [body_off[k], body_off[k + 1]) and DOFs [dof_off[k], dof_off[k + 1]) of
 *   parent, jtype, dof, origin_q, origin_t, axis, anc_mask (total_bodies rows) and dof_lo, dof_hi (total_dofs); parent and dof are
 *   LOCAL to their tree, and each tree obeys that entry's rules (root first, a parent precedes its children, at most 64 x 64).
 *   max_nb, max_nd: the largest body and DOF count of the library (they size the launch; a tree above them is skipped).
 * Per environment e: obj_type[e] in [0, K);  its pose, 7 floats at obj_pose + e * pose_stride (0: one pose for all), the quaternion
 * divided by its norm (root[:, obj_actor, :7] with pose_stride = na * 13);  obj_rb_row0[e] / obj_dof_row0[e]: the first of its
 * nb_k rows of rigid_body / nd_k rows of dof_state.  order (N) int32 or NULL: a permutation of the environments, grouped by type
 * (kinematics.ObjectLibrary.order_of), that only chooses which lane computes which environment; the results do not depend on it.
 * Output: environment e's nb_k body rows in pm_articulation_step_f32's format and by its rules: position and quaternion from the same
 * float64 chain rounded once (a tree gives the same bits through either entry), linear and angular velocity = J qd over the
 * ancestor DOFs, summed in ascending order.  No Jacobian is written.
 * The hold group, all NULL (dof_state is only read: pure forward kinematics) or all given with dt > 0: hold, reset (N) bytes,
 * target_dof (N) int32 local to the object, tip_rows (N, 2) int32: rows of rigid_body (the robot's left and right tip, which this
 * launch must not write: they are read as they stand when it runs, i.e. after the robot's launch on the same stream).  Then for
 * the target DOF, (q, qd) being its row:
 *   hold[e] set and reset[e] not:  p, v = the means of the two tip rows' positions and linear velocities;  a = the joint's world axis,
 *     p_j = the origin of its body (neither depends on q);  c = a (prismatic) or a x (p - p_j) (revolute);
 *     dq = dt (c . v) / (c . c), 0 where c . c == 0 (float64);  q' = clamp(float(q + dq), lo, hi);  qd' = (q' - q) / dt
 *   otherwise:  q' = q, qd' = 0
 *   and (q', qd') is written to the target row.  No other DOF row is ever written.  clamp passes a NaN through.
 * An environment's bits depend on its own rows only: not on N, on order, on its neighbours' types or on the block it lands in; a NaN
 * stays in its environment.  No synchronisation, allocation or atomics; stream-ordered.  An environment whose obj_type is outside
 * [0, K), whose offsets do not lie inside the tables, whose rows would not lie inside [0, rows), or (hold group given) whose
 * target_dof is outside [0, nd_k) or whose tip rows are outside [0, rb_rows) stores nothing and reads nothing out of range.
 * PM_EINVAL: a NULL required pointer (every table, obj_type, obj_pose, both row tables, dof_state, rigid_body), N or K < 1, max_nb or
 * max_nd outside [1, 64], total_bodies or total_dofs < 1, pose_stride other than 0 below 7, rows < 1 or >= 2^31, a hold group given
 * in part, dt <= 0 with it.  The tables' contents are the caller's to validate. */
int pm_articulation_objects_step_f32(const int32_t* body_off, const int32_t* dof_off, int K, int total_bodies, int total_dofs,
                                     int max_nb, int max_nd, const int32_t* parent, const int32_t* jtype, const int32_t* dof,
                                     const float* origin_q, const float* origin_t, const float* axis, const uint64_t* anc_mask,
                                     const float* dof_lo, const float* dof_hi, const int32_t* obj_type, const int32_t* order,
                                     const float* obj_pose, long pose_stride, const int32_t* obj_rb_row0, const int32_t* obj_dof_row0,
                                     float* dof_state, long dof_rows, float* rigid_body, long rb_rows, const uint8_t* hold,
                                     const uint8_t* reset, const int32_t* target_dof, const int32_t* tip_rows, float dt, int N,
                                     void* stream);

/* ------------------------------------------------------------------ kinematic free body (a stand-in for the simulator's cube)
 * One free rigid body per environment, moved by a stated kinematic rule in one launch (csrc/free_body.hip): no dynamics, contact or
 * friction.  It runs after the robot's launch on the same stream and reads the two tip rows as that launch left them.
 * Per environment e: tip_rows (N, 2) int32, the robot's left and right tip as rows of rigid_body (rb_rows, 13), and body_row (N)
 * int32, the body's own row (flat rows, as in pm_articulation_objects_step_f32; for a dense (N, nb, 13) tensor row = e nb + body);
 * root (N, na, 13) whose row obj_actor holds the body's state (c, q_c, velocities), which is what the rules read;  hold, reset (N)
 * bytes;  grip (N, 8) float32, the caller's state that this entry reads and writes: rel_t (3), rel_q (4), a latch (0 or 1);
 * default_pose (7);  u (N, 3) in [0, 1) or NULL.
 * The hand frame H = (p, q_H): p = (p_l + p_r) / 2, q_H = the left tip row's quaternion divided by its norm.  First match wins:
 *   1. reset[e]:  pose = default_pose; with u:  x, y += (2 u[0, 1] - 1) reset_range, theta = 2 pi u[2] - pi,
 *      q = default_q o (0, 0, sin theta, cos theta) (the reference's expressions, theta and not theta / 2; not renormalised);
 *      velocity 0; the latch clears (grip[7] = 0, grip[0..6] kept)
 *   2. hold[e], latch clear:  rel_t = R_H^T (c - p), rel_q = q_H* o q_c into grip, latch = 1;  the pose is kept, velocity 0
 *   3. hold[e], latch set:  c' = p + R_H rel_t, q' = unit(q_H o rel_q);  linear velocity (c' - c) / dt, angular velocity the left tip
 *      row's;  grip is only read
 *   4. otherwise:  the latch clears, the orientation and x, y are kept;  where z > rest_z:  z' = max(rest_z, z - fall_speed dt) and the
 *      velocity is (0, 0, (z' - z) / dt, 0, 0, 0);  else z is kept at velocity 0.  fall_speed = 0: a released body stays where it is.
 * Every output is formed in float64 from the float32 inputs (quaternions (x, y, z, w), Hamilton products) and rounded once; a kept
 * value keeps its bits.  The same 13 values are written to root[e, obj_actor] and to rigid_body[body_row[e]], and grip[e] as stated;
 * nothing else is written.  An environment's bits depend on its own rows only and not on N; a NaN stays in its environment.  An
 * environment with a tip row or body row outside [0, rb_rows) stores nothing and reads nothing out of range.  No synchronisation,
 * allocation or atomics; stream-ordered.  PM_EINVAL: a NULL pointer other than u, N or na < 1, obj_actor outside [0, na), rb_rows < 1
 * or >= 2^31, dt <= 0, fall_speed < 0, reset_range < 0, or a NaN among dt, fall_speed, reset_range, rest_z. */
int pm_free_body_step_f32(float* rigid_body, long rb_rows, const int32_t* tip_rows, const int32_t* body_row, float* root, int na,
                          int obj_actor, const uint8_t* hold, const uint8_t* reset, float* grip, const float* default_pose,
                          const float* u, float reset_range, float dt, float rest_z, float fall_speed, int N, void* stream);

/* ------------------------------------------------------------------ K15 fused set-abstraction level
 * One PointNet++ SA level (north_star; not in the reference snapshot, README.md:23,30) as one forward and
 * one backward kernel: ball-query groups of `nsample` = 32 rows [xyz[idx]-centre | feat[idx]] -> Linear C1,
 * tanh -> Linear C2, tanh -> Linear C3, tanh -> max over the group.  Layer 1's feature part is passed in
 * pre-multiplied per SOURCE point: Y (B*P, C1) = feat * W1[:, 3:3+Cf]^T (pm_linear_fwd_f32, no bias, no
 * activation), NULL when the level has no input features.  The grouped rows and per-row activations never
 * reach HBM.  pooled (B*S, ldp) = tanh(max_j z3 + b3), arg (B*S, C3) = lowest row j attaining the max of the
 * pre-activation.  Instantiated for (C1,C2,C3) in {(64,64,128), (128,128,256)} and nsample = 32
 * (pm_sa_supported); other shapes return PM_EUNSUPPORTED and the caller uses K4/K13-K15 separately.
 * Backward: dpooled (B*S, lddp) -> dW1[:, 0:3] (leading dimension lddw1; other columns untouched), db1, dW2,
 * db2, dW3, db3 (all overwritten) and dY (B*P, C1), which the caller zero-fills (fp32 atomics), or NULL. */
int pm_sa_supported(int C1, int C2, int C3, int nsample);
size_t pm_sa_packed_elems(int C1, int C2, int C3);
int pm_sa_pack_weights_f32(const float* W2, const float* W3, int C1, int C2, int C3, float* packed, void* stream);
int pm_sa_fwd_f32(const float* xyz, const float* centers, const int32_t* idx, const float* Y, int B, int P, int S,
                  int nsample, const float* W1, long ldw1, const float* b1, const float* b2, const float* b3,
                  const float* packed, int C1, int C2, int C3, float* pooled, long ldp, int32_t* arg,
                  float* h2_save /* NULL, or (B*S*32, C2): layer-2 activations kept for the backward */, void* stream);
size_t pm_sa_bwd_workspace_bytes(int C1, int C2, int C3);
int pm_sa_bwd_f32(const float* xyz, const float* centers, const int32_t* idx, const float* Y, int B, int P, int S,
                  int nsample, const float* W1, long ldw1, const float* b1, const float* b2, const float* W3,
                  const float* packed, int C1, int C2, int C3, const float* pooled, long ldp, const int32_t* arg,
                  const float* dpooled, long lddp, float* dW1, long lddw1, float* db1, float* dW2, float* db2,
                  float* dW3, float* db3, float* dY, const float* h2_saved /* NULL = recompute layer 2 */,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Duplicate-free ("packed") form of the fused level.  Ball query pads a short group with copies of its first hit; a
 * copy computes the same activations as row 0 of its group and the max-pool keeps the LOWEST row attaining the maximum,
 * so copies never win and never receive a gradient: the level is exactly the level over each group's DISTINCT rows.
 * pm_sa_plan_i32 (coordinates only: once per neighbourhood table) lists those rows back to back and cuts them into tiles
 * of whole groups; pm_sa_fwd_packed_f32 / pm_sa_bwd_packed_f32 run the same per-row arithmetic as pm_sa_fwd_f32 /
 * pm_sa_bwd_f32 on the tiles.  pooled, arg and the saved layer 2 are bit-identical to the dense entry points' (arg is
 * the row inside the group in both); weight gradients agree to fp32 summation order.
 *   grow    (B*S + 1)         first packed row of each group, grow[B*S] = R
 *   rowmap  (2 * B*S*nsample) capacity: {flat source point b*P + idx, (group - first group of its tile) << 8 | row inside the
 *                             group} per packed row; R pairs are written
 *   relxyz  (4 * B*S*nsample) capacity: xyz[source point] - centre[group] per packed row (x, y, z, 0): the staging of the level
 *                             kernels is two coalesced loads per row (coordinates only: weights never enter the plan)
 *   tiles   (4 * B*S)         capacity: {first row, first group, groups, rows} per tile; T quadruples are written
 *   totals  (4)               [0] = R packed rows, [1] = T tiles -- read by the kernels on the device (persistent
 *                             work-groups), never by the host: nothing here synchronises
 *   h2_save / h2_saved        (R, C2) -- capacity (B*S*nsample, C2) when R is not read back
 * tile_rows / tile_groups come from pm_sa_packed_tile (they are the kernels' tile shapes for that level shape). */
int pm_sa_packed_tile(int C1, int C2, int C3, int* tile_rows, int* tile_groups);
size_t pm_sa_plan_workspace_bytes(int B, int S);
int pm_sa_plan_i32(const int32_t* idx, const float* xyz, const float* centers, int B, int P, int S, int nsample, int tile_rows,
                   int tile_groups, int32_t* grow, int32_t* rowmap, float* relxyz, int32_t* tiles, int32_t* totals, void* workspace,
                   size_t workspace_bytes, void* stream);
int pm_sa_fwd_packed_f32(const float* Y, int B, int P, int S, const int32_t* grow, const int32_t* rowmap, const float* relxyz,
                         const int32_t* tiles, const int32_t* totals, const float* W1, long ldw1, const float* b1, const float* b2,
                         const float* b3, const float* packed, int C1, int C2, int C3, float* pooled, long ldp, int32_t* arg,
                         float* h2_save,
                         const float* tail_xyz /* (B*S, 3) or NULL: columns [C3, C3 + tail_cols) of every pooled row = (x, y, z, 0 ...) -- the
                                                  rows then ARE a group-all level's input rows [features | xyz | 0], no tail copy */,
                         int tail_cols, void* stream);
int pm_sa_bwd_packed_f32(const float* Y, int B, int P, int S, const int32_t* grow, const int32_t* rowmap, const float* relxyz,
                         const int32_t* tiles, const int32_t* totals, const float* W1, long ldw1, const float* b1, const float* b2,
                         const float* W3, const float* packed, int C1, int C2, int C3, const float* pooled, long ldp,
                         const int32_t* arg, const float* dpooled, long lddp, float* dW1, long lddw1, float* db1, float* dW2,
                         float* db2, float* dW3, float* db3, float* dY /* fp32 atomics: A/B only */,
                         float* dz1_rows /* (R, C1): the layer-1 gradient per packed row, plain stores (deterministic path) */,
                         int dw1_zero_end /* columns [3, dw1_zero_end) of dW1 are zeroed (a level without input features: padding) */,
                         const float* h2_saved, void* workspace, size_t workspace_bytes, void* stream);
/* The gradient of a level's per-source-point layer-1 rows (Y) WITHOUT floating-point atomics: a source point sits in several
 * groups, so dY[point] = sum of dz1 over its packed rows.  pm_sa_plan_inverse_i32 (coordinates only, once per plan) lists every
 * point's packed rows in ASCENDING order (CSR: inv_start (B*P + 1), inv_rows (R; capacity B*S*nsample)); pm_sa_dy_segsum_f32 adds
 * them in that order -- bit-reproducible run to run, no zero-fill of dY (points in no group get zeros).  P <= 7000. */
int pm_sa_plan_inverse_i32(const int32_t* rowmap, const int32_t* grow, int B, int P, int S, int32_t* inv_start, int32_t* inv_rows,
                           void* stream);
int pm_sa_dy_segsum_f32(const float* dz1, const int32_t* inv_start, const int32_t* inv_rows, long npoints, int C1, float* dY, long lddy,
                        void* stream);
/* The same sums CONSUMED in place (C1 = CF = 128): dY never reaches HBM.  Per tile of 64 source points the rows are summed into LDS
 * (same order, bit-identical to pm_sa_dy_segsum_f32), then  dfeat = dY * W1f  (the gradient the level below receives) and
 * dW1[:, 3 : 3 + CF] = dY^T * feat  run on fp32 MFMA; columns [3 + CF, dw1_cols) of dW1 are zeroed (pad columns never receive
 * data).  packedW = W1[:, 3 : 3 + CF] in operand order (pm_sa_dy_consume_pack_f32, after every update).  dfeat / dY may be NULL
 * (dY: an optional copy of the sums).  Replaces zero-fill + scatter + two Linear launches + slab reduction + column copy. */
int pm_sa_dy_consume_supported(int C1, int CF);
size_t pm_sa_dy_consume_packed_elems(int C1, int CF);
size_t pm_sa_dy_consume_workspace_bytes(int C1, int CF);
int pm_sa_dy_consume_pack_f32(const float* W1, long ldw1, int C1, int CF, float* packed, void* stream);
int pm_sa_dy_consume_f32(const float* dz1, const int32_t* inv_start, const int32_t* inv_rows, long npoints, int C1, int CF,
                         const float* feat, long ldf, const float* packedW, float* dfeat, long lddf, float* dW1, long lddw1,
                         int dw1_cols, float* dY, long lddy, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PointNet++ group-all level: its LAST layer fused with the max over the cloud (csrc/sa_groupall.hip) ----------------
 * (BASELINE.json cfg 3's backbone; the reference ships no PointNet++ source -- `PointNet2` in algo_utils/network.py.)
 *   feat[b][c] = max_r tanh(H[b*R + r][:] . W[c][:] + bias[c]),  argmax[b][c] = the lowest row r attaining it
 * H: (B*R) x CK activations of the layer before (row-major, ld = CK), W: CO x CK.  Supported: CK = 256, CO = 512, R = 64
 * (pm_sa_groupall_supported; callers fall back to pm_linear_fwd_f32 + pm_maxpool_rows_f32 otherwise).
 * pack: W -> the MFMA operand order the forward streams (pm_sa_groupall_packed_elems floats); re-pack after every update.
 * bwd: dz[b][c] = dfeat[b][c] * (1 - feat[b][c]^2);  dH[b*R + r][:] = (sum over c with argmax[b][c] == r of dz[b][c] * W[c][:]) * (1 - H^2)
 * for EVERY row (rows without a winner: 0);  dW[c][:] = sum_b dz[b][c] * H[b*R + argmax[b][c]][:];  dbias[c] = sum_b dz[b][c].
 * Fixed summation orders (run-to-run identical). */
int pm_sa_groupall_supported(int CK, int CO, int R);
size_t pm_sa_groupall_packed_elems(int CK, int CO);
int pm_sa_groupall_pack_f32(const float* W, int CK, int CO, float* packed, void* stream);
int pm_sa_groupall_fwd_f32(const float* H, int B, int R, int CK, int CO, const float* bias, const float* packed, float* feat, long ldf,
                           int32_t* argmax, void* stream);
size_t pm_sa_groupall_bwd_workspace_bytes(int B, int CK, int CO);
int pm_sa_groupall_bwd_f32(const float* dfeat, long lddf, const float* feat, long ldf, const int32_t* argmax, const float* W,
                           const float* H, int B, int R, int CK, int CO, float* dH, float* dW, float* dbias, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- rollout side ------------------------------------------------------------------------
 * algorithms/algo_utils/actor_critic.py:36-47 `random_act_cri` after the two network forwards: x = mu + sigma^2 * eps
 * (MultivariateNormal(mu, scale_tril = diag(sigma^2)).sample() with the caller's standard-normal eps (B, A), so the
 * torch RNG stream stays the reference's), logp (B) = its log_prob, actions (B, A) = tanh(x) * max_action (or x),
 * log_std_rows (B, A) = log_std repeated (may be NULL). */
int pm_gaussian_sample_f32(const float* mu, long ldmu, const float* log_std, const float* eps, int B, int A,
                           float max_action, int act_tanh, float* actions, float* logp, float* log_std_rows,
                           void* stream);
/* algorithms/algo_utils/RMS.py:10-18 `RunningMeanStd.update(x)` for one (N, D) batch: n_new = the reference's n AFTER
 * its increment; mean / S / std (D floats each) are updated in place.  RMS.py:40-45 `Normalization.__call__`:
 * out = (x - mean) / std. */
size_t pm_rms_update_workspace_bytes(int D);
int pm_rms_update_f32(const float* x, long ldx, int N, int D, int n_new, float* mean, float* S, float* std,
                      void* workspace, size_t workspace_bytes, void* stream);
int pm_rms_normalize_f32(const float* x, long ldx, int N, int D, const float* mean, const float* std, float* out,
                         long ldo, void* stream);
/* The same update in two halves for the data-parallel learner (new functionality: the reference has no distributed
 * path; each rank holds an env shard of the batch RMS.py:10-18 sees): mom[2*c] = sum_r x[r][c], mom[2*c+1] =
 * sum_r x[r][c]^2 (fp64; workspace as pm_rms_update_workspace_bytes(D)) -> the caller all-reduces `mom` ->
 * pm_rms_apply_moments_f32 applies RMS.py:10-18 for a batch of n_rows rows with those moments. */
int pm_rms_moments_f64(const float* x, long ldx, int N, int D, double* mom, void* workspace, size_t workspace_bytes,
                       void* stream);
int pm_rms_apply_moments_f32(const double* mom, long n_rows, int D, int n_new, float* mean, float* S, float* std,
                             void* stream);

/* ------------------------------------------------------------------ sparse-voxel U-Net building blocks
 * `network.name: SparseUNet` -- the "3D Sparse-UNet" backbone README.md:30 names; its code is NOT in the reference
 * snapshot (README.md:23): PARITY UNPINNED, restated in oracle/ref_cpu.py.  Input rows are the reference's 'depth_sparse'
 * observation (tasks/hand_base.py:335-336; utils/depth2tsdf.py:88-120): (x, y, z, f) with integer voxel coordinates.
 * Geometry: dense per-cloud index grids (R^3 int32; empty = 0x7fffffff), duplicates resolve to the lowest row.
 *   pm_voxel_grid0_f32: x (B, ldx) rows of P points x C floats -> grid (B * R^3) = lowest row b*P+i at that coordinate,
 *     coords (B*P, 4) int32 (b, x, y, z) clamped to [0, R), feat (B*P, 4) = (f, x/R, y/R, z/R) (may be NULL).
 *   pm_voxel_nbr27_i32: nbr (rows, 27) = row at coords + (dx,dy,dz), o = (dx+1)*9 + (dy+1)*3 + (dz+1), or -1.
 *   pm_voxel_down_count_i32 / _build_i32: the 2x strided level.  count: grid_c (B * Rc^3, Rc = ceil(Rf/2)) marks the parent
 *     cells, counts[b] = occupied cells of cloud b.  The caller prefix-sums counts into base (and sizes the level:
 *     rows_c = sum), then build numbers the cells in cell order from base[b] (grid_c <- global row; coords_c (rows_c, 4)),
 *     child (rows_c, 8) = fine row in slot (x&1)*4 + (y&1)*2 + (z&1) or -1, and per fine row parent / parent_canon (-1 for a
 *     duplicate coordinate: only the lowest row is its parent's child) / slot.
 * Arithmetic: a sparse convolution = pm_rows_gather_f32 + the Linear kernels on (rows x J*C).
 *   pm_rows_gather_f32: dst[r][j*C + c] = idx[r][j] >= 0 ? src[idx[r][j]][c] : 0      (C % 4 == 0, 16-byte rows)
 *   pm_rows_gather_bwd_f32: dsrc[r][c] (=, or += if accumulate) (sum_j dcols[t][blk*C + c]) * (y_tanh ? 1 - y_tanh[r][c]^2 : 1)
 *     with t = tidx[r][reverse ? J-1-j : j] (skipped when < 0) and blk = j (mode 0), tslot[r][j] (mode 1) or 0 (mode 2);
 *     self_col >= 0: rows with tidx[r][self_col] != r get 0 (duplicates are nobody's neighbour).  Fixed summation order. */
int pm_voxel_grid0_f32(const float* x, long ldx, int B, int P, int C, int R, int32_t* grid, int32_t* coords, float* feat,
                       void* stream);
int pm_voxel_nbr27_i32(const int32_t* coords, long rows, const int32_t* grid, int R, int32_t* nbr,
                       int ld /* row stride of nbr, >= 27; columns 27 .. ld-1 are written as -1 (padding taps) */, void* stream);
/* out[r][o] = nbr[r][26 - o] where row r is the canonical row of its cell (nbr[r][13] == r), else -1: the table the data
 * gradient of a 3^3 submanifold convolution gathers through (pm_sparse_conv_bwd_data_f32). */
int pm_voxel_mirror27_i32(const int32_t* nbr, long rows, int32_t* out, void* stream);
int pm_voxel_down_count_i32(const int32_t* coords_f, long rows_f, int B, int Rc, int32_t* grid_c, int32_t* counts, void* stream);
int pm_voxel_down_build_i32(const int32_t* coords_f, long rows_f, const int32_t* grid_f, int Rf, int B, int Rc,
                            const int32_t* base, int32_t* grid_c, long rows_c, int32_t* coords_c, int32_t* child,
                            int32_t* parent, int32_t* parent_canon, int32_t* slot, void* stream);
int pm_rows_gather_f32(const float* src, long lds, const int32_t* idx, long rows, int J, int C, float* dst, long ldd,
                       void* stream);
/* Fused forms: the gather happens inside the GEMM's LDS-DMA loader, the (rows x J*C) operand never exists in HBM
 * (J*C % 32 == 0; `zero`: >= C zeros, 16-byte aligned, read for absent neighbours).
 *   fwd:        Y[r][n] = act(sum_{j,c} src[idx[r][j]][c] * W[n][j*C + c] + b[n])
 *   bwd_weight: dW[n][j*C + c] = sum_r dY[r][n] * src[idx[r][j]][c],  db[n] = sum_r dY[r][n]   (db may be NULL) */
int pm_sparse_conv_fwd_f32(const float* src, long lds, const int32_t* idx, long rows, int J, int C, const float* W, long ldw,
                           const float* b, float* Y, long ldy, int N, int act, const float* zero, void* stream);
/* Data gradient of a submanifold convolution as a gathered GEMM (no column matrix in HBM):
 *   dX[s][ci] = (sum_{j,co} dY[idxT[s][j]][co] * Wt[ci][j*Cout + co]) * act'(H[s][ci])
 * idxT = the mirrored neighbour table (idxT[s][j] = idx[s][J-1-j], all -1 for rows that are nobody's neighbour),
 * Wt[ci][j*Cout + co] = W[co][j*Cin + ci] (row idxT[s][j] read s through ITS tap j); H = the activation the layer read (NULL: no factor).  (J*Cout) % 32 == 0. */
int pm_sparse_conv_bwd_data_f32(const float* dY, long lddy, const int32_t* idxT, long rows, int J, int Cout, const float* Wt,
                                long ldwt, const float* H, long ldh, float* dX, long lddx, int Cin, int act, const float* zero,
                                void* stream);
/* Data gradient by scatter, for convolutions whose patches do not overlap (stride == kernel size): every input row is
 * idx[r][j] for at most one (r, j), so  dX[idx[r][j]][c] = (sum_co dY[r][co] * W[co][j*C + c]) * act'(H[idx[r][j]][c])
 * is one GEMM whose epilogue stores each 16-byte piece at its destination row (idx < 0: dropped; rows nobody maps to keep
 * their contents).  W = the tap-major weight (Cout x J*C) of the forward. */
int pm_sparse_conv_bwd_data_scatter_f32(const float* dY, long lddy, const float* W, long ldw, const int32_t* idx, long rows,
                                        int J, int C, int Cout, const float* H, float* dX, int act, void* stream);
size_t pm_sparse_conv_bwd_weight_workspace_bytes(long rows, int N, int J, int C);
int pm_sparse_conv_bwd_weight_f32(const float* dY, long lddy, const float* src, long lds, const int32_t* idx, long rows, int J,
                                  int C, float* dW, long lddw, float* db, int N, const float* zero, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* Which kernel would a pm_sparse_conv_* call run on?  As pm_linear_*_variant_f32: the launch's arguments without the stream (and
 * without workspace_bytes; the workspace may be NULL = 16-byte aligned), the SAME host selection the launch consumes, no HIP call,
 * no device, pointers looked at for alignment only; returns what the launch would return for bad arguments.  The weight-gradient
 * query reports the slab count and the reduction range per slab the call chooses for itself. */
int pm_sparse_conv_fwd_variant_f32(const float* src, long lds, const int32_t* idx, long rows, int J, int C, const float* W, long ldw,
                                   const float* b, const float* Y, long ldy, int N, int act, const float* zero,
                                   pm_linear_variant* out);
int pm_sparse_conv_bwd_data_variant_f32(const float* dY, long lddy, const int32_t* idxT, long rows, int J, int Cout, const float* Wt,
                                        long ldwt, const float* H, long ldh, const float* dX, long lddx, int Cin, int act,
                                        const float* zero, pm_linear_variant* out);
int pm_sparse_conv_bwd_data_scatter_variant_f32(const float* dY, long lddy, const float* W, long ldw, const int32_t* idx, long rows,
                                                int J, int C, int Cout, const float* H, const float* dX, int act,
                                                pm_linear_variant* out);
int pm_sparse_conv_bwd_weight_variant_f32(const float* dY, long lddy, const float* src, long lds, const int32_t* idx, long rows,
                                          int J, int C, const float* dW, long lddw, const float* db, int N, const float* zero,
                                          const void* workspace, pm_linear_variant* out);
/* accumulate: 0 = overwrite dsrc; 1 = add the (already multiplied) result to what dsrc holds; 2 = dsrc holds a RAW
 * contribution that is added to the gathered sum BEFORE the activation derivative ((skip + strided) * act'). */
int pm_rows_gather_bwd_f32(const float* dcols, long ldc, const int32_t* tidx, const int32_t* tslot, int mode, int reverse,
                           int self_col, long rows, int J, int C, const float* y_tanh, long ldy, int accumulate, float* dsrc,
                           long lds, void* stream);
/* The same with a COMPACTED column gradient: the table holds rows of a level, dcols only a subset of them; rowmap[row] = that
 * row's row in dcols, or -1 (its contribution is zero).  rowmap NULL: pm_rows_gather_bwd_f32. */
int pm_rows_gather_bwd_mapped_f32(const float* dcols, long ldc, const int32_t* tidx, const int32_t* tslot, int mode, int reverse,
                                  int self_col, long rows, int J, int C, const float* y_tanh, long ldy, int accumulate,
                                  float* dsrc, long lds, const int32_t* rowmap, void* stream);
/* ... and with a SPARSE raw skip contribution added before the activation derivative (accumulate == 2 without the dense
 * zero-filled tensor): row r additionally receives skip[skipmap[r]][:] when skipmap[r] >= 0; dsrc is overwritten. */
int pm_rows_gather_bwd_skip_f32(const float* dcols, long ldc, const int32_t* tidx, const int32_t* tslot, int mode, int reverse,
                                int self_col, long rows, int J, int C, const float* y_tanh, long ldy, float* dsrc, long lds,
                                const float* skip, long ldskip, const int32_t* skipmap, void* stream);

/* ------------------------------------------------------------------ row bookkeeping of the compact decoder backward
 * (partmanip_amd/algo_utils/network.py::SparseUNet._decoder_backward_compact: after the cloud-wide max-pool only the winners'
 * rows and their ancestors carry a gradient through the decoder -- at most S = c0 rows per cloud and level).  Integer work, fixed
 * order, no sort library.  A Level-2 binder reproduces the SparseUNet backward from these + the entry points above.
 *   pm_rows_uniq_i32: per cloud b the ids v[i] = map ? (src[b][i] == pad_in ? pad_out : map[src[b][i]]) : src[b][i] + b*row_base,
 *     i < S <= 64 -> u (B, S) = the cloud's DISTINCT ids ascending, padded with pad_out (a dummy row id >= every real id);
 *     um = u with -1 in the padding slots; rank (B, S) = slot of id i in u[b].
 *   pm_child_sum_f32: y[b*S + j][:] = sum_{i ascending, rank[b][i] == j} x[b*S + i][:]  (children summed into their parent's slot).
 *   pm_rowmap_scatter_i32: map[0..n) = -1; map[ids[k]] = k for ids[k] != pad  (row -> compact slot).
 *   pm_table_rows_i32: out[k][0..J) = sel[k] >= 0 ? table[sel[k]][0..J) : -1  (rows of an index table; -1 rows = absent taps).
 *   pm_voxel_vcat_table_i32: out[r] = {parent[r]*m .. parent[r]*m + m-1, r + m*rows_hi}: the (m + 1)-tap gather table of a
 *     virtual [unpool(coarse) | skip] operand whose halves share one buffer of skip-width rows.
 *   pm_exclusive_scan_i32: base[i] = counts[0] + .. + counts[i-1], total[0] = sum (pm_voxel_down_*'s `base`). */
int pm_rows_uniq_i32(const int32_t* src, long lds, int B, int S, long row_base, const int32_t* map, int pad_in, int pad_out,
                     int32_t* u, int32_t* um, int32_t* rank, void* stream);
int pm_child_sum_f32(const float* x, long ldx, const int32_t* rank, int B, int S, int C, float* y, long ldy, void* stream);
int pm_rowmap_scatter_i32(int32_t* map, long n, const int32_t* ids, long N, int pad, void* stream);
int pm_table_rows_i32(const int32_t* table, long ldt, int J, const int32_t* sel, long N, int32_t* out, void* stream);
int pm_voxel_vcat_table_i32(const int32_t* parent, long rows, int m, long rows_hi, int32_t* out, void* stream);
int pm_exclusive_scan_i32(const int32_t* counts, int n, int32_t* base, int32_t* total, void* stream);

/* ------------------------------------------------------------------ 2-D residual network building blocks
 * `network.name: depthResNet` (reference network.py:237-271: a ResNet-34 on the 1 x 72 x 128 depth image).  Its convolutions
 * are the gathered GEMMs above over host-built 2-D patch tables; these are the layers between them.  Every activation is a
 * channels-last matrix (rows = b*H*W, C) with a row stride ld >= C in elements; C % 4 == 0, C <= 1024, pointers 16-byte aligned,
 * strides multiples of 4.  No atomics: every sum has a fixed order that depends on (rows, C) only, so two runs give the same bits.
 *
 *   pm_bn2d_stats_f32: per channel over the rows, mean, biased variance (var may be NULL) and invstd = 1/sqrt(var + eps).  The
 *     sums are taken in fp64 about the channel's first row (a depth image holds 100.0 beside values near 1: E[x^2] - E[x]^2 in
 *     fp32 loses the variance); a constant channel gives variance exactly 0.  running_mean / running_var (NULL: untouched) become
 *     (1 - momentum) * running + momentum * batch with the unbiased variance var * n / (n - 1); num_batches_tracked (one int64,
 *     NULL: untouched) is incremented.  rows < 2 -> PM_EINVAL (torch.nn.BatchNorm2d refuses the same case in training).
 *     Workspace (8-byte aligned): pm_bn2d_workspace_bytes(rows, C), also what pm_bn2d_bwd_f32 needs.
 *   pm_bn2d_apply_f32: y = gamma * (x - mean) * invstd + beta [+ residual] [then ReLU], one pass; NaN propagates.  Inference: hand
 *     it running_mean and 1/sqrt(running_var + eps).
 *   pm_bn2d_bwd_f32: with dy_m = (dy [+ dy2]) [masked by y > 0 when relu], xhat = (x - mean) * invstd, n = rows:
 *       dbeta = sum dy_m, dgamma = sum dy_m * xhat (fp64 sums), dx = gamma * invstd * (dy_m - dbeta / n - xhat * dgamma / n);
 *     dy_masked (NULL: not wanted) receives dy_m for the residual branch.  dy2 (NULL: none) is a second gradient of the same
 *     output (a block's input feeds its first convolution and its shortcut).  y is the layer's OUTPUT (read only when relu).
 *     Three launches: partial sums, their fixed-order total, the apply pass.
 *   pm_pool2d_max3s2_*: 3 x 3 max pool, stride 2, padding 1 over (B, H, W, C) -> (B, Ho, Wo, C), Ho = pm_pool2d_out(H).  idx
 *     (B*Ho*Wo, C) int32 = ih * W + iw of the winner (torch's return_indices): a tie goes to the first tap in row-major window
 *     order, the padding never wins, a NaN wins.  The backward is a gather: every input pixel sums the (at most four) windows
 *     whose winner it is in ascending window order; dx is written everywhere.
 *   pm_pool2d_avg_*: mean over the HW rows of each sample (ascending order) -> y (B, C) whose row stride may be any value >= C
 *     (the head's [features | proprio] rows); backward dx[b*HW + r] = dy[b] / HW.
 *   pm_im2col2d_c1_f32: patch matrix of a single-channel image, x (B rows of stride ldx, H*W pixels each) -> dst
 *     (B*Ho*Wo, ldd), dst[.][kh*k + kw] = the pixel under tap (kh, kw) or 0 in the padding, columns k*k .. ldd-1 zeros (the stem's
 *     K = 49 is no multiple of 4, so it cannot be a gathered operand; it runs on the Linear kernels over this matrix).
 *   pm_im2col2d_f32: the same for a planar C-channel image (`network.name: ResNet`, the RGB stem), x (B rows of stride ldx, C planes
 *     of H*W each) -> dst[.][c*k*k + kh*k + kw], zero in the padding and in the columns C*k*k .. ldd-1.  The column order is that
 *     of conv.weight viewed (Cout, C*k*k).  C = 1 gives pm_im2col2d_c1_f32's bits.  ldd: the Linear kernels' K-step is 32, so the
 *     RGB stem rounds 147 up to 160.
 *   pm_rgb_planes_f32: view v of a colour frame, rgb uint8 (B, V, h, w, 3), into the head of B float rows of stride ldo:
 *     out[b*ldo + c*h*w + y*w + x] = (float) rgb[b][v][y][x][c] (raw 0..255, the reference's `rgb_img` row); columns >= 3*h*w are
 *     not touched.  v outside [0, V), a non-positive size or ldo < 3*h*w -> PM_EINVAL.  Four pixels per thread (three dwords in,
 *     three 16-byte stores) when h*w % 4 == 0, ldo % 4 == 0 and both pointers are 16-byte aligned, one pixel per thread otherwise. */
size_t pm_bn2d_workspace_bytes(long rows, int C);
int pm_bn2d_stats_f32(const float* x, long ldx, long rows, int C, float eps, float* mean, float* var, float* invstd,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, void* workspace,
                      size_t workspace_bytes, void* stream);
int pm_bn2d_invstd_f32(const float* var, int C, float eps, float* invstd, void* stream); /* invstd = 1/sqrt(var + eps): inference */
int pm_bn2d_apply_f32(const float* x, long ldx, long rows, int C, const float* mean, const float* invstd, const float* gamma,
                      const float* beta, const float* residual, long ldr, int relu, float* y, long ldy, void* stream);
int pm_bn2d_bwd_f32(const float* dy, long lddy, const float* dy2, long lddy2, const float* x, long ldx, const float* y, long ldy,
                    int relu, long rows, int C, const float* mean, const float* invstd, const float* gamma, float* dgamma,
                    float* dbeta, float* dx, long lddx, float* dy_masked, long lddym, void* workspace, size_t workspace_bytes,
                    void* stream);
int pm_pool2d_out(int n);
int pm_pool2d_max3s2_fwd_f32(const float* x, long ldx, int B, int H, int W, int C, float* y, long ldy, int32_t* idx, void* stream);
int pm_pool2d_max3s2_bwd_f32(const float* dy, long lddy, const float* dy2, long lddy2, const int32_t* idx, int B, int H, int W, int C,
                             float* dx, long lddx, void* stream);
int pm_pool2d_avg_fwd_f32(const float* x, long ldx, int B, int HW, int C, float* y, long ldy, void* stream);
int pm_pool2d_avg_bwd_f32(const float* dy, long lddy, int B, int HW, int C, float* dx, long lddx, void* stream);
int pm_im2col2d_c1_f32(const float* x, long ldx, int B, int H, int W, int k, int stride, int pad, float* dst, int ldd, void* stream);
int pm_im2col2d_f32(const float* x, long ldx, int B, int C, int H, int W, int k, int stride, int pad, float* dst, int ldd,
                    void* stream);
int pm_rgb_planes_f32(const uint8_t* rgb, int B, int V, int h, int w, int v, float* out, long ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PARTMANIP_HIP_H */
