#!/usr/bin/env python3
"""bench.py -- PPO learner throughput on MI355X (BASELINE.json metric: PPO env-steps/sec,
4096 envs x 1024-pt clouds).

    python bench.py [--gpus N --steps K --warmup W] [--workload vision|vision_pn2|state|dagger|depth2pc]
                    [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the line: metric, value, unit, ms_per_step and
the roofline of the kernels bracketed inside the timed steps.  `--full` adds everything that needs runs of
its own: the CPU baseline, the opt-in precision / stream paths, the other configs' `secondary` sub-lines
and the single-kernel side timings.  `--dump-outputs DIR` writes what the timed path computed in its last
step (parameters, returns, losses, sampled clouds) as DIR/<name>.npy; the inputs are seeded, so two builds
run with the same arguments can be compared array for array.

A "step" is one learner iteration = the reference's `learn_time` window (ppo.py:256-262:
compute_returns + update + storage.clear) over one synthetic rollout batch that is already
resident in HBM.  env-steps/s = N_env * T * world / (time per step).  One process per GPU:
under torch.distributed.run the ranks come from RANK / LOCAL_RANK / WORLD_SIZE; a bare
`python bench.py --gpus N` starts the N ranks itself (and refuses when fewer than N GPUs are
visible).  Each rank owns its own 4096 envs (weak scaling) and gradients are all-reduced over
RCCL once per optimiser step.

Rank 0 prints ONE JSON line; with --full every workload's line carries
  roofline     : live HIP-event timing of the workload's dominant kernel against the roofline that
                 bounds it (fp32-MFMA 157.3 TFLOP/s or HBM 8 TB/s, MI355X_MICROARCH.md)
  cpu_baseline : the CPU oracle (oracle/ref_cpu.py, pinned to the reference) timed on this box's
                 host cores on a bounded, warmed sample of the same workload (N = 1 only).
"""
import argparse
import contextlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0
ENC_MAC_PER_POINT = 3 * 128 + 128 * 256 + 256 * 512          # 164 224

WORKLOADS = {
    # cfg3: open_drawer vision PPO, ppo.yaml hyper-parameters, PointNet(tanh, max_mean, no sub_mean)
    "vision": dict(name="ppo_vision_pointnet_4096env_x_8step_x_1024pt", N=4096, T=8, O=3072, A=10,
                   net=dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=False)),
    # same rollouts through the PointNet++ (SSG) plug-in backbone: FPS + ball query + grouped shared MLPs
    "vision_pn2": dict(name="ppo_vision_pointnet2ssg_4096env_x_8step_x_1024pt", N=4096, T=8, O=3072, A=10,
                       net=dict(name="PointNet2", activation="tanh")),
    # cfg2: open_drawer state PPO, MLP 53-512-512-512
    "state": dict(name="ppo_state_mlp_4096env_x_128step", N=4096, T=128, O=53, A=10,
                  net=dict(name="MLP", hid_dim=[512, 512, 512], activation="tanh")),
}
SA_LEVELS = {"64x64x128": (64, 64, 128, 256), "128x128x256": (128, 128, 256, 64)}     # C1, C2, C3, groups per cloud
# the Linear launches left around the fused PointNet++ kernels at a 2048-cloud mini-batch (ops.py brackets them by shape): the
# per-source-point layer-1 rows of level 2 (Y = feat W1f^T), the group-all level's first layer and its two gradients
PN2_GLUE_GEMMS = {"linear_fwd_524288x128x128": 2.0 * 524288 * 128 * 128, "linear_fwd_131072x288x256": 2.0 * 131072 * 288 * 256,
                  "linear_bwd_data_131072x256x256": 2.0 * 131072 * 256 * 256, "linear_bwd_weight_131072x256x288": 2.0 * 131072 * 256 * 288}

DAGGER = dict(name="dagger_pointnet_student_4096env_x_16buf_x_{P}pt", N=4096, buf=16, O_t=53, A=10)
DUMP_LIMIT_BYTES = 64 * 2 ** 20


def dump_outputs(args, rank, arrays):
    """--dump-outputs DIR: rank 0 writes each array as DIR/<name>.npy (float64 stays float64, everything else float32).
    Called right after the timed steps, before any side measurement touches the state."""
    import numpy as np
    d = getattr(args, "dump_outputs", None)                 # (tools/ call the runners with a Namespace of their own)
    if not d or rank != 0:
        return
    out = {}
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        out[name.replace("/", "_")] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(d, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(d, name + ".npy"), a)


# ------------------------------------------------------------------------------------------------ CPU baseline
def _pick_threads(trial, ncpu):
    """The oracle is plain PyTorch-CPU; `torch.set_num_threads(os.cpu_count())` on a 2-socket SMT box oversubscribes
    the intra-op pool (round 1 measured 2.6x SLOWER per sample with 256 threads than the survey's 8-thread probe).
    Time a small warm-up pass at a few thread counts and keep the fastest; the passes double as the warm-up."""
    cand = sorted({n for n in (8, 16, 32, 64, 96, 128, ncpu // 2, ncpu) if 1 <= n <= ncpu})
    best, tbest, log, worse = cand[0], float("inf"), {}, 0
    for n in cand:
        torch.set_num_threads(n)
        trial()                                        # first touch at this thread count (allocator, thread pool)
        t0 = time.perf_counter()
        trial()
        dt = time.perf_counter() - t0
        log[n] = round(dt, 3)
        if dt < tbest:
            best, tbest, worse = n, dt, 0
        else:
            # past the knee the curve only gets worse (round 5's lines: 0.33 s at 16 threads, 0.71 at 64, 2.4 at 128, 21.6 at 256;
            # SparseUNet 2.26 at 16, 2.56 at 64, 31.9 at 256): after two counts in a row that do not improve, or one that is 2 x
            # slower, the larger counts are not tried -- they cost the default run two minutes of wall time for nothing
            worse += 1
            if worse >= 2 or dt > 2.0 * tbest:
                log["stopped_after"] = n
                break
    torch.set_num_threads(best)
    return best, log


def cpu_baseline_ppo(w, rollout_cpu, sd_cpu, cfg):
    """the oracle's `ppo_update` (which, like the reference, runs BOTH networks forward in both loops)
    warmed, on >= 3 actor + >= 3 critic mini-batch steps -- B = 512 for the point-cloud backbones (B = 2048 needs ~15 GB
    of activations per net; stated fallback), B = 2048 for the MLP -- plus the full-size GAE, extrapolated by the exact
    step count n_updates * T * N / B per loop."""
    from oracle import ref_cpu as R
    ncpu = os.cpu_count() or 1
    vision = w["net"]["name"] in ("PointNet", "PointNet2")
    pn2 = w["net"]["name"] == "PointNet2"                # its restatement samples / groups in Python loops: a smaller bounded sample
    mb, n_mb = (64, 3) if pn2 else (512, 3) if vision else (2048, 128)
    T, N = w["T"], w["N"]
    keys = ("observations", "actions", "values", "returns", "actions_log_prob", "advantages", "mu", "sigma")

    def sample(mb_, n_):
        return {k: rollout_cpu[k].reshape(-1, rollout_cpu[k].shape[-1])[: mb_ * n_].reshape(n_, mb_, -1).clone() for k in keys}

    def run(mb_, n_):
        c = dict(cfg)
        c.update(n_updates=1, n_minibatches=n_, sampler="sequential", device="cpu")
        p = {k: v.clone() for k, v in sd_cpu.items()}
        t0 = time.perf_counter()
        R.ppo_update(p, sample(mb_, n_), c, 1)          # n_ actor steps + n_ critic steps
        return time.perf_counter() - t0

    used, tried = _pick_threads(lambda: run(8 if pn2 else 32 if vision else 2048, 1), ncpu if not pn2 else min(ncpu, 32))
    gae = lambda: R.gae_returns(rollout_cpu["rewards_full"], rollout_cpu["values_full"], rollout_cpu["dones_full"],
                                rollout_cpu["succs_full"], rollout_cpu["last_values"], 0.99, 0.95, None, False)
    gae()
    t0 = time.perf_counter()
    gae()
    t_gae = time.perf_counter() - t0
    t_upd = run(mb, n_mb)
    per_sample = t_upd / (mb * n_mb)                    # one actor pass + one critic pass of one sample
    t_iter = t_gae + per_sample * cfg["n_updates"] * T * N
    return dict(value=T * N / t_iter, unit="env-steps/s", cores=used, kind="port", host_cpus=ncpu,
                threads_tried_s=tried,
                sample=f"oracle/ref_cpu.py ppo_update, warmed, {n_mb} actor + {n_mb} critic mini-batch steps of {mb} samples "
                       f"({t_upd:.1f} s) + full GAE ({t_gae * 1e3:.1f} ms), extrapolated to {cfg['n_updates']} epochs x "
                       f"{T * N} samples per loop; {used} torch threads (fastest of {sorted(k_ for k_ in tried if isinstance(k_, int))} on {ncpu} host CPUs)")


def cpu_baseline_dagger(d, net, ring_obs, ring_tea, stu_sd, tea_sd, tea_net, rows_total, proprio, mb=128):
    """Oracle `dagger_update` (frozen teacher forward + student forward/backward + Adam) on 3 mini-batches of `mb`
    ring rows, warmed; extrapolated by the row count of one update (n_updates passes over the ring)."""
    from oracle import ref_cpu as R
    ncpu = os.cpu_count() or 1
    model = lambda n, std: dict(action_std=std, action_activate="tanh", clipAction=1.0, network=dict(n))
    cfg = dict(model=model(net, 0.1), tea_model=model(tea_net, 0.5), n_updates=1, n_minibatches=3, sampler="sequential",
               lr=5e-5, lr_schedule="fixed", max_iterations=10000, proprio_shape=proprio)

    def run(mb_, n_):
        c = dict(cfg, n_minibatches=n_)
        stu = {k: v.clone() for k, v in stu_sd.items()}
        t0 = time.perf_counter()
        R.dagger_update(stu, tea_sd, ring_obs[: mb_ * n_], ring_tea[: mb_ * n_], mb_ * n_, c, 1)
        return time.perf_counter() - t0

    used, tried = _pick_threads(lambda: run(16, 1), ncpu)                 # (dagger.update is a no-op below 16 rows, dagger.py:300)
    t = run(mb, 3)
    per_row = t / (3 * mb)
    t_upd = per_row * rows_total
    return dict(value=d["N"] / t_upd, unit="env-steps/s", cores=used, kind="port", host_cpus=ncpu, threads_tried_s=tried,
                sample=f"oracle/ref_cpu.py dagger_update, warmed, 3 mini-batch steps of {mb} ring rows ({t:.1f} s), extrapolated to "
                       f"{rows_total} rows per update; {used} torch threads (fastest of {sorted(k_ for k_ in tried if isinstance(k_, int))} on {ncpu} host CPUs)")


# ------------------------------------------------------------------------------------------------ DAgger
def run_dagger(args, device, rank, world):
    """cfg 5 analogue: DAgger, N=4096, n_steps 1, buf_size 16, PointNet student on 4096-pt
    clouds (`--points`; the reference hard-codes 1024, network.py:146; the 3D-Sparse-UNet cfg 5 names does not exist
    in the reference), frozen MLP teacher (O=53), random sampler, n_updates 2, n_minibatches 16 (-> 2048).
    A step = one `dagger.update` over the full ring (65 536 rows); env-steps/s = N * n_steps / time."""
    import tempfile
    from partmanip_amd import ops
    from partmanip_amd.algorithms import ppo, dagger
    from partmanip_amd.feeder import FeederEnv, ScreenLogger
    conv = args.student == "conv3d"
    if conv:
        # the reference's SHIPPED DAgger configuration (cfg/algos/dagger_tsdf.yaml): 16 envs, 1600-step ring (25 600 rows of
        # a 50^3 TSDF + proprio = 12.8 GB, resident in HBM), Conv3DNet student, 16 mini-batches (-> 1600 rows), 2 passes
        d = dict(DAGGER, N=16, buf=1600, O_s=50 ** 3 + 25, proprio=25, name="dagger_conv3dnet_student_16env_x_1600buf_x_50cube_tsdf")
        obs_mode = "mesh_tsdf"
    elif args.student == "sparse_unet":
        # BASELINE cfg 5 as written: a 3D sparse-voxel U-Net student on 4096-point 'depth_sparse' clouds (x, y, z, tsdf rows)
        d = dict(DAGGER, O_s=4 * args.points, proprio=0, name=f"dagger_sparse_unet_student_4096env_x_16buf_x_{args.points}pt")
        obs_mode = "depth_sparse"
    else:
        d = dict(DAGGER, O_s=3 * args.points, proprio=0, name=DAGGER["name"].format(P=args.points))
        obs_mode = "depth_pc"
    torch.manual_seed(1234)
    tmp = tempfile.mkdtemp()
    env = FeederEnv(d["N"], {"normal_state": d["O_t"], obs_mode: d["O_s"], "proprio_state": d["proprio"]}, d["A"], device,
                    seed=1234 + rank, point_num=args.points)
    tcfg = make_cfg(WORKLOADS["state"], device)
    tcfg.update(num_envs=d["N"], n_steps=1, obs_mode="normal_state")
    tea = ppo(env, tcfg, ScreenLogger(tmp, f"tea{rank}", "n", quiet=True))
    tea.sync = None                                      # every rank writes its own (identical) teacher checkpoint
    tea.save(1)
    sparse = args.student == "sparse_unet"
    net = (dict(name="Conv3DNet", activation="tanh") if conv else
           dict(name="SparseUNet", activation="tanh", point_num=args.points, grid=50) if sparse else
           dict(name="PointNet", activation="tanh", max_mean=True, sub_mean=False, point_num=args.points))
    cfg = dict(num_envs=d["N"], obs_mode=obs_mode,
               model=dict(action_std=0.1, action_activate="tanh", clipAction=1.0, network=net),
               max_iterations=10000, n_steps=1, n_updates=2, n_minibatches=16, device=device, buf_size=d["buf"],
               reward_reset=False, add_proprio_obs=conv, offline_data_pth=None, eval_round=1, eval_frequence=10 ** 9,
               save_frequence=10 ** 9, test_only=False, save_pose=False, save_video=False, lr_schedule="fixed", lr=5e-5,
               teacher=os.path.join(tea.save_ckpt_dir, "model_1.pth"), resume=None, pretrain=None, sampler="random")
    run = dagger(env, cfg, ScreenLogger(tmp, "stu", "n", quiet=True))
    for _ in range(d["buf"]):
        obs = env.reset()
        run.storage.add_transitions_dagger(obs[obs_mode], obs["normal_state"])      # rows = [observation | proprio]
    run.log_dict = {}

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()
    for _ in range(args.warmup):
        run.update(1)
    timed = ("conv3d_c1_wgrad", "conv3d_c1_fwd") if conv else ("sparse_unet_fwd", "sparse_unet_bwd") if sparse else \
        ("pointnet_enc_fwd", "pointnet_enc_bwd")
    ops.TIMER.enable(*timed)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run.update(1)
    fence()
    dt = time.perf_counter() - t0
    ops.TIMER.disable()
    dump_outputs(args, rank, {"student_actor_params": run.student.flat()["actor"],
                              "dagger_loss": torch.tensor([float(run.log_dict["Train/dagger_loss"])], dtype=torch.float64)})
    dt = _max_over_ranks(dt, device, world)
    rows = d["N"] * d["buf"] * 2                        # samples through the student per update
    mb = min(d["N"] * d["buf"] // 16, 2048)
    out = dict(metric="DAgger update throughput (shipped dagger_tsdf.yaml)" if conv else "DAgger update throughput (cfg 5 analogue)",
               value=d["N"] * 1 * world / (dt / args.steps),
               unit="env-steps/s", n_gpus=world, steps=args.steps, warmup=args.warmup,
               ms_per_step=dt / args.steps * 1e3, higher_is_better=True, scaling="weak", vs_baseline=None, dtype="f32",
               data="synthetic", config=dict(workload=d["name"], ring_rows=d["N"] * d["buf"], minibatch=mb,
                                             parallelism=f"dp{world}", world_size_observed=_world_observed(),
                                             student_samples_per_s=rows * world / (dt / args.steps),
                                             dagger_loss=float(run.log_dict["Train/dagger_loss"])))
    if conv:
        # dominant kernel: the input layer's weight gradient (a 125-tap stencil reduction): per sample it reads the 50^3
        # volume (500 KB) and the 17^3 x 16 dz rows (314 KB) once -> HBM-bound by construction (FMA bound 3x lower)
        t = ops.TIMER.mean_ms("conv3d_c1_wgrad")
        if t:
            nbytes = mb * (50 ** 3 + 17 ** 3 * 16) * 4.0
            gbs = nbytes / (t[0] * 1e-3) / 1e9
            out["roofline"] = dict(bound="hbm", kernel="conv3d_c1_wgrad_mfma_kernel", achieved=gbs, peak=PEAK_HBM_GBS, unit="GB/s",
                                   frac=gbs / PEAK_HBM_GBS, traffic=None, launches=t[1], mean_launch_ms=t[0],
                                   bytes_per_launch=nbytes)
            f = ops.TIMER.mean_ms("conv3d_c1_fwd")
            if f:
                out["roofline"]["conv1_fwd_mean_ms"] = f[0]
                out["roofline"]["conv1_fwd_gbs"] = nbytes / (f[0] * 1e-3) / 1e9
    elif sparse:
        # whole backbone forward / backward (gathers + Linear GEMMs); flops = the GEMMs the launch executes, from the level
        # sizes of the last mini-batch: fwd sum_l rows_l * K_l * N_l * 2, bwd twice that minus conv0's absent data gradient
        t, b = ops.TIMER.mean_ms("sparse_unet_fwd"), ops.TIMER.mean_ms("sparse_unet_bwd")
        g = run.student.actor._saved["g"]
        c0, c1, c2 = run.student.actor.channels
        R0, R1, R2 = g["rows"]
        macs = {"conv0": R0 * 108 * c0, "down0": R1 * 8 * c0 * c1, "conv1": R1 * 27 * c1 * c1, "down1": R2 * 8 * c1 * c2,
                "conv2": R2 * 27 * c2 * c2, "up1": R1 * (c2 + c1) * c1, "up0": R0 * (c1 + c0) * c0}
        ffl = 2.0 * sum(macs.values())
        # backward = weight gradients (the forward's MACs) + data gradients: the forward's MACs again, except conv0 (its input
        # is data) and the up layers, whose un-pooled half runs on the COARSE rows (children summed first, linearity)
        dgrad = dict(macs, conv0=0, up1=R1 * c1 * c1 + R2 * c1 * c2, up0=R0 * c0 * c0 + R1 * c0 * c1)
        wgrad = dict(macs)
        compact_rows = None
        if getattr(run.student.actor, "sparse_top", False) and run.student.actor._saved.get("vcat") and run.student.actor._saved.get("cols2") is None:
            # the cloud-wide max-pool leaves one non-zero per (cloud, channel): max-pool, up0, up1 and conv2's weight gradient run
            # over the winners' rows and their ancestors -- mb * c0 rows per level instead of the level's (network.py::
            # _decoder_backward_compact), conv2's data gradient as the column gradient of those rows + a row-mapped gather; everything
            # below conv2 stays dense
            compact_rows = Nc = mb * c0
            wgrad.update(conv2=Nc * 27 * c2 * c2, up1=Nc * (c2 + c1) * c1, up0=Nc * (c1 + c0) * c0)
            dgrad.update(up1=Nc * c1 * c1 + Nc * c1 * c2, up0=Nc * c0 * c0 + Nc * c0 * c1, conv2=Nc * 27 * c2 * c2)
        bfl = 2.0 * sum(wgrad.values()) + 2.0 * sum(dgrad.values())
        # USEFUL flops: a row of a 3^3 convolution multiplies all 27 taps and a strided level all 8 children,
        # whether present or not (absent ones read a zero row) -- `frac` prices what the GEMMs execute, `useful_frac` only the
        # products with a present tap / child.  Fractions of present entries from the tables of the timed mini-batch.
        pres = lambda tbl, J: float((tbl[:, :J] >= 0).float().mean().item())
        occ = dict(conv0=pres(g["nbr0"], 27) * 27 / 27, conv1=pres(g["nbr1"], 27), conv2=pres(g["nbr2"], 27),
                   down0=pres(g["l1"]["child"], 8), down1=pres(g["l2"]["child"], 8), up1=1.0, up0=1.0)
        useful = lambda d_: 2.0 * sum(v * occ[k_] for k_, v in d_.items())
        ufl = useful(macs) + useful(wgrad) + useful(dgrad)
        # algorithmic HBM bytes of one forward + backward (every operand once: a layer reads its input rows, its table and
        # writes its output; its backward reads dY, its own output (tanh'), the input again (weight gradient) and writes dX)
        lay = [(R0, 4, 32, R0, c0), (R0, c0, 8, R1, c1), (R1, c1, 27, R1, c1), (R1, c1, 8, R2, c2), (R2, c2, 27, R2, c2),
               (R1, c1 + c2, 3, R1, c1), (R0, c0 + c1, 3, R0, c0)]            # rows_in, C_in, table entries per output row, rows_out, C_out
        fwd_b = sum(ri * ci * 4.0 + ro * (tb * 4.0 + co * 4.0) for ri, ci, tb, ro, co in lay) + R0 * c0 * 4.0
        bwd_b = sum(ro * (2 * co * 4.0 + tb * 4.0) + 2 * ri * ci * 4.0 for ri, ci, tb, ro, co in lay) - R0 * 4 * 4.0
        tr = _hbm_traffic(f"sparse_unet_{mb}_clouds_bytes_per_pass")[0]
        if t and b:
            tf = (ffl + bfl) / ((t[0] + b[0]) * 1e-3) / 1e12
            out["roofline"] = dict(bound="mfma", kernel="SparseUNet forward + backward (gemm2_dma_kernel with fused neighbour gathers)",
                                   achieved=tf, peak=PEAK_F32_MFMA_TFLOPS, unit="TFLOP/s", frac=tf / PEAK_F32_MFMA_TFLOPS, traffic=tr,
                                   algorithmic_bytes=fwd_b + bwd_b,
                                   traffic_note="HBM bytes of one forward + backward of a mini-batch, ALL its kernels (PMC over "
                                                f"tools/time_sparse_unet.py {mb}, profiles/hbm_traffic.json)",
                                   launches=t[1], fwd_mean_ms=t[0], bwd_mean_ms=b[0], level_rows=[R0, R1, R2],
                                   flops_fwd=ffl, flops_bwd=bfl, compact_decoder_backward_rows=compact_rows,
                                   useful_flops=ufl, useful_tflops=ufl / ((t[0] + b[0]) * 1e-3) / 1e12,
                                   useful_frac=ufl / ((t[0] + b[0]) * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                                   present_tap_fraction={k_: round(v, 4) for k_, v in occ.items()},
                                   useful_note="`frac` = flops the gathered GEMMs EXECUTE (every row multiplies all 27 taps / 8 children; absent "
                                               "ones read a zero row); `useful_frac` = only the products with a present tap / child "
                                               "(present_tap_fraction per layer, from the timed mini-batch's tables).  Skipping absent taps "
                                               "needs rows grouped by presence pattern: in cell order no (64-row tile, tap) pair is empty "
                                               "(profiles/HISTORY.md, round 4 (d))",
                                   flops_bwd_dense_decoder=ffl + 2.0 * sum(dict(macs, conv0=0, up1=R1 * c1 * c1 + R2 * c1 * c2,
                                                                                 up0=R0 * c0 * c0 + R1 * c0 * c1).values()),
                                   note="3^3 / strided convolutions and the up layers' [unpool | skip] operands are gathered inside the "
                                        "GEMM's LDS-DMA loader (forward, weight gradient, the 3^3 data gradient through the mirrored "
                                        "table): no column / concatenated matrix in HBM except the strided layers' data gradients; "
                                        "flops = MACs of the GEMMs as executed (the un-pooled half of an up layer's data gradient runs "
                                        "on the coarse rows); kernel = gemm2_dma_kernel<..., GATHER>, 128 x 64 / 128 x 32 tiles on the "
                                        "64- / 32-channel levels")
    else:
        t = ops.TIMER.mean_ms("pointnet_enc_fwd")
        if t:
            flops = 2.0 * ENC_MAC_PER_POINT * args.points * mb
            tf = flops / (t[0] * 1e-3) / 1e12
            out["roofline"] = dict(bound="mfma", kernel="pn_fwd_kernel", achieved=tf, peak=PEAK_F32_MFMA_TFLOPS, unit="TFLOP/s",
                                   frac=tf / PEAK_F32_MFMA_TFLOPS, traffic=None, launches=t[1], mean_launch_ms=t[0],
                                   flops_per_launch=flops)
            b = ops.TIMER.mean_ms("pointnet_enc_bwd")
            if b:
                bflops = 2.0 * 2 * 256 * 128 * args.points * mb
                out["roofline"].update(enc_bwd_mean_ms=b[0], enc_bwd_executed_tflops=bflops / (b[0] * 1e-3) / 1e12,
                                       enc_bwd_frac=bflops / (b[0] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = lambda t: t.detach().cpu()
        cmb = 8 if sparse else 128            # the sparse restatement builds its voxel tables in Python: a smaller sample
        n_rows = 3 * cmb
        out["cpu_baseline"] = cpu_baseline_dagger(
            d, net, cpu(run.storage.observations.view(-1, d["O_s"])[:n_rows]), cpu(run.storage.tea_obs.view(-1, d["O_t"])[:n_rows]),
            {k: cpu(v).clone() for k, v in run.student.state_dict().items()},
            {k: cpu(v).clone() for k, v in run.teacher.state_dict().items()}, WORKLOADS["state"]["net"], rows, d["proprio"], cmb)
        out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
    return out


def make_cfg(w, device):
    return dict(num_envs=w["N"], obs_mode="obs", succ_value=None,
                model=dict(action_std=0.5, action_activate="tanh", clipAction=1.0, network=dict(w["net"])),
                max_iterations=200000, n_steps=w["T"], n_updates=5, n_minibatches=8, device=device, eval_round=1,
                eval_frequence=10 ** 9, save_frequence=10 ** 9, test_only=False, save_pose=False, save_video=False,
                lr_schedule="fixed", lr=5e-5, desired_kl=0.1, epsilon_clip=0.2, gamma=0.99, lam=0.95,
                tricks=dict(mini_adv_norm=False, whole_adv_norm=False, use_state_norm=False,
                            use_clipped_value_loss=False, use_grad_clip=True, max_grad_norm=0.5),
                sampler="sequential", resume=None)


# ------------------------------------------------------------------------------------------------ depth2pc
def run_depth2pc(args, device):
    """Observation-side step with the only timing the reference publishes: the cloud sampling
    of `TSDFVolume.depth2pc` for 64 envs x 6 views x 180 x 320 px -> 1024 points, "slow.. ~0.5s"
    (utils/depth2tsdf.py:158, unstated NVIDIA GPU).  A step = one depth2pc call (back-projection, crop, compaction,
    FPS, gather); `sampling_ms` isolates the part the reference's comment is about."""
    from partmanip_amd import ops
    from partmanip_amd.depth2tsdf import TSDFVolume
    b, m, h, w_ = 64, 6, 180, 320
    vol = TSDFVolume(device)
    pose = torch.eye(4).repeat(m, 1, 1)
    for i in range(m):
        pose[i, :3, 3] = torch.tensor([0.02 * i, -0.01 * i, -0.6])
    intr = [[250.0, 0.0, w_ / 2 - 0.5], [0.0, 250.0, h / 2 - 0.5], [0.0, 0.0, 1.0]]
    vol.register_camera(pose.numpy(), intr, h, w_, b)
    torch.manual_seed(0)
    depth = torch.rand(b, m, h, w_, device=device) * 0.5 + 0.45

    def timed(fn, n):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    metric = "depth2pc seconds per call, 64 envs x 6 views x 180x320 px -> 1024 pts"
    last = {}
    dt = timed(lambda: last.update(cloud=vol.depth2pc(depth)), args.steps)
    dump_outputs(args, 0, last)
    if not args.full:
        return dict(metric=metric, value=dt, unit="s",
                    n_gpus=1, steps=args.steps, warmup=args.warmup, ms_per_step=dt * 1e3, higher_is_better=False,
                    scaling="weak", dtype="f32", data="synthetic", config=dict(workload="depth2pc_64env_x_6view_x_180x320"))
    lo = vol._vol_origin.cpu().numpy()
    world = ops.depth_backproject(depth, vol.cam_pose, 250.0, 250.0, w_ / 2 - 0.5, h / 2 - 0.5, lo, vol._size + lo)
    ws = ops.Workspace(device)
    c0, n0 = ops.depth_compact(world)

    def sample():
        c, n = ops.depth_compact(world)
        ops.group_points(c, ops.fps_varlen(c, n, 1024, ws).view(b, 1024, 1))
    ds = timed(sample, args.steps)
    dfps = timed(lambda: ops.fps_varlen(c0, n0, 1024, ws), args.steps)
    valid = float((world != 0).any(-1).float().mean())
    # the other sampling call site (depth2tsdf.py:88-120, the 'depth_sparse' observation) on a scene with a surface:
    # a tilted plane seen by all views, 50^3 grid -> integrate + band select + FPS(1024) + gather
    yy, xx = torch.meshgrid(torch.arange(h, device=device), torch.arange(w_, device=device), indexing="ij")
    plane = (0.75 + 0.0004 * xx + 0.0006 * yy).float().expand(b, m, h, w_).contiguous()
    band = vol.integrate(plane).abs().lt(0.2).flatten(1).sum(-1).float().mean().item()
    dv = timed(lambda: vol.sparse_voxel(plane), args.steps)
    out = dict(metric=metric, value=dt, unit="s",
               n_gpus=1, steps=args.steps, warmup=args.warmup, ms_per_step=dt * 1e3, higher_is_better=False,
               scaling="weak", vs_baseline=ds / 0.5, dtype="f32", data="synthetic",
               config=dict(workload="depth2pc_64env_x_6view_x_180x320", sampling_ms=ds * 1e3, in_crop_fraction=valid,
                           sparse_voxel_ms=dv * 1e3, sparse_voxel_band_voxels=band,
                           baseline="'~0.5s' for the sampling alone, utils/depth2tsdf.py:158 (BASELINE.md); "
                                    "vs_baseline = sampling time / 0.5 s"))
    # dominant kernel: farthest-point sampling on G = 256 / envs work-groups per cloud (csrc/pointops.hip: fps_multi_kernel): each keeps
    # 25 600 points of its chunk in registers (512 threads x 50) and 10 176 in LDS for all K rounds; only a remainder beyond those
    # 35 776 re-reads its points (12 B) and running min-distance (4 B + 4 B back) every round
    on_reg, on_lds = (512 * 50, 10176) if not ops.FPS_POLICY.legacy_shape else (1024 * 16, 8192)
    nn = n0.to(torch.int64).cpu()
    G = max(1, min(8, 256 // b))
    chunk = (nn + G - 1) // G
    big = nn > 8192
    streamed = torch.where(big, (chunk - on_reg - on_lds).clamp(min=0) * G, nn.clamp(min=0) * 0).sum().item() if G >= 2 else float(nn[big].sum())
    pts = float(nn.sum().item())
    impl_bytes = 1024.0 * streamed * 20.0 + pts * 12.0          # what THIS implementation moves: the streamed remainder, every round
    algo_bytes = pts * 12.0 + b * 1024 * 4.0                      # the operator's own traffic: every candidate point once in, K indices out
    gbs = algo_bytes / dfps / 1e9
    # FPS is K = 1024 DEPENDENT rounds: round j's arg-max is round j + 1's reference point.  A round cannot be shorter than
    #  (1) the distance update of the largest chunk on ONE CU (G x B = 256 work-groups: one CU each).  Exact fp32, op by op as the
    #      reference rounds (3 sub, 3 mul, 2 add -- no FMA) = 8 packed-fp32 instructions per PAIR of points, + 2 min + 1 max3:
    #      5.5 VALU issue slots per point at the packed-fp32 rate the 157 TF vector peak assumes.  (Measured here packed fp32 runs
    #      at HALF that rate -- the scalar form of the same sweep takes the same time, profiles/round4_h_fps_multi_ab.txt -- i.e.
    #      9.5 slots per point, 2.07 us: `distance_update_valu_as_measured`.)  4 cycles per slot per 64 points per SIMD, 4 SIMDs;
    #  (2) one hand-off between the cloud's work-groups (drained write-through store + flag sweep: MI355X_MICROARCH.md price list,
    #      "handoff-flag", 1.3 us on an idle chip);
    #  (3) the dependent chain inside a work-group (wave maximum -> LDS -> barrier -> index recovery -> barrier, ~0.5 us).
    # That latency floor, not the HBM roofline, bounds the launch.
    sweep_us = float(chunk.max().item()) * 5.5 * 4.0 / 256.0 / 2400.0
    floor_us = sweep_us + 1.3 + 0.5
    out["roofline"] = dict(bound="hbm", kernel="fps_multi_kernel (on-chip chunks, streamed remainder)", achieved=gbs, peak=PEAK_HBM_GBS,
                           unit="GB/s", frac=gbs / PEAK_HBM_GBS, traffic=_hbm_traffic("fps_multi_kernel_bytes_per_launch")[0],
                           algorithmic_bytes=algo_bytes, mean_launch_ms=dfps * 1e3,
                           latency=dict(rounds=1024, us_per_round=dfps * 1e6 / 1024.0, floor_us_per_round=floor_us,
                                        frac_of_floor=floor_us / (dfps * 1e6 / 1024.0),
                                        floor_parts_us=dict(distance_update_valu=sweep_us, hand_off=1.3, work_group_arg_max=0.5,
                                                            distance_update_valu_as_measured=sweep_us * 9.5 / 5.5),
                                        note="K dependent rounds; floor = the exact-fp32 distance update of the largest chunk on one CU "
                                             "(5.5 VALU slots per point at the nominal packed-fp32 rate) + one cross-work-group hand-off (1.3 us, MI355X_MICROARCH.md "
                                             "'handoff-flag') + the in-work-group arg-max chain (~0.5 us)"),
                           implementation=dict(streamed_bytes_per_launch=impl_bytes, streamed_gbs=impl_bytes / dfps / 1e9,
                                               points=pts, points_streamed_per_round=float(streamed),
                                               points_on_chip_per_work_group=on_reg + on_lds,
                                               one_work_group_per_cloud_bytes=1024.0 * pts * 20.0,
                                               note=f"points that fit neither the registers ({on_reg} per work-group) nor LDS ({on_lds}) are "
                                                    "re-read every round (12 B + the running minimum 4 B in, 4 B out), mostly out of L2 / "
                                                    "Infinity Cache: `traffic` (PMC, HBM side) is what reaches memory"),
                           note="`achieved` = the operator's algorithmic bytes (each candidate point once, K indices out) over the launch "
                                "time: a latency-bound sampler sits far below the HBM roofline by construction -- `latency` is the bound "
                                "that applies; `traffic` / `algorithmic_bytes` shows what reaches HBM beyond reading the cloud once")
    if not args.no_cpu_baseline:
        from oracle import ref_cpu as R
        ncpu = os.cpu_count() or 1
        nt = 1                                            # the restatement is numpy, one thread
        nb = 2                                            # bounded sample: 2 of the 64 envs
        dc = depth[:nb].cpu()
        size = float(vol._size)
        R.depth2pc(dc[:1], pose, intr, size, lo, K=16)    # warm-up
        t0 = time.perf_counter()
        R.depth2pc(dc, pose, intr, size, lo, K=1024)
        tc = (time.perf_counter() - t0) * b / nb
        out["cpu_baseline"] = dict(value=tc, unit="s", cores=nt, kind="port", host_cpus=ncpu,
                                   sample=f"oracle/ref_cpu.py depth2pc (numpy, single-threaded) on {nb} of the {b} envs, scaled by {b // nb}")
        out["gpu_over_cpu"] = tc / dt
    return out


# ------------------------------------------------------------------------------------------------ PPO workloads
def build_runner(w, cfg, device, rank):
    """Runner + one synthetic rollout produced by the freshly initialised policy (ratio ~ 1, KL ~ 0) + the
    timed step: restore the initial policy / optimiser state, then the reference's `learn` window."""
    from partmanip_amd.algorithms import ppo
    from partmanip_amd.feeder import FeederEnv, ScreenLogger
    torch.manual_seed(1234)                            # identical initial weights on every rank
    env = FeederEnv(w["N"], {"obs": w["O"]}, w["A"], device, seed=1234 + rank)
    run = ppo(env, cfg, ScreenLogger(quiet=True))
    ac, st = run.actor_critic, run.storage
    obs = env.reset()["obs"]
    for _ in range(w["T"]):
        actions, logp, values, mu, sigma = ac.random_act_cri(obs)
        nxt, rew, done, _ = env.step(actions)
        st.add_transitions(obs, actions, rew, done, env.reset_succ, values, logp, mu, sigma)
        obs = nxt["obs"]
    last_values = ac.cri(obs)
    f = ac.flat()
    snap = dict(a=f["actor"].clone(), c=f["critic"].clone())

    def restore():                                     # every timed step starts from the same policy
        f["actor"].copy_(snap["a"])
        f["critic"].copy_(snap["c"])
        for opt in (run.optimizer_actor, run.optimizer_critic):
            opt.m.zero_()
            opt.v.zero_()
            opt.state_dev.zero_()

    def step():
        restore()
        st.step = w["T"]
        run.log_dict = {}
        run.learn(last_values)

    return run, ac, st, last_values, step


def _world_observed():
    d = torch.distributed
    return d.get_world_size() if d.is_available() and d.is_initialized() else 1


def _max_over_ranks(dt, device, world):
    if world == 1:
        return dt
    tmax = torch.tensor([dt], device=device, dtype=torch.float64)
    torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    return float(tmax.item())


def _dp_report(syncs, flats, dt_local, steps, device, world):
    """Data-parallel evidence for a multi-GPU line: every rank's own wall time per step, the time its all-reduces took
    (HIP events around each call on the issuing stream: partmanip_amd/dist.py GradSync.time_collectives), and an all-rank
    equality check of the parameters after the last step -- replicas that start equal and exchange every gradient must END
    equal, bit for bit; a silent divergence (a rank that skipped a collective, a different KL branch) fails the run here."""
    comm, calls = 0.0, 0
    for s_ in syncs:
        ms, n = s_.comm_ms()
        comm += ms
        calls += n
    mine = torch.tensor([dt_local / steps * 1e3, comm / steps, float(calls) / steps], device=device, dtype=torch.float64)
    cs = torch.stack([t.detach().double().sum() for t in flats] +
                     [t.detach().view(torch.int32).to(torch.int64).sum().double() for t in flats])
    if world > 1:
        allm = [torch.empty_like(mine) for _ in range(world)]
        allc = [torch.empty_like(cs) for _ in range(world)]
        torch.distributed.all_gather(allm, mine)
        torch.distributed.all_gather(allc, cs)
    else:
        allm, allc = [mine], [cs]
    equal = all(bool(torch.equal(allc[0], c)) for c in allc)
    rep = dict(per_rank_ms_per_step=[float(m[0]) for m in allm], comm_ms_per_step=max(float(m[1]) for m in allm),
               per_rank_comm_ms_per_step=[float(m[1]) for m in allm], all_reduces_per_step=float(allm[0][2]),
               param_checksum_equal=equal, param_checksum=[float(x) for x in allc[0]])
    if not equal:
        raise RuntimeError(f"data-parallel replicas diverged: parameter checksums differ across ranks: {[c.tolist() for c in allc]}")
    return rep


def _hbm_traffic(key):
    """HBM bytes per launch from the PMC pass (rocprofv3 --pmc in its own run, gfx950 corrections applied, as
    MI355X_MICROARCH.md prescribes; tools/pmc_run.sh -> profiles/hbm_traffic.json).  Counters cannot be collected from
    inside this process, so the figure is the committed measurement of the same kernel at the same launch shape."""
    tfile = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if not os.path.exists(tfile):
        return None, None
    j = json.load(open(tfile))
    return j.get(key), j.get("source")


def _gae_kernel_ms(st, n=32):
    """Mean duration of the GAE scan kernel over `n` launches captured in one hipGraph (the storage's own rollout tensors)."""
    from partmanip_amd import ops
    ret, adv = torch.empty_like(st.returns), torch.empty_like(st.advantages)
    last = st.values[-1].clone()
    sv = st.default_succ_value
    call = lambda: ops.gae_scan(st.rewards, st.values, st.dones, st.succs, last, ret, adv, 0.99, 0.95, sv)
    call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(n):
            call()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _linear_kernel_us(M, K, N, n=32):
    """Mean duration (us, launch boundary included) of the hidden-layer GEMM of the small-step regime -- forward, data gradient
    and weight gradient at (M x K) -> N -- each over `n` dependent launches replayed from one hipGraph."""
    from partmanip_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    x, w, b = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5, torch.zeros(N, device=dev)
    y, dy, dx = torch.empty(M, N, device=dev), torch.randn(M, N, device=dev), torch.empty(M, K, device=dev)
    dw, db, ws = torch.empty(N, K, device=dev), torch.empty(N, device=dev), ops.Workspace(dev)
    ws.get(ops.lib.pm_linear_bwd_weight_workspace_bytes(M, N, K))
    out = {}
    for name, call in (("fwd", lambda: ops.linear_fwd(x, w, b, y, ops.ACT_TANH)),
                       ("bwd_data", lambda: ops.linear_bwd_data(dy, w, x, dx, ops.ACT_TANH)),
                       ("bwd_weight", lambda: ops.linear_bwd_weight(dy, x, dw, db, ws))):
        call()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(n):
                call()
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) / n * 1e3
    return out


def run_ppo(args, device, rank, world):
    from partmanip_amd import ops
    w = dict(WORKLOADS[args.workload])
    if args.n_steps:
        w["T"] = args.n_steps
        w["name"] = w["name"] + f"_T{args.n_steps}"
    if args.precision != "f32" and w["net"]["name"] == "PointNet":
        w["net"] = dict(w["net"], precision=args.precision)
        w["name"] = w["name"] + "_" + args.precision
    cfg = make_cfg(w, device)
    run, ac, st, last_values, step = build_runner(w, cfg, device, rank)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    syncs = list({id(x): x for x in (run.sync, getattr(run, "sync_c", None)) if x is not None}.values())
    for s_ in syncs:
        s_.time_collectives(True)
    timers = ["gae_scan"]
    if args.workload == "vision":
        timers += ["pointnet_enc_fwd", "pointnet_enc_bwd"]
    ops.TIMER.enable(*timers)
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    ops.TIMER.disable()
    fl = ac.flat()
    dump_outputs(args, rank, dict(actor_params=fl["actor"], critic_params=fl["critic"], returns=st.returns, advantages=st.advantages,
                                  **{k: torch.tensor([float(v)], dtype=torch.float64) for k, v in run.log_dict.items()
                                     if k.startswith("Train/")}))
    if args.workload == "vision_pn2" and args.full:
        # per-kernel durations for the roofline block: ONE more step with actor and critic on one stream (in the timed region
        # they run on two and share the chip, which stretches every launch), outside the timed region
        ov = run.overlap
        run.overlap = False
        ops.TIMER.add(*[f"sa_{d}_{k}" for d in ("fwd", "bwd") for k in SA_LEVELS], "sa_groupall_fwd", "sa_groupall_bwd", "sa_dy_consume",
                      *PN2_GLUE_GEMMS)
        step()
        torch.cuda.synchronize()
        ops.TIMER.disable()
        run.overlap = ov
    dt_local = dt
    dt = _max_over_ranks(dt, device, world)
    ms_per_step = dt / args.steps * 1e3
    value = w["N"] * w["T"] * world / (dt / args.steps)
    dp = None
    if world > 1 or syncs:
        fl = ac.flat()
        dp = _dp_report(syncs, [fl["actor"], fl["critic"]], dt_local, args.steps, device, world)
        dp["graph_mode"] = (run.graph_status or run.dp_graph_mode) if run.use_graphs else "eager (no hipGraph replay for this backbone)"
        # None, or what the learner fell back to when the first all-reduce of its second communicator failed on some rank
        # (partmanip_amd/dist.py GradSync.probe: time-boxed, agreed over the rendezvous store, diagnosis on stderr)
        dp["degraded"] = getattr(run, "dp_degraded", None)
        if dp["degraded"]:
            dp["graph_mode"] = "eager (degraded: see `degraded`)"

    vision = args.workload.startswith("vision")
    metric = ("PPO env-steps/sec (whole node), 4096 envs x 1024-pt clouds" if vision
              else "PPO env-steps/sec (whole node), 4096 envs x 128 steps, state obs (BASELINE cfg 2)")
    out = dict(metric=metric, value=value, unit="env-steps/s",
               n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=ms_per_step, higher_is_better=True,
               scaling="weak", vs_baseline=None, dtype="f32" if args.precision == "f32" else f"f32 (encoder forward: {args.precision} split MFMA)",
               data="synthetic",
               config=dict(workload=w["name"], envs_per_gpu=w["N"], n_steps=w["T"], points=1024 if vision else 0,
                           minibatch=2048, n_updates=5, parallelism=f"dp{world}", world_size_observed=_world_observed(),
                           backend=(torch.distributed.get_backend() if world > 1 else None),
                           train_scalars={k: float(v) for k, v in run.log_dict.items() if k.startswith("Train/")}))
    if args.workload == "vision":
        out["config"]["workload_note"] = ("PointNet -- the backbone the reference ships for this task (algo_utils/network.py:141-198); BASELINE.json "
                                     "configs[2] words it as PointNet2, which the snapshot does not contain: the same 4096 env x 8 step x 1024-pt "
                                     "rollouts through the PointNet2 plug-in (HIP FPS + ball query + fused set-abstraction kernels) are "
                                     "`secondary.vision_pn2` of this line under --full (--workload vision_pn2), with their own roofline, traffic and CPU baseline")
    if dp is not None:
        out["config"]["data_parallel"] = dp
        out["comm_ms_per_step"] = dp["comm_ms_per_step"]
    gae = ops.TIMER.mean_ms("gae_scan")
    gae_blk = None
    if gae and args.full:
        nbytes = 18.0 * w["T"] * w["N"]                    # r, V 8 B + 2 mask B in; ret, adv 8 B out
        # the iteration launches the scan ONCE, between host work: events around that single ~10 us launch mostly time
        # its dispatch.  The kernel's own rate is taken from 32 launches replayed from one hipGraph on scratch outputs.
        k_ms = _gae_kernel_ms(run.storage) if not args.lean else gae[0]
        gae_blk = dict(kernel="gae_scan_kernel", bound="hbm", mean_launch_ms=k_ms, launches=32, bytes_per_launch=nbytes,
                       achieved_gbs=nbytes / (k_ms * 1e-3) / 1e9, frac=nbytes / (k_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                       in_iteration_event_ms=gae[0], in_iteration_launches=gae[1],
                       note="mean_launch_ms: 32 back-to-back launches replayed from a hipGraph (same rollout tensors, scratch "
                            "outputs); in_iteration_event_ms: HIP events around the iteration's single launch (dispatch included)")
    if args.workload == "vision":
        mean_ms, n_launch = ops.TIMER.mean_ms("pointnet_enc_fwd")
        flops = 2.0 * ENC_MAC_PER_POINT * 1024 * 2048           # one launch = 2048 clouds x 1024 points
        achieved = flops / (mean_ms * 1e-3) / 1e12
        traffic, tsrc = _hbm_traffic("pn_fwd_kernel_bytes_per_launch")
        out["roofline"] = dict(bound="mfma", kernel="pn_fwd_kernel", achieved=achieved, peak=PEAK_F32_MFMA_TFLOPS,
                               unit="TFLOP/s", frac=achieved / PEAK_F32_MFMA_TFLOPS, traffic=traffic,
                               launches=n_launch, mean_launch_ms=mean_ms, flops_per_launch=flops,
                               traffic_source=tsrc,
                               traffic_note="the TRAINING forward also writes the layer-2 activations (1 KB/point = 2.15 GB per "
                                            "launch) that spare the backward a recompute: the traffic is ~1.1x the training "
                                            "forward's algorithmic bytes (2.19 GB) but ~60x the op's own 38.5 MB (points in, "
                                            "features out); at < 0.5 TB/s (6 % of the HBM peak) the kernel stays MFMA-bound "
                                            "(DESIGN.md 3.2: backward -0.69 ms, forward +0.25 ms)")
        # What the dominant kernel's time is made of: measured on ablation builds of pn_fwd_kernel in round 6
        # (profiles/round6_pn_fwd_ablation.txt: -DPN_ABLATE builds, tools/time_enc.py, 2048 clouds).  The parts ADD UP to the launch:
        # on gfx950 a SIMD's MFMA, VALU and VMEM issue slots are one port (profiles/HISTORY.md 3.2 micro-benchmarks).
        out["roofline"]["floor_ms"] = dict(
            mfma_at_2p4ghz=2.0 * ENC_MAC_PER_POINT * 1024 * 2048 / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e3,
            mfma_and_barriers_measured=4.58, operand_issue=0.28, valu_stages=0.57,
            valu_stage_parts=dict(layer1=0.095, layer2_tanh=0.087, saved_h2_copy=0.17, pooling=0.0, only_removable_together=0.22),
            sum_of_parts=4.58 + 0.28 + 0.57, measured_same_run=5.43, this_run=mean_ms,
            counters=dict(source="tools/pmc_issue.sh over tools/time_enc.py, profiles/round6_c_pmc_issue_encoder.json (per SIMD, per launch)",
                          launch_cycles=12.94e6, valu_mfma_coexec_cycles=0, mfma_busy_cycles=10.49e6, non_mfma_valu_insts=309e3,
                          vmem_read_insts=24.3e3, lds_insts=42.3e3, sum_of_issue_cycles=12.64e6,
                          note="SQ_VALU_MFMA_COEXEC_CYCLES = 0: VALU and MFMA work never overlapped on a SIMD; 10.49 M MFMA cycles + 309 k VALU "
                               "instructions x 4 + 24.3 k VMEM reads x 27 + 42.3 k LDS instructions x 5 = 12.64 M of the launch's 12.94 M "
                               "cycles -- the counters and the ablation builds give the same sum; pn_bwd16_kernel likewise (5.81 M of 5.79 M)"),
            note="MFMAs + the five barriers per tile alone: 4.58 ms (= the 4.37 ms of 5120 MFMAs per 64-point tile at 2.4 GHz, at the "
                 "~2.29 GHz the chip sustains under this load, barriers included); streaming the operands (ds_read_b128 + "
                 "global_load_dwordx4 per 16 MFMAs) +0.28; layer 1, the two tanh epilogues and the saved-layer-2 copy +0.57 "
                 "(pooling is free: it waits for the MFMA results anyway).  4.58 + 0.28 + 0.57 = 5.43 = the measured launch: "
                 "0.80 of the 2.4 GHz peak (0.84 of the sustained-clock peak) is this structure's SUM, not a scheduling loss; "
                 "0.86 needs 0.35 ms of VALU / VMEM work removed (the saved-h2 copy buys the backward 0.69 ms; halving the operand "
                 "issue needs 128-point tiles = one work-group per CU)")
        bwd = ops.TIMER.mean_ms("pointnet_enc_bwd")
        if bwd:
            out["roofline"]["enc_bwd_mean_ms"] = bwd[0]
            # second kernel of the step: the structured backward EXECUTES 2 dense GEMMs (dW2 = dz2^T h1, dh1 = dz2 W2:
            # 2 x 2*256*128 flops per point); the timer brackets the whole C call (kernel + its five small follow-ups)
            bflops = 2.0 * 2 * 256 * 128 * 1024 * 2048
            out["roofline"]["enc_bwd_executed_tflops"] = bflops / (bwd[0] * 1e-3) / 1e12
            out["roofline"]["enc_bwd_frac"] = out["roofline"]["enc_bwd_executed_tflops"] / PEAK_F32_MFMA_TFLOPS
            # whole iteration: the MFMA flops the two encoder calls EXECUTE per network step (forward 688.8 G + backward
            # 274.9 G, the latter = SQ_INSTS_VALU_MFMA_MOPS_F32 x 512 of pn_bwd16_kernel, profiles/hbm_traffic.json) x the
            # network steps of the iteration, over the iteration's wall time -- every launch gap, head, loss and optimiser inside
            net_steps = 2 * cfg["n_updates"] * (w["N"] * w["T"] // 2048)
            it_flops = net_steps * (flops + bflops)
            it_tf = it_flops / (ms_per_step * 1e-3) / 1e12
            enc_ms = net_steps * (mean_ms + bwd[0])
            out["roofline"]["iteration"] = dict(
                executed_flops=it_flops, network_steps=net_steps, executed_tflops=it_tf, frac=it_tf / PEAK_F32_MFMA_TFLOPS,
                encoder_calls_ms=enc_ms, outside_encoder_calls_ms=ms_per_step - enc_ms,
                survey_30F_useful_tflops=30.0 * 2.0 * (ENC_MAC_PER_POINT * 1024 + 135488) * w["N"] * w["T"] / (ms_per_step * 1e-3) / 1e12,
                note="SURVEY 8d / BASELINE.md 4 price an env-step at 30 F (fwd + 2 x bwd per net and epoch, F = 336.6 MFLOP) "
                     "-> a 15.6 k env-steps/s ceiling at 157.3 TFLOP/s.  That ceiling no longer applies: the structured backward "
                     "(DESIGN.md 3.2) eliminates the 256->512 layer's two backward GEMMs algebraically (max-pool gradient = one row "
                     "per channel, layer 3 linear), so a backward EXECUTES 0.4 F instead of 2 F.  `frac` here is executed flops "
                     "/ wall / peak; survey_30F_useful_tflops (> peak) is the same wall time priced the survey's way")
    if args.workload == "vision_pn2" and args.full:
        # the four fused set-abstraction kernels.  They run over each group's DISTINCT rows (ball query pads a short group with
        # copies of its first hit, and a copy never wins the max-pool: DESIGN.md 3.4), so `achieved` counts the MFMA flops of
        # the distinct rows of one 2048-cloud mini-batch -- fwd: layers 2-3; bwd: dH2 + dW2 + dH1 (layer 2 is loaded from what
        # the forward saved) -- and `dense_equivalent_tflops` what the padded 32-row groups would have needed in the same time
        net = ac.actor
        tabs = net.precompute_geometry(st.observations.view(-1, w["O"])[:2048])
        wsb = ops.Workspace(torch.device(device))
        kern, lv = {}, {}
        for l, (k, (c1, c2, c3, S)) in enumerate(SA_LEVELS.items()):
            # level l samples its centres among level l - 1's centres (level 0: the cloud itself)
            xyz_l = (st.observations.view(-1, w["O"])[:2048, :net.point_num * net.in_channels].reshape(2048, net.point_num, net.in_channels)[..., :3].contiguous()
                     if l == 0 else tabs[l - 1][0].contiguous())
            if getattr(net, "unique_rows", False):
                R_, T_ = ops.sa_plan(tabs[l][1].contiguous(), xyz_l, tabs[l][0].contiguous(), (c1, c2, c3), wsb).counts()
            else:
                R_, T_ = 2048 * S * 32, 2048 * S * 32 // 64
            dense = 2048.0 * S * 32
            G_ = 2048.0 * S
            lv[k] = dict(distinct_rows=R_, padded_rows=int(dense), rows_per_group=R_ / G_, tiles=T_)
            yb = R_ * c1 * 4.0 if l > 0 else 0.0               # level 2 gathers / scatters the per-source-point layer-1 rows
            algo = dict(fwd=R_ * (c2 * 4.0 + 8 + 12) + yb + G_ * c3 * 8.0,                    # h2 out, rowmap, xyz, pooled + arg out
                        bwd=R_ * (c2 * 4.0 + 8 + 12) + 2 * yb + G_ * c3 * 12.0)               # h2 in, Y in, dz1 rows out (round 6: no dY read-modify-write), pooled / dpooled / arg in
            for d_, macs in (("fwd", c1 * c2 + c2 * c3), ("bwd", 2 * c1 * c2 + c2 * c3)):
                t = ops.TIMER.mean_ms(f"sa_{d_}_{k}")
                if t:
                    tf = 2 * R_ * macs / (t[0] * 1e-3) / 1e12
                    traffic = _hbm_traffic(f"sa_{d_}_{k}_bytes_per_launch")[0]
                    kern[f"sa_{d_}_{k}"] = dict(mean_launch_ms=t[0], launches=t[1], tflops=tf, frac=tf / PEAK_F32_MFMA_TFLOPS,
                                                dense_equivalent_tflops=2 * dense * macs / (t[0] * 1e-3) / 1e12,
                                                algorithmic_bytes=algo[d_], traffic=traffic)
        # the consumer of level 2's layer-1 gradient rows (round 6): fixed-order per-source-point sums in LDS + dfeat = dY W1f +
        # dW1f = dY^T feat on MFMA, one launch (was: zero-fill + fp32 atomics + two Linear launches + slab reduction + column copy)
        tcons = ops.TIMER.mean_ms("sa_dy_consume")
        if tcons and "128x128x256" in lv:
            npts, c1_, cf_ = 2048.0 * net.npoints[0], 128, 128
            fl = 2.0 * 2.0 * npts * c1_ * cf_
            tf = fl / (tcons[0] * 1e-3) / 1e12
            kern["sa_dy_consume_128x128"] = dict(mean_launch_ms=tcons[0], launches=tcons[1], tflops=tf, frac=tf / PEAK_F32_MFMA_TFLOPS,
                                                 algorithmic_bytes=lv["128x128x256"]["distinct_rows"] * c1_ * 4.0 + 2 * npts * cf_ * 4.0, traffic=None,
                                                 deterministic=True,
                                                 note="dY = per-source-point sums of the packed rows' gradient in ascending row order (the plan's "
                                                      "inverse table): no floating-point atomics, dY never written to HBM")
        glue = {}
        for n_, fl_ in PN2_GLUE_GEMMS.items():
            tg = ops.TIMER.mean_ms(n_)
            if tg:
                glue[n_] = dict(mean_call_ms=tg[0], calls=tg[1], tflops=fl_ / (tg[0] * 1e-3) / 1e12, frac=fl_ / (tg[0] * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS)
        if glue:
            tot_ms, tot_fl = sum(v["mean_call_ms"] for v in glue.values()), sum(PN2_GLUE_GEMMS[k_] for k_ in glue)
            glue["all"] = dict(ms_per_network_step=tot_ms, tflops=tot_fl / (tot_ms * 1e-3) / 1e12, frac=tot_fl / (tot_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                               note="gemm2_dma_kernel (128 x 64 tiles) on K = 128 / 256 / 288: 4-9 K-steps per tile, i.e. prologue + epilogue per tile "
                                    "weigh as much as the loop; 32 FLOP per HBM byte at K = N = 128 -- these launches sit ON the roofline's ridge "
                                    "(0.10 ms of HBM time against 0.11 ms of MFMA time for the first one)")
        # group-all level: its last layer (256 -> 512 over 64 rows per cloud) fused with the max over the cloud; the backward call
        # = dH (sorted winners, one running sum per column) + dW gather + finish: 3 x 2048 x 512 x 256 multiply-adds instead of
        # the two dense GEMMs (2 x 34.4 GFLOP) on the one-non-zero-per-(cloud, channel) gradient (csrc/sa_groupall.hip)
        ga = {}
        if getattr(net, "_ga_fused", False):
            gf, gb = ops.TIMER.mean_ms("sa_groupall_fwd"), ops.TIMER.mean_ms("sa_groupall_bwd")
            rows_ga = 2048.0 * net.npoints[-1]
            if gf:
                tf = 2.0 * rows_ga * 256 * 512 / (gf[0] * 1e-3) / 1e12
                ga["fwd"] = dict(mean_launch_ms=gf[0], launches=gf[1], tflops=tf, frac=tf / PEAK_F32_MFMA_TFLOPS,
                                 algorithmic_bytes=rows_ga * 256 * 4.0 + 2048 * 512 * 8.0,
                                 traffic=_hbm_traffic("ga_fwd_kernel_bytes_per_launch")[0])
            if gb:
                by = rows_ga * 256 * 4.0 * 2 + 2048 * 512 * 16.0           # H in, dH out, pooled / gradient / arg-max in
                tb = [_hbm_traffic(f"{k}_bytes_per_launch")[0] for k in ("ga_bwd_dh_kernel", "ga_dw_gather_kernel", "ga_dw_finish_kernel")]
                ga["bwd"] = dict(mean_call_ms=gb[0], calls=gb[1], algorithmic_bytes=by, achieved_gbs=by / (gb[0] * 1e-3) / 1e9,
                                 traffic=sum(tb) if all(t is not None for t in tb) else None,
                                 frac_of_hbm=by / (gb[0] * 1e-3) / 1e9 / PEAK_HBM_GBS, dense_gemm_flops_not_executed=2 * 2.0 * rows_ga * 256 * 512)
        if kern:
            name = max(kern, key=lambda n: kern[n]["mean_launch_ms"] * kern[n]["launches"])
            out["roofline"] = dict(group_all=ga, glue_gemms=glue, bound="mfma", kernel=name, achieved=kern[name]["tflops"], peak=PEAK_F32_MFMA_TFLOPS,
                                   unit="TFLOP/s", frac=kern[name]["tflops"] / PEAK_F32_MFMA_TFLOPS, traffic=kern[name]["traffic"],
                                   algorithmic_bytes=kern[name]["algorithmic_bytes"],
                                   launches=kern[name]["launches"], mean_launch_ms=kern[name]["mean_launch_ms"], kernels=kern,
                                   levels=lv, sa_kernels_ms_per_network_step=sum(v["mean_launch_ms"] for v in kern.values()),
                                   actor_critic_on_two_streams=bool(run.overlap),
                                   note="flops = MFMA flops of the DISTINCT rows (no copy of a group's first hit is computed); "
                                        "`dense_equivalent_tflops` prices the same launch at the padded 32 rows per group the "
                                        "round-1..3 kernels executed (it may exceed the peak: that work is not done any more); the "
                                        "distinct-row count is data dependent (`levels`): clouds whose balls hold >= 32 points fall "
                                        "back to the dense cost (tests/test_gpu_kernels.py::test_sa_packed_rows_equal_the_dense_level)")
    if args.workload == "state":
        # 33.3 MFLOP of useful work per env-step (n_updates x 3 x (F_actor + F_critic)); the step is
        # 2 x 1280 dependent mini-batch updates of 2048 samples
        F = lambda dims: 2.0 * sum(a * b for a, b in zip(dims, dims[1:]))
        hid = w["net"]["hid_dim"]
        per_env_step = 5 * 3 * (F([w["O"]] + hid + [w["A"]]) + F([w["O"]] + hid + [1]))
        tf = per_env_step * w["N"] * w["T"] / (dt / args.steps) / 1e12
        # algorithmic HBM bytes of one iteration: GAE 18 B per env-step + the update's rollout reads (actor 340 B +
        # critic 220 B per env-step and epoch) + per optimiser step the fused clip + Adam pass over each network's parameters
        # (p, g, m, v in; p, m, v out = 28 B per parameter; they stay L2-resident between the 2560 steps, so HBM sees far less)
        n_par = sum(a * b + b for a, b in zip([w["O"]] + hid, hid + [w["A"]])) + sum(a * b + b for a, b in zip([w["O"]] + hid, hid + [1]))
        steps_it = cfg["n_updates"] * (w["N"] * w["T"] // 2048)
        algo_roll = (18.0 + cfg["n_updates"] * (340.0 + 220.0)) * w["N"] * w["T"]
        algo_opt = 28.0 * n_par * steps_it
        out["roofline"] = dict(bound="mfma", kernel="whole learner iteration (2 x 1280 dependent MLP mini-batch updates)",
                               achieved=tf, peak=PEAK_F32_MFMA_TFLOPS, unit="TFLOP/s", frac=tf / PEAK_F32_MFMA_TFLOPS,
                               traffic=_hbm_traffic("state_iteration_bytes")[0], algorithmic_bytes=algo_roll + algo_opt,
                               algorithmic_bytes_rollout=algo_roll, algorithmic_bytes_optimiser_state=algo_opt,
                               traffic_note="HBM bytes of ONE iteration, all kernels (PMC FETCH_SIZE x 2 + WRITE_SIZE summed over every "
                                            "launch of `bench.py --workload state --lean`, profiles/hbm_traffic.json); the optimiser-state "
                                            "term of algorithmic_bytes is what the 2560 steps touch, almost all of it out of L2",
                               flops_per_env_step=per_env_step,
                               note="algorithmic flops of the iteration / its wall time: every launch gap is inside")
        if args.full and rank == 0 and world == 1 and not args.lean and run.use_graphs and run.graph_steps > 1:
            # What bounds the iteration with TODAY's kernels ("a stated ceiling rather than an open question").  Each
            # network's epoch is a list of 16-step hipGraphs; replayed ALONE on the idle chip they give that network's dependent-launch
            # chain time -- kernel durations + in-graph launch boundaries, no host, no contention.  The iteration cannot beat
            # n_updates x max(actor chain, critic chain) however well the two streams overlap, and needs no more than their sum.
            g = run._graphs
            floor = {}
            for tag, stream in (("a", torch.cuda.current_stream()), ("c", run._side)):
                keys = [k for k in g if isinstance(k, tuple) and k[0] == tag and k[-1] not in ("pre", "post")]
                if not keys:
                    continue
                with torch.cuda.stream(stream):
                    for k in keys:
                        g[k].replay()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in keys:
                        g[k].replay()
                    torch.cuda.synchronize()
                    floor[tag] = (time.perf_counter() - t0, sum(len(k) - 1 for k in keys))
            if "a" in floor and "c" in floor:
                (ta, na), (tc, nc) = floor["a"], floor["c"]
                mf = lambda dims: 3 * 2048 * F(dims) / (PEAK_F32_MFMA_TFLOPS * 1e12)
                per_it = lambda t_epoch: w["N"] * w["T"] / (cfg["n_updates"] * t_epoch)
                # the PHYSICAL floor: a network step is ~9.1 dependent launches (profiles/round5_d_bench_state_kernel_stats.csv:
                # 79 302 launches of the step's eight kernels over 8 704 network steps) at the guide's dependent-boundary cost inside a
                # GEMM chain (MI355X_MICROARCH.md `boundary` row: 1.1-1.4 us; 1.2 taken) + its MFMA work at the fp32 peak; the two
                # networks' chains share one chip, so a PAIR of steps cannot beat the sum of their MFMA work nor the longer chain
                LPS, BOUNDARY_US = 9.1, 1.2
                mfa, mfc = mf([w["O"]] + hid + [w["A"]]) * 1e6, mf([w["O"]] + hid + [1]) * 1e6
                phys_pair = max(mfa + mfc, max(mfa, mfc) + LPS * BOUNDARY_US)
                out["roofline"]["physical_floor_us_per_step"] = dict(
                    launches_per_network_step=LPS, boundary_us=BOUNDARY_US, mfma_at_peak_actor=mfa, mfma_at_peak_critic=mfc,
                    chain_floor_actor=mfa + LPS * BOUNDARY_US, chain_floor_critic=mfc + LPS * BOUNDARY_US, pair_floor=phys_pair,
                    ceiling_env_steps_per_s=per_it(phys_pair * 1e-6 * na),
                    measured_over_floor=(dt / args.steps / (cfg["n_updates"] * na) * 1e6) / phys_pair,
                    note="what no schedule of THIS algorithm on this chip can beat: per network step 9.1 dependent launch boundaries at 1.2 us "
                         "+ the step's MFMA work at 157.3 TFLOP/s; per (actor, critic) pair the larger of the two networks' summed MFMA "
                         "work and the longer chain.  The measured chains (next block) are 2.5 x their chain floor: a 2048 x 512 x 512 "
                         "layer takes 14.8 us where its MFMAs need 6.8 -- depth of the K loop at 128 tiles per launch, every XCD "
                         "re-fetching W; round 6 A/B: each network on its own half of every XCD's CUs (CU-masked streams; a mask "
                         "cannot select XCDs) measured 2.04 M against 2.29 M env-steps/s, profiles/round6_cfg2_cu_split_ab.txt")
                out["roofline"]["chains_measured_us_per_step"] = dict(
                    actor_chain_alone=ta / na * 1e6, critic_chain_alone=tc / nc * 1e6, steps_per_epoch=na,
                    mfma_at_peak_actor=mf([w["O"]] + hid + [w["A"]]) * 1e6, mfma_at_peak_critic=mf([w["O"]] + hid + [1]) * 1e6,
                    measured_pair=dt / args.steps / (cfg["n_updates"] * na) * 1e6,
                    ceiling_env_steps_per_s_perfect_overlap=per_it(max(ta, tc)), env_steps_per_s_no_overlap=per_it(ta + tc),
                    overlap_efficiency=(ta + tc - dt / args.steps / cfg["n_updates"]) / min(ta, tc),
                    note="a MEASUREMENT of today's kernels, not a floor (it was reported as `floor_us_per_step` in round 5): "
                         "chains = one epoch of a network's 16-step hipGraphs replayed alone on the idle chip (sum of its ~9 kernels per "
                         "step + in-graph launch boundaries); measured_pair = wall time of the iteration per (actor step, critic step) "
                         "pair with both chains sharing the chip; overlap_efficiency = the fraction of the shorter chain hidden under "
                         "the longer one.  Beating ceiling_env_steps_per_s_perfect_overlap needs faster kernels or fewer launch "
                         "boundaries per step, not better scheduling")
        if args.full and rank == 0 and not args.lean:
            # the dominant kernel on its own: a hidden layer (mini-batch x 512 x 512) on gemm2_dma_kernel, 32 dependent launches
            # replayed from a graph on the otherwise idle chip (in the iteration two networks' chains share it)
            Bm, H = 2048, hid[0]
            us = _linear_kernel_us(Bm, H, H)
            fl = 2.0 * Bm * H * H
            out["roofline"]["hidden_layer_gemm"] = dict(
                kernel="gemm2_dma_kernel (LDS-DMA fed v_mfma_f32_32x32x2_f32)", shape=[Bm, H, H], launches=32,
                us_per_launch=us, tflops={k: fl / (v * 1e-6) / 1e12 for k, v in us.items()},
                frac={k: fl / (v * 1e-6) / 1e12 / PEAK_F32_MFMA_TFLOPS for k, v in us.items()},
                traffic={k: _hbm_traffic(f"linear_2048x512x512_{k}_bytes_per_launch")[0] for k in us} if (Bm, H) == (2048, 512) else None,
                algorithmic_bytes=(2 * Bm * H + H * H) * 4,
                note="launch boundary included; bwd_weight = split-K GEMM + slab reduction as the single-problem entry point runs it; "
                     "traffic: HBM bytes per launch of the GEMM kernel from the committed PMC pass (profiles/hbm_traffic.json, "
                     "round2_l_pmc_linear.json) -- every XCD fetches the whole weight matrix into its own L2")
    if gae_blk:
        out.setdefault("roofline", {})["gae_scan"] = gae_blk
    if args.workload == "vision" and args.precision == "f32" and world == 1 and not args.no_optional:
        out["optional_paths"] = optional_paths(run, ac, w, step, fence)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = lambda t: t.detach().cpu()
        roll = dict(observations=cpu(st.observations), actions=cpu(st.actions), values=cpu(st.values),
                    returns=cpu(st.returns), actions_log_prob=cpu(st.actions_log_prob), advantages=cpu(st.advantages),
                    mu=cpu(st.mu), sigma=cpu(st.sigma), rewards_full=cpu(st.rewards), values_full=cpu(st.values),
                    dones_full=cpu(st.dones), succs_full=cpu(st.succs), last_values=cpu(last_values))
        sd_cpu = {k: cpu(v).clone() for k, v in ac.state_dict().items()}
        out["cpu_baseline"] = cpu_baseline_ppo(w, roll, sd_cpu, cfg)
        out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
    return out


def optional_paths(run, ac, w, step, fence):
    """The same workload on the opt-in paths (reported next to, not instead of, the exact-fp32 line)."""
    from partmanip_amd import ops

    enc = {}

    def timed(n=2, tag=None):
        # one untimed step of the SAME variant first (clock / power state after the previous variant's kernels: a bf16-dense
        # launch leaves the next fp32 forward at 5.65-6.3 ms instead of 5.45), then n timed steps with the encoder
        # calls bracketed, so that every variant reports its own encoder_fwd_ms / encoder_bwd_ms
        step()
        fence()
        ops.TIMER.enable("pointnet_enc_fwd", "pointnet_enc_bwd")
        t1 = time.perf_counter()
        for _ in range(n):
            step()
        fence()
        dt_ = (time.perf_counter() - t1) / n
        f_, b_ = ops.TIMER.mean_ms("pointnet_enc_fwd"), ops.TIMER.mean_ms("pointnet_enc_bwd")
        ops.TIMER.disable()
        if tag:
            enc[tag] = dict(encoder_fwd_ms=f_[0] if f_ else None, encoder_bwd_ms=b_[0] if b_ else None)
        return dt_
    res = {}
    ac.actor.precision = ac.critic.precision = "bf16x3"
    dt3 = timed(tag="bf16x3")
    res["encoder_forward_bf16x3"] = dict(
        value=w["N"] * w["T"] / dt3, unit="env-steps/s", ms_per_step=dt3 * 1e3, **enc["bf16x3"],
        note="pm_pointnet_enc_fwd_bf3: a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on bf16 MFMAs, fp32 accumulate; "
             "~1e-5 relative; passes the golden vision-PPO cases at the fp32 path's tolerances; backward stays fp32")
    ac.actor.precision = ac.critic.precision = "bf16x6"
    dt6 = timed(tag="bf16x6")
    ac.actor.precision = ac.critic.precision = "f32"
    res["encoder_forward_bf16x6"] = dict(
        value=w["N"] * w["T"] / dt6, unit="env-steps/s", ms_per_step=dt6 * 1e3, **enc["bf16x6"],
        note="pm_pointnet_enc_fwd_bf6: operands split into three bf16 planes, products a0b0+a0b1+a1b0+a0b2+a1b1+a2b0 "
             "on bf16 MFMAs with fp32 accumulate; error against fp64 no larger than the fp32 MFMA kernel's "
             "(tests/test_gpu_learner.py::test_pointnet_bf16x6_forward_has_fp32_class_error); backward stays fp32")
    # both encoder directions on the three-plane split: forward as above + dW2 / dh1 of the backward
    ac.actor.precision = ac.critic.precision = "bf16x6"
    ac.actor.precision_bwd = ac.critic.precision_bwd = "bf16x6"
    dt66 = timed(tag="bf16x6x2")
    f66 = (enc["bf16x6x2"]["encoder_fwd_ms"],) if enc["bf16x6x2"]["encoder_fwd_ms"] else None
    b66 = (enc["bf16x6x2"]["encoder_bwd_ms"],) if enc["bf16x6x2"]["encoder_bwd_ms"] else None
    ac.actor.precision = ac.critic.precision = "f32"
    ac.actor.precision_bwd = ac.critic.precision_bwd = "f32"
    peak6 = 2500.0 / 6.0                                          # dense bf16 MFMA peak / six products per fp32 product
    fl66 = 2.0 * ENC_MAC_PER_POINT * 1024 * 2048
    res["encoder_bf16x6_forward_and_backward"] = dict(
        value=w["N"] * w["T"] / dt66, unit="env-steps/s", ms_per_step=dt66 * 1e3,
        dtype="bf16 x 3 planes x 6 products, fp32 accumulate (fp32-class error); layer 1, tanh, pooling, dW3, optimiser: f32",
        encoder_fwd_ms=f66[0] if f66 else None, encoder_bwd_ms=b66[0] if b66 else None,
        roofline=dict(bound="mfma", unit="TFLOP/s", peak=peak6,
                      peak_note="2.5 PFLOP/s dense bf16 / 6 MFMAs per fp32-equivalent product = 417 TFLOP/s of fp32-equivalent flops",
                      achieved=(fl66 / (f66[0] * 1e-3) / 1e12) if f66 else None,
                      frac=(fl66 / (f66[0] * 1e-3) / 1e12 / peak6) if f66 else None,
                      kernel="pn_fwd_bf6_kernel (fp32-equivalent flops of a 2048-cloud launch; the rollout's 4096-cloud "
                             "launches are in the mean)"),
        note="pm_pointnet_enc_fwd_bf6 + pm_pointnet_enc_bwd_bf6 (csrc/pointnet_enc_bwd_bf6.h): every parameter gradient within "
             "the fp32 MFMA kernel's error against fp64 (tests/test_gpu_learner.py::"
             "test_pointnet_bf16x6_backward_has_fp32_class_error); golden vision-PPO cases at the fp32 tolerances; "
             "NOT the headline: the default line stays exact fp32")
    run.overlap = True
    dto = timed(tag="two_streams")
    run.overlap = False
    res["actor_critic_on_two_streams"] = dict(
        value=w["N"] * w["T"] / dto, unit="env-steps/s", ms_per_step=dto * 1e3, **enc["two_streams"],
        note="PARTMANIP_OVERLAP=1: same arithmetic, critic step k runs concurrently with actor step k")
    return res


def _brief(line):
    """The part of a workload's line that the default line carries as a `secondary` entry."""
    r = line.get("roofline") or {}
    keep = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes", "fwd_mean_ms", "bwd_mean_ms",
            "level_rows", "flops_per_env_step", "mean_launch_ms", "kernels", "levels", "latency", "traffic_note", "glue_gemms")
    out = dict(metric=line["metric"], value=line["value"], unit=line["unit"], steps=line["steps"], warmup=line["warmup"],
               ms_per_step=line["ms_per_step"], dtype=line["dtype"], workload=line["config"]["workload"],
               roofline={k: r[k] for k in keep if k in r})
    for k in ("hidden_layer_gemm", "gae_scan", "group_all", "physical_floor_us_per_step", "chains_measured_us_per_step", "useful_frac",
              "useful_tflops", "present_tap_fraction", "useful_note", "floor_ms"):
        if k in r:
            out["roofline"][k] = r[k]
    if "cpu_baseline" in line:
        out["cpu_baseline"] = {k: line["cpu_baseline"][k] for k in ("value", "unit", "cores", "kind", "sample")}
        out["gpu_over_cpu"] = line.get("gpu_over_cpu")
    if "train_scalars" in line["config"]:
        out["train_scalars"] = line["config"]["train_scalars"]
    if "dagger_loss" in line["config"]:
        out["dagger_loss"] = line["config"]["dagger_loss"]
    return out


def secondary_lines(args, device):
    """The other single-GPU BASELINE configs, timed by the SAME process right after the headline workload so that the driver's
    clock witnesses them too: cfg 2 (state PPO), cfg 5 as written (DAgger, SparseUNet student on 4096-voxel clouds) and cfg 3's
    rollouts through the PointNet++ plug-in backbone (HIP FPS + ball query + fused set-abstraction kernels).  Fixed 3 timed
    steps + 1 warm-up each (their own `steps` / `warmup` fields say so), each with its roofline and CPU baseline."""
    import copy
    import gc
    res = {}
    for key, kw in (("state", dict(workload="state")), ("dagger_sparse_unet", dict(workload="dagger", student="sparse_unet", points=4096)),
                    ("vision_pn2", dict(workload="vision_pn2")), ("depth2pc", dict(workload="depth2pc"))):
        a = copy.copy(args)
        a.steps, a.warmup, a.n_steps, a.precision, a.dump_outputs = 3, 1, 0, "f32", None
        for k, v in kw.items():
            setattr(a, k, v)
        gc.collect()
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        try:
            line = (run_dagger(a, device, 0, 1) if a.workload == "dagger" else run_depth2pc(a, device) if a.workload == "depth2pc"
                    else run_ppo(a, device, 0, 1))
            res[key] = _brief(line)
            res[key]["wall_s_incl_setup_and_cpu_baseline"] = time.perf_counter() - t0
        except Exception as e:                             # the headline line must survive a secondary's failure -- and say so
            res[key] = dict(error=f"{type(e).__name__}: {e}")
    gc.collect()
    torch.cuda.empty_cache()
    return res


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start N ranks (one per GPU) of this same command line under
    torch.distributed.run on this node and pass rank 0's ONE JSON line through.  Exits non-zero when fewer than N
    devices are visible (PARTMANIP_SHARE_GPU=1 + PARTMANIP_DIST_BACKEND=gloo -- the 1-GPU debugging mode of
    partmanip_amd/dist.py -- lifts that check)."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < n and os.environ.get("PARTMANIP_SHARE_GPU") != "1":
        print(f"bench.py: --gpus {n} but only {have} GPU(s) are visible", file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "8"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


@contextlib.contextmanager
def _collective_diagnosis(rank, world, local):
    """A collective that fails past the start-up probes (partmanip_amd/dist.py) must not end the run as a bare stack trace on one
    of N interleaved stderr streams: say which rank / device it was and what to try, then exit non-zero (no JSON line: a line
    without the collective would be a different measurement)."""
    try:
        yield
    except Exception as e:                                      # noqa: BLE001
        from partmanip_amd import dist as pdist
        if world > 1 and (isinstance(e, pdist.CollectiveError) or "NCCL" in str(e) or "RCCL" in str(e) or "ProcessGroup" in str(e)):
            print(f"[bench] rank {rank}/{world} (cuda:{local}) stopped on a collective: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
            print("[bench] the start-up probes passed, so the communicators were built: look at the launch structure named above "
                  "(PARTMANIP_DP_GRAPHS=split / PARTMANIP_GRAPHS=0 / PARTMANIP_OVERLAP=0 remove the capture, the graphs, the second "
                  "communicator in turn) and at NCCL_DEBUG=INFO", file=sys.stderr, flush=True)
        raise


def _rank_table(rank, world, local):
    """Multi-rank runs: which process drives which device over which collective library -- gathered to rank 0, printed to stderr
    before the first step (a hang in the first all-reduce is then a hang with the topology on the screen) and kept in the line
    (`config.ranks`)."""
    if world <= 1:
        return None
    be = torch.distributed.get_backend()
    try:
        ver = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception as e:                                  # a build without the binding: say so, do not fail the run
        ver = f"unavailable ({type(e).__name__})"
    pr = torch.cuda.get_device_properties(local)
    mine = dict(rank=rank, local_rank=local, pid=os.getpid(), device=f"cuda:{local}", name=pr.name,
                pci=f"{getattr(pr, 'pci_domain_id', 0):04x}:{getattr(pr, 'pci_bus_id', 0):02x}:{getattr(pr, 'pci_device_id', 0):02x}",
                hbm_gib=round(pr.total_memory / 2 ** 30, 1), cus=pr.multi_processor_count)
    table = [None] * world
    torch.distributed.all_gather_object(table, mine)
    info = dict(backend=be, rccl_version=ver if be == "nccl" else None, world=world, ranks=table,
                visible_devices=torch.cuda.device_count(),
                env={k: os.environ.get(k) for k in ("NCCL_DEBUG", "HSA_ENABLE_IPC_MODE_LEGACY", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES",
                                                    "PARTMANIP_SHARE_GPU", "PARTMANIP_DIST_BACKEND", "PARTMANIP_DP_GRAPHS")})
    if rank == 0:
        print(f"[bench] {world} ranks over {be}" + (f" (RCCL {ver})" if be == "nccl" else "") + f"; {info['visible_devices']} device(s) visible",
              file=sys.stderr)
        for r in table:
            print(f"[bench]   rank {r['rank']}: pid {r['pid']} -> {r['device']} {r['name']} pci {r['pci']} {r['hbm_gib']} GiB {r['cus']} CUs", file=sys.stderr)
        if len({r["pci"] for r in table}) < world and os.environ.get("PARTMANIP_SHARE_GPU") != "1":
            print("[bench] WARNING: several ranks drive the same device", file=sys.stderr)
        if not os.environ.get("NCCL_DEBUG"):
            print("[bench] a hang or an RCCL error in the first collective: rerun with NCCL_DEBUG=INFO (NCCL_DEBUG_SUBSYS=INIT,COLL) and "
                  "check HSA_ENABLE_IPC_MODE_LEGACY=0", file=sys.stderr)
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="vision", choices=list(WORKLOADS) + ["dagger", "depth2pc"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-optional", action="store_true", help="vision workload: skip the opt-in paths (profiling runs)")
    ap.add_argument("--lean", action="store_true", help="profiling runs: only the timed iterations (no side measurements of single kernels)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="default (vision) line on one GPU: skip the cfg 2 / cfg 5 sub-lines that the same run otherwise times")
    ap.add_argument("--n-steps", type=int, default=0, help="override the rollout length T (e.g. 128 for the vision workload)")
    ap.add_argument("--student", default="pointnet", choices=["pointnet", "conv3d", "sparse_unet"],
                    help="dagger workload: PointNet on --points clouds (cfg 5 analogue) or the reference's shipped Conv3DNet config")
    ap.add_argument("--points", type=int, default=4096, help="dagger workload: points per student cloud (BASELINE cfg 5: 4096)")
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16x3", "bf16x6"],
                    help="vision encoder forward: exact fp32 MFMA (default) or the opt-in split-bf16 path")
    ap.add_argument("--full", action="store_true",
                    help="also measure what needs runs of its own: CPU baseline, opt-in paths, secondary sub-lines, single-kernel timings "
                         "(the --no-* / --lean switches above then select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step to DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()
    if not args.full:
        args.no_cpu_baseline = args.no_optional = args.no_secondary = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))                  # re-exec as N ranks under torch.distributed.run
    # stdout is ONE JSON line.  Libraries print there too (gloo's "[Gloo] Rank ... is connected", RCCL's version banner): from here
    # to the final print the process's file descriptor 1 IS stderr, so whatever anything writes -- Python or C -- lands there.
    sys.stdout.flush()
    fd_out = os.dup(1)
    os.dup2(2, 1)
    from partmanip_amd import dist as pdist
    rank, world, local = pdist.init_from_env("nccl")
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a line for the wrong "
              "device count", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    if world > 1:
        be = torch.distributed.get_backend()
        if torch.distributed.get_world_size() != args.gpus or (be != "nccl" and not os.environ.get("PARTMANIP_DIST_BACKEND")):
            print(f"bench.py: process group reports world {torch.distributed.get_world_size()} / backend {be}; a --gpus {args.gpus} "
                  "line needs that many ranks over RCCL (backend nccl)", file=sys.stderr)
            sys.exit(2)
    topo = _rank_table(rank, world, local)
    with contextlib.redirect_stdout(sys.stderr), _collective_diagnosis(rank, world, local):   # the runners print progress lines: keep stdout = ONE JSON line
        if args.workload == "depth2pc":
            out = run_depth2pc(args, device) if rank == 0 else None
        elif args.workload == "dagger":
            out = run_dagger(args, device, rank, world)
        else:
            out = run_ppo(args, device, rank, world)
            if args.workload == "vision" and world == 1 and args.precision == "f32" and not args.n_steps and not args.no_secondary:
                out["secondary"] = secondary_lines(args, device)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    sys.stdout.flush()
    os.dup2(fd_out, 1)
    os.close(fd_out)
    if rank == 0:
        if topo is not None and isinstance(out.get("config"), dict):
            out["config"]["ranks"] = topo
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
