"""depthResNet on the GPU against the plain-torch test reference (tests/depth_resnet_ref.py).

Error reference: throughout, e_ref is the LARGER of the errors against float64 of the reference's two float32 evaluations (NCHW, and
channels-last on one thread) -- two correct fp32 orders of torch itself differ by several times per tensor, so a bound of 4 x a
single one of them would be a coin flip.

Gradients are compared with PINNED signs: the reference runs on the tape of the HIP training forward (`saved_signs()`: every ReLU
mask and the pool's winners), which makes the network a smooth function of its parameters.  An unpinned whole-network gradient
comparison is deliberately absent: where one fp32 evaluation flips a mask that sat at round-off, its per-tensor gradient error
jumps by three orders of magnitude, and no implementation can be held to "k x the reference's fp32 error" there except by luck.

Figures of the first run on an MI355X are in profiles/depth_resnet_margins.json (every per-tensor ratio, without a threshold)."""
import copy

import numpy as np
import pytest
import torch

from tests import depth_resnet_ref as ref
from tests.helpers import npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, PROPRIO, OUT = 3, 5, 8
OBS = ref.H * ref.W + PROPRIO
CFG = dict(name="depthResNet", activation="tanh")
FORMATS = ("f64", "nchw", "cl")


def depth_obs(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(n, OBS)
    x[:, :ref.H * ref.W] = 0.3 + 1.5 * torch.rand(n, ref.H * ref.W, generator=g)
    far = torch.rand(n, ref.H * ref.W, generator=g) < 0.2
    x[:, :ref.H * ref.W][far] = 100.0                                  # a fifth of the pixels at the far plane
    x[:, ref.H * ref.W:] = torch.randn(n, PROPRIO, generator=g)
    return x


def run_ref(sd, x, fmt, training=True, tape=None, target=None):
    """One evaluation of the reference from the state `sd` -> (output, state after it, per-parameter gradients or None)."""
    net = ref.DepthResNetRef(OBS, OUT, "tanh", PROPRIO)
    net.load_state_dict(sd)
    net = net.double() if fmt == "f64" else net
    xx = x.double() if fmt == "f64" else x
    threads = torch.get_num_threads()
    if fmt == "cl":
        net = net.to(memory_format=torch.channels_last)
        torch.set_num_threads(1)
    try:
        net.train(training)
        if target is None:
            with torch.no_grad():
                y = net(xx, tape=tape, channels_last=fmt == "cl")
            grads = None
        else:
            y = net(xx, tape=tape, channels_last=fmt == "cl")
            torch.nn.functional.mse_loss(y, target.to(y.dtype)).backward()
            grads = {k: p.grad.detach().double().contiguous() for k, p in net.named_parameters()}
    finally:
        torch.set_num_threads(threads)
    state = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in net.state_dict().items()}
    return y.detach().double(), state, grads


def l2(a, b):
    return float(torch.linalg.vector_norm(a.double().reshape(-1) - b.double().reshape(-1)))


def hip_student(sd):
    from partmanip_amd.algo_utils.network import depthResNet
    net = depthResNet(OBS, OUT, CFG, PROPRIO).to(DEV)
    net.load_state_dict(sd, strict=True)
    views = {k: torch.zeros_like(p) for k, p in net.named_parameters()}
    net.set_grad_views(views)
    return net, views


@pytest.fixture(scope="module")
def world():
    """Everything the comparisons share, computed once: the HIP training forward + backward and the reference's evaluations."""
    torch.manual_seed(11)
    r0 = ref.DepthResNetRef(OBS, OUT, "tanh", PROPRIO)
    g = torch.Generator().manual_seed(12)
    for m in r0.modules():                                               # batch-norm weights and biases off their 1 / 0 initialisation
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.add_(0.1 * torch.randn(m.weight.shape, generator=g))
            m.bias.data.add_(0.1 * torch.randn(m.bias.shape, generator=g))
    sd0 = copy.deepcopy(r0.state_dict())
    x = depth_obs(B, 13)
    target = 0.5 * torch.randn(B, OUT, generator=g)
    w = dict(sd0=sd0, x=x, target=target)
    # ---- the HIP path: training forward, tape, backward of MSE against the fixed target
    net, views = hip_student(sd0)
    net.train()
    y = net.hip_forward(x.to(DEV))
    w["tape"] = [t_.cpu() for t_ in net.saved_signs()]
    w["hip_y"] = y.cpu()
    w["hip_state"] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    dy = (2.0 / y.numel()) * (y - target.to(DEV))
    net.hip_backward(dy.contiguous())
    torch.cuda.synchronize()
    w["hip_grads"] = {k: v.cpu().clone() for k, v in views.items()}
    w["net"] = net
    # ---- the reference: unpinned training forward (outputs, running statistics), pinned forward + backward (gradients)
    w["fwd"] = {f: run_ref(sd0, x, f) for f in FORMATS}
    w["pinned"] = {f: run_ref(sd0, x, f, tape=w["tape"], target=target) for f in FORMATS}
    return w


def test_training_forward_and_running_statistics(world):
    y64, st64, _ = world["fwd"]["f64"]
    e_ref = max(l2(world["fwd"][f][0], y64) for f in ("nchw", "cl"))
    err = l2(world["hip_y"], y64)
    print(f"training output: ||hip - f64|| = {err:.3e}, e_ref = {e_ref:.3e} ({err / e_ref:.2f} e_ref)")
    record_margin("depthResNet training output ||hip - f64||_2 / e_ref", err / e_ref, 4.0, e_ref=e_ref)
    bad = []
    worst = 0.0
    stats = [k for k in st64 if k.endswith("running_mean") or k.endswith("running_var")]
    assert len(stats) == 72
    for k in stats:
        e_k = max(l2(world["fwd"][f][1][k], st64[k]) for f in ("nchw", "cl"))
        err_k = l2(world["hip_state"][k], st64[k])
        worst = max(worst, err_k / e_k)
        if not err_k <= 4 * e_k:
            bad.append((k, err_k, e_k))
    print(f"running statistics: worst ||hip - f64|| / e_ref over {len(stats)} buffers = {worst:.2f}")
    record_margin("depthResNet running statistics: worst ||hip - f64||_2 / e_ref", worst, 4.0)
    assert err <= 4 * e_ref, (err, e_ref)
    assert not bad, bad
    for k, v in world["hip_state"].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k


def test_saved_signs_have_torchs_shapes(world):
    tape = world["tape"]
    assert len(tape) == 2 + 2 * 16
    assert tape[0].dtype == torch.bool and tuple(tape[0].shape) == (B, 64, 36, 64)
    assert tape[1].dtype == torch.int64 and tuple(tape[1].shape) == (B, 64, 18, 32)
    assert int(tape[1].min()) >= 0 and int(tape[1].max()) < 36 * 64
    shapes = [(64, 18, 32)] * 6 + [(128, 9, 16)] * 8 + [(256, 5, 8)] * 12 + [(512, 3, 4)] * 6
    assert [tuple(t_.shape[1:]) for t_ in tape[2:]] == shapes
    # the pinned float64 forward lands on the HIP output: the tape is the one this forward went through
    assert l2(world["pinned"]["f64"][0], world["hip_y"]) <= 1e-3 * float(world["hip_y"].norm())


def test_backward_with_pinned_signs(world):
    """Per parameter tensor err(k) = ||g_hip - g64|| / ||g64||; max_k err <= 4 max_k e_ref and median_k err <= 4 median_k e_ref,
    e_ref(k) = the larger of the two float32 evaluations' errors on the same tape."""
    g64 = world["pinned"]["f64"][2]
    errs, erefs = {}, {}
    for k, g in g64.items():
        n = float(torch.linalg.vector_norm(g))
        assert n > 0, k
        errs[k] = l2(world["hip_grads"][k], g) / n
        erefs[k] = max(l2(world["pinned"][f][2][k], g) for f in ("nchw", "cl")) / n
        record_margin(f"depthResNet pinned gradient {k}: err / e_ref", errs[k] / erefs[k] if erefs[k] > 0 else 0.0, 0.0, err=errs[k],
                      e_ref=erefs[k], note="no threshold")
    assert len(errs) == 108 + 6
    e, r = np.array(list(errs.values())), np.array(list(erefs.values()))
    worst = max(errs, key=lambda k: errs[k] / max(erefs[k], 1e-300))
    print(f"pinned gradients: max err {e.max():.3e} (e_ref {r.max():.3e}), median err {np.median(e):.3e} (e_ref {np.median(r):.3e}); "
          f"worst ratio {errs[worst] / erefs[worst]:.2f} at {worst}")
    record_margin("depthResNet pinned gradients: max_k err / max_k e_ref", e.max() / r.max(), 4.0)
    record_margin("depthResNet pinned gradients: median_k err / median_k e_ref", np.median(e) / np.median(r), 4.0)
    assert e.max() <= 4 * r.max(), (e.max(), r.max(), worst)
    assert np.median(e) <= 4 * np.median(r), (np.median(e), np.median(r))


def test_eval_forward_reads_the_running_statistics_and_writes_nothing(world):
    # the state after the reference's float64 training forward, as a float32 checkpoint with torchvision's `resnet34.` keys
    sd1 = {k: (v.float() if v.is_floating_point() else v.clone()) for k, v in world["fwd"]["f64"][1].items()}
    assert "resnet34.layer2.0.downsample.1.running_var" in sd1 and "resnet34.bn1.num_batches_tracked" in sd1
    net, _ = hip_student(sd1)
    back = net.state_dict()
    assert list(back.keys()) == list(sd1.keys())
    for k, v in sd1.items():                                            # the checkpoint round-trips
        assert back[k].dtype == v.dtype and same_bits(npy(back[k]), v.numpy()), k
    net.eval()
    x = world["x"]
    y = net.hip_forward(x.to(DEV)).cpu()
    y2 = net(x.to(DEV)).cpu()
    assert same_bits(npy(y), npy(y2))
    after = net.state_dict()
    for k, v in sd1.items():                                            # eval touches no buffer (and no parameter)
        assert same_bits(npy(after[k]), v.numpy()), k
    outs = {f: run_ref(sd1, x, f, training=False)[0] for f in FORMATS}
    e_ref = max(l2(outs[f], outs["f64"]) for f in ("nchw", "cl"))
    err = l2(y, outs["f64"])
    print(f"eval output: ||hip - f64|| = {err:.3e}, e_ref = {e_ref:.3e} ({err / e_ref:.2f} e_ref)")
    record_margin("depthResNet eval output ||hip - f64||_2 / e_ref", err / e_ref, 4.0, e_ref=e_ref)
    assert err <= 4 * e_ref, (err, e_ref)
    with pytest.raises(RuntimeError, match="eval mode"):
        net.hip_backward(torch.zeros(B, OUT, device=DEV))


def test_num_batches_tracked_counts_every_training_forward(world):
    net = world["net"]
    nbt = lambda: int(net.resnet34.layer3[2].bn2.num_batches_tracked)      # noqa: E731
    n0 = nbt()
    x = world["x"].to(DEV)
    net.train()
    rm = net.resnet34.bn1.running_mean.clone()
    with torch.no_grad():
        net(x)                                                           # the rollout's forward: training mode, no_grad
    assert nbt() == n0 + 1 and not torch.equal(rm, net.resnet34.bn1.running_mean)
    net.hip_forward(x)
    assert nbt() == n0 + 2
    net.eval()
    net(x)
    assert nbt() == n0 + 2
    net.train()


def model_cfg():
    return dict(action_std=0.1, action_activate="tanh", clipAction=1.0, network=dict(CFG))


def test_actor_critic_constructs_flattens_and_both_backwards_fill_their_views():
    from partmanip_amd.algo_utils import ActorCritic
    from partmanip_amd.autograd import backbone_apply
    torch.manual_seed(3)
    ac = ActorCritic(OBS, OUT, model_cfg(), PROPRIO).to(DEV)
    f = ac.flat()
    n_backbone = 21_278_400 + (512 + PROPRIO) * 128 + 128 + 128 * 32 + 32
    assert f["n_actor"] == n_backbone + 32 * OUT + OUT and f["n_critic"] == n_backbone + 32 + 1
    assert ac.actor.resnet34.conv1.weight.data_ptr() == f["actor"].data_ptr()
    assert all(b_.data_ptr() < f["actor"].data_ptr() or b_.data_ptr() >= f["actor"].data_ptr() + 4 * f["actor"].numel()
               for b_ in ac.actor.buffers())                            # running statistics are not in the flat parameter vector
    x = depth_obs(B, 21).to(DEV)
    ac.train()
    for net_, grad, n, width in ((ac.actor, f["grad_actor"], f["n_actor"], OUT), (ac.critic, f["grad_critic"], f["n_critic"], 1)):
        grad.zero_()
        y = net_.hip_forward(x)
        assert tuple(y.shape) == (B, width) and torch.isfinite(y).all()
        net_.hip_backward(torch.ones_like(y) / y.numel())
        for k, v in net_._views.items():
            assert torch.isfinite(v).all() and float(v.abs().max()) > 0, k
        assert v.data_ptr() >= grad.data_ptr() and v.data_ptr() < grad.data_ptr() + 4 * n
    # ... and through the torch.autograd bridge: the same kernels, the gradients handed to autograd
    want = [v.clone() for v in ac.actor._grad_list]
    for p in ac.actor.parameters():
        p.grad = None
    y = backbone_apply(ac.actor, x)                                      # (training mode: batch statistics, so the same function of x)
    (y.sum() / y.numel()).backward()
    got = [p.grad for p in ac.actor.parameters()]
    assert len(got) == len(want) and all(g_ is not None and g_.shape == w_.shape for g_, w_ in zip(got, want))
    for g_, w_ in zip(got, want):                                        # the same batch, the same parameters: the same bits
        assert same_bits(npy(g_), npy(w_))


def test_twenty_dagger_style_steps_reduce_the_loss():
    from partmanip_amd import ops
    from partmanip_amd.algo_utils import ActorCritic
    from partmanip_amd.algo_utils.optim import FusedAdam
    torch.manual_seed(4)
    ac = ActorCritic(OBS, OUT, model_cfg(), PROPRIO).to(DEV)
    f = ac.flat()
    n_a = f["n_actor"]
    opt = FusedAdam(f["actor"], f["grad_actor"][:n_a + OUT], [list(ac.parameters())], lr=1e-3)
    x = depth_obs(8, 22).to(DEV)
    tea_mu = (0.7 * torch.randn(8, OUT, generator=torch.Generator().manual_seed(23))).to(DEV)
    ac.train()
    losses = []
    for _ in range(20):
        mu = ac.actor.hip_forward(x)
        dmu = torch.empty_like(mu)
        ops.mse_tanh_loss(mu, tea_mu, ac.max_action, 1, 1.0, f["scal_actor"], dmu)
        ac.actor.hip_backward(dmu)
        losses.append(float(f["scal_actor"][0]))
        opt.step(n=n_a, n_clip=0, max_norm=0.0)
    print("dagger-style losses:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    assert int(ac.actor.resnet34.bn1.num_batches_tracked) == 20


def test_kinematic_env_depth_img_row_feeds_random_act_in_place():
    from partmanip_amd import camera
    from partmanip_amd.algo_utils import ActorCritic
    from partmanip_amd.envs import depth_img_observer, make_grasp_cube_env
    from partmanip_amd.mesh2depth import DepthFromMesh
    from tests import depth_render_ref as D
    from tests import kinematic_episode as E
    N = 2
    tree, bp, dof = E.scene()
    env0 = make_grasp_cube_env(dict(E.CFG), N, DEV, tree, E.DT, base_pose=bp, dof=dof, free_body_pose=E.CUBE_POSE)
    env0.reset()
    hand = npy(env0.task.compute_scene_pose()[1])[1, 9].astype(np.float64)
    poses, intr, H, W = camera.shipped_rig(dict(look_at=[float(v) for v in hand], radius=0.6), image_mode=True)
    assert (len(poses), H, W) == (1, ref.H, ref.W)
    cam = DepthFromMesh(N, DEV, poses, intr, H, W, meshes=[D.finger_mesh()] * 12)
    env = make_grasp_cube_env(dict(E.CFG), N, DEV, tree, E.DT, base_pose=bp, dof=dof, free_body_pose=E.CUBE_POSE,
                              observers={"depth_img": depth_img_observer(cam)}, add_proprio_obs=True)
    env.reset()
    a = torch.zeros(N, 7, device=DEV)
    obs, _, _, _ = env.step(a)
    row = obs["depth_img"]
    proprio = env.num_obs["proprio_state"]
    print(f"pixels that show a part: {int((row[:, :H * W] < 100).sum())} of {N * H * W}")
    assert tuple(row.shape) == (N, H * W + proprio) and (row[:, :H * W] == 100).any() and torch.equal(row[:, H * W:], obs["proprio_state"])
    torch.manual_seed(5)
    student = ActorCritic(H * W + proprio, 7, model_cfg(), proprio).to(DEV)
    student.train()
    before = row.clone()
    act = student.random_act(row)                                        # the image is the head of the observation row, read where it lies
    assert tuple(act.shape) == (N, 7) and torch.isfinite(act).all() and float(act.abs().max()) <= 1.0
    assert torch.equal(row, before) and int(student.actor.resnet34.bn1.num_batches_tracked) == 1
    student.eval()
    assert same_bits(npy(student.act(row)), npy(student.act(row.clone())))
