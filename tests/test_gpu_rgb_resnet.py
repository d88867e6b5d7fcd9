"""ResNet (the rgb_img student) on the GPU against the plain-torch test reference (tests/rgb_resnet_ref.py): the scheme of
tests/test_gpu_depth_resnet.py at its shapes.

Error reference: throughout, e_ref is the LARGER of the errors against float64 of the reference's two float32 evaluations (NCHW, and
channels-last on one thread); the bound is the project's standing 4 x e_ref.  Gradients are compared with PINNED signs (the
reference runs on the tape of the HIP training forward, `saved_signs()`), for the reason that file's docstring gives.
`resnet34.conv1.weight` is also held to 4 x e_ref on its own: it is the one tensor whose route differs from the depth student's
(pm_im2col2d_f32's 160-column patch matrix, the weight and its gradient in the weight's own column order).

Figures of the first run on an MI355X are in profiles/rgb_resnet_margins.json."""
import copy

import numpy as np
import pytest
import torch

from tests import rgb_resnet_ref as ref
from tests.helpers import npy, record_margin, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, PROPRIO, OUT = 3, 5, 8
HW = ref.H * ref.W
OBS = 3 * HW + PROPRIO
CFG = dict(name="ResNet", activation="tanh", pretrained=False)
FORMATS = ("f64", "nchw", "cl")
STEM = "resnet34.conv1.weight"


def rgb_obs(n, seed):
    """Image columns: integers 0..255 as floats, a fifth of the pixels set to one background colour; a random proprio tail."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(n, OBS)
    img = torch.randint(0, 256, (n, 3, HW), generator=g).float()
    bg = torch.rand(n, HW, generator=g) < 0.2
    for c, v in enumerate((255.0, 255.0, 255.0)):
        img[:, c][bg] = v
    x[:, :3 * HW] = img.reshape(n, 3 * HW)
    x[:, 3 * HW:] = torch.randn(n, PROPRIO, generator=g)
    return x


def run_ref(sd, x, fmt, training=True, tape=None, target=None):
    """One evaluation of the reference from the state `sd` -> (output, state after it, per-parameter gradients or None)."""
    net = ref.RGBResNetRef(OBS, OUT, "tanh", PROPRIO)
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
    from partmanip_amd.algo_utils.network import ResNet
    net = ResNet(OBS, OUT, CFG, PROPRIO).to(DEV)
    net.load_state_dict(sd, strict=True)
    views = {k: torch.zeros_like(p) for k, p in net.named_parameters()}
    net.set_grad_views(views)
    return net, views


@pytest.fixture(scope="module")
def world():
    """Everything the comparisons share, computed once: the HIP training forward + backward and the reference's evaluations."""
    torch.manual_seed(31)
    r0 = ref.RGBResNetRef(OBS, OUT, "tanh", PROPRIO)
    g = torch.Generator().manual_seed(32)
    for m in r0.modules():                                               # batch-norm weights and biases off their 1 / 0 initialisation
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.add_(0.1 * torch.randn(m.weight.shape, generator=g))
            m.bias.data.add_(0.1 * torch.randn(m.bias.shape, generator=g))
    sd0 = copy.deepcopy(r0.state_dict())
    x = rgb_obs(B, 33)
    target = 0.5 * torch.randn(B, OUT, generator=g)
    w = dict(sd0=sd0, x=x, target=target)
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
    w["fwd"] = {f: run_ref(sd0, x, f) for f in FORMATS}
    w["pinned"] = {f: run_ref(sd0, x, f, tape=w["tape"], target=target) for f in FORMATS}
    return w


def test_training_forward_and_running_statistics(world):
    y64, st64, _ = world["fwd"]["f64"]
    e_ref = max(l2(world["fwd"][f][0], y64) for f in ("nchw", "cl"))
    err = l2(world["hip_y"], y64)
    print(f"training output: ||hip - f64|| = {err:.3e}, e_ref = {e_ref:.3e} ({err / e_ref:.2f} e_ref)")
    record_margin("ResNet training output ||hip - f64||_2 / e_ref", err / e_ref, 4.0, e_ref=e_ref)
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
    record_margin("ResNet running statistics: worst ||hip - f64||_2 / e_ref", worst, 4.0)
    assert err <= 4 * e_ref, (err, e_ref)
    assert not bad, bad
    for k, v in world["hip_state"].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k


def test_saved_signs_are_the_depth_students(world):
    tape = world["tape"]
    assert len(tape) == 2 + 2 * 16
    assert tape[0].dtype == torch.bool and tuple(tape[0].shape) == (B, 64, 36, 64)
    assert tape[1].dtype == torch.int64 and tuple(tape[1].shape) == (B, 64, 18, 32)
    # the pinned float64 forward lands on the HIP output: the tape is the one this forward went through
    assert l2(world["pinned"]["f64"][0], world["hip_y"]) <= 1e-3 * float(world["hip_y"].norm())


def test_backward_with_pinned_signs(world):
    """Per parameter tensor err(k) = ||g_hip - g64|| / ||g64||; max_k err <= 4 max_k e_ref and median_k err <= 4 median_k e_ref,
    e_ref(k) = the larger of the two float32 evaluations' errors on the same tape; the stem's weight also on its own."""
    g64 = world["pinned"]["f64"][2]
    errs, erefs = {}, {}
    for k, g in g64.items():
        n = float(torch.linalg.vector_norm(g))
        assert n > 0, k
        assert tuple(world["hip_grads"][k].shape) == tuple(g.shape), k
        errs[k] = l2(world["hip_grads"][k], g) / n
        erefs[k] = max(l2(world["pinned"][f][2][k], g) for f in ("nchw", "cl")) / n
        record_margin(f"ResNet pinned gradient {k}: err / e_ref", errs[k] / erefs[k] if erefs[k] > 0 else 0.0, 0.0, err=errs[k],
                      e_ref=erefs[k], note="no threshold")
    assert len(errs) == 108 + 6
    e, r = np.array(list(errs.values())), np.array(list(erefs.values()))
    worst = max(errs, key=lambda k: errs[k] / max(erefs[k], 1e-300))
    print(f"pinned gradients: max err {e.max():.3e} (e_ref {r.max():.3e}), median err {np.median(e):.3e} (e_ref {np.median(r):.3e}); "
          f"worst ratio {errs[worst] / erefs[worst]:.2f} at {worst}")
    print(f"stem weight gradient: err {errs[STEM]:.3e}, e_ref {erefs[STEM]:.3e} ({errs[STEM] / erefs[STEM]:.2f} e_ref)")
    record_margin("ResNet pinned gradients: max_k err / max_k e_ref", e.max() / r.max(), 4.0)
    record_margin("ResNet pinned gradients: median_k err / median_k e_ref", np.median(e) / np.median(r), 4.0)
    record_margin(f"ResNet pinned gradient {STEM} alone: err / e_ref", errs[STEM] / erefs[STEM], 4.0, err=errs[STEM], e_ref=erefs[STEM])
    assert e.max() <= 4 * r.max(), (e.max(), r.max(), worst)
    assert np.median(e) <= 4 * np.median(r), (np.median(e), np.median(r))
    assert errs[STEM] <= 4 * erefs[STEM], (errs[STEM], erefs[STEM])


def test_eval_forward_reads_the_running_statistics_and_writes_nothing(world):
    sd1 = {k: (v.float() if v.is_floating_point() else v.clone()) for k, v in world["fwd"]["f64"][1].items()}
    assert tuple(sd1[STEM].shape) == (64, 3, 7, 7) and "resnet34.bn1.num_batches_tracked" in sd1
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
    record_margin("ResNet eval output ||hip - f64||_2 / e_ref", err / e_ref, 4.0, e_ref=e_ref)
    assert err <= 4 * e_ref, (err, e_ref)
    with pytest.raises(RuntimeError, match="eval mode"):
        net.hip_backward(torch.zeros(B, OUT, device=DEV))


def model_cfg():
    return dict(action_std=0.1, action_activate="tanh", clipAction=1.0, network=dict(CFG))


def test_twenty_dagger_style_steps_reduce_the_loss():
    from partmanip_amd import ops
    from partmanip_amd.algo_utils import ActorCritic
    from partmanip_amd.algo_utils.optim import FusedAdam
    torch.manual_seed(34)
    ac = ActorCritic(OBS, OUT, model_cfg(), PROPRIO).to(DEV)
    f = ac.flat()
    n_a = f["n_actor"]
    opt = FusedAdam(f["actor"], f["grad_actor"][:n_a + OUT], [list(ac.parameters())], lr=1e-3)
    x = rgb_obs(4, 35).to(DEV)
    tea_mu = (0.7 * torch.randn(4, OUT, generator=torch.Generator().manual_seed(36))).to(DEV)
    ac.train()
    stem0 = ac.actor.resnet34.conv1.weight.detach().clone()
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
    assert not torch.equal(stem0, ac.actor.resnet34.conv1.weight.detach())      # the three-channel stem is trained too


def test_kinematic_env_rgb_img_row_feeds_random_act_in_place():
    from partmanip_amd import camera
    from partmanip_amd.algo_utils import ActorCritic
    from partmanip_amd.envs import make_grasp_cube_env, rgb_img_observer
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
                              observers={"rgb_img": rgb_img_observer(cam)}, add_proprio_obs=True)
    env.reset()
    a = torch.zeros(N, 7, device=DEV)
    obs, _, _, _ = env.step(a)
    row = obs["rgb_img"]
    proprio = env.num_obs["proprio_state"]
    assert env.num_obs["rgb_img"] == 3 * H * W + proprio and tuple(row.shape) == (N, 3 * H * W + proprio)
    # the head of the row is the colour frame of the same poses, permuted to planes, bit for bit; the tail is the proprio row
    R, T = env.compute_scene_pose()
    rgb = cam.render_frame(R, T, depth=False, seg=False, rgb=True).rgb
    want = rgb[:, 0].permute(0, 3, 1, 2).float().reshape(N, 3 * H * W)
    assert same_bits(npy(row[:, :3 * H * W]), npy(want))
    assert torch.equal(row[:, 3 * H * W:], obs["proprio_state"])
    n_part = int((rgb[:, 0] != rgb[0, 0, 0, 0]).any(-1).sum())
    print(f"pixels that show a part: {n_part} of {N * H * W}")
    assert n_part > 0 and float(row[:, :3 * H * W].min()) >= 0 and float(row[:, :3 * H * W].max()) <= 255
    torch.manual_seed(37)
    student = ActorCritic(3 * H * W + proprio, 7, model_cfg(), proprio).to(DEV)
    student.train()
    before = row.clone()
    act = student.random_act(row)                                        # the image is the head of the observation row, read where it lies
    assert tuple(act.shape) == (N, 7) and torch.isfinite(act).all() and float(act.abs().max()) <= 1.0
    assert torch.equal(row, before) and int(student.actor.resnet34.bn1.num_batches_tracked) == 1
    student.eval()
    assert same_bits(npy(student.act(row)), npy(student.act(row.clone())))
