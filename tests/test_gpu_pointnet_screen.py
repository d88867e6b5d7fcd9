"""The screened PointNet forward (csrc/pointnet_enc_screen.h: layer 3 screened on split-bf16 MFMAs, the pooling's winners
finished in exact fp32) against the dense fp32 kernel on the same weights and input.  GPU box only.

Stated tolerances: h2_save bit-equal; max / mean features within 3e-6 of the feature scale (max |dense feature|); arg-max equal
wherever the dense top-2 gap (fp64 layer 3 of the saved h2) exceeds 1e-5; the returned max equals the fp64 layer 3 at the
returned arg-max within 3e-6 of the feature scale.

Measured on MI355X: the fixed fp32 summation order of the exact finish does NOT reproduce the MFMA chain bit for bit -- 9-13 %
of the max features are bit-equal to the dense kernel's (profiles/round7_pointnet_screen.md; every case prints its figures)."""
import tempfile

import pytest
import torch

from partmanip_amd import ops
from tests.golden import cases
from tests.helpers import load_fixture, t, ppo_cfg, ppo_rollout, FakeEnv, FakeLogger

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEAT_TOL, GAP = 3e-6, 1e-5


def weights(C, seed):
    """Default-initialised shared MLP C -> 128 -> 256 -> 512 on the device + the dense kernel's packed operands."""
    torch.manual_seed(seed)
    lin = [torch.nn.Linear(C, 128), torch.nn.Linear(128, 256), torch.nn.Linear(256, 512)]
    w = {f"{k}{i + 1}": getattr(m, a).detach().to(DEV).contiguous() for i, m in enumerate(lin) for k, a in (("W", "weight"), ("b", "bias"))}
    return repack(w)


def repack(w):
    w["packed"] = torch.empty(ops.pointnet_packed_elems(), device=DEV)
    ops.pointnet_pack(w["W2"], w["W3"], w["packed"])
    w["packed_s"] = torch.empty(ops.pointnet_packed_screen_bytes(), dtype=torch.uint8, device=DEV)
    ops.pointnet_pack_screen(w["W3"], w["b3"], w["packed_s"])
    return w


def clouds(B, P, C, seed):
    g = torch.Generator().manual_seed(seed)          # the distribution of test_pointnet_forward_backward
    return torch.rand(B, P, C, generator=g) * 2 - 1 + (torch.rand(B, 1, C, generator=g) - 0.5)


def forward(w, pts, screen, max_mean=True, sub_mean=False, save_h2=True, count=False):
    B, P, C = pts.shape
    x = pts.reshape(B, -1).to(DEV).contiguous()
    feat = torch.empty(B, 512 * (2 if max_mean else 1), device=DEV)
    am = torch.empty(B, 512, dtype=torch.int32, device=DEV)
    h2 = torch.empty(B, P, 256, device=DEV) if save_h2 else None
    cnt = torch.zeros(3, dtype=torch.int64, device=DEV) if count else None
    if screen:
        ops.pointnet_enc_fwd_screen(x, P, C, sub_mean, w["W1"], w["b1"], w["b2"], w["b3"], w["packed"], w["packed_s"], max_mean,
                                    feat, am, h2, cnt)
    else:
        ops.pointnet_enc_fwd(x, P, C, sub_mean, w["W1"], w["b1"], w["b2"], w["b3"], w["packed"], max_mean, feat, am, h2)
    torch.cuda.synchronize()
    return feat, am.long(), h2, (cnt.tolist() if count else None)


def check_against_dense(w, pts, max_mean=True, sub_mean=False, label="", dense_mean_err=None):
    """Screened against dense as the module docstring states; returns the screened counters and features.  dense_mean_err:
    None, or a (B, 512) tensor with the absolute rounding error of the DENSE kernel's own mean chain, which is then added to
    the 3e-6 bound of the mean feature against the dense kernel (test_degenerate_cloud_runs_the_dense_fallback, the only
    user, derives it by replaying that chain).  Against the fp64 mean of the saved h2 the bound is always 3e-6."""
    fs, ams, h2s, cnt = forward(w, pts, True, max_mean, sub_mean, count=True)
    fd, amd, h2d, _ = forward(w, pts, False, max_mean, sub_mean)
    assert torch.equal(h2s, h2d), "h2_save differs from the dense kernel's"
    z = h2d.double() @ w["W3"].double().t() + w["b3"].double()                 # (B, P, 512) fp64 layer 3 of the saved h2
    scale = float(fd[:, :512].abs().max())
    e_max = float((fs[:, :512] - fd[:, :512]).abs().max()) / scale
    top2 = z.topk(2, dim=1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > GAP
    n_diff = int((ams != amd).sum())
    e_own = float((fs[:, :512].double() - z.gather(1, ams[:, None, :])[:, 0]).abs().max()) / scale
    bit_equal = float((fs[:, :512] == fd[:, :512]).float().mean())
    msg = (f"{label} max {e_max:.2e} own-argmax {e_own:.2e} argmax differing {n_diff} (under the gap: {int((~clear).sum())}) "
           f"max features bit-equal to dense {bit_equal:.4f} counters {cnt}")
    if max_mean:
        mscale = float(fd[:, 512:].abs().max())
        d_mean = (fs[:, 512:] - fd[:, 512:]).abs()
        e_mean = float(d_mean.max()) / mscale
        slack = 0.0 if dense_mean_err is None else dense_mean_err.to(DEV)
        e_mean64 = float((fs[:, 512:].double() - z.mean(dim=1)).abs().max()) / mscale
        msg += f" mean {e_mean:.2e} (against fp64 {e_mean64:.2e})"
    print(msg)
    assert e_max < FEAT_TOL, msg
    assert torch.equal(ams[clear], amd[clear]), msg
    assert e_own < FEAT_TOL, msg
    if max_mean:
        assert bool((d_mean < FEAT_TOL * mscale + slack).all()) and e_mean64 < FEAT_TOL, msg
    return cnt, fs, ams


@pytest.mark.parametrize("C", [3, 4, 6])
@pytest.mark.parametrize("P", [64, 128, 320, 1024])
def test_random_clouds(P, C):
    B = 6
    w = weights(C, 10 * C + 1)
    pts = clouds(B, P, C, P + C)
    for max_mean in (True, False):
        for sub_mean in (False, True):
            cnt, fs, ams = check_against_dense(w, pts, max_mean, sub_mean, f"P={P} C={C} mm={max_mean} sub={sub_mean}")
            # the screen really ran: nothing went to the dense fallback, and few points needed the exact finish
            assert cnt[1] == 0, cnt
            if P == 1024:
                assert cnt[0] <= 16 * B * 512, cnt
            f2, a2, _, _ = forward(w, pts, True, max_mean, sub_mean, save_h2=False)      # the inference forward agrees
            assert torch.equal(f2, fs) and torch.equal(a2, ams)


def test_exact_ties_across_tiles():
    """64 distinct points repeated 16 times: every later tile ties the first exactly; the lowest index must win."""
    w = weights(3, 5)
    pts = clouds(4, 64, 3, 17).repeat(1, 16, 1)
    _, _, ams = check_against_dense(w, pts, label="ties")
    assert int(ams.max()) < 64


def dense_mean_chain(v, P):
    """The dense kernel's mean of a channel whose P layer-3 values all equal v, replayed in fp32 on the host: each lane half
    adds its P / 2 values one by one starting from 0 (pn_fwd_kernel's `vsum += v`), the two halves are added, the sum is
    divided by P."""
    s = torch.zeros_like(v)
    for _ in range(P // 2):
        s = s + v
    return (s + s) / float(P)


def test_degenerate_cloud_runs_the_dense_fallback():
    """All 1024 points equal.  Arg-max 0 everywhere, every (wave, tile) pair on the dense fallback, max features the dense
    kernel's bit for bit.  The mean is the one place where DENSE is the kernel outside 3e-6: it adds a channel's 1024 equal
    values one by one in fp32, and the roundings of equal addends do not average out (7.0e-6 of the mean scale from the fp64
    mean on MI355X; the screened mean, from fp64 column sums, is within 3e-6 of fp64 like everywhere else).  So the bound of
    the screened mean against the dense one is 3e-6 PLUS, per channel, the error of the dense chain itself, obtained by
    replaying that chain on the host from the dense kernel's own layer-3 value -- the replay must reproduce the dense mean to
    4 ulp, which shows that the chain, and nothing else, is where the difference comes from."""
    w = weights(3, 6)
    P = 1024
    pts = clouds(3, 1, 3, 18).repeat(1, P, 1)
    fd = forward(w, pts, False)[0].cpu()
    v = fd[:, :512]                                       # every point's layer-3 value = the max feature
    replay = dense_mean_chain(v, P)
    ulp = (replay.abs() * 2.0 ** -23).clamp_min(1e-30)
    print(f"dense mean replay: bit-equal {float((replay == fd[:, 512:]).float().mean()):.4f}, worst {float(((replay - fd[:, 512:]).abs() / ulp).max()):.1f} ulp; "
          f"dense chain error {float((replay.double() - v.double()).abs().max() / fd[:, 512:].abs().max()):.2e} of the mean scale")
    assert bool(((replay - fd[:, 512:]).abs() <= 4 * ulp).all())
    cnt, fs, ams = check_against_dense(w, pts, label="all points equal", dense_mean_err=(replay.double() - v.double()).abs().float())
    assert int(ams.max()) == 0
    assert cnt[1] == 3 * (P // 64) * 8, cnt               # every (wave, tile) pair of every cloud
    assert torch.equal(fs[:, :512].cpu(), fd[:, :512])    # the fallback IS the dense layer 3


def test_sorted_cloud_sets_records_through_the_screen():
    """A random cloud sorted along a direction: the points stay apart (unlike the line below), and the channels that grow along
    the direction set a new record in most tiles, so later tiles are pruned by the rising running maximum, `!(z + e <= vm)`,
    inside the screen itself.  Bound on the fallback: a sorted tile is a slab holding 64 random points, as spread in the
    other two coordinates as a random tile; the channels that keep rising see about what every channel sees in a random
    cloud's first tile (one survivor or so per channel, ~80 per wave against the cap of 128), the others are pruned.  At most
    one (wave, tile) pair in ten may fall back; records: at least a quarter of the channels move their arg-max past the first
    half of the cloud."""
    w = weights(3, 11)
    pts = clouds(6, 1024, 3, 23)
    g = torch.Generator().manual_seed(24)
    d = torch.randn(6, 1, 3, generator=g)
    order = (pts * d).sum(-1).argsort(dim=1)
    pts = pts.gather(1, order[:, :, None].expand(-1, -1, 3))
    cnt, fs, ams = check_against_dense(w, pts, label="sorted along a direction")
    assert cnt[1] <= 0.1 * 6 * 16 * 8, cnt
    assert float((ams >= 512).float().mean()) >= 0.25


def test_a_record_in_every_tile():
    """Points on a line in increasing order: the channels that grow along it set a new record in every tile.  At 1024 points
    (and at 256) neighbours are closer than the screen's 2 eps band: every (wave, tile) pair exceeded the survivor cap and ran
    the dense fallback on MI355X.  The coarse line (128 points over twice the length) gives the screen itself a chance to
    carry the records; measured, 63 of its 64 (wave, tile) pairs still fell back (tanh saturates towards the ends of the line
    and flattens the channels), so this test mostly exercises the fallback's running-maximum hand-over between tiles -- the
    screen's own is exercised by test_sorted_cloud_sets_records_through_the_screen and the random and repeated clouds.  No
    bound on the counters (they are printed)."""
    w = weights(3, 7)
    g = torch.Generator().manual_seed(19)
    a, d = torch.rand(4, 1, 3, generator=g) - 0.5, torch.randn(4, 1, 3, generator=g)
    for P, half in ((1024, 1.0), (128, 2.0)):
        s = torch.linspace(-half, half, P)[None, :, None]
        check_against_dense(w, a + s * d / d.norm(dim=-1, keepdim=True), label=f"line P={P}")


def test_nan_and_infinity():
    w = weights(3, 8)
    pts = clouds(6, 1024, 3, 20)
    clean = forward(w, pts, True)[0]
    bad = pts.clone()
    bad[2, 517, 1] = float("nan")
    bad[4, 1023, 0] = float("nan")
    f = forward(w, bad, True)[0]
    for b in range(6):
        if b in (2, 4):
            assert torch.isnan(f[b]).all(), b
        else:
            assert torch.equal(f[b], clean[b]), b
    inf = pts.clone()
    inf[1, 300, 2] = float("inf")
    inf[3, 5, 0] = float("-inf")
    cnt, fs, _ = check_against_dense(w, inf, label="infinite coordinate")
    assert torch.isfinite(fs).all()
    w2 = dict(w, W3=w["W3"].clone())
    w2["W3"][77, 13] = float("inf")
    w2["W3"][300, 200] = float("nan")
    repack(w2)
    fs, ams, _, _ = forward(w2, pts, True)
    fd, amd, _, _ = forward(w2, pts, False)
    assert torch.equal(torch.isnan(fs), torch.isnan(fd))
    assert torch.equal(torch.isinf(fs), torch.isinf(fd))
    ok = torch.isfinite(fd)
    assert torch.equal(torch.sign(fs[~ok & ~torch.isnan(fd)]), torch.sign(fd[~ok & ~torch.isnan(fd)]))
    assert int((~ok[:, :512]).sum()) >= 2 * 6                       # the two poisoned channels of every cloud
    scale = float(fd[ok].abs().max())
    assert float((fs[ok] - fd[ok]).abs().max()) / scale < FEAT_TOL


def test_reproducible_and_independent_of_batch_position():
    w = weights(4, 9)
    pts = clouds(8, 1024, 4, 21)
    f1, a1, _, _ = forward(w, pts, True, sub_mean=True)
    f2, a2, _, _ = forward(w, pts, True, sub_mean=True)
    assert torch.equal(f1, f2) and torch.equal(a1, a2)
    for i in (0, 5, 7):
        fi, ai, _, _ = forward(w, pts[i:i + 1], True, sub_mean=True)
        assert torch.equal(fi[0], f1[i]) and torch.equal(ai[0], a1[i]), i


def test_whole_update_screened_against_dense():
    """One PPO mini-batch update at B = 8 (golden case ppo_pn_maxmean cut to 4 envs x 2 steps, one mini-batch, one epoch) with
    the screened default against `screen: False`: every gradient within test_pointnet_forward_backward's 1e-4 of its scale."""
    from partmanip_amd.algorithms import ppo
    fx = load_fixture("ppo_pn_maxmean")
    grads = {}
    for screen in (True, False):
        c = cases.case_copy(cases.PPO_CASES["ppo_pn_maxmean"])
        c.update(T=2, n_minibatches=1, n_updates=1)
        c["net"] = dict(c["net"], screen=screen)
        with tempfile.TemporaryDirectory() as d:
            run = ppo(FakeEnv(c["N"], {"normal_state": c["O"]}, c["A"]), ppo_cfg(c, device=DEV), FakeLogger(d))
        sd = cases.actor_critic_state(c["net"], c["O"], c["A"], c["action_std"], c["seed"])
        run.actor_critic.load_state_dict({k: t(v.copy()) for k, v in sd.items()})
        assert run.actor_critic.actor.screen == screen and run.actor_critic.critic.screen == screen
        st = ppo_rollout(c, fx)
        for tt in range(c["T"]):
            run.storage.add_transitions(st["observations"][tt].to(DEV), st["actions"][tt].to(DEV), st["rewards"][tt, :, 0].to(DEV),
                                        st["dones"][tt, :, 0].to(DEV), st["succs"][tt, :, 0].to(DEV), st["values"][tt].to(DEV),
                                        st["actions_log_prob"][tt, :, 0].to(DEV), st["mu"][tt].to(DEV), st["sigma"][tt].to(DEV))
        run.storage.compute_returns(t(fx["last_values"]).to(DEV), c["gamma"], c["lam"])
        run.log_dict = {}
        run.update(c["it"])
        torch.cuda.synchronize()
        f = run.actor_critic.flat()
        grads[screen] = {}
        for net_name, net in (("actor", run.actor_critic.actor), ("critic", run.actor_critic.critic)):
            off = 0
            for k, v in net.named_parameters():
                grads[screen][f"{net_name}.{k}"] = f["grad_" + net_name][off:off + v.numel()].clone()
                off += v.numel()
    assert any(float(g.abs().max()) > 0 for g in grads[False].values())
    for k, gd in grads[False].items():
        e = float((grads[True][k].double() - gd.double()).abs().max() / (gd.double().abs().max() + 1e-30))
        print(f"{k}: {e:.2e}")
        assert e < 1e-4, (k, e)
