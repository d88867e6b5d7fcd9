"""The two schedules of the screened PointNet forward (csrc/pointnet_enc_screen.h, SCHED: 0 = all eight waves in lock-step,
1 = waves 4-7 run the saved-layer-2 copy before the screen instead of after the finish) order the same work differently and
change no arithmetic: every output of schedule 1 must equal schedule 0's bit for bit, NaN payloads included.  Correctness
against the dense kernel is tests/test_gpu_pointnet_screen.py's, which runs the library's default schedule."""
import ctypes
import tempfile

import pytest
import torch

from partmanip_amd import ops
from tests.golden import cases
from tests.helpers import load_fixture, t, ppo_cfg, ppo_rollout, FakeEnv, FakeLogger

DEV = "cuda:0"


def weights(C, seed):
    torch.manual_seed(seed)
    lin = [torch.nn.Linear(C, 128), torch.nn.Linear(128, 256), torch.nn.Linear(256, 512)]
    w = {f"{k}{i + 1}": getattr(m, a).detach().to(DEV).contiguous() for i, m in enumerate(lin) for k, a in (("W", "weight"), ("b", "bias"))}
    w["packed"] = torch.empty(ops.pointnet_packed_elems(), device=DEV)
    ops.pointnet_pack(w["W2"], w["W3"], w["packed"])
    w["packed_s"] = torch.empty(ops.pointnet_packed_screen_bytes(), dtype=torch.uint8, device=DEV)
    ops.pointnet_pack_screen(w["W3"], w["b3"], w["packed_s"])
    return w


def inputs(B, P, C, seed):
    """name -> (B, P, C) clouds.  `equal_first` / `random_first` alternate 64-point tiles of one repeated point and of random
    points, so the dense fallback and the survivor path alternate from tile to tile (at P = 64 there is only the first kind)."""
    g = torch.Generator().manual_seed(seed)
    rnd = torch.rand(B, P, C, generator=g) * 2 - 1 + (torch.rand(B, 1, C, generator=g) - 0.5)
    one = rnd[:, :1].expand(B, P, C)
    tile = (torch.arange(P) // 64)[None, :, None]
    out = {"random": rnd, "equal_first": torch.where(tile % 2 == 0, one, rnd), "random_first": torch.where(tile % 2 == 1, one, rnd),
           "all_equal": one.clone()}
    nan = rnd.clone()
    nan[B - 1, P - 7, 1] = float("nan")
    inf = rnd.clone()
    inf[0, 5, 0] = float("inf")
    inf[0, 5, 2] = float("-inf")
    out["nan"], out["inf"] = nan, inf
    return out


def forward(w, pts, schedule, max_mean, sub_mean, save_h2):
    B, P, C = pts.shape
    x = pts.reshape(B, -1).to(DEV).contiguous()
    feat = torch.empty(B, 512 * (2 if max_mean else 1), device=DEV)
    am = torch.empty(B, 512, dtype=torch.int32, device=DEV)
    h2 = torch.empty(B, P, 256, device=DEV) if save_h2 else None
    cnt = torch.zeros(3, dtype=torch.int64, device=DEV)
    ops.pointnet_enc_fwd_screen(x, P, C, sub_mean, w["W1"], w["b1"], w["b2"], w["b3"], w["packed"], w["packed_s"], max_mean, feat,
                                am, h2, cnt, schedule=schedule)
    return feat, am, h2, cnt


def bits(a):
    return a.view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 4, 6])
@pytest.mark.parametrize("P", [64, 128, 192, 320])
def test_schedules_agree_bit_for_bit(P, C):
    w = weights(C, 10 * C + 1)
    fallbacks = survivors = 0
    for B in (1, 3):
        for name, pts in inputs(B, P, C, 100 * P + 10 * C + B).items():
            for max_mean in (True, False):
                for sub_mean in (False, True):
                    for save_h2 in (True, False):
                        f0, a0, h0, c0 = forward(w, pts, 0, max_mean, sub_mean, save_h2)
                        f1, a1, h1, c1 = forward(w, pts, 1, max_mean, sub_mean, save_h2)
                        label = f"B={B} P={P} C={C} {name} mm={max_mean} sub={sub_mean} h2={save_h2}"
                        assert torch.equal(bits(f0[:, :512]), bits(f1[:, :512])), label + ": max features"
                        if max_mean:
                            assert torch.equal(bits(f0[:, 512:]), bits(f1[:, 512:])), label + ": mean features"
                        assert torch.equal(a0, a1), label + ": argmax"
                        if save_h2:
                            assert torch.equal(bits(h0), bits(h1)), label + ": h2_save"
                        assert torch.equal(c0, c1), label + ": counters"
                        if name == "all_equal":         # every (wave, tile) pair on the dense fallback, under both schedules
                            assert c1.tolist()[1] == B * (P // 64) * 8, label
                        if name == "nan":
                            assert bool(torch.isnan(f1[B - 1]).all()), label
                        survivors += c1.tolist()[0]
                        fallbacks += c1.tolist()[1]
    assert survivors > 0 and fallbacks > 0              # both paths ran


@pytest.mark.gpu
def test_schedule_is_validated_on_the_device_path():
    w = weights(3, 3)
    pts = inputs(1, 64, 3, 1)["random"]
    for bad in (-1, 2, 7):
        with pytest.raises(RuntimeError):
            forward(w, pts, bad, True, False, True)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_whole_update_gradients_agree_between_schedules():
    """The PPO mini-batch update of test_whole_update_screened_against_dense (B = 8) under schedule 0 and under schedule 1:
    every gradient bit-equal."""
    from partmanip_amd.algorithms import ppo
    fx = load_fixture("ppo_pn_maxmean")
    grads = {}
    for schedule in (0, 1):
        c = cases.case_copy(cases.PPO_CASES["ppo_pn_maxmean"])
        c.update(T=2, n_minibatches=1, n_updates=1)
        c["net"] = dict(c["net"], screen=True)
        with tempfile.TemporaryDirectory() as d:
            run = ppo(FakeEnv(c["N"], {"normal_state": c["O"]}, c["A"]), ppo_cfg(c, device=DEV), FakeLogger(d))
        sd = cases.actor_critic_state(c["net"], c["O"], c["A"], c["action_std"], c["seed"])
        run.actor_critic.load_state_dict({k: t(v.copy()) for k, v in sd.items()})
        for net in (run.actor_critic.actor, run.actor_critic.critic):
            assert net.screen
            net.screen_schedule = schedule
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
        grads[schedule] = {k: f[k].clone() for k in ("grad_actor", "grad_critic")}
    for k, g0 in grads[0].items():
        assert float(g0.abs().max()) > 0, k
        assert torch.equal(bits(g0), bits(grads[1][k])), k


def test_new_entry_point_refuses_bad_arguments_without_gpu():
    """A schedule other than 0 or 1, or a null pointer, is refused (-1) before any launch: safe on a host without a GPU.  The
    pointers of the schedule cases are host buffers that a refused call never touches."""
    from partmanip_amd._lib import lib
    fn = lib.pm_pointnet_enc_fwd_screen_sched_f32
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 63) & ~63
    good = [p, 192, 1, 64, 3, 0, p, p, p, p, p, p, 1, p, 1024, p, None, None]
    for schedule in (-1, 2, 3, 1 << 20):
        assert fn(*good, schedule, None) == -1, schedule
    for schedule in (0, 1):
        assert fn(None, 192, 1, 64, 3, 0, None, None, None, None, None, None, 1, None, 1024, None, None, None, schedule, None) == -1
        for i in (0, 6, 7, 8, 9, 10, 11, 13, 15):      # every required pointer, one at a time
            args = list(good)
            args[i] = None
            assert fn(*args, schedule, None) == -1, (schedule, i)
        assert fn(*good[:3], 65, *good[4:], schedule, None) == -1      # P no multiple of the tile
