"""The ResNet (rgb_img) student without a GPU: parameter names and shapes, the `pretrained` contract (a local file or an explicit
False, never a download), the observer's width, the shipped configuration."""
import os
import types

import pytest
import torch

from tests import rgb_resnet_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPRIO, OUT = 5, 8
OBS = 3 * 72 * 128 + PROPRIO
CFG = dict(name="ResNet", activation="tanh", pretrained=False)
HEAD = {"final_mlp.0.weight": (128, 512 + PROPRIO), "final_mlp.0.bias": (128,), "final_mlp.2.weight": (32, 128),
        "final_mlp.2.bias": (32,), "final_mlp.4.weight": (OUT, 32), "final_mlp.4.bias": (OUT,)}


def student(cfg=CFG):
    from partmanip_amd.algo_utils.network import ResNet
    return ResNet(OBS, OUT, cfg, PROPRIO)


def torchvision_style_state(seed=0):
    """A state_dict with torchvision's bare resnet34 keys (fc.* included), every tensor random: the running statistics too."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in ref.expected_keys().items():
        bare = k[len("resnet34."):]
        if bare.endswith("num_batches_tracked"):
            sd[bare] = torch.tensor(7, dtype=torch.int64)
        elif bare.endswith("running_var"):
            sd[bare] = 0.5 + torch.rand(shape, generator=g)
        else:
            sd[bare] = torch.randn(shape, generator=g)
    sd["fc.weight"] = torch.randn(1000, 512, generator=g)
    sd["fc.bias"] = torch.randn(1000, generator=g)
    return sd


def test_state_dict_keys_and_shapes_are_the_depth_students_with_a_three_channel_stem():
    from partmanip_amd.algo_utils.network import depthResNet
    sd = student().state_dict()
    want = ref.expected_keys()
    assert want["resnet34.conv1.weight"] == (64, 3, 7, 7)
    want.update(HEAD)
    assert list(sd.keys()) == list(want.keys())
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    depth = depthResNet(72 * 128 + PROPRIO, OUT, dict(name="depthResNet", activation="tanh"), PROPRIO).state_dict()
    assert list(depth.keys()) == list(sd.keys())
    assert [k for k in sd if sd[k].shape != depth[k].shape] == ["resnet34.conv1.weight"]
    r = ref.RGBResNetRef(OBS, OUT, "tanh", PROPRIO).state_dict()
    assert list(r.keys()) == list(sd.keys()) and [tuple(v.shape) for v in r.values()] == [tuple(v.shape) for v in sd.values()]


def test_pretrained_false_gives_the_depth_students_initialisation():
    torch.manual_seed(0)
    net = student()
    assert not getattr(net, "supports_row_index", False)                      # (dagger.py reads it so: the depth student's answer)
    w = net.resnet34.layer3[1].conv1.weight.detach()
    assert abs(float(w.std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02          # Kaiming-normal, fan_out
    assert float(net.resnet34.conv1.weight.detach().abs().max()) <= 1.0 / (3 * 49) ** 0.5 + 1e-6      # nn.Conv2d's default: 1 / sqrt(fan_in)
    assert all(p.numel() % 4 == 0 for p in net.resnet34.parameters())         # every flat view starts 16-byte aligned


def test_wrong_input_dim_raises_value_error():
    from partmanip_amd.algo_utils.network import ResNet
    with pytest.raises(ValueError, match="input_dim"):
        ResNet(72 * 128 + PROPRIO, OUT, CFG, PROPRIO)                          # the depth student's width


def test_missing_pretrained_key_says_why_before_anything_else():
    from partmanip_amd.algo_utils.network import ResNet
    for cfg in (dict(name="ResNet", activation="tanh"), dict(name="ResNet", activation="tanh", pretrained=True)):
        with pytest.raises(NotImplementedError, match="pretrained") as e:
            ResNet(1, 1, cfg, 0)                                               # (a wrong input_dim too: this check comes first)
        msg = str(e.value)
        assert "neither ships nor fetches" in msg and "False" in msg and "path" in msg


def test_pretrained_path_round_trip(tmp_path):
    sd = torchvision_style_state()
    path = tmp_path / "resnet34.pth"
    torch.save(sd, path)
    torch.manual_seed(1)
    net = student(dict(CFG, pretrained=str(path)))
    got = net.resnet34.state_dict()
    assert set(got) == set(sd) - {"fc.weight", "fc.bias"}
    for k, v in got.items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    assert torch.equal(net.resnet34.layer2[0].downsample[1].running_var, sd["layer2.0.downsample.1.running_var"])
    assert int(net.resnet34.bn1.num_batches_tracked) == 7
    assert not any(k.startswith("fc") or "fc." in k for k in net.state_dict())
    assert type(student(dict(CFG, pretrained=path))) is type(net)             # a path object works as the string does


def test_pretrained_file_with_a_missing_key_a_foreign_key_or_a_wrong_shape_is_named(tmp_path):
    sd = torchvision_style_state()
    cases = {}
    short = dict(sd)
    del short["layer3.4.bn2.running_mean"]
    cases["layer3.4.bn2.running_mean"] = short
    cases["layer9.0.conv1.weight"] = dict(sd, **{"layer9.0.conv1.weight": torch.zeros(1)})
    cases["conv1.weight"] = dict(sd, **{"conv1.weight": torch.zeros(64, 1, 7, 7)})      # a depth stem
    for i, (key, bad) in enumerate(cases.items()):
        path = tmp_path / f"bad{i}.pth"
        torch.save(bad, path)
        with pytest.raises((ValueError, KeyError, RuntimeError), match=key.replace(".", r"\.")):
            student(dict(CFG, pretrained=str(path)))


def test_pretrained_path_that_does_not_exist(tmp_path):
    with pytest.raises(FileNotFoundError, match="nowhere"):
        student(dict(CFG, pretrained=str(tmp_path / "nowhere.pth")))


def test_actor_critic_constructs_and_flattens():
    from partmanip_amd.algo_utils import ActorCritic
    torch.manual_seed(2)
    ac = ActorCritic(OBS, OUT, dict(action_std=0.1, action_activate="tanh", clipAction=1.0, network=dict(CFG)), PROPRIO)
    f = ac.flat()
    n_backbone = 21_278_400 + 64 * 2 * 49 + (512 + PROPRIO) * 128 + 128 + 128 * 32 + 32        # the depth student's + two stem channels
    assert f["n_actor"] == n_backbone + 32 * OUT + OUT and f["n_critic"] == n_backbone + 32 + 1
    assert ac.actor.resnet34.conv1.weight.data_ptr() == f["actor"].data_ptr()
    assert tuple(ac.actor.resnet34.conv1.weight.shape) == (64, 3, 7, 7)
    assert tuple(ac.actor._views["resnet34.conv1.weight"].shape) == (64, 3, 7, 7)


def test_rgb_img_observer_width_and_view_check():
    from partmanip_amd.envs import rgb_img_observer
    cam = types.SimpleNamespace(num_view=2, im_h=72, im_w=128)
    assert rgb_img_observer(cam).width == 3 * 72 * 128 and rgb_img_observer(cam, view=1).width == 3 * 72 * 128
    assert rgb_img_observer(types.SimpleNamespace(num_view=1, im_h=3, im_w=5)).width == 45
    with pytest.raises(ValueError, match="view"):
        rgb_img_observer(cam, view=2)


def test_shipped_configuration_loads():
    from partmanip_amd.config import process_cfgs
    algo = process_cfgs(["--algocfg", "dagger_rgb_img", "--taskcfg", "open_drawer"], root=ROOT)["algo"]
    assert algo["obs_mode"] == "rgb_img" and algo["add_proprio_obs"] is True and algo["algo"] == "dagger"
    assert algo["model"]["network"] == dict(name="ResNet", activation="tanh", pretrained=False)
    depth = process_cfgs(["--algocfg", "dagger_depth_img", "--taskcfg", "open_drawer"], root=ROOT)["algo"]
    for k, v in depth.items():
        if k not in ("obs_mode", "model"):
            assert algo[k] == v, k
