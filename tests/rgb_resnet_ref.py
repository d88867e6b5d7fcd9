"""The colour-image student in plain torch: the test reference of partmanip_amd's ResNet (reference network.py:202-234).

tests/depth_resnet_ref.py with a three-channel stem and a 3*H*W image slice; everything else (the blocks, the tape of pinned ReLU
masks and pool winners, the head) is that module's own code."""
import torch
import torch.nn as nn

from tests import depth_resnet_ref as D

H, W, IN_CH = D.H, D.W, 3


class RGBResNetRef(D.DepthResNetRef):
    def __init__(self, input_dim, output_dim, activation="tanh", proprio_shape=0):
        super().__init__(input_dim - (IN_CH - 1) * H * W, output_dim, activation, proprio_shape)     # (its assert is on H*W + proprio)
        self.resnet34.conv1 = nn.Conv2d(IN_CH, 64, 7, 2, 3, bias=False)

    def forward(self, x, tape=None, channels_last=False, record=None):
        img = x[:, :IN_CH * H * W].reshape(x.shape[0], IN_CH, H, W)
        if channels_last:
            img = img.contiguous(memory_format=torch.channels_last)
        f = self.resnet34(img, D._Tape(tape, record))
        if self.proprio_shape:
            f = torch.cat((f, x[:, -self.proprio_shape:]), dim=-1)
        return self.final_mlp(f)


def expected_keys():
    """depth_resnet_ref.expected_keys() with the stem changed to three channels."""
    out = D.expected_keys()
    out["resnet34.conv1.weight"] = (64, IN_CH, 7, 7)
    return out
