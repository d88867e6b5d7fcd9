"""The depth-image student in plain torch (nn.Conv2d, nn.BatchNorm2d, ...): the test reference of partmanip_amd's depthResNet.

Written from the published ResNet-34 (He et al. 2016) under torchvision's module names, with the reference's single-channel stem
and head (network.py:237-271).  torchvision is not installed where the tests run, so the reference's own class cannot be
instantiated; this module stands in for it and there are no golden files from it.

`forward(x, tape=...)`: with a tape (what `depthResNet.saved_signs()` returns: the stem's ReLU mask, the max pool's indices, two
ReLU masks per block, NCHW) every ReLU multiplies by the given mask and the pool gathers through the given indices, so that the
network is a smooth function of its parameters and its gradient can be compared across number formats."""
import torch
import torch.nn as nn
import torch.nn.functional as F

H, W = 72, 128
BLOCKS, WIDTHS = (3, 4, 6, 3), (64, 128, 256, 512)
_ACT = {"tanh": nn.Tanh, "relu": nn.ReLU, "elu": nn.ELU, "selu": nn.SELU, "lrelu": nn.LeakyReLU, "sigmoid": nn.Sigmoid}


class _Tape:
    def __init__(self, items, record=None):
        self.items, self.pos, self.record = (list(items) if items is not None else None), 0, record

    def take(self):
        it = self.items[self.pos]
        self.pos += 1
        return it

    def relu(self, x):
        if self.items is None:
            out = F.relu(x)
            if self.record is not None:
                self.record.append(out.detach() > 0)
            return out
        return x * self.take().to(device=x.device, dtype=x.dtype)

    def pool(self, x):
        if self.items is None:
            out, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
            if self.record is not None:
                self.record.append(idx)
            return out
        idx = self.take().to(x.device)
        return x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x, tape):
        out = tape.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        short = x if self.downsample is None else self.downsample(x)
        return tape.relu(out + short)


class ResNet34(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for l, (n, c) in enumerate(zip(BLOCKS, WIDTHS)):
            blocks = []
            for i in range(n):
                blocks.append(BasicBlock(cin, c, 2 if (i == 0 and l > 0) else 1))
                cin = c
            setattr(self, f"layer{l + 1}", nn.Sequential(*blocks))
        for m in self.modules():
            if isinstance(m, nn.Conv2d) and m is not self.conv1:
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, img, tape):
        x = tape.pool(tape.relu(self.bn1(self.conv1(img))))
        for l in range(4):
            for blk in getattr(self, f"layer{l + 1}"):
                x = blk(x, tape)
        return x.mean(dim=(2, 3))


class DepthResNetRef(nn.Module):
    def __init__(self, input_dim, output_dim, activation="tanh", proprio_shape=0):
        super().__init__()
        assert input_dim == H * W + proprio_shape
        self.resnet34 = ResNet34()
        self.proprio_shape = proprio_shape
        self.final_mlp = nn.Sequential(nn.Linear(512 + proprio_shape, 128), _ACT[activation](), nn.Linear(128, 32), _ACT[activation](),
                                       nn.Linear(32, output_dim))

    def forward(self, x, tape=None, channels_last=False, record=None):
        """record: a list that an untaped run appends its own masks and indices to (a tape for a later run)."""
        img = x[:, :H * W].reshape(x.shape[0], 1, H, W)
        if channels_last:
            img = img.contiguous(memory_format=torch.channels_last)
        f = self.resnet34(img, _Tape(tape, record))
        if self.proprio_shape:
            f = torch.cat((f, x[:, -self.proprio_shape:]), dim=-1)
        return self.final_mlp(f)


def expected_keys():
    """torchvision's resnet34 state_dict keys (without fc) under `resnet34.`, and the head's, with their shapes, by rule."""
    out = {}

    def bn(p, c):
        out[p + ".weight"] = (c,)
        out[p + ".bias"] = (c,)
        out[p + ".running_mean"] = (c,)
        out[p + ".running_var"] = (c,)
        out[p + ".num_batches_tracked"] = ()
    out["resnet34.conv1.weight"] = (64, 1, 7, 7)
    bn("resnet34.bn1", 64)
    cin = 64
    for l, (n, c) in enumerate(zip(BLOCKS, WIDTHS)):
        for i in range(n):
            p = f"resnet34.layer{l + 1}.{i}"
            out[p + ".conv1.weight"] = (c, cin, 3, 3)
            bn(p + ".bn1", c)
            out[p + ".conv2.weight"] = (c, c, 3, 3)
            bn(p + ".bn2", c)
            if i == 0 and l > 0:
                out[p + ".downsample.0.weight"] = (c, cin, 1, 1)
                bn(p + ".downsample.1", c)
            cin = c
    return out
