"""ops.im2col2d (pm_im2col2d_f32): the patch matrix of a planar C-channel image, columns (c, kh, kw).  Pure data movement: equality
of bit patterns against torch.nn.functional.unfold reordered to rows (b, oh, ow), and against ops.im2col2d_c1 at C = 1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import npy, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def unfold_rows(x4, k, stride, pad):
    """(B, C, H, W) -> (B*Ho*Wo, C*k*k), rows (b, oh, ow), columns (c, kh, kw): unfold's own column order."""
    u = F.unfold(x4, k, padding=pad, stride=stride)                       # (B, C*k*k, Ho*Wo)
    return u.transpose(1, 2).reshape(-1, u.shape[1]).contiguous()


def run(B, C, H, W, k, stride, pad, row_tail=0, ldd=None, seed=0):
    from partmanip_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C * H * W + row_tail, generator=g)
    x[:, C * H * W:] = float("inf")                                       # a tail that must never be read into the matrix
    want = unfold_rows(x[:, :C * H * W].reshape(B, C, H, W), k, stride, pad)
    ldd = C * k * k if ldd is None else ldd
    dst = torch.full((want.shape[0], ldd), float("nan"), device=DEV)
    got = ops.im2col2d(x.to(DEV), C, H, W, k, stride, pad, dst)
    assert got.data_ptr() == dst.data_ptr()
    full = np.zeros((want.shape[0], ldd), dtype=np.float32)               # pad columns: exactly +0
    full[:, :C * k * k] = want.numpy()
    assert same_bits(npy(dst), full), (B, C, H, W, k, stride, pad, row_tail, ldd)


def test_kernel_wider_than_the_image_padding_on_every_side():
    run(2, 3, 5, 7, 7, 2, 3)


def test_three_by_three_stride_one():
    run(2, 3, 6, 9, 3, 1, 1, seed=1)


def test_one_by_one_stride_two_no_padding():
    run(2, 2, 4, 4, 1, 2, 0, seed=2)


def test_rows_with_a_tail():
    run(2, 3, 5, 7, 7, 2, 3, row_tail=5, seed=3)                          # ldx > C*H*W


def test_pad_columns_are_zero_on_a_nan_destination():
    run(2, 3, 5, 7, 7, 2, 3, ldd=160, seed=4)                             # the RGB stem's own 147 -> 160
    run(2, 3, 6, 9, 3, 1, 1, row_tail=2, ldd=32, seed=5)


def test_the_stems_geometry_and_more_groups_than_one_grid_pass():
    run(3, 3, 72, 128, 7, 2, 3, row_tail=5, ldd=160, seed=6)              # the RGB stem as the student calls it
    # 44 * 36 * 64 rows x 22 groups = 2 230 272 threads' worth against a grid capped at 8192 x 256: the grid-stride loop turns
    run(44, 3, 72, 128, 7, 2, 3, seed=8)


def test_one_channel_at_the_stems_geometry_gives_im2col2d_c1s_bits():
    from partmanip_amd import ops
    B, H, W = 2, 72, 128
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H * W + 5, generator=g).to(DEV)
    rows = B * 36 * 64
    old = ops.im2col2d_c1(x[:, :H * W], H, W, 7, 2, 3, torch.full((rows, 64), float("nan"), device=DEV))
    new = ops.im2col2d(x, 1, H, W, 7, 2, 3, torch.full((rows, 64), float("nan"), device=DEV))
    assert same_bits(npy(new), npy(old))


def test_bad_arguments_are_rejected_without_a_launch():
    from partmanip_amd import ops
    from partmanip_amd._lib import lib
    x = torch.zeros(2, 3 * 5 * 7, device=DEV)
    with pytest.raises(ValueError, match="im2col2d"):
        ops.im2col2d(x, 3, 5, 7, 7, 2, 3, torch.empty(2 * 3 * 4, 146, device=DEV))       # ldd < C*k*k
    with pytest.raises(ValueError, match="im2col2d"):
        ops.im2col2d(x, 4, 5, 7, 7, 2, 3, torch.empty(2 * 3 * 4, 196, device=DEV))       # rows shorter than C*H*W
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.im2col2d(x.cpu(), 3, 5, 7, 7, 2, 3, torch.empty(2 * 3 * 4, 147, device=DEV))
    d = torch.empty(2 * 3 * 4, 147, device=DEV)
    assert lib.pm_im2col2d_f32(x.data_ptr(), 105, 2, 3, 5, 7, 7, 2, 3, d.data_ptr(), 146, None) == -1
    assert lib.pm_im2col2d_f32(x.data_ptr(), 104, 2, 3, 5, 7, 7, 2, 3, d.data_ptr(), 147, None) == -1
    assert lib.pm_im2col2d_f32(x.data_ptr(), 105, 2, 0, 5, 7, 7, 2, 3, d.data_ptr(), 147, None) == -1
    assert lib.pm_im2col2d_f32(x.data_ptr(), 105, 2, 3, 5, 7, 7, 0, 3, d.data_ptr(), 147, None) == -1
