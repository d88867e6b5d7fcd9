"""ops.rgb_planes (pm_rgb_planes_f32): a view of a colour frame, uint8 (B, V, h, w, 3), as float planes at the head of observation
rows.  Pure data movement, so every comparison is an equality of bit patterns against rgb[:, v].permute(0, 3, 1, 2).float()."""
import numpy as np
import pytest
import torch

from tests.helpers import npy, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, V = 2, 2
SENTINEL = -12345.5


def frame(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (B, V, h, w, 3), generator=g, dtype=torch.uint8)
    rgb[0, 0, 0, 0, 0], rgb[0, 0, 0, 0, 1] = 0, 255                      # both ends of the range, in every view
    rgb[1, 1, h - 1, w - 1, 2], rgb[1, 1, h - 1, w - 1, 0] = 255, 0
    rgb[0, 1, 0, w - 1, 1], rgb[1, 0, h - 1, 0, 2] = 0, 255
    return rgb


def check(h, w, tail, offset=0):
    """Both views into rows of 3*h*w + tail columns that start `offset` floats into their buffer's rows; the tail keeps its sentinel."""
    from partmanip_amd import ops
    n = 3 * h * w
    rgb = frame(h, w, 100 * h + w)
    dev = rgb.to(DEV)
    for v in range(V):
        buf = torch.full((B, offset + n + tail), SENTINEL, device=DEV)
        out = buf[:, offset:] if offset else buf
        got = ops.rgb_planes(dev, v, out)
        assert got.data_ptr() == out.data_ptr()
        want = rgb[:, v].permute(0, 3, 1, 2).float().reshape(B, n)
        assert same_bits(npy(out[:, :n]), want.numpy()), (h, w, tail, offset, v)
        assert same_bits(npy(out[:, n:]), np.full((B, tail), SENTINEL, dtype=np.float32))
        if offset:
            assert same_bits(npy(buf[:, :offset]), np.full((B, offset), SENTINEL, dtype=np.float32))


def test_vector_path_four_pixels_per_thread():
    check(2, 4, 8)                                                      # h*w % 4 == 0, ldo % 4 == 0, aligned bases


def test_scalar_path_pixel_count_no_multiple_of_four():
    check(3, 5, 8)                                                      # h*w = 15


def test_scalar_path_misaligned_row_stride():
    check(2, 4, 5)                                                      # ldo = 29


def test_scalar_path_misaligned_base():
    check(2, 4, 4, offset=4)                                            # ldo = 32, rows start 16 bytes in: still the vector path
    check(2, 4, 7, offset=1)                                            # ldo = 32, rows start 4 bytes in: the scalar path


def test_the_image_rig_size():
    check(72, 128, 22)                                                  # more than one work-group; a proprio-sized tail


def test_without_out_a_fresh_row_is_returned():
    from partmanip_amd import ops
    rgb = frame(2, 4, 7)
    got = ops.rgb_planes(rgb.to(DEV), 1, None)
    assert tuple(got.shape) == (B, 24) and same_bits(npy(got), rgb[:, 1].permute(0, 3, 1, 2).float().reshape(B, 24).numpy())


def test_bad_view_and_short_rows_are_rejected_without_a_launch():
    from partmanip_amd import ops
    from partmanip_amd._lib import lib
    h, w = 2, 4
    dev = frame(h, w, 9).to(DEV)
    out = torch.full((B, 3 * h * w), SENTINEL, device=DEV)
    for v in (-1, V):
        with pytest.raises(RuntimeError, match="PM_EINVAL"):
            ops.rgb_planes(dev, v, out)
    with pytest.raises(ValueError, match="out"):
        ops.rgb_planes(dev, 0, out[:, :3 * h * w - 1])
    with pytest.raises(ValueError, match="uint8"):
        ops.rgb_planes(dev.float(), 0, out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgb_planes(dev.cpu(), 0, out)
    p, o = dev.data_ptr(), out.data_ptr()
    assert lib.pm_rgb_planes_f32(p, B, V, h, w, 0, o, 3 * h * w - 1, None) == -1      # ldo < 3*h*w
    assert lib.pm_rgb_planes_f32(p, B, V, h, w, V, o, 3 * h * w, None) == -1
    assert lib.pm_rgb_planes_f32(p, B, V, 0, w, 0, o, 3 * h * w, None) == -1
    assert lib.pm_rgb_planes_f32(p, 0, V, h, w, 0, o, 3 * h * w, None) == -1
    assert lib.pm_rgb_planes_f32(None, B, V, h, w, 0, o, 3 * h * w, None) == -1
    torch.cuda.synchronize()
    assert same_bits(npy(out), np.full((B, 3 * h * w), SENTINEL, dtype=np.float32))    # nothing was written
