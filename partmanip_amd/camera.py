"""Camera poses of the reference's hemisphere rig (utils/camera.py:103-209, the last item of the tuple gen_camera_pose returns)
and the shipped rig built from them (tasks/hand_base.py:162-191).  Host code, numpy only.

Written from the geometry.  A camera sits on a sphere of radius r around `look_at` at azimuth alpha (from the x axis, counter-
clockwise about z) and polar angle beta (from the z axis):
    position = look_at + r (sin beta cos alpha, sin beta sin alpha, cos beta).
It looks at `look_at` with the world's z axis as `up`.  The returned matrices are camera->world in the convention of
TSDFVolume.register_camera and DepthFromMesh: the camera looks along its +z axis, x to the right, y down, so the columns are
    z = (look_at - position) / |look_at - position|,   x = z x up / |z x up|,   y = z x x,
and the last column is the position.  (The reference gets a frame looking along -z by fitting a rotation to four points and then
flips y and z; the result is the same matrix.)  The camera-noise option of the reference (is_camera_rand) is left out.
"""
import math

import numpy as np

HORIZONTAL_FOV = 69.75                                                        # hand_base.py:166, degrees
HEMISPHERE_ALPHA_RANGE_LIST = [(-45 * math.pi / 180, 225 * math.pi / 180)]    # hand_base.py:164
HEMISPHERE_NUM_POINT_VER_LIST = [3]                                           # hand_base.py:162
HEMISPHERE_NUM_POINT_HOR = 1                                                  # hand_base.py:163
HEMISPHERE_BETA_RANGE = (40 * math.pi / 180, 70 * math.pi / 180)              # hand_base.py:165
IMAGE_WIDTH, IMAGE_HEIGHT = 512, 288                                          # hand_base.py:176-177; a quarter of each in image mode


def _steps(lo, hi, count):
    """`count` equally spaced values from lo to hi inclusive; lo alone for one."""
    return [lo + (hi - lo) * i / (count - 1) for i in range(count)] if count > 1 else [lo]


def look_at_pose(position, look_at, up=(0.0, 0.0, 1.0)):
    """(4, 4) camera->world of a camera at `position` looking at `look_at` along its +z axis, x right, y down."""
    position, look_at, up = (np.asarray(a, dtype=np.float64) for a in (position, look_at, up))
    z = look_at - position
    z = z / np.linalg.norm(z)
    x = np.cross(z, up)
    if not np.linalg.norm(x) > 0:
        raise ValueError("look_at_pose: the viewing direction is parallel to `up`")
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, position
    return pose


def gen_camera_pose(look_at, alpha_range_list, num_point_ver_list, num_point_hor, beta_range, r):
    """(V, 4, 4) float64 camera->world matrices, V = sum(num_point_ver_list) * num_point_hor, ordered as the reference orders them:
    for every alpha range in turn, its num_point_ver azimuths from the first to the last of the range, and for every azimuth the
    num_point_hor polar angles from beta_range[0] to beta_range[1]."""
    if len(alpha_range_list) != len(num_point_ver_list):
        raise ValueError("gen_camera_pose: one num_point_ver per alpha range is needed")
    look_at = np.asarray(look_at, dtype=np.float64)
    poses = []
    for (a_lo, a_hi), count in zip(alpha_range_list, num_point_ver_list):
        for alpha in _steps(a_lo, a_hi, count):
            for beta in _steps(beta_range[0], beta_range[1], num_point_hor):
                offset = r * np.array([math.sin(beta) * math.cos(alpha), math.sin(beta) * math.sin(alpha), math.cos(beta)])
                poses.append(look_at_pose(look_at + offset, look_at))
    return np.stack(poses)


def shipped_rig(cfg_cam, image_mode=False):
    """(cam_pose (V, 4, 4), intrinsic (3, 3), im_h, im_w) as hand_base.py:162-191 derives them from a task config's `cam` block
    ({'look_at': [x, y, z], 'radius': r}): three views at 512 x 288, or view 0 alone at 128 x 72 when the observation is an image
    (image_mode, the reference's "'img' in learn_input_mode"); fx = fy = width / 2 / tan(horizontal_fov / 2) with a horizontal
    field of view of 69.75 degrees, principal point (width // 2, height // 2)."""
    poses = gen_camera_pose(cfg_cam['look_at'], HEMISPHERE_ALPHA_RANGE_LIST, HEMISPHERE_NUM_POINT_VER_LIST, HEMISPHERE_NUM_POINT_HOR,
                            HEMISPHERE_BETA_RANGE, cfg_cam['radius'])
    im_w, im_h = (IMAGE_WIDTH // 4, IMAGE_HEIGHT // 4) if image_mode else (IMAGE_WIDTH, IMAGE_HEIGHT)
    if image_mode:
        poses = poses[:1]
    fx = im_w / 2.0 / math.tan((HORIZONTAL_FOV / 180.0 * math.pi) / 2.0)
    intrinsic = np.array([[fx, 0, im_w // 2], [0, fx, im_h // 2], [0, 0, 1]])
    return poses, intrinsic, im_h, im_w
