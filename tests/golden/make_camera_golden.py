"""Dev-machine generator of the camera-pose fixture (tests/test_mesh_depth_host.py): runs the REFERENCE's own gen_camera_pose
(utils/camera.py:103-209) with the arguments of tasks/hand_base.py:162-191, for the `cam` blocks of both shipped task configs.

    python tests/golden/make_camera_golden.py /path/to/reference

The reference module imports scipy.spatial.transform at its top and uses it only on its camera-noise path, which is not run: where
scipy is missing an empty stand-in is put into sys.modules first.  Writes camera_poses_ref.npz: per task `<task>_look_at`,
`<task>_radius` and `<task>_pose_mat` (V, 4, 4) float64, the last item of the tuple the reference returns, plus the shared arguments
alpha_range_list, num_point_ver_list, num_point_hor and beta_range.  Only the matrices and the arguments are stored."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
TASKS = ("grasp_cube", "open_drawer")
ALPHA_RANGE_LIST = [(-45 * math.pi / 180, 225 * math.pi / 180)]               # hand_base.py:164
NUM_POINT_VER_LIST = [3]                                                      # hand_base.py:162
NUM_POINT_HOR = 1                                                             # hand_base.py:163
BETA_RANGE = (40 * math.pi / 180, 70 * math.pi / 180)                         # hand_base.py:165


def main(reference_root):
    try:
        import scipy.spatial.transform  # noqa: F401
    except ImportError:
        for name in ("scipy", "scipy.spatial", "scipy.spatial.transform"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["scipy.spatial.transform"].Rotation = None
    spec = importlib.util.spec_from_file_location("ref_camera", os.path.join(reference_root, "utils", "camera.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = dict(alpha_range_list=np.asarray(ALPHA_RANGE_LIST, dtype=np.float64), num_point_ver_list=np.asarray(NUM_POINT_VER_LIST),
               num_point_hor=np.int64(NUM_POINT_HOR), beta_range=np.asarray(BETA_RANGE, dtype=np.float64))
    for task in TASKS:
        with open(os.path.join(reference_root, "cfg", "tasks", task + ".yaml")) as f:
            cam = yaml.safe_load(f)["cam"]
        pose_mat = ref.gen_camera_pose(np.asarray(cam["look_at"], dtype=np.float64), ALPHA_RANGE_LIST, NUM_POINT_VER_LIST,
                                       NUM_POINT_HOR, BETA_RANGE, cam["radius"])[-1]
        assert pose_mat.shape == (3, 4, 4) and pose_mat.dtype == np.float64
        out[task + "_look_at"] = np.asarray(cam["look_at"], dtype=np.float64)
        out[task + "_radius"] = np.float64(cam["radius"])
        out[task + "_pose_mat"] = pose_mat
    path = os.path.join(HERE, "camera_poses_ref.npz")
    np.savez_compressed(path, **out)
    print(f"camera_poses_ref: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
