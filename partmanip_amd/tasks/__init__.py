"""The task steps of the reference (tasks/grasp_cube.py, tasks/open_drawer.py, tasks/load_robot.py, tasks/hand_base.py) as tensor
programs without a simulator: see grasp_cube.GraspCubeTensors and open_drawer.OpenDrawerTensors;
franka.MobileFranka is the shipped open_drawer robot."""
from .franka import Franka, MobileFranka  # noqa: F401
from .grasp_cube import GraspCubeTensors  # noqa: F401
from .open_drawer import OpenDrawerTensors  # noqa: F401
