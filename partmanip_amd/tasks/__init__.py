"""The task step of the reference's grasp_cube (tasks/grasp_cube.py, tasks/load_robot.py, tasks/hand_base.py) as tensor programs
without a simulator: see grasp_cube.GraspCubeTensors."""
from .franka import Franka  # noqa: F401
from .grasp_cube import GraspCubeTensors  # noqa: F401
