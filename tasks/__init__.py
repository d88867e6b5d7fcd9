"""Import surface in the manner of the reference's `tasks` package: `from tasks import GraspCubeTensors, OpenDrawerTensors, Franka, MobileFranka`
resolve to the MI355X-native tensor programs in `partmanip_amd.tasks` (no simulator inside)."""
from partmanip_amd.tasks import Franka, GraspCubeTensors, MobileFranka, OpenDrawerTensors  # noqa: F401
