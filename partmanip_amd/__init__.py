"""partmanip_amd: the MI355X learner and the simulator-free task loop.  Importing the package loads nothing; the submodules load the
HIP library when they are first used (`from partmanip_amd import KinematicEnv` resolves to partmanip_amd.envs.KinematicEnv)."""


def __getattr__(name):
    if name == "KinematicEnv":
        from .envs import KinematicEnv
        return KinematicEnv
    raise AttributeError(f"module 'partmanip_amd' has no attribute {name!r}")
