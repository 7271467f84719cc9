"""pyracecarsimulator_amd — MI355X-native batched 2D lidar scan path.

Scope: ``ScanSimulator2D.scan/scanMany`` over a ``range_libc``-compatible
``PyOMap`` / ``PyRayMarching[GPU]`` / ``PyCDDTCast`` surface, implemented as hand-written
HIP kernels for gfx950 behind the C ABI in ``include/scanlib.h``.
"""
from . import league, maps, racecar, range_libc     # noqa: F401
from .scan_simulator import ScanSimulator2D          # noqa: F401
from .racecar_simulator import RacecarSimulator      # noqa: F401
from .policy import Policy                           # noqa: F401
from .population import PolicyPopulation             # noqa: F401
from .league import round_robin                      # noqa: F401
from .mcts import MCTS                               # noqa: F401
from .particle_filter import ParticleFilter          # noqa: F401
from .env import DriveEnv, RaceEnv                   # noqa: F401
from .track import Track                             # noqa: F401

__all__ = ["league", "maps", "racecar", "range_libc", "ScanSimulator2D", "RacecarSimulator", "Policy", "PolicyPopulation",
           "round_robin", "MCTS", "ParticleFilter", "DriveEnv", "RaceEnv", "Track"]
