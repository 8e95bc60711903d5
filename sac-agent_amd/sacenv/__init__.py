"""sacenv — MI355X-native vectorised boat environment engine.

Hot path of Nilau1998/SAC-Agent (environment/boat_env.py, wind.py,
reward_functions.py, control_theory/control_blocks.py) as gfx950 HIP kernels
behind the reference's Gym surface. See DESIGN.md / INTEGRATION.md.
"""
from . import _lib
from .config import BoatConfig
from .spaces import Box

__all__ = ["BoatConfig", "Box", "VecBoatEnv", "BoatEnv", "ParachuteEnv", "CarEnv", "VecToyEnv",
           "MixedBatch", "NativeSACPopulation", "sample_hpsets", "HPRanges", "PopulationReplay", "PolicyNoise",
           "MemberScoreboard", "PopulationSelection", "BestEpisodes", "EpisodeFrames",
           "PrioritizedPopulationReplay", "_lib"]


def __getattr__(name):  # lazy: importing torch-dependent classes only when used
    if name == "VecBoatEnv":
        from .vec_env import VecBoatEnv
        return VecBoatEnv
    if name == "BoatEnv":
        from .boat_env import BoatEnv
        return BoatEnv
    if name in ("ParachuteEnv", "CarEnv", "VecToyEnv", "MixedBatch"):
        from . import toys
        return getattr(toys, name)
    if name in ("NativeSACPopulation", "sample_hpsets", "HPRanges"):
        from . import population
        return getattr(population, name)
    if name == "PopulationReplay":
        from .population_replay import PopulationReplay
        return PopulationReplay
    if name == "PrioritizedPopulationReplay":
        from .prioritized import PrioritizedPopulationReplay
        return PrioritizedPopulationReplay
    if name == "PolicyNoise":
        from .noise import PolicyNoise
        return PolicyNoise
    if name == "MemberScoreboard":
        from .scoreboard import MemberScoreboard
        return MemberScoreboard
    if name == "PopulationSelection":
        from .selection import PopulationSelection
        return PopulationSelection
    if name == "BestEpisodes":
        from .traces import BestEpisodes
        return BestEpisodes
    if name == "EpisodeFrames":
        from .frames import EpisodeFrames
        return EpisodeFrames
    raise AttributeError(name)
