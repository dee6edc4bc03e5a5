__all__ = ["VectorRecurrentDQNPopulation"]


def __getattr__(name):  # (on first use: the trainers import torch and load libmazerl)
    if name == "VectorRecurrentDQNPopulation":
        from .drqn_population import VectorRecurrentDQNPopulation
        return VectorRecurrentDQNPopulation
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
