"""The agents. The vectorised tabular populations, the REINFORCE drop-in and the recurrent DQN
drop-in (as LSTMDQN / LSTMDQNAgent: its classes are named DQN / DQNAgent like dqn_agent's) are
exported here by name; they are imported on first use, so importing a sibling module stays as light as it was."""
_EXPORTS = {"VectorQAgent": "vector_q", "VectorDoubleQAgent": "vector_dq", "RFAgent": "rf_agent",
            "PolicyNetwork": "rf_agent", "LSTMDQN": ("lstm_dqn_agent", "DQN"),
            "LSTMDQNAgent": ("lstm_dqn_agent", "DQNAgent")}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        mod, attr = _EXPORTS[name] if isinstance(_EXPORTS[name], tuple) else (_EXPORTS[name], name)
        return getattr(importlib.import_module("." + mod, __name__), attr)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
