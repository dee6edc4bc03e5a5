"""The agents. The vectorised tabular populations and the REINFORCE drop-in are exported here by
name; they are imported on first use, so importing a sibling module stays as light as it was."""
_EXPORTS = {"VectorQAgent": "vector_q", "VectorDoubleQAgent": "vector_dq", "RFAgent": "rf_agent",
            "PolicyNetwork": "rf_agent"}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
