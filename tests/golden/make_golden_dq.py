#!/usr/bin/env python3
"""Fixture for the double Q-learning agent from the reference's own code: agents/dq_agent.py:5-73
driven by gymnasium_env SimpleMazeEnv on the two golden 9x9 plain traces, replayed as
make_golden_agents.py replays its QAgent trace (the trace's ops are the actions; DQAgent.update
alone, no update_hyperparameter).

Per update the script records what the update drew — the coin (the first np.random.random() inside
update, < 0.5 = table A) and best_action (the inner get_action's return) — by wrapping
np.random.random and agent.get_action from here; the reference is not edited.

Test infrastructure only (build container). Writes tests/golden/dq_agent.npz (data only).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import golden_io as G  # noqa: E402

OPS, NP_SEED = 600, 7
HP = dict(learning_rate=0.1, initial_epsilon=0.95, epsilon_decay=40, final_epsilon=0.05,
          discount_factor=0.7, eta=0.01)


def replay(t, dq_agent, simple_maze_env):
    grid = [list(map(int, r)) for r in t["grid"]]
    fixed = lambda self, shape: (t["start"], t["goal"], [r[:] for r in grid])  # noqa: E731
    Env = type("FixedEnv", (simple_maze_env.SimpleMazeEnv,), {"generate_maze": fixed})
    np.random.seed(NP_SEED)
    env = Env((t["n"], t["n"]))
    agent = dq_agent.DQAgent(env, **HP)
    draws, best = [], []
    inner = agent.get_action

    def get_action(obs):
        best.append(inner(obs))
        return best[-1]
    agent.get_action = get_action
    plain = np.random.random

    def random(*a, **k):
        draws.append(plain(*a, **k))
        return draws[-1]
    seq = {k: [] for k in ("obs", "act", "rew", "term", "next", "coin", "best")}
    obs, _ = env.reset()
    np.random.random = random
    try:
        for op in t["op"][:OPS]:
            if op == 4:
                obs, _ = env.reset()
                continue
            nobs, r, tr, te, _ = env.step(int(op))
            del draws[:], best[:]
            agent.update(obs, int(op), r, te, nobs)
            assert len(draws) == 2 and len(best) == 1  # the coin, then get_action's draw
            seq["obs"].append(str(obs)); seq["act"].append(int(op)); seq["rew"].append(float(r))
            seq["term"].append(bool(te)); seq["next"].append(str(nobs))
            seq["coin"].append(bool(draws[0] < 0.5)); seq["best"].append(int(best[0]))
            obs = nobs
    finally:
        np.random.random = plain
    return agent, seq


def main(ref="/root/reference"):
    sys.path.insert(0, HERE)
    import _refstubs
    _refstubs.install()
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from agents import dq_agent
    from gymnasium_env.envs import simple_maze_env
    out = {}
    simple = [t for t in G.traces() if t["kind"] == G.KIND_SIMPLE]
    assert len(simple) == 2
    for j, t in enumerate(simple):
        agent, seq = replay(t, dq_agent, simple_maze_env)
        p = f"dq{j}."
        out[p + "obs"] = np.array(seq["obs"]); out[p + "next"] = np.array(seq["next"])
        out[p + "act"] = np.array(seq["act"]); out[p + "rew"] = np.array(seq["rew"])
        out[p + "term"] = np.array(seq["term"]); out[p + "coin"] = np.array(seq["coin"])
        out[p + "best"] = np.array(seq["best"])
        for name, table in (("a", agent.q_a_values), ("b", agent.q_b_values)):
            keys = sorted(table)
            out[p + name + ".keys"] = np.array(keys)
            out[p + name + ".values"] = np.stack([table[k] for k in keys])
        out[p + "steps_done"] = np.int64(agent.steps_done)
        print("trace", j, "updates", len(seq["act"]), "terminated", int(np.sum(seq["term"])),
              "non-zero rows A/B", int(out[p + "a.values"].any(1).sum()),
              int(out[p + "b.values"].any(1).sum()), "steps_done", agent.steps_done)
    np.savez_compressed(os.path.join(HERE, "dq_agent.npz"), **out)


if __name__ == "__main__":
    main(*sys.argv[1:])
