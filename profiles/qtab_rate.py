#!/usr/bin/env python3
"""Tabular Q-learning rates at 9x9 r-prim, in one process:

  (a) the single-env drop-in path exactly as bench.py's cfg1 leg sets it up: TabularTrainer +
      QAgent on one SimpleMazeEnv (a kernel launch and a stream synchronisation per env step);
  (b) VectorTabularTrainer + VectorQAgent: 4,096 independent learners (one table each), and
      4,096 instances on one shared table. 5 warm-up and 2,000 timed vector steps between two
      device events; no host synchronisation inside the window.

Prints one JSON line: env steps/s of each case, the launches per vector step of (b), and the
ratio (b) / (a). (a) pays a launch and a sync per env step, (b) a handful of launches per 4,096
env steps: a ratio under 100 means a host synchronisation hides in the vectorised loop.

With --storage the script measures the table storages of (b) instead (no drop-in leg): for each
of --tables (independent, shared) it runs --repeats rounds, and in every round each named storage
once, in the order given (so `--storage dense hash` alternates them in one process), on
--size x --size r-prim mazes; hashed tables take --capacity slots and, with --grow-every, double
when half full. One JSON line: per case and storage the raw repeats (us per vector step, env
steps/s, and for hashed tables the final capacity, largest load and dropped updates), their
median, and the hashed / dense ratio of the medians where both ran. Examples:
  qtab_rate.py --storage dense hash --capacity 256               9x9, both storages, both cases
  qtab_rate.py --storage hash --tables independent --size 41 --capacity 4096

With --agent (and --storage) the learners are measured against each other in the same way: q is
VectorQAgent, double is VectorDoubleQAgent (two tables per state, one more launch per vector
step). In every round each storage runs each named agent once, in the order given; the JSON line
then holds one entry per "storage:agent" and the double / q ratio of the medians per storage.
  qtab_rate.py --agent q double --storage dense --tables independent
  qtab_rate.py --agent q double --storage hash --capacity 65536 --tables shared
"""
import argparse
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "maze-solving-agent-gymnasium_amd"))

HP = dict(learning_rate=1e-3, initial_epsilon=0.95, final_epsilon=0.05, epsilon_decay=9 * 9 // 2,
          discount_factor=0.7, eta=1e-2)


def dropin(episodes):
    from mazerl.agents.q_agent import QAgent
    from mazerl.envs import SimpleMazeEnv
    from mazerl.trainers.tabular import TabularTrainer
    random.seed(0xC0F1)
    np.random.seed(0xC0F1)
    env = SimpleMazeEnv((9, 9))
    trn = TabularTrainer(env, QAgent(env, **HP))
    wins, steps, secs = trn.train(episodes)
    env.close()
    return {"episodes": episodes, "env_steps": steps, "wins": wins, "seconds": round(secs, 3),
            "env_steps_per_s": steps / secs}


def vectorised(n, tables, warmup, steps, size=9, storage="dense", capacity=None, grow_every=0,
               agent="q"):
    import torch
    import mazerl
    from mazerl.agents import VectorDoubleQAgent, VectorQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env = mazerl.VectorMazeEnv(n, size, enrich=False, reward64=True, done_list=False)
    hp = dict(HP, epsilon_decay=size * size // 2)
    double = agent == "double"
    cls = VectorDoubleQAgent if double else VectorQAgent
    if double:  # 4,096 dense double tables at 9x9 are 8.6 GB, just above the default limit
        hp["max_bytes"] = 16 << 30
    if storage == "hash":
        agent = cls(env, tables=tables, storage="hash", capacity=capacity, **hp)
    else:
        agent = cls(env, tables=tables, **hp)
    trn = VectorTabularTrainer(env, agent, regen_won=True, grow_every=grow_every)
    for _ in range(warmup):
        trn.vector_step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        trn.vector_step()
    t1.record()
    t1.synchronize()
    secs = t0.elapsed_time(t1) * 1e-3
    out = {"instances": n, "tables": agent.num_tables, "vector_steps": steps,
           "seconds": round(secs, 4), "us_per_vector_step": secs / steps * 1e6,
           "env_steps_per_s": n * steps / secs, "launches_per_vector_step": trn.launches_per_step,
           "episodes": int(agent.episodes.sum()), "wins": int(agent.wins.sum())}
    if storage == "hash":
        out.update(storage="hash", capacity=agent.capacity, max_load=int(agent.load.max()),
                   overflow=int(agent.overflow.sum()),
                   table_bytes=agent.num_tables * agent.capacity * (68 if double else 36))
    env.close()
    return out


def storages(a):
    """--storage: the storages against each other, alternating, a.repeats rounds per case."""
    res = {"size": a.size, "instances": a.instances, "warmup": a.warmup, "steps": a.steps}
    cases = {"independent": None, "shared": 1}
    for case in (("independent", "shared") if a.tables == "both" else (a.tables,)):
        agents = a.agent or ["q"]
        name = (lambda st, ag: f"{st}:{ag}") if a.agent else (lambda st, ag: st)
        runs = {name(st, ag): [] for st in a.storage for ag in agents}
        for _ in range(a.repeats):
            for st in a.storage:
                grow = a.grow_every if st == "hash" else 0
                for ag in agents:
                    runs[name(st, ag)].append(
                        vectorised(a.instances, cases[case], a.warmup, a.steps, a.size, st,
                                   a.capacity if st == "hash" else None, grow, ag))
        out = {st: {"us_per_vector_step": [round(r["us_per_vector_step"], 2) for r in rs],
                    "median_us": float(np.median([r["us_per_vector_step"] for r in rs])),
                    "env_steps_per_s": [round(r["env_steps_per_s"]) for r in rs],
                    "launches_per_vector_step": rs[0]["launches_per_vector_step"],
                    "wins": [r["wins"] for r in rs], "episodes": [r["episodes"] for r in rs]}
               for st, rs in runs.items()}
        for key, rs in runs.items():
            if key.startswith("hash"):
                for k in ("capacity", "max_load", "overflow", "table_bytes"):
                    out[key][k] = [r[k] for r in rs]
        if not a.agent and len(runs) == 2:
            out["hash_over_dense_time"] = out["hash"]["median_us"] / out["dense"]["median_us"]
        if a.agent and set(a.agent) == {"q", "double"}:
            out["double_over_q_time"] = {st: out[f"{st}:double"]["median_us"] /
                                         out[f"{st}:q"]["median_us"] for st in a.storage}
        res[case] = out
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=350)
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--storage", nargs="+", choices=("dense", "hash"), default=None,
                    help="measure these table storages against each other (no drop-in leg)")
    ap.add_argument("--agent", nargs="+", choices=("q", "double"), default=None,
                    help="with --storage: measure these learners against each other")
    ap.add_argument("--tables", choices=("independent", "shared", "both"), default="both")
    ap.add_argument("--size", type=int, default=9, help="maze size of the --storage runs")
    ap.add_argument("--capacity", type=int, default=256, help="slots of a hashed table")
    ap.add_argument("--grow-every", type=int, default=0,
                    help="hashed: check the load every this many vector steps and double")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.agent and not a.storage:
        ap.error("--agent needs --storage")
    if a.storage:
        return storages(a)
    res = {"dropin_single_env": dropin(a.episodes),
           "vector_independent": vectorised(a.instances, None, a.warmup, a.steps),
           "vector_shared_one_table": vectorised(a.instances, 1, a.warmup, a.steps)}
    base = res["dropin_single_env"]["env_steps_per_s"]
    for k in ("vector_independent", "vector_shared_one_table"):
        res[k]["times_dropin"] = res[k]["env_steps_per_s"] / base
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
