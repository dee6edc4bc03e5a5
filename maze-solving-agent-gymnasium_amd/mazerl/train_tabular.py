"""Tabular Q-learning / double Q-learning populations with the reference's whole protocol: its
training_examples' test_q.py / test_dq.py (constant size), test_q_variable_maze.py /
test_dq_variable_maze.py (SimpleVariableMazeEnv: +4 per win up to max_shape, the max-shape stop)
and test_q_toroid.py / test_q_variable_toroid.py, over a population of instances on one GPU.

  python -m mazerl.train_tabular --agent q --growth 9 17 --envs 64 --steps 4000

Every instance is one of the reference's runs: its own env, its own table (--tables T: instance i
learns on table i % T), its own list of explored mazes (--archive-slots entries each, the newest
kept). Prints one JSON line: the training throughput and the three win rates of the reference's
tables — "explored" (test(n, new=False): every maze the instance trained on, replayed through the
archive), "current" (the mazes the instances hold at the end) and "new" (freshly generated mazes,
under --growth each of the size its instance reached) — with the archive's `dropped` count, the
growth schedule's summary and the README row the configuration corresponds to.
"""
import argparse
import json

ROWS = {(False, False): "labirinti di dimensione costante (r-prim)",
        (True, False): "labirinti di dimensione variabile (r-prim)",
        (False, True): "labirinti toroidali di dimensione costante",
        (True, True): "labirinti toroidali di dimensione variabile"}


def parse(argv=None):
    """The arguments, checked: every refusal is raised here, before any GPU call."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", default="q", choices=["q", "dq"],
                    help="QAgent (agents/q_agent.py) or DQAgent (agents/dq_agent.py)")
    ap.add_argument("--storage", default="dense", choices=["dense", "hash"])
    ap.add_argument("--capacity", type=int, default=None, help="slots per hashed table (a power of two)")
    ap.add_argument("--grow-every", type=int, default=0,
                    help="hashed tables: double the capacity when half full, checked every so many steps")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--tables", type=int, default=None, help="instance i learns on table i %% T "
                                                             "(default: one table per instance)")
    ap.add_argument("--dim", type=int, default=None, help="constant maze size (default 9)")
    ap.add_argument("--growth", type=int, nargs=2, default=None, metavar=("START", "MAX"),
                    help="+4 per win from START while <= MAX, and the max-shape stop "
                         "(simple_variable_maze_env.py:93-112, off_policy_trainer.py:60-75)")
    ap.add_argument("--toroidal", action="store_true")
    ap.add_argument("--algo", default="r-prim", choices=["r-prim", "dfs", "prim&kill"])
    ap.add_argument("--steps", type=int, default=4000, help="vector steps")
    ap.add_argument("--archive-slots", type=int, default=16)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--gamma", type=float, default=0.7)
    ap.add_argument("--eta", type=float, default=0.01)
    ap.add_argument("--eps-decay", type=float, default=None,
                    help="default: max size^2 // 2, as the reference's scripts")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--resume", default=None, help="checkpoint to continue from")
    ap.add_argument("--save", default=None, help="checkpoint written after training")
    a = ap.parse_args(argv)
    if a.growth is not None and a.dim is not None:
        raise ValueError("--growth START MAX and --dim exclude each other")
    sizes = list(a.growth) if a.growth is not None else [9 if a.dim is None else a.dim]
    for n in sizes:
        if n % 2 == 0 or n < 5 or n > 127:
            raise ValueError(f"maze size {n}: odd, in [5, 127]")
    if a.growth is not None and a.growth[0] > a.growth[1]:
        raise ValueError(f"--growth {a.growth[0]} {a.growth[1]}: START <= MAX")
    if a.storage == "hash":
        if a.capacity is None:
            raise ValueError("--storage hash needs --capacity")
        if a.capacity < 16 or a.capacity > 1 << 30 or a.capacity & (a.capacity - 1):
            raise ValueError(f"--capacity {a.capacity}: a power of two in [16, 2^30]")
    elif a.capacity is not None or a.grow_every:
        raise ValueError("--capacity / --grow-every belong to --storage hash")
    if a.grow_every < 0:
        raise ValueError("--grow-every must be >= 0")
    for name in ("envs", "steps", "archive_slots"):
        if getattr(a, name) < 1:
            raise ValueError(f"--{name.replace('_', '-')} must be >= 1")
    if a.tables is not None and not 1 <= a.tables <= a.envs:
        raise ValueError(f"--tables {a.tables}: in [1, --envs]")
    a.start, a.max_dim = sizes[0], sizes[-1]
    if a.eps_decay is None:
        a.eps_decay = float(a.max_dim * a.max_dim // 2)
    return a


def main(argv=None):
    a = parse(argv)
    import torch

    from .agents.vector_dq import VectorDoubleQAgent
    from .agents.vector_q import VectorQAgent
    from .trainers.vector_tabular import VectorTabularTrainer
    from .vector_env import VectorMazeEnv
    dev = torch.device("cuda", torch.cuda.current_device())
    env = VectorMazeEnv(a.envs, a.start, toroidal=a.toroidal, enrich=False, device=dev,
                        max_dim=a.max_dim, algorithm=a.algo, reward64=True, done_list=False)
    cls = VectorQAgent if a.agent == "q" else VectorDoubleQAgent
    agent = cls(env, tables=a.tables, learning_rate=a.lr, initial_epsilon=0.95,
                epsilon_decay=a.eps_decay, final_epsilon=0.05, discount_factor=a.gamma, eta=a.eta,
                seed=a.seed, storage=a.storage, capacity=a.capacity)
    tr = VectorTabularTrainer(env, agent, regen_won=True, grow_every=a.grow_every,
                              archive=a.archive_slots,
                              growth=None if a.growth is None else tuple(a.growth))
    if a.resume:
        from .checkpoint import load_checkpoint
        load_checkpoint(a.resume, tr)
    before = tr.vector_steps
    secs = tr.train(a.steps)
    if a.save:
        from .checkpoint import save_checkpoint
        save_checkpoint(a.save, tr)
    steps = tr.vector_steps - before
    _, played, explored = tr.evaluate_explored()
    _, current = tr.evaluate(new=False)
    summary = tr.summary()  # (before new=True replaces the training mazes)
    _, new = tr.evaluate(new=True, algorithm=a.algo)
    print(json.dumps({
        "config": ("double Q-learning" if a.agent == "dq" else "Q-learning") + ", " +
                  ("toroidal" if a.toroidal else "euclidean") +
                  (" variable" if a.growth else " constant"),
        "readme_row": ("Double Q-learning" if a.agent == "dq" else "Q-learning") + " — " +
                      ROWS[(a.growth is not None, a.toroidal)],
        "envs": a.envs, "tables": agent.num_tables, "storage": a.storage,
        "capacity": getattr(agent, "capacity", None), "growth": a.growth, "dim": a.start,
        "max_dim": a.max_dim, "algorithm": a.algo, "seed": a.seed, "vector_steps": steps,
        "train_seconds": secs, "train_env_steps_per_s": a.envs * steps / secs if secs else None,
        "episodes": int(agent.episodes.sum()), "wins": int(agent.wins.sum()),
        "win_rate_explored": explored, "explored_episodes": int(played.sum()),
        "win_rate_current": current, "win_rate_new": new,
        "new_maze_sizes": "the size each instance reached" if a.growth else a.start,
        "archive_slots": a.archive_slots, "dropped": summary["archive"]["dropped"],
        "stopped_at": tr.stopped_at, "schedule": summary["schedule"],
        "timing": "one wall-clock reading of train(), not a benchmark"}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
