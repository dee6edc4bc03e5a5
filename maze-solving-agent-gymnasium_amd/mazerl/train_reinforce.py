"""REINFORCE on variable-size euclidean Enrich mazes: the reference's training_examples/
test_reinforce.py (SimpleEnrichVariableMazeEnv up to 35x35, lr 1e-3, gamma 0.99, the 5 / 10-win
algorithm curriculum) over a population of instances on one GPU.

  python -m mazerl.train_reinforce --envs 4096 --steps 600

Every instance starts at the growth's first size (15: SimpleVariableMazeEnv.START_SHAPE, the
smallest euclidean maze that holds the 15x15 window) and grows by 4 per win (--growth START,MAX);
--growth none keeps fixed per-instance sizes from --dims. Prints one JSON line with the training
throughput and the win-rate on fresh mazes, sampled at temperature 2 (the reference's own test())
and greedy (argmax of the logits). With --archive C the run keeps the mazes it trains on in a
MazePool of C entries and the line gains both win rates on them, the reference's
ValueBasedTrainer.test(n, new=False), with the pool's fill.
"""
import argparse
import json

import torch

from .archive import add_pool_arguments, check_pool_arguments
from .trainers.episodic import episode_bound
from .trainers.reinforce_trainer import VectorReinforceTrainer
from .trainers.schedule import growth_sizes
from .trainers.vector_trainer import evaluate, evaluate_explored, make_env


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--growth", default="15,35",
                    help="START,MAX: +4 per win from START while <= MAX, and the max-shape stop "
                         "(simple_variable_maze_env.py:93-112, value_based_trainer.py:74-83); "
                         "'none': fixed sizes from --dims")
    ap.add_argument("--dims", default=None, help="odd range lo-hi or comma list (with --growth none; "
                                                 "also the evaluation sizes)")
    ap.add_argument("--toroidal", action="store_true")
    ap.add_argument("--algo", default="r-prim")
    ap.add_argument("--curriculum", default="global", choices=["none", "global", "per-instance"],
                    help="change_algorithm (value_based_trainer.py:132-136)")
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--update-rows", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--entropy-coef", type=float, default=0.01)
    ap.add_argument("--eval-mazes", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--candidates", type=int, default=1,
                    help="training mazes: each the easiest of C by McClendon difficulty")
    ap.add_argument("--no-bank", action="store_true",
                    help="build winners' new mazes inline instead of copying them from a maze bank")
    ap.add_argument("--resume", default=None, help="checkpoint to continue from")
    ap.add_argument("--save", default=None, help="checkpoint written after training")
    add_pool_arguments(ap)
    a = ap.parse_args(argv)
    check_pool_arguments(a)  # refused here, before any GPU call
    if a.dims is None and a.growth in ("none", ""):
        ap.error("--growth none needs --dims")
    return a


def main(argv=None):
    a = parse(argv)
    growth = None if a.growth in ("none", "") else tuple(int(x) for x in a.growth.split(","))
    if a.dims is None:
        dims = growth_sizes(*growth)
    elif "-" in a.dims:
        lo, hi = (int(x) for x in a.dims.split("-"))
        dims = list(range(lo, hi + 1, 2))
    else:
        dims = [int(x) for x in a.dims.split(",")]
    dev = torch.device("cuda", torch.cuda.current_device())
    env = make_env(a.envs, [growth[0]] if growth else dims, toroidal=a.toroidal, algorithm=a.algo,
                   seed=0x5EED0000, device=dev, done_list=False, reward64=True, window=False,
                   window_bits=True, candidates=a.candidates,
                   max_dim=max(growth[1] if growth else 0, max(dims)))
    tr = VectorReinforceTrainer(env, dev, lr=a.lr, gamma=a.gamma, update_rows=a.update_rows,
                                batch_size=a.batch, temperature=a.temperature,
                                entropy_coef=a.entropy_coef, seed=a.seed, bank=not a.no_bank,
                                curriculum=None if a.curriculum == "none" else a.curriculum,
                                growth=growth, algorithm=a.algo, bank_candidates=a.candidates,
                                archive=a.archive or None)
    if a.resume:
        from .checkpoint import load_checkpoint
        load_checkpoint(a.resume, tr)
    secs = tr.train(a.steps, log_every=100, log=lambda r: print(json.dumps(r), flush=True))
    if a.save:
        from .checkpoint import save_checkpoint
        save_checkpoint(a.save, tr)
    steps = tr.stopped_at or a.steps
    kw = dict(toroidal=a.toroidal, device=dev, eps=0.0)
    sampled, k = evaluate(tr.sampler(), a.eval_mazes, dims, a.algo, seed=0x7E570000, **kw)
    greedy, _ = evaluate(tr, a.eval_mazes, dims, a.algo, seed=0x7E570000, **kw)
    explored = {}
    if tr.archive is not None:
        pool = tr.archive
        n = min(a.explored_mazes or pool.capacity, int(pool.held))
        xkw = dict(eps=0.0, chunk=min(n, a.envs), seed=0x7E590000,
                   max_vector_steps=episode_bound(pool.pitch, pool.toroidal) + 1)
        xs, _ = evaluate_explored(tr.sampler(), pool, n, **xkw)
        xg, _ = evaluate_explored(tr, pool, n, **xkw)
        explored = {"win_rate_explored_sample": xs, "win_rate_explored_greedy": xg,
                    "explored_mazes": n, "archive": tr.summary()["archive"]}
    print(json.dumps({"config": "reinforce " + ("toroidal" if a.toroidal else "euclidean") +
                      (" variable" if growth else ""), "envs": a.envs, "growth": growth,
                      "dims": [dims[0], dims[-1]], "vector_steps": steps, "train_seconds": secs,
                      "train_env_steps_per_s": a.envs * steps / secs, "episodes": tr.episodes,
                      "wins": tr.wins, "updates": tr.updates, "rows_trained": tr.rows_trained,
                      "seed": a.seed, "acting": "f32 (select_action as the reference)",
                      "win_rate_sampled": sampled, "win_rate_greedy": greedy,
                      "stopped_at": tr.stopped_at,
                      "schedule": tr.schedule.summary() if tr.schedule is not None else None,
                      "eval_mazes": a.eval_mazes, "eval_steps": k, **explored}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
