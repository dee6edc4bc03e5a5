"""The recurrent DQN (the reference's agents/lstm_dqn_agent.py: LSTMCell(6, 32) + Linear(32, 4)
over obs6, whole episodes as the unit of replay) over a population of plain mazes on one GPU.

  python -m mazerl.train_lstm_dqn --envs 4096 --dim 9 --steps 2000

The reference has no trainer for this agent; the semantics are VectorRecurrentDQNTrainer's
(trainers/drqn_trainer.py, six stated departures). Prints one JSON line with the training
throughput and the greedy win-rate on fresh mazes before and after training, under the same
evaluation seed.
"""
import argparse
import json

import torch

from .trainers.drqn_trainer import VectorRecurrentDQNTrainer, evaluate_plain
from .vector_env import VectorMazeEnv


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=9)
    ap.add_argument("--toroidal", action="store_true")
    ap.add_argument("--algo", default="r-prim")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--eps-start", type=float, default=0.9)
    ap.add_argument("--eps-final", type=float, default=0.05)
    ap.add_argument("--eps-decay", type=float, default=1000.0)
    ap.add_argument("--batch", type=int, default=32, help="episodes per update")
    ap.add_argument("--memory", type=int, default=20000, help="replay capacity in episodes")
    ap.add_argument("--target-update", type=int, default=10, help="updates between target syncs")
    ap.add_argument("--explore-actions", type=int, default=4,
                    help="2 reproduces the reference's randrange(2)")
    ap.add_argument("--train-every", type=int, default=1)
    ap.add_argument("--eval-mazes", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-bank", action="store_true")
    ap.add_argument("--resume", default=None, help="checkpoint to continue from")
    ap.add_argument("--save", default=None, help="checkpoint written after training")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    env = VectorMazeEnv(a.envs, a.dim, toroidal=a.toroidal, enrich=False, device=dev,
                        algorithm=a.algo, seed=0x5EED0000, pos=False, done_list=False)
    tr = VectorRecurrentDQNTrainer(
        env, dev, lr=a.lr, starting_epsilon=a.eps_start, final_epsilon=a.eps_final,
        epsilon_decay=a.eps_decay, discount_factor=a.gamma, batch_size=a.batch,
        memory_size=a.memory, target_update_frequency=a.target_update,
        explore_actions=a.explore_actions, train_every=a.train_every, seed=a.seed,
        bank=not a.no_bank, algorithm=a.algo)
    if a.resume:
        from .checkpoint import load_checkpoint
        load_checkpoint(a.resume, tr)
    kw = dict(algorithm=a.algo, seed=0x7E570000, toroidal=a.toroidal, device=dev)
    before, _ = evaluate_plain(tr.evaluator(), a.eval_mazes, a.dim, **kw)
    secs = tr.train(a.steps, log_every=500, log=lambda r: print(json.dumps(r), flush=True))
    if a.save:
        from .checkpoint import save_checkpoint
        save_checkpoint(a.save, tr)
    after, k = evaluate_plain(tr.evaluator(), a.eval_mazes, a.dim, **kw)
    print(json.dumps({"config": "lstm-dqn " + ("toroidal" if a.toroidal else "euclidean"),
                      "envs": a.envs, "dim": a.dim, "vector_steps": a.steps, "train_seconds": secs,
                      "train_env_steps_per_s": a.envs * a.steps / secs, "episodes": tr.episodes,
                      "wins": tr.wins, "updates": tr.updates, "batch_episodes": a.batch,
                      "seed": a.seed, "win_rate_greedy_untrained": before,
                      "win_rate_greedy": after, "eval_mazes": a.eval_mazes, "eval_steps": k}),
          flush=True)
    env.close()


if __name__ == "__main__":
    main()
