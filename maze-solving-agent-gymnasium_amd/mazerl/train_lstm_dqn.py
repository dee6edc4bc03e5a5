"""The recurrent DQN (the reference's agents/lstm_dqn_agent.py: LSTMCell(6, 32) + Linear(32, 4)
over obs6, whole episodes as the unit of replay) over a population of plain mazes on one GPU.

  python -m mazerl.train_lstm_dqn --envs 4096 --dim 9 --steps 2000

The reference has no trainer for this agent; the semantics are VectorRecurrentDQNTrainer's
(trainers/drqn_trainer.py, its stated departures). Prints one JSON line with the training
throughput and the greedy win-rate on fresh mazes before and after training, under the same
evaluation seed.

  python -m mazerl.train_lstm_dqn --envs 4096 --dim 9 --learners 8 --seeds 0,1,2,3,4,5,6,7
  python -m mazerl.train_lstm_dqn --learners 4 --sweep lr=1e-3,3e-4,1e-4,3e-5 --sweep gamma=0.99

--window T trains on one window of T steps per sampled episode instead of the whole episode,
--burn-in K (a multiple of T) unrolls K steps before it without loss or gradient, --initial-state
stored | zero starts from the recurrent state recorded while acting or from zero (departures 7-9).

--learners P trains P independent learners in one run (trainers/drqn_population.py), each on
envs / P instances; --seeds and --sweep NAME=v1,v2,... (repeatable; NAME one of lr, gamma,
eps-start, eps-final, eps-decay, target-update, seed, burn-in, initial-state, priority-alpha,
priority-beta, priority-eta, priority-eps, double-q, n-step; P values or one) set them apart. The final line then
reports every learner's trained greedy win-rate on the same mazes, their mean and spread, and every
learner's window and priority settings.

  python -m mazerl.train_lstm_dqn --dim 41 --learners 16 --window 40 --burn-in 40 \\
      --sweep initial-state=stored,stored,...,zero,zero --seeds 0,1,...

With --learners, --window T is shared by the population (it fixes the layouts and cannot be
swept); --burn-in and --initial-state are per learner.

--priority-alpha A beside --window samples the windows in proportion to (their TD error)^A over
the whole memory, with importance weights of exponent --priority-beta B (or B0,B1,N: linear over N
updates); --priority-eta H and --priority-eps X shape a window's priority (departures 10-12). A = 0
is uniform over the memory's windows.

  python -m mazerl.train_lstm_dqn --dim 41 --window 40 --burn-in 40 --priority-alpha 0.9

With --learners the exponent is per learner and comes through --sweep priority-alpha=A or
=A1,A2,... (a value may be none: that learner keeps the uniform-per-episode window sampler);
--priority-beta, --priority-eta and --priority-eps then apply to every prioritized learner unless
swept too (a schedule inside a sweep is written B0:B1:N). The final line lists every learner's
settings beside its greedy win rate (by_learner).

  python -m mazerl.train_lstm_dqn --dim 41 --learners 12 --window 40 --burn-in 40 \\
      --sweep priority-alpha=none,none,none,none,0,0,0,0,0.9,0.9,0.9,0.9 \\
      --sweep priority-beta=0.6,0.6,0.6,0.6,0,0,0,0,0.6,0.6,0.6,0.6 --seeds 0,1,2,3,0,1,2,3,0,1,2,3

--double-q bootstraps from the target net's value of the source net's own greedy action (double
Q-learning, departure 13); --n-step N forms N-step returns, cut at the end of an episode or of a
window (departure 14). Both work with whole episodes and with windows, uniform or prioritized; with
--learners they apply to every learner unless --sweep double-q=0,1,... or --sweep n-step=1,3,5,...
sets them per learner. The final line lists both per learner.

  python -m mazerl.train_lstm_dqn --dim 41 --window 40 --burn-in 40 --double-q --n-step 5

--archive C keeps the mazes the run trains on in a MazePool of C entries (with --learners: one
pool of C entries per learner, all filled by one launch per vector step) and the final line gains
the greedy win rate on its oldest --explored-mazes entries, the reference's test(n, new=False)
(per learner, with the spread), and the pool's fill.
"""
import argparse
import json

import torch

from .archive import add_pool_arguments, check_pool_arguments
from .trainers.drqn_trainer import (VectorRecurrentDQNTrainer, check_priority, check_returns,
                                    check_window, evaluate_plain)
from .trainers.episodic import episode_bound
from .trainers.vector_trainer import evaluate_explored
from .vector_env import VectorMazeEnv


def state(v):
    """An --initial-state value."""
    if v not in ("stored", "zero"):
        raise ValueError(v)
    return v


def alpha(v):
    """A priority-alpha value of a sweep: a number, or none (that learner is not prioritized)."""
    return None if v.strip().lower() == "none" else float(v)


def flag(v):
    """A double-q value of a sweep: 0 or 1."""
    if v.strip() not in ("0", "1"):
        raise ValueError(v)
    return v.strip() == "1"


def beta(v):
    """A --priority-beta value: B, or B0,B1,N (linear from B0 to B1 over N updates; inside a
    --sweep, whose values the commas separate, B0:B1:N)."""
    parts = v.replace(":", ",").split(",")
    if len(parts) == 1:
        return float(v)
    if len(parts) != 3:
        raise ValueError(v)
    return (float(parts[0]), float(parts[1]), int(parts[2]))


# --sweep names -> (the constructor's argument, the value type). --window is shared by the
# population (it fixes the layouts) and stays out.
SWEEPABLE = {"lr": ("lr", float), "gamma": ("discount_factor", float),
             "eps-start": ("starting_epsilon", float), "eps-final": ("final_epsilon", float),
             "eps-decay": ("epsilon_decay", float), "target-update": ("target_update_frequency", int),
             "seed": ("seed", int), "burn-in": ("burn_in", int), "initial-state": ("initial_state", state),
             "priority-alpha": ("priority_alpha", alpha), "priority-beta": ("priority_beta", beta),
             "priority-eta": ("priority_eta", float), "priority-eps": ("priority_eps", float),
             "double-q": ("double_q", flag), "n-step": ("n_step", int)}


def parse_sweeps(sweeps, seeds, P):
    """--sweep NAME=v1,v2,... and --seeds s1,... -> {constructor argument: list of P values}.
    Each list has P values or one (then every learner gets it)."""
    out = {}
    items = list(sweeps or [])
    if seeds is not None:
        items.append("seed=" + seeds)
    for item in items:
        name, eq, vals = item.partition("=")
        name = name.strip().replace("_", "-")
        if not eq or name not in SWEEPABLE:
            raise ValueError(f"--sweep {item!r}: NAME=v1,v2,... with NAME one of "
                             f"{', '.join(SWEEPABLE)}")
        arg, kind = SWEEPABLE[name]
        if arg in out:
            raise ValueError(f"--sweep {name} given twice")
        try:
            vs = [kind(v) for v in vals.split(",")]
        except ValueError:
            raise ValueError(f"--sweep {item!r}: values must be {kind.__name__}s") from None
        if len(vs) == 1:
            vs = vs * P
        if len(vs) != P:
            raise ValueError(f"--sweep {name}: {len(vs)} values for {P} learners")
        out[arg] = vs
    return out


def spread(rates):
    """Mean, sample standard deviation (0 for one value), min and max of the learners' rates."""
    n = len(rates)
    mean = sum(rates) / n
    sd = (sum((r - mean) ** 2 for r in rates) / (n - 1)) ** 0.5 if n > 1 else 0.0
    return {"mean": mean, "std": sd, "min": min(rates), "max": max(rates)}


def parse_args(argv=None):
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
    ap.add_argument("--window", type=int, default=None, metavar="T",
                    help="train on replay windows of T steps (default: whole episodes)")
    ap.add_argument("--burn-in", type=int, default=0, metavar="K",
                    help="burn-in steps before a window, a multiple of --window")
    ap.add_argument("--initial-state", choices=("stored", "zero"), default="stored",
                    help="a window's starting state: the snapshot recorded while acting, or zero")
    ap.add_argument("--priority-alpha", type=float, default=None, metavar="A",
                    help="prioritized replay windows with exponent A (needs --window; 0: uniform "
                         "over the memory's windows)")
    ap.add_argument("--priority-beta", type=beta, default=0.6, metavar="B | B0,B1,N",
                    help="importance-weight exponent, or a linear schedule over N updates")
    ap.add_argument("--priority-eta", type=float, default=0.9, metavar="H",
                    help="a window's priority: H max + (1 - H) mean of its |TD errors|")
    ap.add_argument("--priority-eps", type=float, default=1e-3, metavar="X")
    ap.add_argument("--double-q", action="store_true",
                    help="bootstrap from the target net's value of the source net's greedy action")
    ap.add_argument("--n-step", type=int, default=1, metavar="N",
                    help="N-step returns, cut at the end of an episode or a window")
    ap.add_argument("--learners", type=int, default=None,
                    help="P independent learners in one run, each on envs / P instances")
    ap.add_argument("--sweep", action="append", default=None, metavar="NAME=v1,v2,...",
                    help="per-learner values (P or one) of lr, gamma, eps-start, eps-final, "
                         "eps-decay, target-update, seed, burn-in, initial-state, "
                         "priority-alpha / -beta / -eta / -eps, double-q or n-step; repeatable")
    ap.add_argument("--seeds", default=None, metavar="s1,s2,...", help="--sweep seed=...")
    add_pool_arguments(ap, "the run (with --learners: each learner)")
    a = ap.parse_args(argv)
    check_pool_arguments(a)  # refused here, before any GPU call
    try:
        check_window(a.window, a.burn_in, a.initial_state)
        check_priority(a.window, a.priority_alpha, a.priority_beta, a.priority_eta, a.priority_eps)
        check_returns(a.double_q, a.n_step)
    except ValueError as e:
        ap.error(str(e))
    given = [f for f in ("--priority-beta", "--priority-eta", "--priority-eps")
             if ap.get_default(f[2:].replace("-", "_")) != getattr(a, f[2:].replace("-", "_"))]
    if a.learners is None and a.priority_alpha is None and given:
        ap.error(f"{', '.join(given)} need --priority-alpha")
    if a.learners is not None and a.priority_alpha is not None:
        ap.error("--priority-alpha is the single trainer's flag; with --learners the exponent is "
                 "per learner: --sweep priority-alpha=A (or A1,A2,..., a value may be none)")
    if a.learners is None:
        if a.sweep or a.seeds:
            ap.error("--sweep / --seeds need --learners")
        a.per_learner = None
        return a
    if a.learners < 1 or a.envs % a.learners:
        ap.error("--envs must be a multiple of --learners >= 1")
    try:
        a.per_learner = parse_sweeps(a.sweep, a.seeds, a.learners)
        for K in a.per_learner.get("burn_in", ()):  # every learner's K_p against the shared T
            check_window(a.window, K, a.initial_state)
        per = a.per_learner
        for N in per.get("n_step", ()):
            check_returns(False, N)
        alphas = per.get("priority_alpha", [None] * a.learners)
        for p, al in enumerate(alphas):  # every learner's priority settings against the shared T
            check_priority(a.window, al, *(per[k][p] if k in per else getattr(a, k) for k in
                                           ("priority_beta", "priority_eta", "priority_eps")))
    except ValueError as e:
        ap.error(str(e))
    swept = ["--sweep " + k.replace("_", "-") for k in per
             if k in ("priority_beta", "priority_eta", "priority_eps")]
    if all(al is None for al in alphas) and (given or swept):
        ap.error(f"{', '.join(given + swept)} need --sweep priority-alpha=... with a value that "
                 "is not none")
    return a


def by_learner(tr, rates):
    """The report of a population with prioritized learners or learners off the target's defaults:
    the per-learner settings and, learner by learner, its seed and settings beside its greedy win
    rate. Empty without either."""
    pr, rt = tr._priority_settings(), tr._returns_settings()
    if pr is None and rt is None:
        return {}
    rows = [{"learner": p, "seed": tr.seed[p], **{"priority_" + k: pr[k][p] for k in pr or ()},
             "double_q": tr.double_q[p], "n_step": tr.n_step[p], "win_rate_greedy": rates[p]}
            for p in range(tr.P)]
    return {**({} if pr is None else {"priority": pr}), "by_learner": rows}


def main_population(a):
    from .trainers.drqn_population import VectorRecurrentDQNPopulation
    dev = torch.device("cuda", torch.cuda.current_device())
    env = VectorMazeEnv(a.envs, a.dim, toroidal=a.toroidal, enrich=False, device=dev,
                        algorithm=a.algo, seed=0x5EED0000, pos=False, done_list=False)
    kw = dict(lr=a.lr, starting_epsilon=a.eps_start, final_epsilon=a.eps_final,
              epsilon_decay=a.eps_decay, discount_factor=a.gamma,
              target_update_frequency=a.target_update, seed=a.seed, burn_in=a.burn_in,
              initial_state=a.initial_state, priority_beta=a.priority_beta,
              priority_eta=a.priority_eta, priority_eps=a.priority_eps, double_q=a.double_q,
              n_step=a.n_step)
    kw.update(a.per_learner)
    tr = VectorRecurrentDQNPopulation(
        env, dev, learners=a.learners, batch_size=a.batch, memory_size=a.memory,
        explore_actions=a.explore_actions, train_every=a.train_every, bank=not a.no_bank,
        algorithm=a.algo, window=a.window, archive=a.archive or None, **kw)
    if a.resume:
        from .checkpoint import load_checkpoint
        load_checkpoint(a.resume, tr)
    ev = dict(algorithm=a.algo, seed=0x7E570000, toroidal=a.toroidal)
    before = tr.evaluate_all(a.eval_mazes, a.dim, **ev)
    secs = tr.train(a.steps, log_every=500, log=lambda r: print(json.dumps(r), flush=True))
    if a.save:
        from .checkpoint import save_checkpoint
        save_checkpoint(a.save, tr)
    after = tr.evaluate_all(a.eval_mazes, a.dim, **ev)
    explored = {}
    if tr.archive is not None:  # every learner on its own oldest n mazes, n the same for all
        n = min(a.explored_mazes or tr.archive.capacity, min(tr.archive.held.tolist()))
        rates = tr.evaluate_explored_all(n)
        explored = {"win_rate_explored_greedy": rates,
                    "win_rate_explored_greedy_spread": spread(rates), "explored_mazes": n,
                    "archive": tr.summary()["archive"]}
    print(json.dumps({"config": "lstm-dqn population " + ("toroidal" if a.toroidal else "euclidean"),
                      "envs": a.envs, "learners": a.learners, "dim": a.dim,
                      "vector_steps": a.steps, "train_seconds": secs,
                      "train_env_steps_per_s": a.envs * a.steps / secs, "episodes": tr.episodes,
                      "wins": tr.wins, "updates": tr.updates, "batch_episodes": a.batch,
                      "per_learner": {k: v for k, v in a.per_learner.items()},
                      "window": tr._window_settings(),  # T and every learner's K_p, S_p
                      "double_q": tr.double_q, "n_step": tr.n_step,
                      **by_learner(tr, after),
                      "replay_bytes": tr.memory_bytes()["replay"],
                      "win_rate_greedy_untrained": before, "win_rate_greedy": after,
                      "win_rate_greedy_spread": spread(after), "eval_mazes": a.eval_mazes,
                      **explored}),
          flush=True)
    env.close()


def main(argv=None):
    a = parse_args(argv)
    if a.learners is not None:
        return main_population(a)
    dev = torch.device("cuda", torch.cuda.current_device())
    env = VectorMazeEnv(a.envs, a.dim, toroidal=a.toroidal, enrich=False, device=dev,
                        algorithm=a.algo, seed=0x5EED0000, pos=False, done_list=False)
    tr = VectorRecurrentDQNTrainer(
        env, dev, lr=a.lr, starting_epsilon=a.eps_start, final_epsilon=a.eps_final,
        epsilon_decay=a.eps_decay, discount_factor=a.gamma, batch_size=a.batch,
        memory_size=a.memory, target_update_frequency=a.target_update,
        explore_actions=a.explore_actions, train_every=a.train_every, seed=a.seed,
        bank=not a.no_bank, algorithm=a.algo, window=a.window, burn_in=a.burn_in,
        initial_state=a.initial_state, archive=a.archive or None,
        priority_alpha=a.priority_alpha, priority_beta=a.priority_beta,
        priority_eta=a.priority_eta, priority_eps=a.priority_eps, double_q=a.double_q,
        n_step=a.n_step)
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
    explored = {}
    if tr.archive is not None:
        pool = tr.archive
        n = min(a.explored_mazes or pool.capacity, int(pool.held))
        xg, _ = evaluate_explored(tr.evaluator(), pool, n, chunk=min(n, a.envs), seed=0x7E590000,
                                  max_vector_steps=episode_bound(pool.pitch, pool.toroidal) + 1)
        explored = {"win_rate_explored_greedy": xg, "explored_mazes": n,
                    "archive": tr.summary()["archive"]}
    print(json.dumps({"config": "lstm-dqn " + ("toroidal" if a.toroidal else "euclidean"),
                      "envs": a.envs, "dim": a.dim, "vector_steps": a.steps, "train_seconds": secs,
                      "train_env_steps_per_s": a.envs * a.steps / secs, "episodes": tr.episodes,
                      "wins": tr.wins, "updates": tr.updates, "batch_episodes": a.batch,
                      "seed": a.seed, "window": a.window, "burn_in": a.burn_in,
                      "initial_state": a.initial_state if a.window else None,
                      "double_q": tr.double_q, "n_step": tr.n_step,
                      **({} if a.priority_alpha is None else {"priority": tr._priority_settings()}),
                      "win_rate_greedy_untrained": before,
                      "win_rate_greedy": after, "eval_mazes": a.eval_mazes, "eval_steps": k,
                      **explored}),
          flush=True)
    env.close()


if __name__ == "__main__":
    main()
