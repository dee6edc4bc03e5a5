"""Timings for DESIGN §6za (the per-learner explored-maze pools), one process, JSON lines on stdout.

  python profiles/pools_rate.py kernel    # mz_archive_push_pools alone, HIP events
  python profiles/pools_rate.py trainers  # the vector step with and without archive=

kernel: B = 4,096 instances at 9x9 (plain) and 81x81 (Enrich), flags at ~1 % and 100 %, G in
{1, 8, 64}; per case WINDOWS windows of CALLS launches between two HIP events after a warm-up
window, the counters zeroed before each window so that every launch writes its entries; median
(min-max) microseconds per launch. G = 1 is timed against mz_archive_push_pool on the same flags,
the two alternating window by window, the pair twice ("run" 0 and 1). G launches of
mz_archive_push_pool on G envs of B / G instances with their own flag arrays are timed against
the one segmented launch.
trainers: two trainers with the same seeds, one with archive=, windows of STEPS vector steps
alternating between them (host clock around train(), which ends in a synchronise); median
(min-max) microseconds per vector step.
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, "maze-solving-agent-gymnasium_amd")

DEV = "cuda"
WINDOWS, CALLS, STEPS = 7, 50, 100


def emit(**kw):
    print(json.dumps(kw), flush=True)


def stat(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
            "max": round(max(xs), 2), "n": len(xs)}


def window(fn, calls, before=None):
    """Microseconds per call of `calls` back-to-back fn() between two HIP events."""
    if before is not None:
        before()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def alternate(cases, calls=CALLS, windows=WINDOWS):
    """cases: name -> (fn, before). One warm-up window each, then `windows` rounds in turn."""
    out = {k: [] for k in cases}
    for r in range(windows + 1):
        for k, (fn, before) in cases.items():
            us = window(fn, calls, before)
            if r:
                out[k].append(us)
    return {k: stat(v) for k, v in out.items()}


def kernel():
    import mazerl
    from mazerl.archive import MazePool, MazePoolSet
    B = 4096
    for dim, enrich in ((9, False), (81, True)):
        env = mazerl.VectorMazeEnv(B, dim, enrich=enrich, device=DEV, pos=False, done_list=False,
                                   window=False, window_bits=False)
        g = torch.Generator().manual_seed(1)
        flagsets = {"1%": (torch.rand(B, generator=g) < 0.01).to(torch.uint8).to(DEV),
                    "100%": torch.ones(B, dtype=torch.uint8, device=DEV)}
        for fname, flags in flagsets.items():
            n = int(flags.sum())
            # G = 1 against the single-pool entry point, twice
            for run in (0, 1):
                s, p = MazePoolSet(env, 1, CALLS * n), MazePool(env, CALLS * n)
                res = alternate({
                    "push_pools_G1": (lambda: s.record(flags, 1), lambda: s._count2.zero_()),
                    "push_pool": (lambda: p.record(flags, 1), lambda: p._count2.zero_())})
                emit(what="G=1 vs push_pool", dim=dim, flags=fname, flagged=n, run=run, us=res)
                del s, p
            for G in (1, 8, 64):
                b = B // G
                per = [int(flags[k * b:(k + 1) * b].sum()) for k in range(G)]
                s = MazePoolSet(env, G, CALLS * max(max(per), 1))
                cases = {"push_pools": (lambda: s.record(flags, 1), lambda: s._count2.zero_())}
                small = []
                if G > 1:  # G launches of the single-pool push on G envs of b instances
                    small = [mazerl.VectorMazeEnv(b, dim, enrich=enrich, device=DEV, pos=False,
                                                  done_list=False, window=False, window_bits=False,
                                                  seed=0x5EED0000 + k * b) for k in range(G)]
                    pools = [MazePool(e, CALLS * max(per[k], 1)) for k, e in enumerate(small)]
                    parts = [flags[k * b:(k + 1) * b].clone() for k in range(G)]

                    def many():
                        for q, f in zip(pools, parts):
                            q.record(f, 1)

                    def zero():
                        for q in pools:
                            q._count2.zero_()
                    cases["G x push_pool"] = (many, zero)
                res = alternate(cases, calls=CALLS if G < 64 else 10)
                emit(what="segmented vs G launches", dim=dim, flags=fname, flagged=n, G=G, us=res)
                for e in small:
                    e.close()
        env.close()


def _pair(make, steps=STEPS, windows=5):
    """make(archive) -> trainer; alternating windows of `steps` vector steps."""
    t0, t1 = make(None), make(True)
    out = {"archive=None": [], "archive=C": []}
    for r in range(windows + 1):
        for k, t in (("archive=None", t0), ("archive=C", t1)):
            torch.cuda.synchronize()
            c = time.perf_counter()
            t.train(steps)
            us = (time.perf_counter() - c) * 1e6 / steps
            if r:
                out[k].append(us)
    fill = t1.summary()["archive"]
    same = t0.wins == t1.wins and t0.episodes == t1.episodes
    for t in (t0, t1):
        t.env.close()
    return {k: stat(v) for k, v in out.items()}, fill, same


def trainers():
    import mazerl
    from mazerl.trainers import VectorRecurrentDQNPopulation
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    from mazerl.trainers.ppo_trainer import VectorPPOTrainer
    from mazerl.trainers.reinforce_trainer import VectorReinforceTrainer
    from mazerl.trainers.vector_trainer import make_env
    B = 4096

    def plain():
        return mazerl.VectorMazeEnv(B, 9, enrich=False, device=DEV, pos=False, done_list=False)

    def drqn(a):
        return VectorRecurrentDQNTrainer(plain(), DEV, archive=150 * B if a else None)

    def pop(a):
        return VectorRecurrentDQNPopulation(plain(), DEV, learners=8, seed=list(range(8)),
                                            archive=150 * B // 8 if a else None)

    def ppo(a):
        dims = list(range(17, 80, 2))
        env = make_env(B, dims, toroidal=True, device=DEV, done_list=False, reward64=True,
                       window=False, window_bits=True, candidates=6)
        return VectorPPOTrainer(env, DEV, ppo_steps=2, pool_size=32768, bank_candidates=6,
                                archive=16 * B if a else None)

    def rf(a):
        env = make_env(B, [15], device=DEV, done_list=False, reward64=True, window=False,
                       window_bits=True, max_dim=35)
        return VectorReinforceTrainer(env, DEV, growth=(15, 35), curriculum="global",
                                      archive=16 * B if a else None)
    for name, make, steps in (("recurrent DQN 4096 x 9x9", drqn, 300),
                              ("recurrent DQN population 8 x 512 x 9x9", pop, 300),
                              ("PPO 4096 toroidal 17..79", ppo, 100),
                              ("REINFORCE 4096 growth 15..35", rf, 100)):
        us, fill, same = _pair(make, steps)
        emit(what="vector step", run=name, steps_per_window=steps, us_per_step=us, fill=fill,
             same_wins_and_episodes=same)


if __name__ == "__main__":
    {"kernel": kernel, "trainers": trainers}[sys.argv[1]]()
