"""Prioritized replay windows per learner in VectorRecurrentDQNPopulation: what one
population update costs with all learners prioritized beside all learners uniform and beside the
same number of single prioritized updates, and 6zb's training table as one population run per maze
size.

  exp_lstm_dqn_pop_prio_probe.py all [OUTDIR [KIND ...]]   every case below (or those of the KINDs
        update / train), each in a process of its own under its own time limit; stops at the first
        failure
  exp_lstm_dqn_pop_prio_probe.py update OUT    41x41 plain mazes, capacity 20,000, E = 32, (T, K) =
        (40, 40), stored state, P = 8 learners x 512 instances: one population update (sample,
        target and source forward, [mz_drqn_pop_prio_update,] BPTT + reduce, AdamW) with all
        learners uniform, with all prioritized (alpha 0.9, beta 0.6), uniform again, and 8 updates
        of one single prioritized trainer on 512 instances run one after the other; then the two
        samplers and the write-back alone. All three run the same number of vector steps first
  exp_lstm_dqn_pop_prio_probe.py train DIM OUT   python -m mazerl.train_lstm_dqn --learners 12
        --envs 12288 --steps 30000 --eps-decay 5000 --window 40 --burn-in 40: uniform, alpha 0 /
        beta 0 and alpha 0.9 / beta 0.6, each over seeds 0 to 3 (6zb's flags, 1,024 instances per
        learner)
HIP events in one process, 10 warm-up calls, then REPS windows per figure: median (min-max) in
microseconds. One JSON line per figure, appended to OUT (default directory:
profiles/lstm_dqn_pop_prio)."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "maze-solving-agent-gymnasium_amd")
REPS, H, E, CAP, P, PER = 7, 32, 32, 20000, 8, 512
FILL = 1800          # vector steps before the updates are timed (as 6zb's probe at 41x41)
LIMIT = {"update": 300, "train 21": 300, "train 41": 420}
ALPHAS = ["none"] * 4 + ["0"] * 4 + ["0.9"] * 4
BETAS = ["0.6"] * 4 + ["0"] * 4 + ["0.6"] * 4
SEEDS = ["0", "1", "2", "3"] * 3


def emit(path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def timed(torch, f, n):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) / n * 1e3  # us


def stat(torch, f, n):
    for _ in range(10):
        f()
    ts = sorted(timed(torch, f, n) for _ in range(REPS))
    return {"median": round(statistics.median(ts), 1), "min": round(ts[0], 1),
            "max": round(ts[-1], 1)}


def case_update(out):
    sys.path.insert(0, PKG)
    import torch
    import mazerl
    from mazerl import _native as N
    from mazerl.trainers import VectorRecurrentDQNPopulation
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer

    def env(n):
        return mazerl.VectorMazeEnv(n, 41, enrich=False, device="cuda", pos=False, done_list=False)

    kw = dict(batch_size=E, memory_size=CAP, train_every=10 ** 9, bank=False, window=40, burn_in=40)
    uni = VectorRecurrentDQNPopulation(env(P * PER), "cuda", learners=P, seed=list(range(P)), **kw)
    pri = VectorRecurrentDQNPopulation(env(P * PER), "cuda", learners=P, seed=list(range(P)),
                                       priority_alpha=0.9, priority_beta=0.6, **kw)
    one = VectorRecurrentDQNTrainer(env(PER), "cuda", priority_alpha=0.9, priority_beta=0.6, **kw)
    for tr in (uni, pri, one):
        for _ in range(FILL):
            tr.vector_step()
    for tr in (uni, pri):
        tr.filled = [int(n) for n in tr.ring[:, 1].tolist()]
        assert min(tr.filled) >= E, tr.filled
    one.filled = int(one.ring[1])
    assert one.filled >= E, one.filled
    one.opt.param_groups[0]["lr"].fill_(1e-3)
    assert torch.equal(uni.mem_len, pri.mem_len)
    due = [True] * P

    def pop_update(tr):
        def f():
            tr._upload(due, [0] * P, [1e-3] * P)
            tr.sample(due)
            tr.update()
            tr.updates = [u + 1 for u in tr.updates]
        return f

    def singles():
        for _ in range(P):
            one.sample()
            one.update(1e-3)
            one.updates += 1

    n = 15
    rec = dict(probe="lstm-dqn population prioritized update", dim=41, L=pri.L, E=E, window=40,
               burn_in=40, capacity=CAP, learners=P, instances_per_learner=PER,
               episodes_in_memory=pri.filled, episodes_in_memory_single=one.filled,
               windows_per_slot=pri.snaps)
    rec["pop_uniform_update_us"] = stat(torch, pop_update(uni), n)
    rec["pop_prioritized_update_us"] = stat(torch, pop_update(pri), n)
    rec["pop_uniform_update_again_us"] = stat(torch, pop_update(uni), n)
    rec["single_prioritized_updates_x8_us"] = stat(torch, singles, n)
    u, p = rec["pop_uniform_update_us"]["median"], rec["pop_prioritized_update_us"]["median"]
    rec["prioritized_over_uniform"] = round(p / u, 3)
    rec["uniform_again_over_uniform"] = round(rec["pop_uniform_update_again_us"]["median"] / u, 3)
    rec["singles_over_pop_prioritized"] = round(
        rec["single_prioritized_updates_x8_us"]["median"] / p, 3)
    rec["prioritized_minus_uniform_us_per_learner"] = round((p - u) / P, 1)
    tr, st = pri, pri._stream()
    dirs = (tr.wdir.data_ptr(), tr.d_off.data_ptr(), tr.d_tot.data_ptr())

    def sample():
        N.check(tr.lib.mz_drqn_pop_prio_sample(
            tr.seed_dev.data_ptr(), tr.cnt_dev.data_ptr(), tr.burn_in_dev.data_ptr(),
            tr.beta_dev.data_ptr(), tr.due_prio_dev.data_ptr(), H, P, E, tr.L, 40, 40, CAP,
            tr.mem_len.data_ptr(), tr.mem_prio.data_ptr(), tr.mem_psum.data_ptr(), *dirs,
            tr.isw.data_ptr(), st))

    def write_back():  # (on the last update's rows; d is scaled again each call, which costs the same)
        N.check(tr.lib.mz_drqn_pop_prio_update(
            tr.prio_alpha_dev.data_ptr(), tr.prio_eta_dev.data_ptr(), tr.prio_eps_dev.data_ptr(),
            tr.due_prio_dev.data_ptr(), H, P, E, tr.L, 40, CAP, *dirs, tr.qa.data_ptr(),
            tr.y.data_ptr(), tr.d.data_ptr(), tr.ep_loss.data_ptr(), tr.isw.data_ptr(),
            tr.mem_prio.data_ptr(), tr.mem_psum.data_ptr(), tr.prio_max.data_ptr(), st))

    def uniform_sample():
        uni.sample(due)
    rec["mz_drqn_pop_window_sample_us"] = stat(torch, uniform_sample, 100)
    rec["mz_drqn_pop_prio_sample_us"] = stat(torch, sample, 100)
    rec["mz_drqn_pop_prio_update_us"] = stat(torch, write_back, 100)
    rec["prio_max"] = [v / (1 << 20) for v in tr.prio_max.tolist()]
    rec["mean_weight_last_batch"] = [round(v, 4) for v in tr.isw.mean(dim=1).tolist()]
    emit(out, rec)


def case_train(dim, out):
    cmd = [sys.executable, "-m", "mazerl.train_lstm_dqn", "--learners", "12", "--envs", "12288",
           "--steps", "30000", "--eps-decay", "5000", "--dim", str(dim), "--window", "40",
           "--burn-in", "40", "--sweep", "priority-alpha=" + ",".join(ALPHAS),
           "--sweep", "priority-beta=" + ",".join(BETAS), "--seeds", ",".join(SEEDS)]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode)
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    rates = rec["win_rate_greedy"]
    from statistics import mean
    rec["by_setting"] = {
        name: {"rates": rates[4 * k:4 * k + 4], "mean": round(mean(rates[4 * k:4 * k + 4]), 4),
               "min": min(rates[4 * k:4 * k + 4]), "max": max(rates[4 * k:4 * k + 4])}
        for k, name in enumerate(("uniform", "alpha 0 / beta 0", "alpha 0.9 / beta 0.6"))}
    emit(out, rec)


def run_all(outdir, kinds):
    os.makedirs(outdir, exist_ok=True)
    for c in (["update"], ["train", "21"], ["train", "41"]):
        if kinds and c[0] not in kinds:
            continue
        out = os.path.join(outdir, {"update": "update.jsonl",
                                    "train": "train_pop12_1024x30000.jsonl"}[c[0]])
        cmd = ["timeout", "-k", "10", str(LIMIT[" ".join(c)]), sys.executable,
               os.path.abspath(__file__)] + c + [out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # a fault, a hang or an error: nothing more runs on the GPU
            print(f"{' '.join(c)}: exit status {rc}; stopping", flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a or a[0] == "all":
        run_all(a[1] if len(a) > 1 else os.path.join(HERE, "lstm_dqn_pop_prio"), a[2:])
    elif a[0] == "update":
        case_update(a[1])
    elif a[0] == "train":
        case_train(int(a[1]), a[2])
    else:
        sys.exit(__doc__)
