"""Double-Q targets and n-step returns of the recurrent DQN: what an update costs
with them beside the default update, whether the default update kept its time, and one training
comparison. Method: exp_lstm_dqn_window_probe.py's (6w).

  exp_lstm_dqn_returns_probe.py all OUTDIR [PARENT]   every case below, each in a process of its
        own under its own time limit; stops at the first failure. PARENT: a checkout of the parent
        commit with its library built (its package directory); the update cases then alternate
        parent, this tree, parent, this tree
  exp_lstm_dqn_returns_probe.py update DIM OUT [PKG]  one update (sample, both forwards, [returns,]
        BPTT + reduce, AdamW; E = 32, (T, K) = (40, 40), stored state) on DIM x DIM plain mazes at
        4,096 instances, on the memory a windowed run filled: the default chain, then (double_q,
        n_step) = (1, 1), (0, 5), (1, 5) through the new chain on the same trainer and memory, then
        the default again. With PKG (a tree without the options): the default chain alone, twice
  exp_lstm_dqn_returns_probe.py train OUT             python -m mazerl.train_lstm_dqn --dim 41
        --envs 8192 --learners 8 --steps 30000 --eps-decay 5000 --window 40 --burn-in 40, seeds
        0 .. 3 at the defaults and 0 .. 3 with double-q 1, n-step 5: 1,024 instances per learner
HIP events in one process, 10 warm-up calls, then REPS windows per figure: median (min-max) in
microseconds. One JSON line per figure, appended to OUT."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "maze-solving-agent-gymnasium_amd")
REPS, E, T, K = 7, 32, 40, 40
FILL = {41: 1800, 81: 6500}     # vector steps that fill the memory (6w's)
CALLS = {41: 15, 81: 5}
LIMIT = {"update": 240, "train": 1100}


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


def case_update(dim, out, pkg=None):
    import torch
    sys.path.insert(0, pkg or PKG)
    import mazerl
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    env = mazerl.VectorMazeEnv(4096, dim, enrich=False, device="cuda", pos=False, done_list=False)
    new = {} if pkg else dict(double_q=True, n_step=5)  # (so that q4, sel and n_step_dev exist)
    tr = VectorRecurrentDQNTrainer(env, "cuda", batch_size=E, memory_size=4096, train_every=10 ** 9,
                                   bank=False, window=T, burn_in=K, **new)
    for _ in range(FILL[dim]):
        tr.vector_step()
    tr.filled = int(tr.ring[1])
    assert tr.filled >= E, tr.filled
    tr.opt.param_groups[0]["lr"].fill_(1e-3)

    def update():
        tr.sample()
        tr.update(1e-3)
        tr.updates += 1

    def setting(chain, dq, n):
        """The same trainer and memory under another setting; chain False: the default update."""
        tr._returns = chain
        if chain:
            tr._double_q = [bool(dq)]
            tr.double_dev.fill_(int(dq))
            tr.n_step = n

    base = dict(probe="lstm-dqn returns update", tree="parent" if pkg else "this", dim=dim, L=tr.L,
                E=E, window=T, burn_in=K, episodes_in_memory=tr.filled)
    cases = [("default", False, 0, 1)]
    if not pkg:
        cases += [("new chain", True, 1, 1), ("new chain", True, 0, 5), ("new chain", True, 1, 5)]
    for name, chain, dq, n in cases + [("default, again", False, 0, 1)]:
        if not pkg:
            setting(chain, dq, n)
        t = stat(torch, update, CALLS[dim])
        emit(out, dict(base, chain=name, double_q=dq, n_step=n, update_us=t,
                       last_batch_steps=int(tr.d_tot[1])))
    env.close()


def case_train(out):
    cmd = [sys.executable, "-m", "mazerl.train_lstm_dqn", "--dim", "41", "--envs", "8192",
           "--learners", "8", "--steps", "30000", "--eps-decay", "5000", "--window", "40",
           "--burn-in", "40", "--seeds", "0,1,2,3,0,1,2,3", "--sweep", "double-q=0,0,0,0,1,1,1,1",
           "--sweep", "n-step=1,1,1,1,5,5,5,5"]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode)
    emit(out, json.loads(r.stdout.strip().splitlines()[-1]))


def run_all(outdir, parent):
    os.makedirs(outdir, exist_ok=True)
    out = os.path.join(outdir, "update.jsonl")
    cases = []
    for dim in (41, 81):
        for _ in range(2):
            if parent:
                cases.append(["update", str(dim), out, parent])
            cases.append(["update", str(dim), out])
    cases.append(["train", os.path.join(outdir, "train_8x1024x30000.jsonl")])
    for c in cases:
        cmd = ["timeout", "-k", "10", str(LIMIT[c[0]]), sys.executable, os.path.abspath(__file__)] + c
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # a fault, a hang or an error: nothing more runs on the GPU
            print(f"{' '.join(c)}: exit status {rc}; stopping", flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "all" and len(a) >= 2:
        run_all(a[1], a[2] if len(a) > 2 else None)
    elif a and a[0] == "update" and len(a) >= 3:
        case_update(int(a[1]), a[2], a[3] if len(a) > 3 else None)
    elif a and a[0] == "train" and len(a) == 2:
        case_train(a[1])
    else:
        sys.exit(__doc__)
