"""Prioritized replay windows of the recurrent DQN: what the prioritized update and
the entry launch cost beside the uniform windowed trainer, and training runs per setting.

  exp_lstm_dqn_prio_probe.py all [OUTDIR [KIND ...]]   every case below (or those of the KINDs
        update / step / train), each in a process of its own under its own time limit; stops at
        the first failure
  exp_lstm_dqn_prio_probe.py update DIM OUT    one update (sample, target and source forward,
        [mz_drqn_prio_update,] BPTT + reduce, AdamW; E = 32, (T, K) = (40, 40), stored state,
        capacity 20,000) on DIM x DIM plain mazes at 4,096 instances: uniform windows, prioritized
        (alpha 0.9, beta 0.6), uniform again, and mz_drqn_prio_sample / mz_drqn_prio_update alone.
        Both trainers run the same vector steps from the same seed, so their memories hold the same
        episodes
  exp_lstm_dqn_prio_probe.py step OUT          a vector step without updates at 4,096 instances of
        9x9, window=40 without and with priorities (mz_drqn_prio_store), and that launch alone
  exp_lstm_dqn_prio_probe.py train DIM MODE SEED OUT   python -m mazerl.train_lstm_dqn --envs 1024
        --steps 30000 --eps-decay 5000 --window 40 --burn-in 40; MODE uniform | a0 (alpha 0, beta
        0) | a09 (alpha 0.9, beta 0.6)
HIP events in one process, 10 warm-up calls, then REPS windows per figure: median (min-max) in
microseconds. One JSON line per figure, appended to OUT (default directory: profiles/lstm_dqn_prio)."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "maze-solving-agent-gymnasium_amd")
REPS, H, E, CAP = 7, 32, 32, 20000
FILL = {9: 200, 41: 1800, 81: 6500}     # vector steps that fill the memory (as 6w's probe)
LIMIT = {"update 9": 120, "update 41": 240, "update 81": 600, "step": 120, "train 21": 240,
         "train 41": 420}
SEEDS = (0, 1, 2, 3)


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


def make(dim, instances, **kw):
    sys.path.insert(0, PKG)
    import mazerl
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    env = mazerl.VectorMazeEnv(instances, dim, enrich=False, device="cuda", pos=False,
                               done_list=False)
    return VectorRecurrentDQNTrainer(env, "cuda", batch_size=E, memory_size=CAP,
                                     train_every=10 ** 9, bank=False, window=40, burn_in=40, **kw)


def case_update(dim, out):
    import torch
    uni, pri = make(dim, 4096), make(dim, 4096, priority_alpha=0.9, priority_beta=0.6)
    from mazerl import _native as N
    for tr in (uni, pri):
        for _ in range(FILL[dim]):
            tr.vector_step()
        tr.filled = int(tr.ring[1])
        assert tr.filled >= E, tr.filled
        tr.opt.param_groups[0]["lr"].fill_(1e-3)
    assert torch.equal(uni.mem_len, pri.mem_len)

    def update(tr):
        def f():
            tr.sample()
            tr.update(1e-3)
            tr.updates += 1
        return f

    n = {9: 40, 41: 15, 81: 5}[dim]
    lens = pri.mem_len[:pri.filled].float()
    rec = dict(probe="lstm-dqn prioritized update", dim=dim, L=pri.L, E=E, window=40, burn_in=40,
               capacity=CAP, episodes_in_memory=pri.filled, windows_per_slot=pri.snaps,
               mean_episode_steps=round(float(lens.mean()), 1))
    rec["uniform_update_us"] = stat(torch, update(uni), n)
    rec["prioritized_update_us"] = stat(torch, update(pri), n)
    rec["uniform_update_again_us"] = stat(torch, update(uni), n)
    rec["prioritized_over_uniform"] = round(
        rec["prioritized_update_us"]["median"] / rec["uniform_update_us"]["median"], 3)
    tr, st = pri, pri._stream()
    dirs = (tr.wdir.data_ptr(), tr.d_off.data_ptr(), tr.d_tot.data_ptr())

    def sample():
        N.check(tr.lib.mz_drqn_prio_sample(
            tr.seed, tr.updates, H, E, tr.L, 40, 40, CAP, tr.mem_len.data_ptr(),
            tr.mem_prio.data_ptr(), tr.mem_psum.data_ptr(), *dirs, tr.isw.data_ptr(), 0.6, st))

    def write_back():  # (on the last update's rows; d is scaled again each call, which costs the same)
        N.check(tr.lib.mz_drqn_prio_update(
            H, E, tr.L, 40, CAP, *dirs, tr.qa.data_ptr(), tr.y.data_ptr(), tr.d.data_ptr(),
            tr.ep_loss.data_ptr(), tr.isw.data_ptr(), 0.9, 0.9, 1e-3, tr.mem_prio.data_ptr(),
            tr.mem_psum.data_ptr(), tr.prio_max.data_ptr(), st))

    def uniform_sample():
        uni.sample()
    rec["mz_drqn_window_sample_us"] = stat(torch, uniform_sample, 100)
    rec["mz_drqn_prio_sample_us"] = stat(torch, sample, 100)
    rec["mz_drqn_prio_update_us"] = stat(torch, write_back, 100)
    rec["prio_max"] = int(tr.prio_max) / (1 << 20)
    rec["mean_weight_last_batch"] = round(float(tr.isw.mean()), 4)
    emit(out, rec)


def case_step(out):
    import torch
    a, b = make(9, 4096), make(9, 4096, priority_alpha=0.9)
    from mazerl import _native as N
    for tr in (a, b):
        for _ in range(200):
            tr.vector_step()
    rec = dict(probe="lstm-dqn vector step without updates", instances=4096, dim=9, window=40,
               capacity=CAP)
    rec["uniform_us"] = stat(torch, a.vector_step, 300)
    rec["prioritized_us"] = stat(torch, b.vector_step, 300)
    rec["uniform_again_us"] = stat(torch, a.vector_step, 300)
    st = b._stream()

    def store():  # (reads the last step's finished list; the ring is not advanced)
        N.check(b.lib.mz_drqn_prio_store(H, 4096, b.L, 40, b.fin_id.data_ptr(),
                                         b.fin_len.data_ptr(), b.fin_count.data_ptr(), CAP,
                                         b.mem_prio.data_ptr(), b.mem_psum.data_ptr(),
                                         b.prio_max.data_ptr(), b.ring.data_ptr(), st))
    rec["mz_drqn_prio_store_us"] = stat(torch, store, 300)
    emit(out, rec)


def case_train(dim, mode, seed, out):
    cmd = [sys.executable, "-m", "mazerl.train_lstm_dqn", "--envs", "1024", "--steps", "30000",
           "--eps-decay", "5000", "--seed", str(seed), "--dim", str(dim), "--window", "40",
           "--burn-in", "40"]
    cmd += {"uniform": [], "a0": ["--priority-alpha", "0", "--priority-beta", "0"],
            "a09": ["--priority-alpha", "0.9", "--priority-beta", "0.6"]}[mode]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode)
    emit(out, dict(json.loads(r.stdout.strip().splitlines()[-1]), mode=mode))


def run_all(outdir, kinds):
    os.makedirs(outdir, exist_ok=True)
    cases = [["update", "41"], ["update", "81"], ["step"]] + \
        [["train", str(d), m, str(s)] for d in (21, 41) for m in ("uniform", "a0", "a09")
         for s in SEEDS]
    for c in cases:
        if kinds and c[0] not in kinds:
            continue
        out = os.path.join(outdir, {"update": "update.jsonl", "step": "step.jsonl",
                                    "train": "train_1024x30000.jsonl"}[c[0]])
        limit = LIMIT[" ".join(c[:2]) if c[0] != "step" else "step"]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + c + [out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # a fault, a hang or an error: nothing more runs on the GPU
            print(f"{' '.join(c)}: exit status {rc}; stopping", flush=True)
            sys.exit(rc)


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a or a[0] == "all":
        run_all(a[1] if len(a) > 1 else os.path.join(HERE, "lstm_dqn_prio"), a[2:])
    elif a[0] == "update":
        case_update(int(a[1]), a[2])
    elif a[0] == "step":
        case_step(a[1])
    elif a[0] == "train":
        case_train(int(a[1]), a[2], int(a[3]), a[4])
    else:
        sys.exit(__doc__)
