"""Replay windows of the recurrent DQN: what a windowed update and the state
snapshots cost beside the whole-episode trainer, and one training run per setting.

  exp_lstm_dqn_window_probe.py all [OUTDIR [KIND ...]]   every case below (or those of the KINDs
        update / step / train), each in a process of its own under its own time limit; stops at
        the first failure
  exp_lstm_dqn_window_probe.py update DIM OUT    one update (sample, target and source forward,
        BPTT + reduce, AdamW; E = 32) on DIM x DIM plain mazes at 4,096 instances: whole episodes
        (the single-learner entry points on buffers of E (L + 1) rows) and windows (T, K) = (40, 0),
        (40, 40), (80, 0), (80, 80) with stored state, all on the one memory a windowed run filled
        ((80, 40) is no legal setting: the burn-in is a multiple of the window)
  exp_lstm_dqn_window_probe.py step OUT          a vector step without updates at 4,096 instances
        of 9x9, window=None against window=40 (snapshot + snapshot store), and the two launches alone
  exp_lstm_dqn_window_probe.py train DIM MODE OUT   python -m mazerl.train_lstm_dqn --envs 1024
        --steps 30000 --eps-decay 5000 --seed 0; MODE whole | stored | zero ((40, 40) windows)
HIP events in one process, 10 warm-up calls, then REPS windows per figure: median (min-max) in
microseconds. One JSON line per figure, appended to OUT (default directory: profiles/lstm_dqn_window)."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "maze-solving-agent-gymnasium_amd")
REPS, H, E, STASH, PARAMS = 7, 32, 32, 192, 5252
FILL = {9: 200, 41: 1800, 81: 6500}     # vector steps that fill the memory (9, 41: as 6q's probe)
LIMIT = {"update 9": 120, "update 41": 180, "update 81": 420, "step": 120, "train 21": 240,
         "train 41": 420}


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


def case_update(dim, out):
    import torch
    sys.path.insert(0, PKG)
    import mazerl
    from mazerl import _native as N
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer, param_ptrs
    env = mazerl.VectorMazeEnv(4096, dim, enrich=False, device="cuda", pos=False, done_list=False)
    tr = VectorRecurrentDQNTrainer(env, "cuda", batch_size=E, memory_size=4096,
                                   train_every=10 ** 9, bank=False, window=40)
    for _ in range(FILL[dim]):
        tr.vector_step()
    tr.filled = int(tr.ring[1])
    assert tr.filled >= E, tr.filled
    L, cap, st = tr.L, tr.capacity, tr._stream()
    pt = param_ptrs(tr.target_net)  # (the single-learner entry points' pointer arrays)
    pg = (ctypes.c_void_p * 6)(*[p.grad.data_ptr() for p in tr.source_net.parameters()])
    lens = tr.mem_len[:tr.filled].float()
    kw = dict(device=tr.device)
    rows = E * (L + 1)
    d_slot, d_len = (torch.zeros(E, dtype=torch.int32, **kw) for _ in range(2))
    d_off, d_tot = torch.zeros(E, dtype=torch.int64, **kw), torch.zeros(2, dtype=torch.int64, **kw)
    qmax, qa, y, d = (torch.zeros(rows, **kw) for _ in range(4))
    stash = torch.zeros(rows, STASH, **kw)
    dirs = (d_slot.data_ptr(), d_len.data_ptr(), d_off.data_ptr(), d_tot.data_ptr())

    def whole():  # the whole-episode update of window=None, on this memory
        N.check(tr.lib.mz_drqn_sample(tr.seed, tr.updates, E, L, cap, tr.filled, tr.ring.data_ptr(),
                                      tr.mem_len.data_ptr(), *dirs, st))
        N.check(tr.lib.mz_drqn_seq_forward(pt, H, 1, E, L, cap, tr.gamma, tr.mem.data_ptr(),
                                           tr.mem_term.data_ptr(), *dirs, qmax.data_ptr(), None,
                                           None, None, None, None, st))
        N.check(tr.lib.mz_drqn_seq_forward(tr._ps, H, 0, E, L, cap, tr.gamma, tr.mem.data_ptr(),
                                           tr.mem_term.data_ptr(), *dirs, qmax.data_ptr(),
                                           stash.data_ptr(), qa.data_ptr(), y.data_ptr(),
                                           d.data_ptr(), tr.ep_loss.data_ptr(), st))
        N.check(tr.lib.mz_drqn_seq_backward(tr._ps, H, E, L, cap, tr.mem.data_ptr(), *dirs,
                                            stash.data_ptr(), d.data_ptr(), tr.ep_loss.data_ptr(),
                                            tr.gpart.data_ptr(), pg, tr.loss.data_ptr(), st))
        tr.opt.step()
        tr.updates += 1

    def windowed():
        tr.sample()
        tr.update(1e-3)
        tr.updates += 1

    def retarget(T, K):
        """The same memory under another (T, K): snapshot j of T = 80 is snapshot 2 j of T = 40."""
        if T != tr.window:
            assert T == 2 * tr.window
            tr.mem_state = tr.mem_state[:, ::2].contiguous()
            tr.window, tr.snaps = T, (L - 1) // T + 1
            assert tr.mem_state.shape[1] == tr.snaps
            r = E * (min(T, L) + 2)
            tr.qmax, tr.qa, tr.y, tr.d = (torch.zeros(r, **kw) for _ in range(4))
            tr.stash = torch.zeros(r, STASH, **kw)
        tr.burn_in = K

    n = {9: 40, 41: 15, 81: 5}[dim]
    base = dict(probe="lstm-dqn window update", dim=dim, L=L, E=E, episodes_in_memory=tr.filled,
                mean_episode_steps=round(float(lens.mean()), 1), max_episode_steps=int(lens.max()))
    tr.opt.param_groups[0]["lr"].fill_(1e-3)
    t = stat(torch, whole, n)
    emit(out, dict(base, unit="whole episodes", update_us=t, last_batch_steps=int(d_tot[1]),
                   last_batch_longest=int(d_len.max()), row_buffer_rows=rows))
    for T, K in ((40, 0), (40, 40), (80, 0), (80, 80)):
        retarget(T, K)
        t = stat(torch, windowed, n)
        w = tr.wdir.cpu()
        emit(out, dict(base, unit="windows", window=T, burn_in=K, update_us=t,
                       last_batch_steps=int(tr.d_tot[1]),
                       last_batch_longest_unroll=int((w[3] + w[4]).max()) + 1,
                       row_buffer_rows=tr.qmax.numel()))
    emit(out, dict(base, unit="whole episodes, again", update_us=stat(torch, whole, n)))
    env.close()


def case_step(out):
    import torch
    sys.path.insert(0, PKG)
    import mazerl
    from mazerl import _native as N
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer

    def mk(**kw):
        env = mazerl.VectorMazeEnv(4096, 9, enrich=False, device="cuda", pos=False, done_list=False)
        return VectorRecurrentDQNTrainer(env, "cuda", batch_size=E, memory_size=4096,
                                         train_every=10 ** 9, bank=False, **kw)
    a, b = mk(), mk(window=40)
    for tr in (a, b):
        for _ in range(200):
            tr.vector_step()
    rec = dict(probe="lstm-dqn vector step without updates", instances=4096, dim=9, window=40)
    rec["window_none_us"] = stat(torch, a.vector_step, 300)
    rec["window_40_stored_us"] = stat(torch, b.vector_step, 300)
    rec["window_none_again_us"] = stat(torch, a.vector_step, 300)
    st = b._stream()

    def snap():
        N.check(b.lib.mz_drqn_snapshot(H, 4096, b.L, 40, b.t.data_ptr(), b.h.data_ptr(),
                                       b.c.data_ptr(), b.snap_rec.data_ptr(), st))

    def store():  # (reads the last step's finished list; the ring is not advanced)
        N.check(b.lib.mz_drqn_snap_store(H, 4096, b.L, 40, b.fin_id.data_ptr(),
                                         b.fin_len.data_ptr(), b.fin_count.data_ptr(),
                                         b.snap_rec.data_ptr(), b.capacity,
                                         b.mem_state.data_ptr(), b.ring.data_ptr(), st))
    rec["mz_drqn_snapshot_us"] = stat(torch, snap, 300)
    rec["mz_drqn_snap_store_us"] = stat(torch, store, 300)
    emit(out, rec)


def case_train(dim, mode, out):
    cmd = [sys.executable, "-m", "mazerl.train_lstm_dqn", "--envs", "1024", "--steps", "30000",
           "--eps-decay", "5000", "--seed", "0", "--dim", str(dim)]
    if mode != "whole":
        cmd += ["--window", "40", "--burn-in", "40", "--initial-state", mode]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        sys.exit(r.returncode)
    emit(out, dict(json.loads(r.stdout.strip().splitlines()[-1]), mode=mode))


def run_all(outdir, kinds):
    os.makedirs(outdir, exist_ok=True)
    cases = [["update", "9"], ["update", "41"], ["update", "81"], ["step"]] + \
        [["train", str(d), m] for d in (21, 41) for m in ("whole", "stored", "zero")]
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
        run_all(a[1] if len(a) > 1 else os.path.join(HERE, "lstm_dqn_window"), a[2:])
    elif a[0] == "update":
        case_update(int(a[1]), a[2])
    elif a[0] == "step":
        case_step(a[1])
    elif a[0] == "train":
        case_train(int(a[1]), a[2], a[3])
    else:
        sys.exit(__doc__)
