"""Replay windows in recurrent DQN populations: one windowed population update
(window sample, target and source window forward, window BPTT + reduce, AdamW; E = 32) at P = 1, 8
and 32 learners of 128 instances each and (T, K) = (40, 0), (40, 40), beside P single windowed
updates run back to back on the same rings through the single-learner entry points, and beside the
whole-episode population update on the same rings; 9x9 and 41x41 plain mazes whose rings a windowed
run filled. Then the acting step at P b = 4,096 with and without the snapshot launch. HIP events in
one process, 10 warm-up calls, then REPS windows per figure: median (min-max) in microseconds. One
JSON line per case (profiles/lstm_dqn_pop_window/update.jsonl).
  exp_lstm_dqn_pop_window_probe.py [OUT.jsonl]"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "maze-solving-agent-gymnasium_amd"))
import mazerl  # noqa: E402
from mazerl import _native as N  # noqa: E402
from mazerl.trainers.drqn_population import (ADAM_EPS, BETAS, CLAMP, PARAMS, SHAPES, STASH,  # noqa: E402
                                             WEIGHT_DECAY, VectorRecurrentDQNPopulation)

REPS, H, E, b = 7, 32, 32, 128
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(f, n):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) / n * 1e3  # us


def stat(f, n):
    for _ in range(10):
        f()
    ts = sorted(timed(f, n) for _ in range(REPS))
    return {"median": round(statistics.median(ts), 1), "min": round(ts[0], 1),
            "max": round(ts[-1], 1)}


def row_ptrs(row):
    off, ptrs = 0, []
    for s in SHAPES:
        ptrs.append(row.data_ptr() + 4 * off)
        off += int(torch.Size(s).numel())
    return (C.c_void_p * 6)(*ptrs)


def single_updates(tr):
    """P single windowed updates back to back on the population's own rings, nets and buffers."""
    lib, L, cap, st, T = tr.lib, tr.L, tr.capacity, tr._stream(), tr.window
    lrs = [torch.full((1,), 1e-3, device=tr.device) for _ in range(tr.P)]
    keep, calls = [], []
    for p in range(tr.P):
        ps, pt, pg = row_ptrs(tr.src[p]), row_ptrs(tr.tgt[p]), row_ptrs(tr.grad[p])
        dirs = (tr.wdir[p].data_ptr(), tr.d_off[p].data_ptr(), tr.d_tot[p].data_ptr())
        garr, glen = (C.c_void_p * 1)(tr.grad[p].data_ptr()), (C.c_int64 * 1)(PARAMS)
        state = tr.mem_state[p].data_ptr() if tr.stored[p] else None
        keep.append((ps, pt, pg, garr, glen))
        calls.append((p, ps, pt, pg, dirs, garr, glen, state))

    def run():
        for p, ps, pt, pg, dirs, garr, glen, state in calls:
            K = tr.burn_in[p]
            N.check(lib.mz_drqn_window_sample(p, tr.updates[p], H, E, L, T, K, cap, tr.filled[p],
                                              tr.ring[p].data_ptr(), tr.mem_len[p].data_ptr(),
                                              *dirs, st))
            N.check(lib.mz_drqn_window_forward(pt, H, 1, E, L, T, K, cap, 0.99,
                                               tr.mem[p].data_ptr(), tr.mem_term[p].data_ptr(),
                                               state, *dirs, tr.qmax[p].data_ptr(), None, None,
                                               None, None, None, st))
            N.check(lib.mz_drqn_window_forward(ps, H, 0, E, L, T, K, cap, 0.99,
                                               tr.mem[p].data_ptr(), tr.mem_term[p].data_ptr(),
                                               state, *dirs, tr.qmax[p].data_ptr(),
                                               tr.stash[p].data_ptr(), tr.qa[p].data_ptr(),
                                               tr.y[p].data_ptr(), tr.d[p].data_ptr(),
                                               tr.ep_loss[p].data_ptr(), st))
            N.check(lib.mz_drqn_window_backward(ps, H, E, L, T, K, cap, tr.mem[p].data_ptr(), *dirs,
                                                tr.stash[p].data_ptr(), tr.d[p].data_ptr(),
                                                tr.ep_loss[p].data_ptr(), tr.gpart[p].data_ptr(),
                                                pg, tr.loss[p:].data_ptr(), st))
            N.check(lib.mz_adamw_flat(tr.src[p].data_ptr(), tr.exp_avg[p].data_ptr(),
                                      tr.exp_avg_sq[p].data_ptr(), garr, glen, 1,
                                      lrs[p].data_ptr(), tr.step[p:].data_ptr(), BETAS[0], BETAS[1],
                                      ADAM_EPS, WEIGHT_DECAY, CLAMP, 1.0, 1, st))
    return run, keep


def whole_update(tr):
    """The whole-episode population update on the same rings (row buffers of its own)."""
    P, L, cap, st, lib = tr.P, tr.L, tr.capacity, tr._stream(), tr.lib
    kw = dict(device=tr.device, dtype=torch.float32)
    rows = E * (L + 1)
    qmax, qa, y, d = (torch.zeros(P, rows, **kw) for _ in range(4))
    stash = torch.zeros(P, rows, STASH, **kw)
    dirs = (tr.d_slot.data_ptr(), tr.d_len.data_ptr(), tr.d_off.data_ptr(), tr.d_tot.data_ptr())
    due, gam = tr.due_dev.data_ptr(), tr.gamma_dev.data_ptr()

    def run():
        N.check(lib.mz_drqn_pop_sample(
            tr.seed_dev.data_ptr(), tr.cnt_dev.data_ptr(), due, P, E, L, cap, min(tr.filled),
            tr.ring.data_ptr(), tr.mem_len.data_ptr(), *dirs, st))
        N.check(lib.mz_drqn_pop_seq_forward(
            tr.tgt.data_ptr(), H, 1, P, E, L, cap, gam, due, tr.mem.data_ptr(),
            tr.mem_term.data_ptr(), *dirs, qmax.data_ptr(), None, None, None, None, None, st))
        N.check(lib.mz_drqn_pop_seq_forward(
            tr.src.data_ptr(), H, 0, P, E, L, cap, gam, due, tr.mem.data_ptr(),
            tr.mem_term.data_ptr(), *dirs, qmax.data_ptr(), stash.data_ptr(), qa.data_ptr(),
            y.data_ptr(), d.data_ptr(), tr.ep_loss.data_ptr(), st))
        N.check(lib.mz_drqn_pop_seq_backward(
            tr.src.data_ptr(), H, P, E, L, cap, due, tr.mem.data_ptr(), *dirs, stash.data_ptr(),
            d.data_ptr(), tr.ep_loss.data_ptr(), tr.gpart.data_ptr(), tr.grad.data_ptr(),
            tr.loss.data_ptr(), st))
        tr._adamw(due, st)
    return run, (qmax, qa, y, d, stash)


for dim, fill_steps, n in ((9, 200, 40), (41, 1800, 15)):
    for P in (1, 8, 32):
        for T, K in ((40, 0), (40, 40)):
            env = mazerl.VectorMazeEnv(P * b, dim, enrich=False, device="cuda", pos=False,
                                       done_list=False)
            tr = VectorRecurrentDQNPopulation(env, "cuda", learners=P, batch_size=E,
                                              memory_size=1024, train_every=10 ** 9, bank=False,
                                              seed=list(range(P)), window=T, burn_in=K)
            for _ in range(fill_steps):
                tr.vector_step()
            tr.filled = [int(v) for v in tr.ring[:, 1].tolist()]
            assert min(tr.filled) >= E, tr.filled
            due = [True] * P
            tr._upload(due, [0] * P, [1e-3] * P)

            def pop_update():
                tr.sample(due)
                tr.update()

            singles, keep = single_updates(tr)
            t_pop, t_one = stat(pop_update, n), stat(singles, max(2, n // P))
            t_pop2 = stat(pop_update, n)  # again after the singles: the spread between two windows
            rec = {"probe": "lstm-dqn windowed population update", "dim": dim, "L": tr.L,
                   "learners": P, "instances_per_learner": b, "E": E, "T": T, "K": K,
                   "episodes_in_memory_min": min(tr.filled),
                   "last_batch_training_steps": [int(v) for v in tr.d_tot[:, 1].tolist()][:4],
                   "windowed_population_update_us": t_pop,
                   "windowed_population_update_again_us": t_pop2,
                   "single_windowed_updates_back_to_back_us": t_one,
                   "memory_bytes": tr.memory_bytes()}
            if K == 0:
                whole, bufs = whole_update(tr)
                rec["whole_episode_population_update_us"] = stat(whole, n)
                lens = torch.cat([tr.mem_len[p, :tr.filled[p]] for p in range(P)]).float()
                rec["mean_episode_steps"] = round(float(lens.mean()), 1)
                rec["max_episode_steps"] = int(lens.max())
                del whole, bufs
            emit(rec)
            env.close()
            del tr, env, singles, keep
            torch.cuda.empty_cache()

# the acting step at 4,096 instances: the population act alone, and with the snapshot launch
for P in (8,):
    env = mazerl.VectorMazeEnv(4096, 9, enrich=False, device="cuda", pos=False, done_list=False)
    tr = VectorRecurrentDQNPopulation(env, "cuda", learners=P, batch_size=4, memory_size=8,
                                      train_every=10 ** 9, bank=False, window=40)
    st = tr._stream()

    def pop_act():
        N.check(tr.lib.mz_drqn_pop_act(
            tr.src.data_ptr(), H, tr.P, tr.b, env.obs6.data_ptr(), tr.L, tr.eps_dev.data_ptr(), 4,
            tr.seed_dev.data_ptr(), 5, tr.t.data_ptr(), tr.h.data_ptr(), tr.c.data_ptr(),
            tr.rec_x.data_ptr(), tr.rec_a.data_ptr(), tr.act_out.data_ptr(), None, st))

    def snap_act():
        N.check(tr.lib.mz_drqn_snapshot(H, 4096, tr.L, 40, tr.t.data_ptr(), tr.h.data_ptr(),
                                        tr.c.data_ptr(), tr.snap_rec.data_ptr(), st))
        pop_act()

    tr.eps_dev.fill_(0.5)
    a, s = stat(pop_act, 300), stat(snap_act, 300)
    emit({"probe": "mz_drqn_pop_act with snapshot", "learners": P, "instances": 4096,
          "pop_act_us": a, "snapshot_and_pop_act_us": s, "pop_act_again_us": stat(pop_act, 300)})
    env.close()
