"""VectorRecurrentDQNTrainer with replay windows (window=4, burn_in 0 or 4) on the GPU: 64 instances
of 9x9 plain mazes, L = episode_bound(9) = 65. The bounds are tests/test_drqn_trainer_gpu.py's:
e_k <= 4 e_ref + 8 u max|tensor| with torch's float32 CPU path as the reference beside the float64
model (tests/drqn_window_model.py). The constructor's refusals need no GPU."""
import numpy as np
import pytest
import torch

import drqn_model as M
import drqn_window_model as W
import learner_model as LM

gpu = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
B, DIM, T = 64, 9, 4


def _mk(env_seed=0x5EED0D00, **kw):
    import mazerl
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    env = mazerl.VectorMazeEnv(B, DIM, enrich=False, device=DEV, seed=env_seed)
    kw.setdefault("bank", False)
    kw.setdefault("memory_size", 256)
    kw.setdefault("batch_size", 4)
    kw.setdefault("epsilon_decay", 200.0)
    return env, VectorRecurrentDQNTrainer(env, DEV, **kw)


def _state(tr):
    o = tr.opt
    ts = [tr.source_net._flat_params, tr.target_net._flat_params, o.exp_avg, o.exp_avg_sq,
          o._step_buf, tr.h, tr.c, tr.t, tr.ring, tr.mem, tr.mem_len, tr.mem_term, tr.stats,
          tr.env.obs6, tr.loss]
    if tr.stored:
        ts += [tr.mem_state[:int(tr.ring[1])]]
    return [t.clone() for t in ts]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _live_snaps(tr):
    """The in-flight snapshots that matter: 1 .. (t - 1) // T of every instance."""
    rec, t = tr.snap_rec.cpu().numpy(), tr.t.cpu().numpy()
    return [rec[i, 1:(t[i] - 1) // T + 1].copy() if t[i] > 0 else rec[i, :0] for i in range(B)]


def _windows(tr):
    """The windows of the last update's directory, read back from the memory."""
    slot, n, b, k, m = tr.wdir.cpu().numpy()
    mem, tm = tr.mem.cpu().numpy(), tr.mem_term.cpu().numpy()
    state = tr.mem_state.cpu().numpy() if tr.stored else None
    assert len(set(slot.tolist())) == len(slot) and (n == tr.mem_len.cpu().numpy()[slot]).all()
    ws = []
    for e, s in enumerate(slot):
        ep = dict(x=mem[s, :n[e] + 1, :6].view(np.float32).copy(), a=mem[s, :n[e], 6].astype(np.int64),
                  r=mem[s, :n[e], 7].view(np.float32).copy(), term=bool(tm[s]))
        j = (b[e] + k[e]) // T
        assert (b[e] + k[e]) % T == 0 and 0 <= j < W.windows_in(n[e], T)
        w = W.window_of(ep, T, tr.burn_in, j, None if state is None else state[s])
        assert (w["b"], w["k"], w["m"]) == (b[e], k[e], m[e])
        ws.append(w)
    return ws


@gpu
@pytest.mark.parametrize("K,mode", [(0, "stored"), (4, "stored"), (4, "zero")])
def test_one_vector_step_is_flat_adamw_on_the_window_model_gradient(K, mode):
    """train_every = 1, E = 4, after 12 updates: one more vector_step gives the parameters
    learner_model.adamw_step gives from the window model's gradient on the sampled windows."""
    from mazerl.agents.lstm_dqn_agent import DQN, window_td_loss
    from mazerl.agents.rf_agent import cosine_lr
    env, tr = _mk(lr=1e-3, target_update_frequency=5, window=T, burn_in=K, initial_state=mode)
    assert tr.qmax.numel() == 4 * (T + 2) and tr.stash.shape == (4 * (T + 2), 192)
    assert tr.stored == (mode == "stored") and hasattr(tr, "mem_state") == tr.stored
    for _ in range(400):
        tr.vector_step()
        if tr.updates == 12:
            break
    assert tr.updates == 12
    src = {k: v.detach().cpu().clone() for k, v in tr.source_net.state_dict().items()}
    tgt = {k: v.detach().cpu().clone() for k, v in tr.target_net.state_dict().items()}
    m0, v0 = tr.opt.exp_avg.cpu().numpy().copy(), tr.opt.exp_avg_sq.cpu().numpy().copy()
    step0 = float(tr.opt._step_buf[0])
    assert step0 == 12.0
    tr.vector_step()
    assert tr.updates == 13
    lr = cosine_lr(12, 1e-3, 30, 1e-6)
    assert tr.last_lr == lr
    ws = _windows(tr)
    steps = sum(w["m"] for w in ws)
    assert int(tr.d_tot[1]) == steps and int(tr.d_tot[0]) == steps + 2 * len(ws)
    print(f"K {K} {mode}: windows (b, k, m) {[(w['b'], w['k'], w['m']) for w in ws]}")
    out = W.window_td_loss(M.as_f64({k: v.numpy() for k, v in src.items()}),
                           M.as_f64({k: v.numpy() for k, v in tgt.items()}), ws, tr.gamma)
    ns, nt = DQN(6, 4, 32, torch.device("cpu")), DQN(6, 4, 32, torch.device("cpu"))
    ns.load_state_dict(src), nt.load_state_dict(tgt)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
    loss = window_td_loss(ns, nt, [(t32(w["x"]), torch.from_numpy(w["a"]), t32(w["r"]), t32(w["h0"]),
                                    t32(w["c0"]), w["k"], w["term"]) for w in ws], tr.gamma)
    loss.backward()
    e_k, e_ref = abs(float(tr.loss) - out["loss"]), abs(loss.item() - out["loss"])
    print(f"loss: e_k {e_k:.3e} e_ref {e_ref:.3e}")
    assert e_k <= 4 * e_ref + 8 * U * abs(out["loss"])
    off = 0
    for k, p, size in zip(M.KEYS, ns.parameters(), tr.source_net._flat_sizes):
        n = p.numel()
        args = (lr, step0, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0)
        pm = LM.adamw_step(src[k].numpy().ravel(), out["grads"][k].ravel(), m0[off:off + n],
                           v0[off:off + n], *args)[0]
        pr = LM.adamw_step(src[k].numpy().ravel(), p.grad.numpy().ravel(), m0[off:off + n],
                           v0[off:off + n], *args)[0]
        got = tr.source_net.state_dict()[k].cpu().numpy().ravel().astype(np.float64)
        ek, er, mx = np.abs(got - pm).max(), np.abs(pr - pm).max(), np.abs(pm).max()
        print(f"{k}: e_k {ek:.3e} e_ref {er:.3e} ratio {ek / (er + 2 * U * mx):.2f}")
        assert ek <= 4 * er + 8 * U * mx, k
        gk = tr.source_net.get_parameter(k).grad.cpu().numpy().ravel().astype(np.float64)
        gm, gr = np.clip(out["grads"][k].ravel(), -1, 1), np.clip(p.grad.numpy().ravel(), -1, 1)
        assert np.abs(gk - gm).max() <= 4 * np.abs(gr - gm).max() + 8 * U * np.abs(gm).max(), k
        off += size


@gpu
def test_stored_snapshots_are_the_state_the_trainer_acted_from():
    """No update in L + 1 vector steps (train_every beyond the horizon): snapshot j of every
    stored episode is the (h, c) its instance held before the vector step at which t = j T, in
    the slot mz_drqn_store gave the episode; slots beyond the count are untouched."""
    env, tr = _mk(memory_size=4096, train_every=10 ** 9, window=T)
    assert tr.snaps == 17 and tr.mem_state.shape == (4096, 17, 64)
    tr.mem_state.fill_(float("nan"))
    cur = [dict() for _ in range(B)]
    stored = 0
    for _ in range(tr.L + 1):
        t0 = tr.t.cpu().numpy().copy()
        h0, c0 = tr.h.cpu().numpy().copy(), tr.c.cpu().numpy().copy()
        head = int(tr.ring[0])
        tr.vector_step()
        t1 = tr.t.cpu().numpy()
        for i in range(B):
            if t0[i] > 0 and t0[i] % T == 0:
                cur[i][t0[i] // T] = np.concatenate([h0[:, i], c0[:, i]])
        done = [i for i in range(B) if t1[i] == 0 and t0[i] >= 1]  # (1-step episodes are dropped)
        ms = tr.mem_state.cpu().numpy()
        for k, i in enumerate(done):
            n = t0[i] + 1
            assert int(tr.mem_len[head + k]) == n
            for j in range(1, W.windows_in(n, T)):
                assert np.array_equal(ms[head + k, j], cur[i][j]), (i, n, j)
                stored += 1
            assert np.isnan(ms[head + k, W.windows_in(n, T):]).all() and np.isnan(ms[head + k, 0]).all()
        for i in range(B):
            if t1[i] == 0:
                cur[i] = dict()
        assert int(tr.ring[0]) == head + len(done)
    count = int(tr.ring[1])
    assert stored > 0 and 0 < count < 4096 and torch.isnan(tr.mem_state[count:]).all()
    print(f"{count} episodes, {stored} snapshots checked")


@gpu
@pytest.mark.parametrize("K,mode", [(0, "stored"), (4, "stored"), (4, "zero")])
def test_checkpoint_restored_into_a_fresh_trainer_continues_bit_identically(tmp_path, K, mode):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    kw = dict(target_update_frequency=4, window=T, burn_in=K, initial_state=mode)
    env, tr = _mk(**kw)
    for _ in range(60):
        tr.vector_step()
    assert tr.updates > 8 and int((tr.t > T).sum()) > 0
    path = save_checkpoint(str(tmp_path / "drqn.pt"), tr)
    env2, tr2 = _mk(env_seed=0x5EED0D99, seed=5, **kw)
    load_checkpoint(path, tr2)
    assert _same(_state(tr), _state(tr2))
    if tr.stored:
        assert all(np.array_equal(a, b) for a, b in zip(_live_snaps(tr), _live_snaps(tr2)))
    for _ in range(20):
        tr.vector_step()
        tr2.vector_step()
    assert tr.updates == tr2.updates and tr.steps_done == tr2.steps_done
    assert _same(_state(tr), _state(tr2))
    assert torch.equal(tr.wdir, tr2.wdir)
    if tr.stored:
        assert all(np.array_equal(a, b) for a, b in zip(_live_snaps(tr), _live_snaps(tr2)))


@gpu
def test_two_trainers_with_the_same_seed_are_bit_identical():
    kw = dict(window=T, burn_in=4)
    _, a = _mk(seed=3, **kw)
    _, b = _mk(seed=3, **kw)
    _, c = _mk(seed=4, **kw)
    _, z = _mk(seed=3, initial_state="zero", **kw)
    for _ in range(50):
        for tr in (a, b, c, z):
            tr.vector_step()
    assert a.updates == b.updates > 0
    assert _same(_state(a), _state(b)) and not _same(_state(a), _state(c))
    assert torch.equal(a.wdir, b.wdir)
    # stored state is not zero state: the same draws, another loss
    assert not torch.equal(a.source_net._flat_params, z.source_net._flat_params)


@gpu
def test_window_none_is_the_trainer_without_the_arguments():
    _, a = _mk(seed=3)
    _, b = _mk(seed=3, window=None, burn_in=0, initial_state="zero")
    for _ in range(50):
        a.vector_step()
        b.vector_step()
    assert a.updates == b.updates > 0 and _same(_state(a), _state(b))
    for tr in (a, b):
        assert not tr.stored and not hasattr(tr, "wdir") and not hasattr(tr, "snap_rec")
        assert tr.qmax.numel() == 4 * (tr.L + 1)
    assert set(a.state_dict()) == set(b.state_dict()) and "window" not in a.state_dict()


@gpu
def test_a_checkpoint_with_other_window_settings_is_refused():
    made = {}
    for name, kw in [("none", {}), ("w4", dict(window=T)), ("w4k4", dict(window=T, burn_in=4)),
                     ("w4zero", dict(window=T, initial_state="zero")), ("w2", dict(window=2))]:
        made[name] = _mk(train_every=10 ** 9, **kw)[1]
        made[name].vector_step()
    sds = {k: tr.state_dict() for k, tr in made.items()}
    for a in made:
        for b in made:
            if a == b:
                made[b].load_state_dict(sds[a])
            else:
                with pytest.raises(ValueError, match="replay windows"):
                    made[b].load_state_dict(sds[a])
    old = dict(sds["none"])  # a checkpoint from before the option: no "window" key at all
    assert "window" not in old
    made["none"].load_state_dict(old)


def test_constructor_refuses_bad_window_arguments_without_a_gpu():
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    bad = [dict(window=0), dict(window=-4), dict(window=4, burn_in=-4), dict(window=4, burn_in=6),
           dict(burn_in=4), dict(window=4, initial_state="snapshot"), dict(window=4.0),
           dict(window=4, burn_in=4.0), dict(initial_state=None), dict(window=True)]
    for kw in bad:
        with pytest.raises(ValueError, match="window"):
            VectorRecurrentDQNTrainer(None, "cpu", **kw)
