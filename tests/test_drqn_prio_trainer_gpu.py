"""VectorRecurrentDQNTrainer with prioritized replay windows (window=4, burn_in 0 or 4, stored or
zero state, priority_alpha=0.9, priority_beta=0.6) on the GPU: 64 instances of 9x9 plain mazes,
L = episode_bound(9) = 65. The bounds are tests/test_drqn_window_trainer_gpu.py's: e_k <= 4 e_ref +
8 u max|tensor| with torch's float32 CPU path as the reference beside the float64 model
(tests/drqn_prio_model.py); the sampler is compared with the integer model bit for bit."""
import numpy as np
import pytest
import torch

import drqn_model as M
import drqn_prio_model as PM
import drqn_window_model as W
import learner_model as LM

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
B, DIM, T = 64, 9, 4
PRIO = dict(priority_alpha=0.9, priority_beta=0.6)


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
    n = int(tr.ring[1])
    ts = [tr.source_net._flat_params, tr.target_net._flat_params, o.exp_avg, o.exp_avg_sq,
          o._step_buf, tr.h, tr.c, tr.t, tr.ring, tr.mem, tr.mem_len, tr.mem_term, tr.stats,
          tr.env.obs6, tr.loss]
    if tr.stored:
        ts += [tr.mem_state[:n]]
    if tr.priority_alpha is not None:
        ts += [tr.mem_prio[:n], tr.mem_psum[:n], tr.prio_max]
    return [t.clone() for t in ts]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _psum_holds(tr):
    prio = tr.mem_prio.cpu().numpy().astype(np.int64)
    lens = tr.mem_len.cpu().numpy()
    n = int(tr.ring[1])
    assert np.array_equal(tr.mem_psum.cpu().numpy(), prio.sum(axis=1))
    nw = np.where(lens > 0, (lens - 1) // T + 1, 0)
    filled = np.arange(tr.snaps)[None, :] < nw[:, None]
    assert (prio[filled] >= 1).all() and (prio[~filled] == 0).all() and (prio[n:] == 0).all()
    assert prio.max() <= int(tr.prio_max) or n == 0


def _spy(tr, seen):
    """Keep what the sampler reads: the masses, sums and prio_max between the store and the update."""
    orig = tr.sample

    def sample():
        seen["prio"] = tr.mem_prio.cpu().numpy().astype(np.int64)
        seen["pmax"] = int(tr.prio_max)
        seen["updates"] = tr.updates
        orig()
    tr.sample = sample


def _windows(tr):
    """The windows of the last update's directory, read back from the memory (a window, or an
    episode, may come twice)."""
    slot, n, b, k, m = tr.wdir.cpu().numpy()
    mem, tm = tr.mem.cpu().numpy(), tr.mem_term.cpu().numpy()
    state = tr.mem_state.cpu().numpy() if tr.stored else None
    assert (n == tr.mem_len.cpu().numpy()[slot]).all()
    ws = []
    for e, s in enumerate(slot):
        ep = dict(x=mem[s, :n[e] + 1, :6].view(np.float32).copy(), a=mem[s, :n[e], 6].astype(np.int64),
                  r=mem[s, :n[e], 7].view(np.float32).copy(), term=bool(tm[s]))
        j = (b[e] + k[e]) // T
        w = W.window_of(ep, T, tr.burn_in, j, None if state is None else state[s])
        assert (w["b"], w["k"], w["m"]) == (b[e], k[e], m[e])
        ws.append(w)
    return ws


@pytest.mark.parametrize("K,mode", [(0, "stored"), (4, "stored"), (4, "zero"), (0, "zero")])
def test_one_vector_step_is_flat_adamw_on_the_weighted_model_gradient(K, mode):
    """train_every = 1, E = 4, after 12 updates: one more vector_step samples the integer model's
    windows from the masses of that moment, writes the model's masses back, and gives the
    parameters learner_model.adamw_step gives from the weighted model's gradient."""
    from mazerl.agents.lstm_dqn_agent import DQN, window_td_loss
    from mazerl.agents.rf_agent import cosine_lr
    env, tr = _mk(lr=1e-3, target_update_frequency=5, window=T, burn_in=K, initial_state=mode, **PRIO)
    assert tr.mem_prio.shape == (256, tr.snaps) and int(tr.prio_max) == PM.ONE
    seen = {}
    _spy(tr, seen)
    for _ in range(400):
        tr.vector_step()
        _psum_holds(tr)
        if tr.updates == 12:
            break
    assert tr.updates == 12
    src = {k: v.detach().cpu().clone() for k, v in tr.source_net.state_dict().items()}
    tgt = {k: v.detach().cpu().clone() for k, v in tr.target_net.state_dict().items()}
    m0, v0 = tr.opt.exp_avg.cpu().numpy().copy(), tr.opt.exp_avg_sq.cpu().numpy().copy()
    step0 = float(tr.opt._step_buf[0])
    tr.vector_step()
    assert tr.updates == 13 and seen["updates"] == 12
    lr = cosine_lr(12, 1e-3, 30, 1e-6)
    assert tr.last_lr == lr
    # the sampler: the model on the masses it read
    wdir = tr.wdir.cpu().numpy()
    sm = PM.sample(seen["prio"], tr.mem_len.cpu().numpy(), tr.seed, 12, 4, T, K, 0.6)
    for row, key in enumerate(("slot", "n", "b", "k", "m")):
        assert np.array_equal(wdir[row], np.array(sm[key])), key
    isw = tr.isw.cpu().numpy()
    want = sm["isw"].astype(np.float32)
    assert (np.abs(isw.astype(np.float64) - want) <= np.spacing(want)).all()
    ws = _windows(tr)
    steps = sum(w["m"] for w in ws)
    assert int(tr.d_tot[1]) == steps and int(tr.d_tot[0]) == steps + 2 * len(ws)
    print(f"K {K} {mode}: windows (slot, b, k, m) "
          f"{[(int(s), w['b'], w['k'], w['m']) for s, w in zip(wdir[0], ws)]}, weights {isw}")
    # the write-back: the masses from the forward's own residuals, the sums, the running max
    off = tr.d_off.cpu().numpy()
    qa, y = tr.qa.cpu().numpy(), tr.y.cpu().numpy()
    prio = tr.mem_prio.cpu().numpy().astype(np.int64)
    js = (wdir[2] + wdir[3]) // T
    masses = [PM.mass_of(np.abs(qa[o + 1:o + 1 + w["m"]] - y[o + 1:o + 1 + w["m"]]), 0.9, 0.9, 1e-3)
              for o, w in zip(off, ws)]
    assert (np.abs(prio[wdir[0], js] - np.array(masses)) <= 1).all()
    touched = np.zeros_like(prio, bool)
    touched[wdir[0], js] = True
    assert np.array_equal(prio[~touched], seen["prio"][~touched])
    assert int(tr.prio_max) == max(seen["pmax"], int(prio[wdir[0], js].max()))
    _psum_holds(tr)
    # the optimizer step
    wts = isw.astype(np.float64)
    out = PM.weighted_td_loss(M.as_f64({k: v.numpy() for k, v in src.items()}),
                              M.as_f64({k: v.numpy() for k, v in tgt.items()}), ws, tr.gamma, wts)
    ns, nt = DQN(6, 4, 32, torch.device("cpu")), DQN(6, 4, 32, torch.device("cpu"))
    ns.load_state_dict(src), nt.load_state_dict(tgt)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
    loss = window_td_loss(ns, nt, [(t32(w["x"]), torch.from_numpy(w["a"]), t32(w["r"]), t32(w["h0"]),
                                    t32(w["c0"]), w["k"], w["term"]) for w in ws], tr.gamma,
                          weights=torch.from_numpy(isw))
    loss.backward()
    e_k, e_ref = abs(float(tr.loss) - out["loss"]), abs(loss.item() - out["loss"])
    print(f"loss: e_k {e_k:.3e} e_ref {e_ref:.3e}")
    assert e_k <= 4 * e_ref + 8 * U * abs(out["loss"])
    o = 0
    for k, p, size in zip(M.KEYS, ns.parameters(), tr.source_net._flat_sizes):
        n = p.numel()
        args = (lr, step0, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0)
        pm = LM.adamw_step(src[k].numpy().ravel(), out["grads"][k].ravel(), m0[o:o + n],
                           v0[o:o + n], *args)[0]
        pr = LM.adamw_step(src[k].numpy().ravel(), p.grad.numpy().ravel(), m0[o:o + n],
                           v0[o:o + n], *args)[0]
        got = tr.source_net.state_dict()[k].cpu().numpy().ravel().astype(np.float64)
        ek, er, mx = np.abs(got - pm).max(), np.abs(pr - pm).max(), np.abs(pm).max()
        print(f"{k}: e_k {ek:.3e} e_ref {er:.3e} ratio {ek / (er + 2 * U * mx):.2f}")
        assert ek <= 4 * er + 8 * U * mx, k
        gk = tr.source_net.get_parameter(k).grad.cpu().numpy().ravel().astype(np.float64)
        gm, gr = np.clip(out["grads"][k].ravel(), -1, 1), np.clip(p.grad.numpy().ravel(), -1, 1)
        assert np.abs(gk - gm).max() <= 4 * np.abs(gr - gm).max() + 8 * U * np.abs(gm).max(), k
        o += size
    f = tr._log_fields()
    assert f["prio_max"] == int(tr.prio_max) / PM.ONE and abs(f["mean_weight"] - float(isw.mean())) <= 4 * U


def test_new_episodes_enter_at_the_current_prio_max():
    """Every vector step: the episodes the step stored hold, when the sampler runs (or after the
    step where no update is due), the prio_max of before the step on their ceil(n / T) windows
    and zero beyond; the sums hold after every step. The ring (64 slots) wraps several times."""
    env, tr = _mk(memory_size=64, window=T, burn_in=4, **PRIO)
    seen = {}
    _spy(tr, seen)
    entered, raised = 0, 0
    for _ in range(120):
        head, pmax = int(tr.ring[0]), int(tr.prio_max)
        seen.clear()
        tr.vector_step()
        _psum_holds(tr)
        prio = seen.get("prio", tr.mem_prio.cpu().numpy().astype(np.int64))
        lens = tr.mem_len.cpu().numpy()
        count = (int(tr.ring[0]) - head) % 64  # (never all 64 instances in one step)
        for slot in [(head + k) % 64 for k in range(count)]:
            nw = (lens[slot] - 1) // T + 1
            assert (prio[slot, :nw] == pmax).all() and (prio[slot, nw:] == 0).all(), (slot, pmax)
        entered += count
        raised += int(tr.prio_max) > pmax
    assert entered > 64 and raised > 0 and int(tr.prio_max) > PM.ONE
    print(f"{entered} episodes entered, prio_max rose {raised} times to {int(tr.prio_max) / PM.ONE:.3f}")


@pytest.mark.parametrize("K,mode", [(0, "stored"), (4, "stored"), (4, "zero")])
def test_checkpoint_restored_into_a_fresh_trainer_continues_bit_identically(tmp_path, K, mode):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    kw = dict(target_update_frequency=4, window=T, burn_in=K, initial_state=mode,
              priority_alpha=0.9, priority_beta=(0.4, 1.0, 1000))
    env, tr = _mk(**kw)
    for _ in range(60):
        tr.vector_step()
    assert tr.updates > 8 and int(tr.prio_max) != PM.ONE
    path = save_checkpoint(str(tmp_path / "drqn.pt"), tr)
    env2, tr2 = _mk(env_seed=0x5EED0D99, seed=5, **kw)
    load_checkpoint(path, tr2)
    assert _same(_state(tr), _state(tr2))
    for _ in range(20):
        tr.vector_step()
        tr2.vector_step()
    assert tr.updates == tr2.updates and tr.beta() == tr2.beta() and 0.4 < tr.beta() < 1.0
    assert _same(_state(tr), _state(tr2))
    assert torch.equal(tr.wdir, tr2.wdir) and torch.equal(tr.isw, tr2.isw)


def test_two_trainers_with_the_same_seed_are_bit_identical():
    kw = dict(window=T, burn_in=4, **PRIO)
    _, a = _mk(seed=3, **kw)
    _, b = _mk(seed=3, **kw)
    _, c = _mk(seed=4, **kw)
    _, u = _mk(seed=3, window=T, burn_in=4)
    for _ in range(50):
        for tr in (a, b, c, u):
            tr.vector_step()
    assert a.updates == b.updates > 0
    assert _same(_state(a), _state(b)) and not _same(_state(a), _state(c))
    assert torch.equal(a.wdir, b.wdir) and torch.equal(a.isw, b.isw)
    # prioritized is not uniform: the same seed, other windows, another net
    assert not torch.equal(a.source_net._flat_params, u.source_net._flat_params)


def test_priority_alpha_none_is_the_trainer_without_the_arguments():
    _, a = _mk(seed=3, window=T, burn_in=4)
    _, b = _mk(seed=3, window=T, burn_in=4, priority_alpha=None, priority_beta=0.3,
               priority_eta=0.5, priority_eps=0.1)
    for _ in range(50):
        a.vector_step()
        b.vector_step()
    assert a.updates == b.updates > 0 and _same(_state(a), _state(b))
    assert torch.equal(a.wdir, b.wdir) and torch.equal(a.mem_state, b.mem_state)
    for tr in (a, b):
        assert tr.priority_alpha is None
        assert not any(hasattr(tr, k) for k in ("mem_prio", "mem_psum", "prio_max", "isw"))
        assert set(tr._log_fields()) == {"loss"}
    assert set(a.state_dict()) == set(b.state_dict())
    assert not {"priority", "mem_prio", "mem_psum", "prio_max"} & set(a.state_dict())


def test_a_checkpoint_with_other_priority_settings_is_refused():
    made = {}
    for name, kw in [("none", {}), ("a9", dict(priority_alpha=0.9)), ("a0", dict(priority_alpha=0.0)),
                     ("b4", dict(priority_alpha=0.9, priority_beta=0.4)),
                     ("sched", dict(priority_alpha=0.9, priority_beta=(0.6, 1.0, 100))),
                     ("eta", dict(priority_alpha=0.9, priority_eta=0.5)),
                     ("eps", dict(priority_alpha=0.9, priority_eps=1e-2))]:
        made[name] = _mk(train_every=10 ** 9, window=T, **kw)[1]
        made[name].vector_step()
    sds = {k: tr.state_dict() for k, tr in made.items()}
    assert {"priority", "mem_prio", "mem_psum", "prio_max"} <= set(sds["a9"])
    for a in made:
        for b in made:
            if a == b:
                made[b].load_state_dict(sds[a])
            else:
                with pytest.raises(ValueError, match="prioritized replay"):
                    made[b].load_state_dict(sds[a])
    old = dict(sds["none"])  # a checkpoint from before the option: no "priority" key at all
    assert "priority" not in old
    made["none"].load_state_dict(old)
