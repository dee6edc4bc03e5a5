"""VectorRecurrentDQNTrainer and VectorRecurrentDQNPopulation with double_q and n_step on the GPU:
64 instances of 9x9 plain mazes per learner, E = 4, windows of T = 4 steps or whole episodes. The
single trainer is held to the float64 model (tests/drqn_nstep_model.py) under the project's bound
e_k <= 4 e_ref + 8 u max|tensor|; a population's learner is defined as the single trainer with its
arguments on its block, so those comparisons are `==` on the bits."""
import numpy as np
import pytest
import torch

import drqn_model as M
import drqn_nstep_model as NM
import learner_model as LM
from test_drqn_window_trainer_gpu import T, _mk, _same, _state, _windows

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
b, DIM, ENV_SEED = 64, 9, 0x5EED0D00


def _episodes(tr):
    """The whole episodes of the last update's directory, read back from the memory, as spans."""
    slot, n = tr.d_slot.cpu().numpy(), tr.d_len.cpu().numpy()
    mem, tm = tr.mem.cpu().numpy(), tr.mem_term.cpu().numpy()
    return [NM.episode_span(dict(x=mem[s, :k + 1, :6].view(np.float32).copy(),
                                 a=mem[s, :k, 6].astype(np.int64),
                                 r=mem[s, :k, 7].view(np.float32).copy(), term=bool(tm[s])))
            for s, k in zip(slot, n)]


@pytest.mark.parametrize("dq,N,window,K", [(True, 3, T, 4), (True, 1, T, 0), (False, 5, T, 4),
                                            (True, 3, None, 0)])
def test_one_vector_step_is_flat_adamw_on_the_model_gradient(dq, N, window, K):
    """train_every = 1, E = 4, after 12 updates: one more vector_step gives the parameters
    learner_model.adamw_step gives from the model's gradient on the batch the sampler drew. The
    argmax is a constant of the loss and the C ABI tests hold it to the model where the inputs
    separate the two best actions; here the model bootstraps from the trainer's own sel rows, and
    those must be the model's argmax wherever its top-two gap is above 1000 times the bound."""
    from mazerl.agents.lstm_dqn_agent import DQN
    from mazerl.agents.rf_agent import cosine_lr
    env, tr = _mk(lr=1e-3, target_update_frequency=5, window=window, burn_in=K, double_q=dq,
                  n_step=N)
    rows = 4 * (T + 2) if window else 4 * (tr.L + 1)
    assert tr.q4.shape == (rows, 4) and tr.sel.shape == (rows,) and tr.sel.dtype == torch.int32
    assert tr.n_step_dev.tolist() == [N] and tr.double_dev.tolist() == [int(dq)]
    for _ in range(400):
        tr.vector_step()
        if tr.updates == 12:
            break
    assert tr.updates == 12
    src = {k: v.detach().cpu().clone() for k, v in tr.source_net.state_dict().items()}
    tgt = {k: v.detach().cpu().clone() for k, v in tr.target_net.state_dict().items()}
    m0, v0 = tr.opt.exp_avg.cpu().numpy().copy(), tr.opt.exp_avg_sq.cpu().numpy().copy()
    step0 = float(tr.opt._step_buf[0])
    tr.vector_step()
    assert tr.updates == 13 and step0 == 12.0
    lr = cosine_lr(12, 1e-3, 30, 1e-6)
    assert tr.last_lr == lr
    ws = _windows(tr) if window else _episodes(tr)
    off = tr.d_off.cpu().numpy() + (1 if window else 0)
    sel_dev = tr.sel.cpu().numpy()
    given = [sel_dev[o:o + len(w["a"]) + 1] for o, w in zip(off, ws)]
    assert all(set(g.tolist()) <= {0, 1, 2, 3} for g in given)
    f64 = lambda sd: M.as_f64({k: v.numpy() for k, v in sd.items()})  # noqa: E731
    out = NM.nstep_td_loss(f64(src), f64(tgt), ws, tr.gamma, dq, N, given=given)
    ns, nt = DQN(6, 4, 32, torch.device("cpu")), DQN(6, 4, 32, torch.device("cpu"))
    ns.load_state_dict(src), nt.load_state_dict(tgt)
    ref = NM.torch_nstep(ns, nt, ws, tr.gamma, dq, N, given=given)
    qa_m = np.concatenate(out["qa"])
    need = 1000 * (4 * np.abs(ref["qa"] - qa_m).max() + 8 * U * np.abs(qa_m).max())
    clear = [g >= need for g in out["gap"]]
    print(f"rows with a clear argmax: {sum(int(c.sum()) for c in clear)} of "
          f"{sum(len(c) for c in clear)}")
    assert sum(int(c.sum()) for c in clear) > 0
    for c, g, s in zip(clear, given, out["sel"]):
        assert np.array_equal(g[c], s[c])
    e_k, e_ref = abs(float(tr.loss) - out["loss"]), abs(ref["loss"] - out["loss"])
    print(f"loss: e_k {e_k:.3e} e_ref {e_ref:.3e}")
    assert e_k <= 4 * e_ref + 8 * U * abs(out["loss"])
    o = 0
    for k, p, size in zip(M.KEYS, ns.parameters(), tr.source_net._flat_sizes):
        n = p.numel()
        args = (lr, step0, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0)
        pm = LM.adamw_step(src[k].numpy().ravel(), out["grads"][k].ravel(), m0[o:o + n],
                           v0[o:o + n], *args)[0]
        pr = LM.adamw_step(src[k].numpy().ravel(), ref["grads"][k].ravel(), m0[o:o + n],
                           v0[o:o + n], *args)[0]
        got = tr.source_net.state_dict()[k].cpu().numpy().ravel().astype(np.float64)
        ek, er, mx = np.abs(got - pm).max(), np.abs(pr - pm).max(), np.abs(pm).max()
        print(f"{k}: e_k {ek:.3e} e_ref {er:.3e} ratio {ek / (er + 2 * U * mx):.2f}")
        assert ek <= 4 * er + 8 * U * mx, k
        gk = tr.source_net.get_parameter(k).grad.cpu().numpy().ravel().astype(np.float64)
        gm, gr = np.clip(out["grads"][k].ravel(), -1, 1), np.clip(ref["grads"][k].ravel(), -1, 1)
        assert np.abs(gk - gm).max() <= 4 * np.abs(gr - gm).max() + 8 * U * np.abs(gm).max(), k
        o += size
    env.close()


@pytest.mark.parametrize("window", [None, T])
def test_the_defaults_are_the_trainer_without_the_arguments(window):
    kw = dict(window=window, burn_in=4) if window else {}
    _, a = _mk(seed=3, **kw)
    _, c = _mk(seed=3, double_q=False, n_step=1, **kw)
    _, n3 = _mk(seed=3, n_step=3, **kw)
    for _ in range(50):
        for tr in (a, c, n3):
            tr.vector_step()
    assert a.updates == c.updates > 0 and _same(_state(a), _state(c))
    for tr in (a, c):
        assert not hasattr(tr, "q4") and not hasattr(tr, "sel") and not hasattr(tr, "n_step_dev")
        assert tr.double_q is False and tr.n_step == 1
    assert set(a.state_dict()) == set(c.state_dict()) and "returns" not in c.state_dict()
    assert n3.updates == a.updates and not _same(_state(a), _state(n3))  # another target
    with pytest.raises(ValueError, match="n_step"):
        a.n_step = 3  # the default update has no launch that reads it
    n3.n_step = 2
    assert n3.n_step == 2 and n3.n_step_dev.tolist() == [2]
    with pytest.raises(ValueError, match="n_step"):
        n3.n_step = 0
    assert n3.n_step == 2


PER = dict(seed=[0, 1, 2, 3], double_q=[False, True, False, True], n_step=[1, 1, 3, 5],
           priority_alpha=[None, None, 0.9, None], burn_in=[4, 0, 4, 4],
           initial_state=["stored", "stored", "stored", "zero"],
           target_update_frequency=[2, 3, 4, 2])
KW = dict(bank=False, memory_size=64, batch_size=4, epsilon_decay=200.0, window=T)


def _env(B, seed=ENV_SEED):
    import mazerl
    return mazerl.VectorMazeEnv(B, DIM, toroidal=False, enrich=False, device=DEV, seed=seed)


def _pop(per=PER, env_seed=ENV_SEED, **kw):
    from mazerl.trainers import VectorRecurrentDQNPopulation
    return VectorRecurrentDQNPopulation(_env(4 * b, env_seed), DEV, learners=4, **{**KW, **per, **kw})


def _single(p, per=PER):
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    return VectorRecurrentDQNTrainer(_env(b, ENV_SEED + p * b), DEV,
                                     **dict(KW, **{k: v[p] for k, v in per.items()}))


def _pop_state(tr, rows=True):
    """What a checkpoint carries and, with rows, the last update's directory and row buffers."""
    out = [tr.stats, tr.src, tr.tgt, tr.exp_avg, tr.exp_avg_sq, tr.step, tr.ring, tr.mem,
           tr.mem_len, tr.mem_term, tr.h, tr.c, tr.t, tr.loss, tr.env.obs6, tr.mem_prio,
           tr.mem_psum, tr.prio_max, torch.tensor([tr.steps_done, tr.updates])]
    if rows:
        out += [tr.wdir, tr.y, tr.d, tr.sel, tr.q4]
    return [t.clone() for t in out]


def test_learner_p_is_the_single_trainer_with_its_settings_bit_for_bit():
    """(double_q, n_step) = (0, 1), (1, 1), (0, 3), (1, 5), learner 2 prioritized, until every
    learner has updated at least 8 times (target syncs included). Learner 0 is at the defaults:
    its single trainer runs the old chain."""
    pop = _pop()
    ones = [_single(p) for p in range(4)]
    assert not hasattr(ones[0], "q4") and all(hasattr(o, "q4") for o in ones[1:])
    assert pop.q4.shape == (4, 4 * (T + 2), 4) and pop.n_step_dev.tolist() == [1, 1, 3, 5]
    assert pop.double_dev.tolist() == [0, 1, 0, 1] and pop.prio == [False, False, True, False]
    for k in range(300):
        pop.vector_step()
        for one in ones:
            one.vector_step()
        if min(pop.updates) >= 8:
            break
    print(f"vector steps {k + 1}, updates {pop.updates}, log {pop._log_fields()}")
    assert min(pop.updates) >= 8
    for p, one in enumerate(ones):
        s, o = slice(p * b, (p + 1) * b), one.opt
        pairs = [(pop.src[p], one.source_net._flat_params[:5252]),
                 (pop.tgt[p], one.target_net._flat_params[:5252]),
                 (pop.exp_avg[p], o.exp_avg[:5252]), (pop.exp_avg_sq[p], o.exp_avg_sq[:5252]),
                 (pop.step[p:p + 1], o._step_buf), (pop.ring[p], one.ring), (pop.mem[p], one.mem),
                 (pop.mem_len[p], one.mem_len), (pop.mem_term[p], one.mem_term),
                 (pop.h[:, s], one.h), (pop.c[:, s], one.c), (pop.t[s], one.t),
                 (pop.loss[p:p + 1], one.loss), (pop.wdir[p], one.wdir), (pop.d_off[p], one.d_off),
                 (pop.d_tot[p], one.d_tot), (pop.qa[p], one.qa), (pop.y[p], one.y),
                 (pop.d[p], one.d), (pop.ep_loss[p], one.ep_loss), (pop.gpart[p], one.gpart),
                 (pop.stash[p], one.stash), (pop.env.obs6[s], one.env.obs6)]
        if p:
            pairs += [(pop.q4[p], one.q4), (pop.sel[p], one.sel)]
        if pop.prio[p]:
            pairs += [(pop.mem_prio[p], one.mem_prio), (pop.mem_psum[p], one.mem_psum),
                      (pop.prio_max[p:p + 1], one.prio_max), (pop.isw[p], one.isw)]
        for j, (x, y) in enumerate(pairs):
            assert _same([x], [y]), (p, j)
        assert (pop.steps_done[p], pop.updates[p]) == (one.steps_done, one.updates)
    m2 = pop.mem_prio[2]
    assert bool(((m2 != 0) & (m2 != 1 << 20)).any())  # masses that follow the new residuals
    for t in [pop] + ones:
        t.env.close()


def test_checkpoint_resume_and_mismatched_settings(tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    pop = _pop()
    for _ in range(60):
        pop.vector_step()
    assert min(pop.updates) > 4
    sd = pop.state_dict()
    assert sd["returns"] == {"double_q": PER["double_q"], "n_step": PER["n_step"]}
    path = save_checkpoint(str(tmp_path / "pop.pt"), pop)
    other = _pop(env_seed=0x5EED0D99, per=dict(PER, seed=[9, 8, 7, 6]))
    load_checkpoint(path, other)
    assert _same(_pop_state(pop, False), _pop_state(other, False))
    for _ in range(20):
        pop.vector_step()
        other.vector_step()
    assert pop.updates == other.updates and _same(_pop_state(pop), _pop_state(other))
    # a single trainer: the key is there only off the defaults, and decides what loads
    made = {name: _mk(train_every=10 ** 9, window=T, **kw)[1] for name, kw in
            [("default", {}), ("double", dict(double_q=True)), ("n3", dict(n_step=3)),
             ("double-n3", dict(double_q=True, n_step=3))]}
    for tr in made.values():
        tr.vector_step()
    sds = {k: tr.state_dict() for k, tr in made.items()}
    assert "returns" not in sds["default"]
    assert sds["double-n3"]["returns"] == {"double_q": True, "n_step": 3}
    for a in made:
        for c in made:
            if a == c:
                made[c].load_state_dict(sds[a])
            else:
                with pytest.raises(ValueError, match="targets"):
                    made[c].load_state_dict(sds[a])
    with pytest.raises(ValueError, match="targets"):  # and a population's other lists
        _pop(per=dict(PER, n_step=[1, 1, 3, 3])).load_state_dict(sd)
    for t in [pop, other] + list(made.values()):
        t.env.close()


def test_single_trainer_checkpoint_continues_bit_identically(tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    kw = dict(target_update_frequency=4, window=T, burn_in=4, double_q=True, n_step=3)
    env, tr = _mk(**kw)
    for _ in range(60):
        tr.vector_step()
    assert tr.updates > 8
    path = save_checkpoint(str(tmp_path / "drqn.pt"), tr)
    env2, tr2 = _mk(env_seed=0x5EED0D99, seed=5, **kw)
    load_checkpoint(path, tr2)
    assert _same(_state(tr), _state(tr2))
    for _ in range(20):
        tr.vector_step()
        tr2.vector_step()
    assert tr.updates == tr2.updates and _same(_state(tr), _state(tr2))
    assert torch.equal(tr.sel, tr2.sel) and torch.equal(tr.y, tr2.y)
