"""VectorRecurrentDQNTrainer (trainers/drqn_trainer.py) on the GPU: 64 instances of 9x9 plain
(enrich=False) mazes, L = episode_bound(9), euclidean and one case on the torus. The bounds are
tests/test_drqn_gpu.py's: e_k <= 4 e_ref + 8 u max|tensor| with torch's float32 CPU path as the
reference beside the float64 model (tests/drqn_model.py)."""
import numpy as np
import pytest
import torch

import drqn_model as M
import learner_model as LM

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
B, DIM = 64, 9


def _mk(tor=False, env_seed=0x5EED0D00, **kw):
    import mazerl
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    env = mazerl.VectorMazeEnv(B, DIM, toroidal=tor, enrich=False, device=DEV, seed=env_seed)
    kw.setdefault("bank", False)
    kw.setdefault("memory_size", 256)
    kw.setdefault("batch_size", 4)
    kw.setdefault("epsilon_decay", 200.0)
    return env, VectorRecurrentDQNTrainer(env, DEV, **kw)


def _state(tr):
    o = tr.opt
    return [t.clone() for t in (tr.source_net._flat_params, tr.target_net._flat_params, o.exp_avg,
                                o.exp_avg_sq, o._step_buf, tr.h, tr.c, tr.t, tr.ring, tr.mem,
                                tr.mem_len, tr.mem_term, tr.stats, tr.env.obs6, tr.loss)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("tor", [False, True])
def test_stored_episodes_replay_through_a_second_env(tor):
    """After L + 1 vector steps (every instance has finished an episode) every stored episode
    equals the trajectory the recorded actions give in a second env with the same seed."""
    import mazerl
    env, tr = _mk(tor, memory_size=4096, train_every=10 ** 9)
    env2 = mazerl.VectorMazeEnv(B, DIM, toroidal=tor, enrich=False, device=DEV, seed=0x5EED0D00)
    assert tr.L == 65 or tor
    cur = [dict(x=[], a=[], r=[]) for _ in range(B)]
    want, finished = [], np.zeros(B, bool)
    for _ in range(tr.L + 1):
        x = env2.obs6.cpu().numpy().copy()
        assert np.array_equal(x, env.obs6.cpu().numpy())
        tr.vector_step()
        a = tr.act_out.clone()
        env2.step(a)
        a = a.cpu().numpy()
        r, term = env2.reward.cpu().numpy(), env2.terminated.cpu().numpy()
        trunc, xn = env2.truncated.cpu().numpy(), env2.obs6.cpu().numpy().copy()
        for i in range(B):
            c = cur[i]
            c["x"].append(x[i]), c["a"].append(a[i]), c["r"].append(r[i])
            if term[i] or trunc[i]:
                finished[i] = True
                if len(c["a"]) >= 2:  # mz_ppo_scan drops 1-step episodes
                    want.append(dict(x=np.array(c["x"] + [xn[i]]), a=np.array(c["a"]),
                                     r=np.array(c["r"], np.float32), term=bool(term[i])))
                cur[i] = dict(x=[], a=[], r=[])
        env2.reset_done(regen_won=True)
    assert finished.all()
    head, count = (int(v) for v in tr.ring.cpu())
    assert count == len(want) == head and 0 < count < 4096
    assert tr.episodes == count + int(tr.stats[2]) and int(tr.stats[3]) == 0
    mem, ln, tm = tr.mem.cpu().numpy(), tr.mem_len.cpu().numpy(), tr.mem_term.cpu().numpy()
    for s, ep in enumerate(want):
        n = len(ep["a"])
        assert ln[s] == n and bool(tm[s]) == ep["term"], s
        assert np.array_equal(mem[s, :n + 1, :6].view(np.float32), ep["x"]), s
        assert np.array_equal(mem[s, :n, 6], ep["a"]) and \
            np.array_equal(mem[s, :n, 7].view(np.float32), ep["r"]), s
    print(f"toroidal {tor}: {count} episodes, {sum(e['term'] for e in want)} terminated, "
          f"longest {max(len(e['a']) for e in want)} steps")


def _episodes(tr):
    """The episodes of the last update's directory, read back from the memory."""
    slots, lens = tr.d_slot.cpu().numpy(), tr.d_len.cpu().numpy()
    mem, tm = tr.mem.cpu().numpy(), tr.mem_term.cpu().numpy()
    assert len(set(slots.tolist())) == len(slots) and (lens == tr.mem_len.cpu().numpy()[slots]).all()
    return [dict(x=mem[s, :n + 1, :6].view(np.float32).copy(), a=mem[s, :n, 6].astype(np.int64),
                 r=mem[s, :n, 7].view(np.float32).copy(), term=bool(tm[s]))
            for s, n in zip(slots, lens)]


def test_one_vector_step_is_flat_adamw_on_the_model_gradient():
    """train_every = 1, E = 4, after 12 updates (the second moments carry history, so the step is
    well conditioned in the gradient): one more vector_step gives the parameters
    learner_model.adamw_step gives from the gradient drqn_model computes on the sampled slots."""
    from mazerl.agents.lstm_dqn_agent import DQN, td_loss
    from mazerl.agents.rf_agent import cosine_lr
    env, tr = _mk(lr=1e-3, target_update_frequency=5)
    for _ in range(400):
        tr.vector_step()
        if tr.updates == 12:
            break
    assert tr.updates == 12
    keys = list(M.KEYS)
    src = {k: v.detach().cpu().clone() for k, v in tr.source_net.state_dict().items()}
    tgt = {k: v.detach().cpu().clone() for k, v in tr.target_net.state_dict().items()}
    m0, v0 = tr.opt.exp_avg.cpu().numpy().copy(), tr.opt.exp_avg_sq.cpu().numpy().copy()
    step0 = float(tr.opt._step_buf[0])
    assert step0 == 12.0
    tr.vector_step()
    assert tr.updates == 13
    lr = cosine_lr(12, 1e-3, 30, 1e-6)
    assert tr.last_lr == lr and float(tr.opt.param_groups[0]["lr"]) == np.float32(lr)
    eps = _episodes(tr)
    steps = sum(len(e["a"]) for e in eps)
    assert int(tr.d_tot[1]) == steps and int(tr.d_tot[0]) == steps + len(eps)
    out = M.td_loss(M.as_f64({k: v.numpy() for k, v in src.items()}),
                    M.as_f64({k: v.numpy() for k, v in tgt.items()}), eps, tr.gamma)
    ns, nt = DQN(6, 4, 32, torch.device("cpu")), DQN(6, 4, 32, torch.device("cpu"))
    ns.load_state_dict(src), nt.load_state_dict(tgt)
    loss = td_loss(ns, nt, [(torch.from_numpy(e["x"]), torch.from_numpy(e["a"]),
                             torch.from_numpy(e["r"]), e["term"]) for e in eps], tr.gamma)
    loss.backward()
    e_k, e_ref = abs(float(tr.loss) - out["loss"]), abs(loss.item() - out["loss"])
    print(f"loss: e_k {e_k:.3e} e_ref {e_ref:.3e}")
    assert e_k <= 4 * e_ref + 8 * U * abs(out["loss"])
    off = 0
    for k, p, size in zip(keys, ns.parameters(), tr.source_net._flat_sizes):
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
        # the clamped gradient left in .grad (FlatAdamW writes it back) against the model's
        gk = tr.source_net.get_parameter(k).grad.cpu().numpy().ravel().astype(np.float64)
        gm, gr = np.clip(out["grads"][k].ravel(), -1, 1), np.clip(p.grad.numpy().ravel(), -1, 1)
        assert np.abs(gk - gm).max() <= 4 * np.abs(gr - gm).max() + 8 * U * np.abs(gm).max(), k
        off += size


def test_target_sync_and_learning_rate_schedule():
    from mazerl.agents.rf_agent import cosine_lr
    env, tr = _mk(lr=2e-3, target_update_frequency=3)
    flat_s, flat_t = tr.source_net._flat_params, tr.target_net._flat_params
    assert torch.equal(flat_s, flat_t)  # the target starts as a copy
    seen = 0
    for _ in range(400):
        tr.vector_step()
        if tr.updates == seen:
            assert seen > 0 or tr.filled < tr.batch_size
            continue
        seen = tr.updates
        lr = cosine_lr(seen - 1, 2e-3, 30, 1e-6)
        assert float(tr.opt.param_groups[0]["lr"]) == np.float32(lr)
        assert torch.equal(flat_s, flat_t) == (seen % 3 == 0), seen
        if seen == 35:  # past T_max = 30: the rate rises again, as the reference's scheduler
            break
    assert seen == 35
    assert cosine_lr(30, 2e-3, 30, 1e-6) == pytest.approx(1e-6) and cosine_lr(31, 2e-3, 30, 1e-6) > 1e-6


def test_epsilon_clock_and_update_steps_done():
    from mazerl.agents.lstm_dqn_agent import epsilon_at
    env, tr = _mk(train_every=10 ** 9, starting_epsilon=0.9, final_epsilon=0.05)
    for k in range(7):
        assert tr.steps_done == k and tr.epsilon() == epsilon_at(k, 0.9, 0.05, 200.0)
        tr.vector_step()
    tr.update_steps_done()
    assert tr.steps_done == 3 and tr.counter == 7


def test_checkpoint_restored_into_a_fresh_trainer_continues_bit_identically(tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    env, tr = _mk(target_update_frequency=4)
    for _ in range(60):
        tr.vector_step()
    assert tr.updates > 8 and int((tr.t > 0).sum()) > 0
    path = save_checkpoint(str(tmp_path / "drqn.pt"), tr)
    env2, tr2 = _mk(target_update_frequency=4, env_seed=0x5EED0D99, seed=5)
    load_checkpoint(path, tr2)
    assert _same(_state(tr), _state(tr2))
    for _ in range(20):
        tr.vector_step()
        tr2.vector_step()
    assert tr.updates == tr2.updates and tr.steps_done == tr2.steps_done
    assert _same(_state(tr), _state(tr2))
    assert torch.equal(tr.rec_x[:, :tr.L][tr._live(tr.L)], tr2.rec_x[:, :tr.L][tr2._live(tr.L)])


def test_two_trainers_with_the_same_seed_are_bit_identical():
    _, a = _mk(seed=3)
    _, b = _mk(seed=3)
    _, c = _mk(seed=4)
    for _ in range(50):
        a.vector_step()
        b.vector_step()
        c.vector_step()
    assert a.updates == b.updates > 0
    assert _same(_state(a), _state(b)) and not _same(_state(a), _state(c))


def test_evaluator_state_is_zero_after_reset_and_follows_the_model():
    from mazerl.agents.lstm_dqn_agent import DQN
    env, tr = _mk(train_every=10 ** 9)
    torch.manual_seed(21)
    net = DQN(6, 4, 32, torch.device("cpu"))
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
        tr.source_net.load_state_dict(net.state_dict())
    P = M.as_f64({k: v.detach().numpy() for k, v in net.state_dict().items()})
    ev = tr.evaluator()
    rng = np.random.default_rng(22)
    n = 37
    for rollout in range(2):
        h = c = np.zeros((n, 32))
        rh = rc = torch.zeros(n, 32)
        for k in range(3):
            x = rng.random((n, 6)).astype(np.float32)
            h, c, _ = M.cell(P, x.astype(np.float64), h, c)
            mq = M.head(P, h)
            with torch.no_grad():
                rh, rc = net.lstm_cell(torch.from_numpy(x), (rh, rc))
                rq = net.fc(rh).numpy()
            bound = 4 * np.abs(rq - mq).max() + 8 * U * np.abs(mq).max()
            top = np.sort(mq, axis=1)
            assert ((top[:, 3] - top[:, 2]) > 2 * bound).all()
            a = ev.greedy(torch.from_numpy(x).to(DEV), None, None)
            assert a.dtype == torch.int64 and np.array_equal(a.cpu().numpy(), mq.argmax(axis=1))
            for name, got, mod, ref in (("h", ev.h, h, rh), ("c", ev.c, c, rc)):
                g = got.cpu().numpy().T.astype(np.float64)
                ek, er = np.abs(g - mod).max(), np.abs(ref.numpy() - mod).max()
                print(f"rollout {rollout} step {k} {name}: e_k {ek:.3e} e_ref {er:.3e}")
                assert ek <= 4 * er + 8 * U * np.abs(mod).max()
        ev.reset()
        assert not ev.h.any() and not ev.c.any() and not ev.t.any()
