"""VectorRecurrentDQNPopulation with replay windows (window=T shared, burn_in and initial_state per
learner) on the GPU: 64 instances of 9x9 plain mazes per learner, E = 4, T = 4. Learner p is
defined as VectorRecurrentDQNTrainer(window=T, burn_in=K_p, initial_state=S_p) on its block, which
tests/test_drqn_window_trainer_gpu.py holds to the model, so every comparison here is `==` on the
bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIM, b, T = 9, 64, 4
KW = dict(bank=False, memory_size=64, batch_size=4, epsilon_decay=200.0)


def _env(B, seed=0x5EED0D00):
    import mazerl
    return mazerl.VectorMazeEnv(B, DIM, toroidal=False, enrich=False, device=DEV, seed=seed)


def _pop(P, env_seed=0x5EED0D00, per=b, **kw):
    from mazerl.trainers import VectorRecurrentDQNPopulation
    env = _env(P * per, env_seed)
    return env, VectorRecurrentDQNPopulation(env, DEV, learners=P, **{**KW, **kw})


def _learner(tr, p):
    """Everything that belongs to learner p."""
    s = slice(p * tr.b, (p + 1) * tr.b)
    own = [tr.src[p], tr.tgt[p], tr.exp_avg[p], tr.exp_avg_sq[p], tr.step[p], tr.ring[p],
           tr.mem[p], tr.mem_len[p], tr.mem_term[p], tr.h[:, s], tr.c[:, s], tr.t[s], tr.loss[p],
           tr.env.obs6[s]]
    if tr.window is not None and tr.stored[p]:
        n = int(tr.ring[p, 1])
        own += [tr.mem_state[p, :n, 1:], tr.snap_rec[s]]
    return [t.clone() for t in own] + [torch.tensor([tr.steps_done[p], tr.updates[p]])]


def _state(tr):
    return [x for p in range(tr.P) for x in _learner(tr, p)] + [tr.stats.clone()]


def _same(a, c):
    def bits(t):
        return t.contiguous().reshape(-1).view(torch.uint8)
    return len(a) == len(c) and all(x.shape == y.shape and x.dtype == y.dtype and
                                    torch.equal(bits(x), bits(y)) for x, y in zip(a, c))


@pytest.mark.parametrize("K,S", [(0, "stored"), (4, "stored"), (4, "zero")])
def test_one_learner_is_the_single_windowed_trainer_bit_for_bit(K, S):
    """Target sync every 3 updates (two syncs in 8 updates), one update_steps_done() on the way:
    both nets, the moments, the ring and its contents, the state memory, the in-flight snapshots,
    (h, c), the records, the window directory and the counters."""
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    kw = dict(KW, target_update_frequency=3, lr=2e-3, seed=9, window=T, burn_in=K, initial_state=S)
    env1 = _env(b)
    one = VectorRecurrentDQNTrainer(env1, DEV, **kw)
    _, pop = _pop(1, **kw)
    assert pop.L == one.L and torch.equal(pop.src[0], one.source_net._flat_params[:5252])
    assert pop.qmax.shape == (1, 4 * (T + 2)) and hasattr(pop, "mem_state") == (S == "stored")
    halved = False
    for k in range(300):
        one.vector_step()
        pop.vector_step()
        if one.updates == 2 and not halved:
            one.update_steps_done()
            pop.update_steps_done()
            halved = True
        if one.updates >= 8:  # target syncs after updates 3 and 6
            break
    assert halved and one.updates == 8 and one.steps_done < one.counter
    o = one.opt
    pairs = [(pop.src[0], one.source_net._flat_params[:5252]),
             (pop.tgt[0], one.target_net._flat_params[:5252]),
             (pop.exp_avg[0], o.exp_avg[:5252]), (pop.exp_avg_sq[0], o.exp_avg_sq[:5252]),
             (pop.step, o._step_buf), (pop.ring[0], one.ring), (pop.mem[0], one.mem),
             (pop.mem_len[0], one.mem_len), (pop.mem_term[0], one.mem_term), (pop.h, one.h),
             (pop.c, one.c), (pop.t, one.t), (pop.loss, one.loss), (pop.stats, one.stats),
             (pop.rec_x, one.rec_x), (pop.rec_a, one.rec_a), (pop.rec_r, one.rec_r),
             (pop.wdir[0], one.wdir), (pop.d_off[0], one.d_off), (pop.d_tot[0], one.d_tot),
             (pop.qa[0], one.qa), (pop.gpart[0], one.gpart), (pop.env.obs6, env1.obs6)]
    if S == "stored":
        pairs += [(pop.mem_state[0], one.mem_state), (pop.snap_rec, one.snap_rec)]
        assert int((one.mem_state != 0).sum()) > 0
    for j, (x, y) in enumerate(pairs):
        assert _same([x], [y]), j
    assert (pop.steps_done[0], pop.counter, pop.updates[0], pop.filled[0]) == \
        (one.steps_done, one.counter, one.updates, one.filled)
    assert pop.last_lr[0] == one.last_lr and pop.epsilon(0) == one.epsilon()
    assert not torch.equal(pop.src[0], pop.tgt[0])  # two updates past the last sync


def test_learners_are_independent():
    """P = 3, no bank: a second run with only learner 1's burn_in (0 -> 4), initial_state and seed
    changed leaves everything of learners 0 and 2 as it was, and changes learner 1's nets."""
    runs = []
    for K1, S1, seed1 in ((0, "stored", 1), (4, "zero", 77)):
        _, tr = _pop(3, window=T, burn_in=[0, K1, 4], initial_state=["stored", S1, "stored"],
                     seed=[0, seed1, 2], target_update_frequency=[2, 3, 4])
        for _ in range(40):
            tr.vector_step()
        assert min(tr.updates) > 3, tr.updates
        runs.append(tr)
    x, y = runs
    for p in (0, 2):
        assert _same(_learner(x, p), _learner(y, p)), p
        assert torch.equal(x.wdir[p], y.wdir[p]) and torch.equal(x.rec_a[p * b:(p + 1) * b],
                                                                 y.rec_a[p * b:(p + 1) * b])
    assert not torch.equal(x.src[1], y.src[1]) and not torch.equal(x.tgt[1], y.tgt[1])
    assert int((x.wdir[:, 3] > 0).sum()) > 0 or int((y.wdir[:, 3] > 0).sum()) > 0  # burn-in ran


def test_staggered_start():
    """P = 2, one learner acting greedily and one at random, so their rings reach E episodes at
    different vector steps: each learner's parameters keep their initial bits until its own first
    due step, updates[p] counts its due steps and the device's optimizer step count equals it.
    8 instances per learner, tests/test_drqn_pop_trainer_gpu.py's shape: with 64 per learner each
    block holds six mazes of the shortest step limit, and both rings reach E = 6 at the step those
    truncate (19 and 19)."""
    _, tr = _pop(2, per=8, batch_size=6, starting_epsilon=[0.0, 1.0], final_epsilon=[0.0, 1.0],
                 seed=[4, 5], window=T, burn_in=[4, 0], initial_state=["stored", "zero"])
    init = tr.src.clone()
    due_steps, first = [0, 0], [None, None]
    for k in range(200):
        before = tr.src.clone()
        tr.vector_step()
        for p in range(2):
            if tr.last_due[p]:
                due_steps[p] += 1
                if first[p] is None:
                    first[p] = k
                    assert torch.equal(before[p], init[p]), p
                assert not torch.equal(tr.src[p], before[p]), p
            else:
                assert torch.equal(tr.src[p], before[p]), p
        if min(due_steps) >= 3:
            break
    print(f"first due steps {first}, due steps {due_steps}")
    assert min(due_steps) >= 3 and first[0] != first[1], (first, due_steps)
    assert tr.updates == due_steps
    assert tr.step.tolist() == [float(n) for n in due_steps]


def test_window_none_is_the_population_of_before():
    """The default and an explicit window=None: the same bits over the same run, no window
    buffers, and a checkpoint with the keys of before (none of the window's)."""
    kw = dict(lr=[1e-3, 2e-3], seed=[3, 4], target_update_frequency=[4, 3])
    _, plain = _pop(2, **kw)
    _, none = _pop(2, window=None, burn_in=0, initial_state="stored", **kw)
    for _ in range(40):
        plain.vector_step()
        none.vector_step()
    assert min(plain.updates) > 4 and _same(_state(plain), _state(none))
    for tr in (plain, none):
        assert tr.window is None and not any(hasattr(tr, k) for k in
                                             ("wdir", "snap_rec", "mem_state", "burn_in_dev"))
        assert tr.qmax.shape == (2, 4 * (tr.L + 1))
        assert set(tr.memory_bytes()) == {"replay", "records", "update", "total"}
    sa, sb = plain.state_dict(), none.state_dict()
    assert list(sa) == list(sb) and not {"window", "snap_rec", "mem_state"} & set(sa)
    _, win = _pop(2, window=T, burn_in=[0, 4], **kw)
    assert set(win.state_dict()) - set(sa) == {"window", "snap_rec", "mem_state"}
    _, zero = _pop(2, window=T, initial_state="zero", **kw)
    assert set(zero.state_dict()) - set(sa) == {"window"} and not hasattr(zero, "mem_state")
    mb = win.memory_bytes()
    snaps = (win.L - 1) // T + 1
    assert mb["state"] == 2 * 64 * snaps * 256 and mb["snap_rec"] == 2 * b * snaps * 256
    assert mb["update"] < plain.memory_bytes()["update"]  # E (T + 2) rows, not E (L + 1)


def test_checkpoint_resume_same_seed_repeatability_and_mismatched_settings(tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    kw = dict(lr=[1e-3, 2e-3], seed=[3, 4], target_update_frequency=[4, 3], window=T,
              burn_in=[4, 0], initial_state=["stored", "zero"])
    _, tr = _pop(2, **kw)
    _, twin = _pop(2, **kw)
    for _ in range(30):
        tr.vector_step()
        twin.vector_step()
    assert min(tr.updates) > 4 and int((tr.t > 0).sum()) > 0
    assert _same(_state(tr), _state(twin))  # the same seeds: the same bits
    path = save_checkpoint(str(tmp_path / "pop.pt"), tr)
    _, tr2 = _pop(2, env_seed=0x5EED0D99, **dict(kw, seed=[8, 9]))
    assert not _same(_state(tr), _state(tr2))
    load_checkpoint(path, tr2)
    assert _same(_state(tr), _state(tr2)) and tr2.seed == [3, 4]
    for _ in range(15):
        tr.vector_step()
        tr2.vector_step()
    assert tr.updates == tr2.updates and tr.steps_done == tr2.steps_done
    assert _same(_state(tr), _state(tr2)) and torch.equal(tr.wdir, tr2.wdir)
    live = tr._live(tr.L)
    assert torch.equal(tr.rec_x[:, :tr.L][live], tr2.rec_x[:, :tr.L][live])
    # a population with other window settings refuses the checkpoint
    for other in (dict(burn_in=[4, 4]), dict(initial_state=["stored", "stored"]),
                  dict(window=2, burn_in=[4, 0]), dict(window=None, burn_in=0,
                                                       initial_state="stored")):
        _, tr3 = _pop(2, **dict(kw, **other))
        with pytest.raises(ValueError, match="replay windows"):
            load_checkpoint(path, tr3)


def test_evaluate_all_is_unaffected_by_windows():
    from mazerl.agents.lstm_dqn_agent import DQN
    _, plain = _pop(2, seed=[1, 2], train_every=10 ** 9)
    _, win = _pop(2, seed=[1, 2], train_every=10 ** 9, window=T, burn_in=[0, 4],
                  initial_state=["zero", "stored"])
    for p, s in enumerate((100, 101)):  # two nets that win a few of the 256 mazes greedily
        torch.manual_seed(s)
        net = DQN(6, 4, 32, torch.device("cpu"))
        with torch.no_grad():
            for q in net.parameters():
                q.mul_(16.0)
        plain.load_learner(p, net.state_dict())
        win.load_learner(p, net.state_dict())
    for _ in range(3):
        win.vector_step()
    rates = win.evaluate_all(256, DIM, seed=0x7E57)
    print(f"rates {rates}")
    assert rates == plain.evaluate_all(256, DIM, seed=0x7E57) and min(rates) > 0
