"""VectorRecurrentDQNPopulation (trainers/drqn_population.py) on the GPU, 9x9 plain mazes,
L = episode_bound(9). Learner p is defined as VectorRecurrentDQNTrainer on its block, which
tests/test_drqn_trainer_gpu.py holds to the float64 model, so every comparison here is `==` on the
bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIM = 9
KW = dict(bank=False, memory_size=64, batch_size=4, epsilon_decay=200.0)


def _env(B, seed=0x5EED0D00):
    import mazerl
    return mazerl.VectorMazeEnv(B, DIM, toroidal=False, enrich=False, device=DEV, seed=seed)


def _pop(B, P, env_seed=0x5EED0D00, **kw):
    from mazerl.trainers import VectorRecurrentDQNPopulation
    env = _env(B, env_seed)
    return env, VectorRecurrentDQNPopulation(env, DEV, learners=P, **{**KW, **kw})


def _learner(tr, p):
    """Everything that belongs to learner p."""
    s = slice(p * tr.b, (p + 1) * tr.b)
    return [t.clone() for t in (tr.src[p], tr.tgt[p], tr.exp_avg[p], tr.exp_avg_sq[p],
                                tr.step[p], tr.ring[p], tr.mem[p], tr.mem_len[p], tr.mem_term[p],
                                tr.h[:, s], tr.c[:, s], tr.t[s], tr.loss[p], tr.env.obs6[s])] + \
        [torch.tensor([tr.steps_done[p], tr.updates[p]])]


def _state(tr):
    return [x for p in range(tr.P) for x in _learner(tr, p)] + [tr.stats.clone()]


def _same(a, b):
    def bits(t):
        return t.contiguous().reshape(-1).view(torch.uint8)
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and
                                    torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_one_learner_is_the_single_trainer_bit_for_bit():
    """B = 32, E = 4, capacity 64, target sync every 3 updates, one update_steps_done() on the way:
    both nets, the moments, the ring and its contents, (h, c) and the counters."""
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    kw = dict(KW, target_update_frequency=3, lr=2e-3, seed=9)
    env1 = _env(32)
    one = VectorRecurrentDQNTrainer(env1, DEV, **kw)
    _, pop = _pop(32, 1, **kw)
    assert pop.L == one.L and torch.equal(pop.src[0], one.source_net._flat_params[:5252])
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
             (pop.rec_x, one.rec_x), (pop.rec_a, one.rec_a), (pop.d_slot[0], one.d_slot),
             (pop.env.obs6, env1.obs6)]
    for j, (a, b) in enumerate(pairs):
        assert _same([a], [b]), j
    assert (pop.steps_done[0], pop.counter, pop.updates[0], pop.filled[0]) == \
        (one.steps_done, one.counter, one.updates, one.filled)
    assert pop.last_lr[0] == one.last_lr and pop.epsilon(0) == one.epsilon()
    assert not torch.equal(pop.src[0], pop.tgt[0])  # two updates past the last sync


def test_learners_are_independent():
    """P = 3, b = 16, no bank: a second run with only learner 1's lr and seed changed leaves
    everything of learners 0 and 2 as it was, and changes learner 1's nets."""
    runs = []
    for lr1, seed1 in ((1e-3, 1), (3e-3, 77)):
        _, tr = _pop(48, 3, lr=[1e-3, lr1, 2e-3], seed=[0, seed1, 2],
                     target_update_frequency=[2, 3, 4])
        for _ in range(80):
            tr.vector_step()
        assert min(tr.updates) > 3, tr.updates
        runs.append(tr)
    a, b = runs
    for p in (0, 2):
        assert _same(_learner(a, p), _learner(b, p)), p
    assert not torch.equal(a.src[1], b.src[1]) and not torch.equal(a.tgt[1], b.tgt[1])


def test_staggered_start():
    """P = 2, one learner acting greedily and one at random, so their rings reach E episodes at
    different vector steps: each learner's parameters keep their initial bits until its own first
    due step, updates[p] counts its due steps and the device's optimizer step count equals it."""
    _, tr = _pop(16, 2, batch_size=6, starting_epsilon=[0.0, 1.0], final_epsilon=[0.0, 1.0],
                 seed=[4, 5])
    init = tr.src.clone()
    due_steps, first = [0, 0], [None, None]
    for k in range(150):
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


def test_checkpoint_resume_and_same_seed_repeatability(tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    kw = dict(lr=[1e-3, 2e-3], seed=[3, 4], target_update_frequency=[4, 3])
    _, tr = _pop(32, 2, **kw)
    _, twin = _pop(32, 2, **kw)
    for _ in range(60):
        tr.vector_step()
        twin.vector_step()
    assert min(tr.updates) > 4 and int((tr.t > 0).sum()) > 0
    assert _same(_state(tr), _state(twin))  # the same seeds: the same bits
    path = save_checkpoint(str(tmp_path / "pop.pt"), tr)
    _, tr2 = _pop(32, 2, env_seed=0x5EED0D99, lr=[1e-3, 2e-3], seed=[8, 9],
                  target_update_frequency=[4, 3])
    assert not _same(_state(tr), _state(tr2))
    load_checkpoint(path, tr2)
    assert _same(_state(tr), _state(tr2)) and tr2.seed == [3, 4]
    for _ in range(20):
        tr.vector_step()
        tr2.vector_step()
    assert tr.updates == tr2.updates and tr.steps_done == tr2.steps_done
    assert _same(_state(tr), _state(tr2))
    live = tr._live(tr.L)
    assert torch.equal(tr.rec_x[:, :tr.L][live], tr2.rec_x[:, :tr.L][live])


def test_evaluate_all_and_learner_state_dicts():
    from mazerl.agents.lstm_dqn_agent import DQN
    from mazerl.trainers.drqn_trainer import evaluate_plain
    _, tr = _pop(24, 3, seed=[1, 2, 3], train_every=10 ** 9)
    for p, s in enumerate((100, 101, 107)):  # three nets that win a few of the 256 mazes greedily
        torch.manual_seed(s)
        net = DQN(6, 4, 32, torch.device("cpu"))
        with torch.no_grad():
            for q in net.parameters():
                q.mul_(16.0)
        tr.load_learner(p, net.state_dict())
    for _ in range(3):  # (the acting state of a run in flight must not leak into an evaluation)
        tr.vector_step()
    sd = tr.learner_state_dict(1)
    net = DQN(6, 4, 32, torch.device("cpu"))
    assert list(sd) == list(net.state_dict())
    net.load_state_dict(sd)
    assert torch.equal(torch.cat([q.detach().reshape(-1) for q in net.parameters()]),
                       tr.src[1].cpu())
    distinct = tr.evaluate_all(256, DIM, seed=0x7E57)
    singles = [evaluate_plain(tr.evaluator(p), 256, DIM, seed=0x7E57, device=DEV)[0]
               for p in range(3)]
    print(f"rates {distinct}")
    assert distinct == singles  # every learner plays evaluate_plain's mazes
    assert min(distinct) > 0 and len(set(distinct)) == 3
    for p in range(3):
        tr.load_learner(p, sd)
    assert torch.equal(tr.src[0], tr.src[1]) and torch.equal(tr.src[2], tr.src[1])
    rates = tr.evaluate_all(256, DIM, seed=0x7E57)
    assert rates[0] == rates[1] == rates[2] == singles[1]
    assert tr.memory_bytes()["replay"] == 3 * 64 * ((tr.L + 1) * 32 + 8)
