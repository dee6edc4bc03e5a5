"""The episodic trainers' explored-maze pool (trainers/episodic.py: VectorPPOTrainer,
VectorReinforceTrainer, VectorRecurrentDQNTrainer with archive=) on the GPU: attaching the pool
changes nothing in the run, the pool holds what the reference env's `env.mazes` would hold (every
instance's first maze, then each winner's new one, step by step and in instance order), the
growth rule (a winner past max_shape appends nothing), evaluate_explored against an evaluation on
the same mazes, and checkpoints. Every comparison is exact."""
import numpy as np
import pytest
import torch

from test_vector_trainer_pool_gpu import assert_entry, host_entry

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_PRIM = 0  # vector_env.ALGOS["r-prim"]

# kind -> (instances, maze size, growth of test (c), vector steps T)
SHAPE = {"ppo": (256, 15, (15, 23), 64), "reinforce": (256, 15, (15, 23), 64),
         "drqn": (64, 9, (9, 17), 150)}
kinds = pytest.mark.parametrize("kind", list(SHAPE))


def guide(head, K=12.0):
    """Hand-set weights for a Linear - LeakyReLU - Linear - LeakyReLU - Linear(4) head over
    [conv features | obs6]: everything zero but a path from obs6's last two entries, "best dir" =
    agent - best next cell (br, bc), to the logits (-K' br, K' br, -K' bc, K' bc), K' = K (1 +
    alpha)^2 — LeakyReLU(x) - LeakyReLU(-x) = (1 + alpha) x carries the sign through. Action 0 / 1
    moves a row down / up and 2 / 3 a column right / left (mz_common.h), so the policy steps
    along the shortest path and its episodes end in wins; acting uniformly at random wins a
    15 x 15 maze about once in 10^5 steps."""
    l1, l2, l3 = head[0], head[2], head[4]
    with torch.no_grad():
        for lin in (l1, l2, l3):
            lin.weight.zero_()
            lin.bias.zero_()
        d0 = l1.weight.shape[1]
        for j, (col, sign) in enumerate(((d0 - 2, 1.0), (d0 - 2, -1.0), (d0 - 1, 1.0), (d0 - 1, -1.0))):
            l1.weight[j, col] = sign
        for j, (plus, minus) in enumerate(((0, 1), (1, 0), (2, 3), (3, 2))):
            l2.weight[j, plus], l2.weight[j, minus] = 1.0, -1.0
        for a, (plus, minus) in enumerate(((1, 0), (0, 1), (3, 2), (2, 3))):
            l3.weight[a, plus], l3.weight[a, minus] = K, -K


def guided_lstm(K=4.0, sign=1.0):
    """A state_dict for the recurrent DQN's LSTMCell(6, 32) + Linear(32, 4) that follows obs6's
    "best dir" (br, bc) as guide() does: no recurrence (W_hh = 0, the forget gates shut, the input
    and output gates open by their biases), cell 0 / 1 = tanh(br) / tanh(bc), and Q = (-K h0, K h0,
    -K h1, K h1) — odd functions all the way, so the greedy action is the step along the shortest
    path. Acting uniformly at random wins a 9 x 9 maze about once in 60,000 steps. sign = -1 walks
    away from the goal."""
    w_ih, w_hh = torch.zeros(128, 6), torch.zeros(128, 32)
    b_ih, b_hh = torch.zeros(128), torch.zeros(128)
    b_ih[0:32], b_ih[32:64], b_ih[96:128] = 10.0, -10.0, 10.0  # gates i, f, o (order i, f, g, o)
    w_ih[64, 4], w_ih[65, 5] = 1.0, 1.0                         # g0 = tanh(br), g1 = tanh(bc)
    fc_w = torch.zeros(4, 32)
    fc_w[0, 0], fc_w[1, 0], fc_w[2, 1], fc_w[3, 1] = -K * sign, K * sign, -K * sign, K * sign
    return {"lstm_cell.weight_ih": w_ih, "lstm_cell.weight_hh": w_hh, "lstm_cell.bias_ih": b_ih,
            "lstm_cell.bias_hh": b_hh, "fc.weight": fc_w, "fc.bias": torch.zeros(4)}


def _trainer(kind, env_seed, seed, archive=None, growth=None, num=None, bank=None):
    """PPO / REINFORCE on euclidean Enrich 15 x 15 mazes with a small head whose initial weights
    follow the observation's best direction (guide), so that their episodes end in wins; the
    recurrent DQN on 64 plain 9 x 9 mazes with such a net too (guided_lstm) and epsilon 0.3. The
    maze bank is on under growth (it holds every size) and off otherwise."""
    import mazerl
    from mazerl.trainers.vector_trainer import make_env
    B, dim, _, _ = SHAPE[kind]
    B = num or B
    pitch = growth[1] if growth else dim
    kw = dict(seed=seed, archive=archive, growth=growth, bank=bool(growth) if bank is None else bank)
    if kind == "drqn":
        from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
        env = mazerl.VectorMazeEnv(B, dim, toroidal=False, enrich=False, device=DEV, seed=env_seed,
                                   max_dim=pitch, done_list=False)
        from mazerl.agents.flat import copy_flat
        t = VectorRecurrentDQNTrainer(env, DEV, memory_size=256, batch_size=4, lr=1e-4,
                                      starting_epsilon=0.3, final_epsilon=0.3, **kw)
        with torch.no_grad():
            t.source_net.load_state_dict(guided_lstm())
        copy_flat(t.target_net, t.source_net)
        return t
    env = make_env(B, dim, seed=env_seed, device=DEV, max_dim=pitch, done_list=False,
                   reward64=True, window=False, window_bits=True)
    if kind == "ppo":
        from mazerl.trainers.ppo_trainer import VectorPPOTrainer
        t = VectorPPOTrainer(env, DEV, hidden_dim=64, batch_size=256, ppo_steps=2,
                             pool_size=1024, **kw)
        guide(t.net.actor_head)
        return t
    from mazerl.trainers.reinforce_trainer import VectorReinforceTrainer
    t = VectorReinforceTrainer(env, DEV, hidden_dim=64, update_rows=512, batch_size=512, **kw)
    guide(t.net.fc)
    return t


def same(x, y, path="sd"):
    """x and y — nested dicts / lists of tensors, numbers, strings — are equal to the bit."""
    if torch.is_tensor(x):
        assert torch.is_tensor(y) and x.shape == y.shape and x.dtype == y.dtype, path
        bits = lambda t: t.detach().contiguous().reshape(-1).view(torch.uint8)  # noqa: E731
        assert torch.equal(bits(x), bits(y.to(x.device))), path
    elif isinstance(x, dict):
        assert isinstance(y, dict) and list(x) == list(y), path
        for k in x:
            same(x[k], y[k], f"{path}[{k!r}]")
    elif isinstance(x, (list, tuple)):
        assert isinstance(y, (list, tuple)) and len(x) == len(y), path
        for j, (a, b) in enumerate(zip(x, y)):
            same(a, b, f"{path}[{j}]")
    else:
        assert x == y, path


def assert_same_runs(a, b, pools=False):
    """The whole checkpoint but the env's raw device state — parameters, optimizer moments,
    in-flight records, update pool or replay ring, counters, schedule — and the env through its
    observations, flags and mazes' meta words."""
    torch.cuda.synchronize()
    sa, sb = a.state_dict(), b.state_dict()
    for sd in (sa, sb):
        del sd["env"]
        if not pools:
            sd.pop("archive", None)
    same(sa, sb)
    assert torch.equal(a.env.meta(), b.env.meta())
    assert torch.equal(a.env.terminated, b.env.terminated)
    assert torch.equal(a.env.truncated, b.env.truncated)
    assert a.counter == b.counter and a.updates == b.updates
    assert torch.equal(a.stats, b.stats) and torch.equal(a.t, b.t)
    assert torch.equal(a.env.obs6, b.env.obs6)
    if a.env.window_bits is not None:
        assert torch.equal(a.env.window_bits, b.env.window_bits)


def watch_winners(t):
    """The step's terminated flags as the reset sees them, kept per reset_done call: the winners
    of every vector step, taken beside the trainer's own recording."""
    seen, real = [], t.env.reset_done

    def reset_done(*a, **k):
        seen.append(t.env.terminated.clone())
        return real(*a, **k)
    t.env.reset_done = reset_done
    return seen


# (a) the pool changes nothing
@kinds
def test_the_pool_changes_nothing_in_the_run(kind):
    B, dim, _, T = SHAPE[kind]
    a = _trainer(kind, 0xA11CE, 3, archive=16 * B)
    b = _trainer(kind, 0xA11CE, 3, archive=None)
    assert b.archive is None and "archive" not in b.state_dict() and b.summary()["archive"] is None
    sd = a.state_dict()
    assert set(sd) - set(b.state_dict()) == {"archive"}
    del sd["archive"]
    b.load_state_dict(sd)
    for t in (a, b):
        t.train(T)
    assert_same_runs(a, b)
    print(kind, "wins:", a.wins, "updates:", a.updates)
    assert a.wins >= 4 and a.updates >= 1 and "archive" not in b.state_dict()
    s = a.summary()
    assert s["vector_steps"] == T
    assert s["archive"] == {"capacity": 16 * B, "recorded": B + a.wins, "held": B + a.wins,
                            "dropped": 0}
    # a pool of another env, or a set of pools where one pool is kept, is refused
    from mazerl.archive import MazePoolSet
    for bad in (a.archive, MazePoolSet(b.env, 2, 8)):
        with pytest.raises(ValueError):
            type(b)(b.env, DEV, archive=bad)
    a.env.close()
    b.env.close()


# (b) it records what env.mazes would hold
@kinds
def test_the_pool_records_what_env_mazes_would_hold(kind):
    """Observed on an MI355X with these seeds: PPO 442 winners over 46 of the 64 vector steps (the
    first 4 in step 14), REINFORCE 565 over 49 of 64 (the first 4 in step 14), the recurrent DQN
    496 over 137 of 150 (the first 2 in step 10); the test prints the winners per step. At least 4
    winners over at least 2 vector steps are asserted below."""
    B, dim, _, T = SHAPE[kind]
    t = _trainer(kind, 0xA11CE, 3, archive=16 * B)
    env, pool = t.env, t.archive
    first = [host_entry(env, i, dim, R_PRIM) for i in range(B)]
    assert int(pool.count) == B
    for i in (0, 1, 63, B // 2, B - 1):
        assert_entry(pool, i, first[i], i, 0)
    assert np.array_equal(pool.bits[:B].cpu().numpy(), np.stack([e[0] for e in first]))
    assert pool.owner[:B].tolist() == list(range(B)) and not pool.stamp[:B].any()
    flags = watch_winners(t)
    seen, per_step = B, []
    for k in range(T):
        t.vector_step()
        assert len(flags) == k + 1 and t.counter == k + 1
        winners = torch.nonzero(flags[k]).reshape(-1).tolist()
        assert int(pool.count) == seen + len(winners)
        for r, i in enumerate(winners):  # their new mazes, in ascending id
            assert_entry(pool, seen + r, host_entry(env, i, dim, R_PRIM), i, t.counter)
        seen += len(winners)
        per_step.append(len(winners))
    print(kind, "winners per vector step:", per_step)
    assert sum(per_step) >= 4 and sum(1 for w in per_step if w) >= 2
    assert sum(per_step) == t.wins
    # the first B entries are still the initial mazes
    assert np.array_equal(pool.bits[:B].cpu().numpy(), np.stack([e[0] for e in first]))
    assert not pool.stamp[:B].any() and not pool.bits[seen:].any()
    env.close()


# (c) growth
@kinds
def test_growth_a_winner_at_the_maximum_size_appends_nothing(kind):
    """The schedule of every odd instance is put at the maximum size before the run (their mazes
    keep the start size, so they win as often as the others): their next size is 0 and a win of
    theirs must append nothing, while an even winner's new maze of the next size is appended.
    Observed on an MI355X (printed below): PPO 176 winners moved and 235 won at the maximum size,
    sizes 15, 19, 23 in the pool; REINFORCE 119 and 145, sizes 15, 19, 23; the recurrent DQN 64
    and 365, sizes 9, 13, 17. Asserted: at least 2 winners of each kind, entries of at least 2
    sizes."""
    B, dim, growth, T = SHAPE[kind]
    t = _trainer(kind, 0xBEE, 5, archive=16 * B, growth=growth)
    env, pool, sch = t.env, t.archive, t.schedule
    odd = torch.arange(B, device=env.device) % 2 == 1
    sch.dim = torch.where(odd, growth[1], sch.dim)
    sch._set_next()
    assert int(pool.count) == B
    seen, moved_total, stayed_total = B, 0, 0
    wins = sch.inst_wins.clone()
    for _ in range(T):
        nxt = sch.next_dim.clone()
        t.vector_step()
        now = sch.inst_wins.clone()
        won = now > wins
        wins = now
        movers = torch.nonzero(won & (nxt > 0)).reshape(-1).tolist()
        stayed_total += int((won & (nxt == 0)).sum())
        assert int(pool.count) == seen + len(movers)
        for r, i in enumerate(movers):
            want = host_entry(env, i, growth[1], R_PRIM)
            assert want[1][0] & 0xFF == int(nxt[i]) and i % 2 == 0
            assert_entry(pool, seen + r, want, i, t.counter)
        seen += len(movers)
        moved_total += len(movers)
    sizes = sorted(set((pool.meta[:seen, 0] & 0xFF).tolist()))
    print(kind, "winners that moved:", moved_total, "winners at the maximum size:", stayed_total,
          "sizes in the pool:", sizes)
    assert moved_total >= 2 and stayed_total >= 2 and len(sizes) >= 2
    assert not (pool.owner[B:seen] % 2).any()
    env.close()


# (d) evaluate_explored against an evaluation on the same mazes
@pytest.mark.parametrize("kind", ["ppo", "reinforce"])
def test_evaluate_explored_equals_evaluate_on_the_same_mazes(kind):
    from mazerl.archive import MazePool
    from mazerl.trainers.episodic import episode_bound
    from mazerl.trainers.vector_trainer import evaluate, evaluate_explored
    B, dim, _, T = SHAPE[kind]
    t = _trainer(kind, 0xC0DE, 9, archive=16 * B)
    t.train(T)
    pool = t.archive
    held = int(pool.held)
    assert held == B + t.wins > B
    seed, limit = 0x7E57, episode_bound(pool.pitch, pool.toroidal) + 1
    learners = [("greedy", lambda: t)]
    if kind == "reinforce":  # the reference's own test(): one draw per step, from a counter
        learners.append(("sample", t.sampler))
    for name, get in learners:
        for n in (held, 37):
            if kind == "reinforce":
                t.sample_counter = 1000
            r0, k0, w0 = evaluate(get(), n, dim, mazes=pool.to_mazes(0, n), eps=0.0, seed=seed,
                                  max_vector_steps=limit, return_won=True)
            if kind == "reinforce":
                t.sample_counter = 1000
            r1, k1, w1 = evaluate_explored(get(), pool, n, eps=0.0, seed=seed,
                                           max_vector_steps=limit, return_won=True)
            assert w1.dtype == np.bool_ and w1.shape == (n,)
            assert np.array_equal(w0, w1) and k0 == k1 and abs(r0 - r1) < 1e-6
            print(kind, name, "won", int(w1.sum()), "of", n)
    for bad in (held + 1, 0):
        with pytest.raises(ValueError):
            evaluate_explored(t, pool, n=bad)
    assert int(pool.errors) == 0
    # a corrupt pool is void
    bad = MazePool(t.env, 16 * B)
    bad.load_state_dict(pool.state_dict())
    bad.algo[5] = 7
    with pytest.raises(RuntimeError):
        evaluate_explored(t, bad, eps=0.0, seed=seed, max_vector_steps=limit)
    t.env.close()


def test_evaluate_explored_equals_a_greedy_rollout_on_the_same_mazes():
    """The recurrent DQN: a plain env (the pool's enrich is False), every chunk from zero state."""
    import mazerl
    from mazerl.trainers.drqn_trainer import RecurrentDQNBase
    from mazerl.trainers.episodic import episode_bound
    from mazerl.trainers.vector_trainer import evaluate_explored, load_selected
    B, dim, _, T = SHAPE["drqn"]
    t = _trainer("drqn", 0xC0DE, 9, archive=16 * B)
    t.train(T)
    pool = t.archive
    assert not pool.enrich and pool.pitch == dim
    held = int(pool.held)
    assert held == B + t.wins > B + 4
    limit = episode_bound(dim, False) + 1
    env = mazerl.VectorMazeEnv(held, dim, toroidal=False, enrich=False, device=DEV, pos=False,
                               done_list=False)
    load_selected(env, pool.to_mazes())
    ev = t.evaluator()
    won, k0 = RecurrentDQNBase.greedy_rollout(
        env, lambda k: ev.greedy(env.obs6, None, None).to(torch.int32), limit)
    w0 = won.cpu().numpy()
    r1, k1, w1 = evaluate_explored(t.evaluator(), pool, max_vector_steps=limit, return_won=True)
    print("drqn won", int(w1.sum()), "of", held)
    assert np.array_equal(w0, w1) and k0 == k1 and r1 == w0.sum() / held
    # chunks that do not divide n, through one evaluator that is reset before each chunk
    ev = t.evaluator()
    for chunk in (50 if held % 50 else 51, held - 1):
        assert held % chunk
        r2, _, w2 = evaluate_explored(ev, pool, chunk=chunk, max_vector_steps=limit,
                                      return_won=True)
        assert np.array_equal(w0, w2) and r2 == r1
    r3, _, w3 = evaluate_explored(ev, pool, n=37, max_vector_steps=limit, return_won=True)
    assert np.array_equal(w3, w0[:37]) and r3 == w0[:37].sum() / 37
    assert int(pool.errors) == 0
    env.close()
    t.env.close()


# (e) checkpoint
@kinds
def test_a_checkpoint_carries_the_pool(kind, tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    B = SHAPE[kind][0]
    a = _trainer(kind, 0xA11CE, 3, archive=16 * B)
    a.train(40)
    path = save_checkpoint(str(tmp_path / "run.pt"), a)
    a.train(24)
    b = _trainer(kind, 0x5EED, 8, archive=16 * B)
    assert not torch.equal(a.archive.bits, b.archive.bits)
    load_checkpoint(path, b)
    b.train(24)
    assert a.counter == b.counter == 64
    assert_same_runs(a, b, pools=True)
    for k in ("bits", "meta", "algo", "owner", "stamp", "count", "errors"):
        assert torch.equal(getattr(a.archive, k), getattr(b.archive, k)), k
    assert int(a.archive.count) == B + a.wins
    # presence must match, either way, and nothing changes on a refusal
    c = _trainer(kind, 0x5EED, 8, archive=None)
    before = c.env.obs6.clone()
    with pytest.raises(ValueError):
        load_checkpoint(path, c)
    assert torch.equal(c.env.obs6, before) and c.counter == 0
    plain = save_checkpoint(str(tmp_path / "plain.pt"), c)
    count, obs = b.archive.count.clone(), b.env.obs6.clone()
    with pytest.raises(ValueError):
        load_checkpoint(plain, b)
    assert torch.equal(b.archive.count, count) and torch.equal(b.env.obs6, obs) and b.counter == 64
    # another capacity is refused by the pool's own check, before anything changes
    d = _trainer(kind, 0x5EED, 8, archive=16 * B + 1)
    before = d.env.obs6.clone()
    with pytest.raises(ValueError):
        load_checkpoint(path, d)
    assert d.counter == 0 and int(d.archive.count) == B and torch.equal(d.env.obs6, before)
    for t in (a, b, c, d):
        t.env.close()
