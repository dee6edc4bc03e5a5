"""VectorOffPolicyTrainer(archive=) and evaluate_explored on the GPU: attaching the explored-maze
pool changes nothing in the run, the pool holds what the reference env's `env.mazes` would hold
(every instance's first maze, then each winner's new one, step by step and in instance order),
the growth rule (a winner past max_shape appends nothing), evaluate_explored against evaluate on
the same mazes, and checkpoints. Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, DIM, T = 1024, 15, 128
R_PRIM = 0  # vector_env.ALGOS["r-prim"]


def _trainer(env_seed, seed, archive=None, variant="ddqn", growth=None, num=B, **kw):
    """tests/test_checkpoint_gpu.py::_trainer's learner on a smaller population of 15 x 15 mazes
    (the smallest an euclidean enrich handle loads back), where random acting wins within a few
    vector steps. The stems' dropout salts are a net's construction number within the process
    (QNet._count; tests/test_determinism_gpu.py runs fresh processes for that reason), so a run's
    wins would depend on which tests ran before: the learner is built with the count a fresh
    process has, and the count is then put back to what it would have been."""
    from mazerl.agents.dqn import VectorDQNLearner
    from mazerl.agents.nets import QNet
    from mazerl.trainers.vector_trainer import VectorOffPolicyTrainer, make_env
    env = make_env(num, DIM, seed=env_seed, device="cuda", max_dim=growth[1] if growth else DIM,
                   done_list=False, pos=True, window=False, window_bits=True)
    before, QNet._count = QNet._count, 0
    try:
        L = VectorDQNLearner(num, "cuda:0", variant=variant, batch_size=128, capacity=1 << 15,
                             eps_decay=60.0, target_every=5, updates_per_epoch=7, overlap=True,
                             seed=seed)
    finally:
        QNet._count += before
    return VectorOffPolicyTrainer(env, L, seed=seed + 1, archive=archive, growth=growth, **kw)


def host_entry(env, i, pitch, algo):
    """What the pool must hold for instance i, from the host accessors alone."""
    from mazerl.archive import pack_grid
    q, g = env.query(i), env.grid(i)
    n = q["n"]
    maxs = int(env.meta()[i, 5])
    m0 = n | n << 8 | q["start_r"] << 16 | q["start_c"] << 24
    m1 = q["goal_r"] | q["goal_c"] << 8 | maxs << 16
    assert q["max_steps"] == maxs
    return pack_grid(g, pitch), (m0, m1), algo


def assert_entry(pool, j, want, owner, stamp):
    wb, wm, wa = want
    assert np.array_equal(pool.bits[j].cpu().numpy(), wb), j
    assert tuple(int(x) & 0xFFFFFFFF for x in pool.meta[j].tolist()) == wm, j
    assert int(pool.algo[j]) == wa and int(pool.owner[j]) == owner and int(pool.stamp[j]) == stamp, j


def assert_same_runs(a, b, pools=False):
    torch.cuda.synchronize()
    assert a.counter == b.counter and a.learner.n_updates == b.learner.n_updates
    assert int(a.wins) == int(b.wins) and int(a.episodes) == int(b.episodes)
    assert torch.equal(a.learner.steps_done, b.learner.steps_done)
    assert torch.equal(a.env.obs6, b.env.obs6) and torch.equal(a.env.window_bits, b.env.window_bits)
    ra, rb = a.learner.replay, b.learner.replay
    assert (ra.ptr, ra.size) == (rb.ptr, rb.size)
    for k in ("sw", "a"):
        assert torch.equal(getattr(ra, k)[:ra.size], getattr(rb, k)[:rb.size]), k
    for (ka, pa), (kb, pb) in zip(a.learner.source.state_dict().items(),
                                  b.learner.source.state_dict().items()):
        assert torch.equal(pa, pb), ka
    for pa, pb in zip(a.learner.target.parameters(), b.learner.target.parameters()):
        assert torch.equal(pa, pb)
    if pools:
        for k in ("bits", "meta", "algo", "owner", "stamp", "count", "errors"):
            assert torch.equal(getattr(a.archive, k), getattr(b.archive, k)), k


# 1. the pool changes nothing
def test_the_pool_changes_nothing_in_the_run():
    a = _trainer(0xA11CE, 3, archive=4 * B)
    b = _trainer(0xA11CE, 3, archive=None)
    assert b.archive is None and "archive" not in b.state_dict() and b.summary()["archive"] is None
    # the stems' dropout salts follow the nets' construction order within a process (tests/
    # test_determinism_gpu.py): b starts from a's initial state, salts included, without the pool
    sd = a.state_dict()
    assert set(sd) - set(b.state_dict()) == {"archive"}
    del sd["archive"]
    b.load_state_dict(sd)
    for t in (a, b):
        t.train(T)
    assert_same_runs(a, b)
    print("wins:", int(a.wins))
    assert int(a.wins) >= 4  # mazes were replaced (and recorded) along the way
    s = a.summary()
    assert s["vector_steps"] == T
    assert s["archive"] == {"capacity": 4 * B, "recorded": B + int(a.wins), "held": B + int(a.wins),
                            "dropped": 0}
    # a pool of another env is refused
    from mazerl.trainers.vector_trainer import VectorOffPolicyTrainer
    with pytest.raises(ValueError):
        VectorOffPolicyTrainer(b.env, b.learner, regen_won=False, archive=a.archive)
    a.env.close()
    b.env.close()


# 2. it records what env.mazes would hold
def test_the_pool_records_what_env_mazes_would_hold():
    """Observed on an MI355X with these seeds, alone and after other tests that build Q-nets: 102
    winners over 42 of the 128 vector steps (the first in step 23; the test prints the winners per
    step). At least 4 winners over at least 2 vector steps are asserted below."""
    t = _trainer(0xA11CE, 3, archive=2 * B, track_wins=True)
    env, pool = t.env, t.archive
    first = [host_entry(env, i, DIM, R_PRIM) for i in range(B)]
    assert int(pool.count) == B
    for i in (0, 1, 63, 64, B // 2, B - 1):
        assert_entry(pool, i, first[i], i, 0)
    assert np.array_equal(pool.bits[:B].cpu().numpy(), np.stack([e[0] for e in first]))
    assert pool.owner[:B].tolist() == list(range(B)) and not pool.stamp[:B].any()
    seen, per_step = B, []
    wins = t.inst_wins.clone()
    for _ in range(T):
        t.vector_step()
        now = t.inst_wins.clone()
        winners = torch.nonzero(now > wins).reshape(-1).tolist()
        wins = now
        assert int(pool.count) == seen + len(winners)
        for r, i in enumerate(winners):  # their new mazes, in ascending id
            assert_entry(pool, seen + r, host_entry(env, i, DIM, R_PRIM), i, t.counter)
        seen += len(winners)
        per_step.append(len(winners))
    t.learner.finish()
    print("winners per vector step:", per_step)
    assert sum(per_step) >= 4 and sum(1 for w in per_step if w) >= 2
    assert sum(per_step) == int(t.wins)
    # the first B entries are still the initial mazes
    assert np.array_equal(pool.bits[:B].cpu().numpy(), np.stack([e[0] for e in first]))
    assert not pool.stamp[:B].any() and not pool.bits[seen:].any()
    env.close()


# 3. growth
def test_growth_a_winner_at_the_maximum_size_appends_nothing():
    """growth=(15, 23) on 512 instances; the schedule of every odd instance is put at the maximum
    size before the run (their mazes stay 15 x 15, so they win as often as the others): their
    next size is 0 and a win of theirs must append nothing, while an even winner's new 19 x 19
    maze is appended. Observed on an MI355X: 16 winners moved, 17 won at the maximum size, sizes
    15 and 19 in the pool (printed below). Asserted: at least 2 winners of each kind, entries of
    at least 2 sizes."""
    n = 512
    t = _trainer(0xBEE, 5, archive=2 * n, growth=(15, 23), num=n)
    env, pool, sch = t.env, t.archive, t.schedule
    odd = torch.arange(n, device=env.device) % 2 == 1
    sch.dim = torch.where(odd, 23, sch.dim)
    sch._set_next()
    assert int(pool.count) == n
    seen, moved_total, stayed_total = n, 0, 0
    wins = t.inst_wins.clone()
    for _ in range(96):
        nxt = sch.next_dim.clone()
        t.vector_step()
        now = t.inst_wins.clone()
        won = now > wins
        wins = now
        movers = torch.nonzero(won & (nxt > 0)).reshape(-1).tolist()
        stayed_total += int((won & (nxt == 0)).sum())
        assert int(pool.count) == seen + len(movers)
        for r, i in enumerate(movers):
            want = host_entry(env, i, 23, R_PRIM)
            assert want[1][0] & 0xFF == int(nxt[i]) and i % 2 == 0
            assert_entry(pool, seen + r, want, i, t.counter)
        seen += len(movers)
        moved_total += len(movers)
    t.learner.finish()
    sizes = sorted(set((pool.meta[:seen, 0] & 0xFF).tolist()))
    print("winners that moved:", moved_total, "winners at the maximum size:", stayed_total,
          "sizes in the pool:", sizes)
    assert moved_total >= 2 and stayed_total >= 2 and len(sizes) >= 2
    assert not (pool.owner[n:seen] % 2).any()
    env.close()


# 4. evaluate_explored against evaluate
def test_evaluate_explored_equals_evaluate_on_the_same_mazes():
    from mazerl.archive import MazePool
    from mazerl.trainers.vector_trainer import evaluate, evaluate_explored, steps_done_epsilon
    t = _trainer(0xC0DE, 9, archive=600, variant="dqn", num=256)
    t.train(20)
    L, pool = t.learner, t.archive
    held = int(pool.held)
    assert held == 256 + int(t.wins)
    seed = 0x7E57
    for eps in (0.0, 1.0):  # greedy, and a random walk that wins on some mazes
        r0, k0, w0 = evaluate(L, held, DIM, mazes=pool.to_mazes(), eps=eps, seed=seed,
                              return_won=True)
        r1, k1, w1 = evaluate_explored(L, pool, eps=eps, seed=seed, return_won=True)
        assert w1.dtype == np.bool_ and w1.shape == (held,)
        assert np.array_equal(w0, w1) and k0 == k1 and abs(r0 - r1) < 1e-6
        print("eps", eps, "won", int(w1.sum()), "of", held)
    assert w1.any() and not w1.all()
    # chunks that do not divide n: the same wins, entry by entry (greedy)
    r0, k0, w0 = evaluate_explored(L, pool, eps=0.0, seed=seed, return_won=True)
    for chunk in (100, held - 1):
        assert held % chunk
        r2, k2, w2 = evaluate_explored(L, pool, eps=0.0, chunk=chunk, seed=seed, return_won=True)
        assert np.array_equal(w0, w2) and r2 == r0
    # the oldest n: a prefix
    r3, _, w3 = evaluate_explored(L, pool, n=37, eps=0.0, seed=seed, return_won=True)
    assert np.array_equal(w3, w0[:37]) and r3 == w0[:37].sum() / 37
    assert evaluate_explored(L, pool, n=37, eps=0.0, seed=seed) == (r3, _)
    for bad in (held + 1, 0):
        with pytest.raises(ValueError):
            evaluate_explored(L, pool, n=bad)
    # the reference's epsilon protocol: every maze continues its owner's epsilon
    n = held - 3
    eps = steps_done_epsilon(L, n, instances=pool.owner[:n])
    rate, _ = evaluate_explored(L, pool, n=n, eps=eps, chunk=101, seed=seed)
    assert 0.0 <= rate <= 1.0
    assert int(pool.errors) == 0
    # a corrupt pool is void
    bad = MazePool(t.env, 600)
    bad.load_state_dict(pool.state_dict())
    bad.algo[5] = 7
    with pytest.raises(RuntimeError):
        evaluate_explored(L, bad, eps=0.0, seed=seed)
    t.env.close()


# 5. checkpoint
def test_a_checkpoint_carries_the_pool(tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    a = _trainer(0xA11CE, 3, archive=2 * B)
    a.train(25)
    path = save_checkpoint(str(tmp_path / "run.pt"), a)
    a.train(15)
    b = _trainer(0x5EED, 8, archive=2 * B)
    assert not torch.equal(a.archive.bits, b.archive.bits)
    load_checkpoint(path, b)
    b.train(15)
    assert a.counter == b.counter == 40
    assert_same_runs(a, b, pools=True)
    assert int(a.archive.count) == B + int(a.wins)
    # presence must match, either way, and nothing changes on a refusal
    c = _trainer(0x5EED, 8, archive=None, num=B)
    before = c.env.obs6.clone()
    with pytest.raises(ValueError):
        load_checkpoint(path, c)
    assert torch.equal(c.env.obs6, before) and c.counter == 0
    plain = save_checkpoint(str(tmp_path / "plain.pt"), c)
    count = b.archive.count.clone()
    with pytest.raises(ValueError):
        load_checkpoint(plain, b)
    assert torch.equal(b.archive.count, count) and b.counter == 40
    # another capacity is refused by the pool's own check, before anything changes
    d = _trainer(0x5EED, 8, archive=2 * B + 1)
    with pytest.raises(ValueError):
        load_checkpoint(path, d)
    assert d.counter == 0 and int(d.archive.count) == B
    for t in (a, b, c, d):
        t.env.close()
