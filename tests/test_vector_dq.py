"""VectorDoubleQAgent (csrc/mz_qtab.hip): a population of the reference's double Q-learning agent,
DQAgent (agents/dq_agent.py:5-73), on the GPU — against the reference's own fixture
(tests/golden/dq_agent.npz, written by tests/golden/make_golden_dq.py) and against a CPU
restatement written here, as Restated in test_vector_q.py: one oracle env per instance, a dict of
np.zeros((2, 4)) rows per table (row 0 = Q_A, row 1 = Q_B) keyed by (pos, goal, best_dir), the same
Philox draws, math.exp for epsilon. One instance per table must be equal bit for bit; shared
tables are pinned where the float64 adds commute exactly (disjoint rows; equal addends).

The restatement tracks the smallest distance of every epsilon draw from its epsilon, for act and
for the inner choice of update; every bit-exact test first asserts it is >= 1e-9 (the device exp
may differ from libm in the last place). Seed 0x7AB gives that for every run below."""
import ctypes
import functools
import math
import re

import numpy as np
import pytest

import golden_io as G
import pyoracle as O
from test_vector_q import (GAP, HP, SEED, assert_log, need_gpu, nine, per_table, run_logged,
                           varied_hp)

STREAM = 0x71746162   # MZ_QTAB_STREAM: act
DSTREAM = 0x64717462  # MZ_DQTAB_STREAM: the update's coin and inner choice


class RestatedDQ:
    """The CPU yardstick: DQAgent per table under OffPolicyTrainer.train's step. table_of None:
    one table per instance."""

    def __init__(self, mazes, toroidal, table_of=None, seed=SEED, **hp):
        self.toroidal = toroidal
        self.n = len(mazes)
        self.table_of = list(range(self.n)) if table_of is None else list(table_of)
        T = self.T = max(self.table_of) + 1
        self.lr = per_table(hp["learning_rate"], T)
        self.ei = per_table(hp["initial_epsilon"], T)
        self.ef = per_table(hp["final_epsilon"], T)
        self.decay = per_table(hp["epsilon_decay"], T)
        self.gamma = per_table(hp["discount_factor"], T)
        self.eta = per_table(hp["eta"], T)
        self.tables = [dict() for _ in range(T)]
        self.steps_done = [0] * T
        self.episodes = [0] * T
        self.wins = [0] * T
        self.cum = [0.0] * self.n
        self.seed, self.counter, self.ucounter = seed, 0, 0
        self.min_gap = float("inf")
        self.envs, self.goal, self.obs = [None] * self.n, [None] * self.n, [None] * self.n
        self.written = [set() for _ in range(self.n)]        # keys written, in either table
        self.written_ab = [set() for _ in range(self.n)]     # which tables were written
        self.read = [set() for _ in range(self.n)]
        for i, m in enumerate(mazes):
            self.envs[i] = O.Env(m["grid"], m["start"], m["goal"], toroidal, False)
            self.goal[i] = tuple(m["goal"])
            self.obs[i] = self.envs[i].reset()

    def key(self, i, o=None):
        o = self.obs[i] if o is None else o
        return (tuple(o["pos"]), self.goal[i], tuple(o["best_dir"]))

    def row(self, t, k):
        return self.tables[t].setdefault(k, np.zeros((2, 4)))

    def eps(self, t, steps_done):
        return self.ef[t] + (self.ei[t] - self.ef[t]) * math.exp(-1. * steps_done / self.decay[t])

    def act(self, active=None):
        """get_action (dq_agent.py:35-46): argmax of Q_A."""
        before = list(self.steps_done)
        acts = []
        for i in range(self.n):
            if active is not None and not active[i]:
                acts.append(-1)
                continue
            t = self.table_of[i]
            eps = self.eps(t, before[t])
            w = O.philox(self.seed, STREAM ^ (i << 32), self.counter)
            u = (w[0] >> 8) * 2.0 ** -24
            self.min_gap = min(self.min_gap, abs(u - eps))
            self.read[i].add(self.key(i))
            acts.append(w[1] >> 30 if u < eps else int(np.argmax(self.row(t, self.key(i))[0])))
            self.steps_done[t] += 1
        self.counter += 1
        return acts

    def coin(self, i):
        """0: update A (the draw is < 0.5), 1: update B."""
        w = O.philox(self.seed, DSTREAM ^ (i << 32), self.ucounter)
        return 0 if (w[0] >> 8) * 2.0 ** -24 < 0.5 else 1

    def step(self, actions=None, coins=None, next_actions=None, episode_end=True, auto_reset=True):
        """One vector step on independent tables (or tables whose instances touch disjoint
        rows): act, env.step, update (dq_agent.py:48-66), the episode end. Returns (actions,
        terminated, truncated)."""
        acts = self.act() if actions is None else list(actions)
        before = list(self.steps_done)  # as every instance's update finds it
        term, trunc = [], []
        for i, a in enumerate(acts):
            t = self.table_of[i]
            k = self.key(i)
            o = self.envs[i].step(a)
            k2 = self.key(i, o)
            r, te, tr = o["reward"], o["terminated"], o["truncated"]
            which = self.coin(i) if coins is None else int(coins[i])
            nxt = self.row(t, k2)
            if next_actions is None:  # the inner get_action on Q_A[s']
                eps = self.eps(t, before[t])
                w = O.philox(self.seed, DSTREAM ^ (i << 32), self.ucounter)
                u2 = (w[1] >> 8) * 2.0 ** -24
                self.min_gap = min(self.min_gap, abs(u2 - eps))
                best = w[2] >> 30 if u2 < eps else int(np.argmax(nxt[0]))
            else:
                best = int(next_actions[i])
            self.steps_done[t] += 1
            self.read[i].add(k2)
            self.written[i].add(k)
            self.written_ab[i].add(which)
            q = self.row(t, k)
            td = (r + self.gamma[t] * nxt[1 - which][best]) - q[which][a]
            q[which][a] = q[which][a] + self.lr[t] * td
            self.cum[i] += r
            self.obs[i] = o
            if te or tr:
                if episode_end:
                    self.gamma[t] += self.eta[t] if self.cum[i] > 0 else -self.eta[t]
                    self.cum[i] = 0.0
                    self.episodes[t] += 1
                    self.wins[t] += int(te)
                if auto_reset:
                    self.obs[i] = self.envs[i].reset()
            term.append(te)
            trunc.append(tr)
        self.ucounter += 1
        return acts, term, trunc

    def evaluate(self):
        """One episode per instance on the current mazes, act() only."""
        for i in range(self.n):
            self.obs[i] = self.envs[i].reset()
        active = [True] * self.n
        won = [False] * self.n
        for _ in range(max(e.max_steps for e in self.envs) + 1):
            acts = self.act(active)
            for i, a in enumerate(acts):
                if a < 0:
                    continue
                o = self.obs[i] = self.envs[i].step(a)
                won[i] |= o["terminated"]
                if o["terminated"] or o["truncated"]:
                    active[i] = False
        for i in range(self.n):
            self.obs[i] = self.envs[i].reset()
        return won


@functools.lru_cache(maxsize=None)
def restated_run(toroidal, steps, n=24, varied=False, eta=None):
    """The restatement after `steps` vector steps on the first n golden 9x9 mazes, and its
    per-step (actions, terminated, truncated). Shared by the tests; never modified."""
    hp = dict(HP)
    if varied:
        hp.update(varied_hp(n))
    if eta is not None:
        hp["eta"] = eta
    rs = RestatedDQ(nine(toroidal)[:n], toroidal, **hp)
    log = [rs.step() for _ in range(steps)]
    assert rs.min_gap >= GAP, rs.min_gap  # the precondition of every bit-exact comparison
    return rs, log


def simple_traces():
    return [t for t in G.traces() if t["kind"] == G.KIND_SIMPLE]


def index_of(text):
    """The state index of one of the fixture's str(obs) keys."""
    from mazerl.agents.vector_q import state_index
    x = [int(s) for s in re.findall(r"-?\d+", str(text).replace("int32", ""))]
    assert len(x) == 6, text
    return state_index(9, x[0:2], x[2:4], x[4:6])


@functools.lru_cache(maxsize=None)
def fixture(j):
    """Trace j of the reference's fixture: (the trace, its per-update arrays, the reference's
    final tables as a dense [rows, 2, 4] array, its steps_done), with the conditions the fixture
    was made for."""
    from mazerl.agents.vector_q import table_rows
    fx = G.load("dq_agent.npz")
    t = simple_traces()[j]
    p = f"dq{j}."
    upd = {k: fx[p + k] for k in ("obs", "act", "rew", "term", "next", "coin", "best")}
    want = np.zeros((table_rows(9), 2, 4))
    for x, name in enumerate("ab"):
        for k, v in zip(fx[p + name + ".keys"], fx[p + name + ".values"]):
            want[index_of(k), x] = v
    assert np.count_nonzero(want[:, 0].any(1)) > 10 and np.count_nonzero(want[:, 1].any(1)) > 10
    assert upd["coin"].any() and not upd["coin"].all()  # both tables were updated
    assert set(upd["best"].tolist()) == {0, 1, 2, 3}
    assert int(upd["term"].sum()) == (0, 1)[j]  # trace 1 holds the terminated step
    assert len(upd["act"]) == sum(int(op) != 4 for op in t["op"][:600]) == (599, 598)[j]
    return t, upd, want, int(fx[p + "steps_done"])


def dense_of(rs, t=0):
    """Table t of a restatement as a dense [rows, 2, 4] array."""
    from mazerl.agents.vector_q import state_index, table_rows
    out = np.zeros((table_rows(9), 2, 4))
    for k, v in rs.tables[t].items():
        out[state_index(9, *k)] = v
    return out


# ---------------------------------------------------------------------------------------------
# 1. the restatement is the reference's agent (CPU)
@pytest.mark.parametrize("j", [0, 1])
def test_restatement_replays_the_reference_fixture(j):
    from mazerl.agents.vector_q import state_index
    t, upd, want, steps_done = fixture(j)
    rs = RestatedDQ([t], False, **HP)  # lr 0.1, gamma 0.7 (make_golden_dq.py)
    u = 0
    for op in t["op"][:600]:
        if op == 4:
            rs.obs[0] = rs.envs[0].reset()
            continue
        k = rs.key(0)
        assert state_index(9, *k) == index_of(upd["obs"][u]) and int(op) == upd["act"][u]
        # coin True = the reference's draw was < 0.5 = table A = 0
        _, te, _ = rs.step(actions=[int(op)], coins=[0 if upd["coin"][u] else 1],
                           next_actions=[upd["best"][u]], episode_end=False, auto_reset=False)
        assert state_index(9, *rs.key(0)) == index_of(upd["next"][u])
        assert te[0] == upd["term"][u]
        u += 1
    assert u == len(upd["act"])
    assert np.array_equal(dense_of(rs), want)
    assert rs.steps_done == [steps_done] == [u]  # one get_action per update, none for acting
    assert rs.gamma == [0.7]


# 2. the ABI's argument checks need no GPU
def test_dq_abi_refuses_bad_arguments_without_a_gpu():
    from mazerl import _native as N
    L = N.load()
    buf = ctypes.create_string_buffer(16384)
    p = (ctypes.addressof(buf) + 63) & ~63  # a 64-B aligned host address: never dereferenced
    act = [p, 4, 9, None, 4, None, p, p, p, p, p, 0, 0, p, p, None]
    dq = [p, p, p, p, 0, 0, None, None, p, None, None]  # steps_done .. which, the stream
    upd = [p, 4, 9, None, 4, p] + [p] * 11 + [p, 1] + dq
    hact = [p, 4, 9, None, 4, None, p, p, 64, p, p, p, p, 0, 0, p, p, None]
    hupd = [p, 4, 9, None, 4, p, p, 64] + [p] * 13 + [p, 1] + dq
    reh = [p, p, 64, p + 8192, p + 8192, 128, 4, p, None]
    look = [p, p, 64, 4, p, p, 4, p, p, None]
    assert len(upd) == len(L.mz_dqtab_update.argtypes) == 30
    assert len(hupd) == len(L.mz_dqtab_hash_update.argtypes) == 34
    caps = (0, 8, 24, 100, -16, (1 << 30) + 1, 1 << 31)
    cases = [
        (L.mz_dqtab_act, act, {6: (None,), 1: (0, -1), 2: (4, 200), 7: (None,), 13: (None,),
                               14: (None,)}),
        (L.mz_dqtab_update, upd, {5: (None,), 1: (0, -1), 2: (4, 200), 6: (None,), 16: (None,),
                                  19: (None,), 20: (None,), 27: (None,), 4: (3,)}),
        (L.mz_dqtab_hash_act, hact, {8: caps, 6: (None,), 7: (None,), 1: (0, -1), 2: (200,),
                                     9: (None,)}),
        (L.mz_dqtab_hash_update, hupd, {7: caps, 5: (None,), 6: (None,), 1: (-1,), 2: (4,),
                                        8: (None,), 9: (None,), 23: (None,), 31: (None,)}),
        (L.mz_dqtab_hash_rehash, reh, {2: (24,), 5: (8, 96), 0: (None,), 1: (None,), 3: (None,),
                                       4: (None,), 6: (0, -1), 7: (None,)}),
        (L.mz_dqtab_hash_lookup, look, {2: (63,), 0: (None,), 1: (None,), 6: (-1,), 4: (None,),
                                        5: (None,), 7: (None,), 8: (None,)}),
    ]
    for fn, good, bads in cases:
        for pos, values in bads.items():
            for v in values:
                a = list(good)
                a[pos] = v
                assert fn(*a) == -1, (fn.__name__, pos, v)
                assert L.mz_last_error()
    # shared tables need the td and the which workspaces
    for fn, good, td, which in ((L.mz_dqtab_update, upd, 17, 28),
                                (L.mz_dqtab_hash_update, hupd, 21, 32)):
        for none in ((td,), (which,)):
            a = list(good)
            a[3], a[which] = p, p
            for pos in none:
                a[pos] = None
            assert fn(*a) == -1, (fn.__name__, none)
    a = list(reh)
    a[3] = a[0]
    assert L.mz_dqtab_hash_rehash(*a) == -1  # rehash needs fresh arrays
    look[6] = 0
    assert L.mz_dqtab_hash_lookup(*look) == 0  # nothing to look up: no launch, no GPU
    # a state's two rows are read as one 64-B segment
    for fn, good, pos in ((L.mz_dqtab_act, act, 6), (L.mz_dqtab_update, upd, 5),
                          (L.mz_dqtab_hash_act, hact, 7), (L.mz_dqtab_hash_update, hupd, 6),
                          (L.mz_dqtab_hash_rehash, reh, 4), (L.mz_dqtab_hash_lookup, look, 1)):
        a = list(good)
        a[pos] += 32
        assert fn(*a) == -5, fn.__name__


# ---------------------------------------------------------------------------------------------
# GPU
torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


def make(mazes, toroidal=False, tables=None, regen_won=False, seed=SEED, grow_every=0, **kw):
    import mazerl
    from mazerl.agents import VectorDoubleQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env = mazerl.VectorMazeEnv(len(mazes), 9, toroidal=toroidal, enrich=False, reward64=True,
                               generate=False)
    env.load_mazes(np.stack([m["grid"] for m in mazes]),
                   np.array([list(m["start"]) + list(m["goal"]) for m in mazes]))
    env.reset()
    agent = VectorDoubleQAgent(env, tables=tables, seed=seed, **{**HP, **kw})
    return env, agent, VectorTabularTrainer(env, agent, regen_won=regen_won, keep_flags=True,
                                            grow_every=grow_every)


def written_items(rs, t, instances=None):
    """The restatement's written rows of table t as items() gives them."""
    from mazerl.agents.vector_q import state_index
    rows = {}
    for i in ([t] if instances is None else instances):
        for k in rs.written[i]:
            rows[state_index(9, *k)] = rs.tables[rs.table_of[i]][k]
    keys = sorted(rows)
    return np.array(keys, dtype=np.int64), np.array([rows[k] for k in keys]).reshape(-1, 2, 4)


def items_np(agent, t):
    k, r = agent.items(t)
    return k.cpu().numpy(), r.cpu().numpy()


def assert_counters(agent, rs, tables=None):
    for name in ("gamma", "steps_done", "wins", "episodes"):
        have, want = getattr(agent, name).cpu().tolist(), getattr(rs, name)
        if tables is not None:
            have, want = [have[t] for t in tables], [want[t] for t in tables]
        assert have == want, name


def assert_agent(agent, rs, tables=None):
    """Dense: exactly the restatement's rows, every other row zero. Hashed: exactly its written
    keys with their rows, load and no overflow."""
    for t in (range(rs.T) if tables is None else tables):
        if agent.hashed:
            (gk, gr), (wk, wr) = items_np(agent, t), written_items(rs, t)
            assert np.array_equal(gk, wk), ("table", t, gk, wk)
            assert np.array_equal(gr, wr), ("table", t)
            assert int(agent.load[t]) == len(wk) and int(agent.overflow[t]) == 0
        else:
            got, want = agent.q[t].cpu().numpy(), dense_of(rs, t)
            bad = np.argwhere(got != want)
            assert bad.size == 0, ("table", t, "row", bad[0], got[bad[0][0]], want[bad[0][0]])
    assert_counters(agent, rs, tables)
    assert agent.ucounter == rs.ucounter and agent.counter == rs.counter


# 3. the reference's own fixture on the device
@gpu
@pytest.mark.parametrize("storage", ["dense", "hash"])
@pytest.mark.parametrize("j", [0, 1])
def test_fixture_replay_matches_reference_tables(j, storage):
    """act() (for the row acted from; its own action is not taken), env.step(op), update with the
    fixture's coin and best_action. The reference's replay calls get_action only inside update,
    so its steps_done counts the inner get_actions alone; here act() counts one more per op."""
    need_gpu()
    t, upd, want, steps_done = fixture(j)
    kw = dict(storage="hash", capacity=64) if storage == "hash" else {}
    env, agent, _ = make([t], **kw)
    dev = env.device
    u = 0
    for op in t["op"][:600]:
        if op == 4:
            env.reset()
            continue
        agent.act()
        a = torch.tensor([int(op)], dtype=torch.int32, device=dev)
        env.step(a)
        agent.update(actions=a, coins=torch.tensor([0 if upd["coin"][u] else 1], device=dev),
                     next_actions=torch.tensor([int(upd["best"][u])], device=dev),
                     episode_end=False)
        u += 1
    got = agent.to_dense(0).cpu().numpy()
    assert np.array_equal(got, want)  # A and B, and every other row zero
    if not agent.hashed:  # qa / qb are the two tables
        assert np.array_equal(agent.qa[0].cpu().numpy(), want[:, 0])
        assert np.array_equal(agent.qb[0].cpu().numpy(), want[:, 1])
    assert agent.gamma.cpu().tolist() == [0.7]
    assert int(agent.steps_done[0]) - u == steps_done == u and agent.ucounter == u
    if agent.hashed:
        assert int(agent.overflow[0]) == 0 and 10 < int(agent.load[0]) <= 64
    env.close()


# 4. independent learners, fixed mazes (and 8: evaluate)
@pytest.fixture(scope="module")
def trained():
    """Per geometry: the dense GPU population after 600 vector steps on the 24 golden mazes."""
    out = {}

    def get(toroidal):
        if toroidal not in out:
            env, agent, trainer = make(nine(toroidal), toroidal)
            got = run_logged(trainer, 600)
            out[toroidal] = (env, agent, trainer, got, agent.state_dict())
        return out[toroidal]
    yield get
    for env, *_ in out.values():
        env.close()


@gpu
@pytest.mark.parametrize("toroidal", [False, True])
def test_independent_learners_equal_the_restatement(trained, toroidal):
    need_gpu()
    from mazerl.agents import VectorDoubleQAgent
    rs, log = restated_run(toroidal, 600)
    env, agent, trainer, got, sd = trained(toroidal)
    assert trainer.launches_per_step - int(env._out.done_count is not None) == 6 + 2
    assert_log(got, log)
    assert sum(rs.wins) > 20 and sum(rs.episodes) > sum(rs.wins)  # every branch was taken
    assert all(ab == {0, 1} for ab in rs.written_ab)  # every learner has written both tables
    fresh = VectorDoubleQAgent(env, **HP)
    fresh.load_state_dict(sd)  # (evaluate, in another test, may have advanced the fixture's agent)
    assert_agent(fresh, rs)
    assert tuple(fresh.q.shape) == (24, 5 * 9 ** 4, 2, 4)
    assert all(bool(fresh.qa[t].any()) and bool(fresh.qb[t].any()) for t in range(24))
    assert sd["steps_done"].cpu().tolist() == [1200] * 24  # 2 per training step


@gpu
def test_per_table_hyperparameters():
    need_gpu()
    rs, log = restated_run(False, 200, varied=True)
    env, agent, trainer = make(nine(False), **varied_hp(24))
    assert_log(run_logged(trainer, 200), log)
    assert_agent(agent, rs)
    env.close()


# 5. hashed tables
@gpu
def test_hashed_learners_through_a_rehash(trained):
    need_gpu()
    from mazerl.agents.vector_q import hash_slot
    rs, log = restated_run(False, 600)
    env, agent, trainer = make(nine(False), storage="hash", capacity=64)
    assert not hasattr(agent, "q") and tuple(agent.vals.shape) == (24, 64, 2, 4)
    got = run_logged(trainer, 300)
    # probing happened: some key sits away from its start slot
    kt = agent.keys.cpu().numpy()
    assert sum(int(hash_slot(int(k), 64) != slot) for row in kt for slot, k in enumerate(row)
               if k >= 0) > 0
    before = [items_np(agent, t) for t in range(24)]
    load = agent.load.clone()
    agent.rehash(256)
    assert agent.capacity == 256 and tuple(agent.vals.shape) == (24, 256, 2, 4)
    for t in range(24):
        k, r = items_np(agent, t)
        assert np.array_equal(k, before[t][0]) and np.array_equal(r, before[t][1])
    assert torch.equal(agent.load, load)
    rest = run_logged(trainer, 300)
    assert_log([np.concatenate([a, b]) for a, b in zip(got, rest)], log)
    assert_agent(agent, rs)
    # q_row, lookup and to_dense read the same rows; the dense run holds the same tables
    t = max(range(24), key=lambda i: len(rs.written[i]))
    for k in list(rs.written[t])[:5]:
        assert agent.q_row(t, *k).cpu().tolist() == rs.tables[t][k].tolist()
    keys, rows = agent.items(t)
    r, s = agent.lookup([t, t], [int(keys[0]), 5 * 9 ** 4 - 1])
    assert tuple(r.shape) == (2, 2, 4) and torch.equal(r[0], rows[0])
    assert s.cpu().tolist()[1] == -1 and not bool(r[1].any())
    dense_sd = trained(False)[4]
    for t in range(24):
        assert torch.equal(agent.to_dense(t), dense_sd["q"][t]), t
    env.close()


@gpu
def test_growth_from_a_small_capacity_drops_nothing():
    need_gpu()
    rs, log = restated_run(False, 600)
    env, agent, trainer = make(nine(False), storage="hash", capacity=16, grow_every=8)
    assert_log(run_logged(trainer, 600), log)
    assert_agent(agent, rs)
    assert int(agent.overflow.sum()) == 0
    assert agent.capacity >= 64 and int(agent.load.max()) <= agent.capacity // 2
    env.close()


# 6. which table is read
@gpu
def test_acting_reads_a_and_the_target_reads_the_other_table():
    """epsilon = 0. Fails for max-of-B, for argmax-of-B and for acting on A + B."""
    need_gpu()
    from mazerl.agents.vector_q import state_index
    m = nine(False)[0]
    lr, g = 0.1, 0.7

    def setup():
        env, agent, _ = make([m], initial_epsilon=0.0, final_epsilon=0.0)
        e = O.Env(m["grid"], m["start"], m["goal"], False, False)
        o = e.reset()
        s = state_index(9, tuple(o["pos"]), tuple(m["goal"]), tuple(o["best_dir"]))
        return env, agent, e, s

    def f64(x):
        return torch.tensor(x, dtype=torch.float64, device="cuda")

    env, agent, e, s = setup()
    agent.q[0, s, 1] = f64([0, 9, 0, 0])
    assert agent.act().cpu().tolist() == [0]  # A[s] is zero: its first maximum, whatever B holds
    agent.q[0, s, 0] = f64([0, 0, 4, 0])
    assert agent.act().cpu().tolist() == [2]
    assert int(agent.sidx[0]) == s
    env.close()
    # an action that moves: s' != s
    def moves(a):
        e = O.Env(m["grid"], m["start"], m["goal"], False, False)
        e.reset()
        return tuple(e.step(a)["pos"]) != tuple(m["start"])
    a = next(a for a in range(4) if moves(a))
    for coin in (0, 1):
        env, agent, e, s = setup()
        o = e.step(a)
        r = o["reward"]
        s2 = state_index(9, tuple(o["pos"]), tuple(m["goal"]), tuple(o["best_dir"]))
        assert s2 != s and not o["terminated"]
        agent.q[0, s, 0, a], agent.q[0, s, 1, a] = 0.25, -0.5
        agent.q[0, s2, 0], agent.q[0, s2, 1] = f64([0, 3, 1, 0]), f64([5, 7, 9, 2])
        before = agent.q.clone()
        assert agent.act().cpu().tolist() == [a]  # 0.25 is A[s]'s maximum
        env.step(agent.actions)
        assert env.reward64.cpu().tolist() == [r]
        agent.update(coins=torch.tensor([coin]), episode_end=False)
        # best = argmax A[s'] = 1; the value comes from the table that is not updated
        if coin == 0:
            want = 0.25 + lr * ((r + g * 7.0) - 0.25)
        else:
            want = -0.5 + lr * ((r + g * 3.0) - (-0.5))
        assert float(agent.q[0, s, coin, a]) == want
        before[0, s, coin, a] = want
        assert torch.equal(agent.q, before)  # the other table, and every other element, untouched
        assert int(agent.steps_done[0]) == 2
        env.close()


# 7. shared tables
@gpu
@pytest.mark.parametrize("storage", ["dense", "hash"])
def test_shared_table_on_disjoint_rows_is_the_union(storage):
    """As test_vector_q's test of that name, on the toroidal mazes (15 targets; at least 8
    instances share table 0): instances whose rows (read or written over the run) meet nobody
    else's written rows share table 0, the others keep a table each. eta = 0; the shared table's
    decay is scaled by its instances: its steps_done advances by that many per get_action, and
    (k m) / (40 m) rounds like k / 40. Hashed: concurrent inserts of different keys."""
    need_gpu()
    from mazerl.agents.vector_q import state_index
    mazes = nine(True)
    rs, log = restated_run(True, 300, eta=0.0)
    rows_w = [{state_index(9, *k) for k in rs.written[i]} for i in range(24)]
    rows_r = [{state_index(9, *k) for k in rs.read[i]} for i in range(24)]
    kept = []
    for i in range(24):
        if all(not (rows_w[i] & (rows_w[j] | rows_r[j])) and not (rows_r[i] & rows_w[j])
               for j in kept):
            kept.append(i)
    assert len(kept) >= 8, kept
    m = len(kept)
    table_of, decay = [], [40.0 * m]
    for i in range(24):
        table_of.append(0 if i in kept else len(decay))
        if i not in kept:
            decay.append(40.0)
    kw = dict(storage="hash", capacity=1024) if storage == "hash" else {}
    env, agent, trainer = make(mazes, True, tables=torch.tensor(table_of), eta=0.0,
                               epsilon_decay=decay, **kw)
    assert trainer.launches_per_step - int(env._out.done_count is not None) == 7 + 2
    assert_log(run_logged(trainer, 300), log)
    union = np.zeros((agent.rows, 2, 4))
    for i in kept:
        for k in rs.written[i]:
            s = state_index(9, *k)
            assert not union[s].any()
            union[s] = rs.tables[i][k]
    assert np.array_equal(agent.to_dense(0).cpu().numpy(), union)
    if agent.hashed:
        assert int(agent.load[0]) == len(set().union(*(rows_w[i] for i in kept)))
        assert int(agent.overflow.sum()) == 0
    assert int(agent.steps_done[0]) == 2 * 300 * m
    assert int(agent.episodes[0]) == sum(rs.episodes[i] for i in kept)
    assert int(agent.wins[0]) == sum(rs.wins[i] for i in kept)
    # the same union from the GPU's own independent run
    env2, agent2, trainer2 = make(mazes, True, eta=0.0, **kw)
    trainer2.train(300)
    assert np.array_equal(union, sum(agent2.to_dense(i) for i in kept).cpu().numpy())
    env.close()
    env2.close()


@gpu
@pytest.mark.parametrize("storage", ["dense", "hash"])
def test_shared_table_collisions_add(storage):
    """256 instances on one maze and one zero table: every td is lr * r_a, so Q_X[s0][a] is that
    addend added k_{a,X} times (equal addends commute)."""
    need_gpu()
    from mazerl.agents.vector_q import state_index
    m = nine(False)[0]
    rs = RestatedDQ([m] * 256, False, table_of=[0] * 256, **HP)
    acts = rs.act()
    assert rs.min_gap >= GAP
    coins = [rs.coin(i) for i in range(256)]
    kw = dict(storage="hash", capacity=16) if storage == "hash" else {}
    env, agent, trainer = make([m] * 256, tables=1, **kw)
    trainer.vector_step()
    assert agent.actions.cpu().tolist() == acts
    counts = np.zeros((2, 4), dtype=np.int64)
    for a, c in zip(acts, coins):
        counts[c, a] += 1
    assert counts.min() > 10  # eps = 0.95, a fair coin: every (table, action) is met many times
    s0 = state_index(9, *rs.key(0))
    want = np.zeros((agent.rows, 2, 4))
    for a in range(4):
        e = O.Env(m["grid"], m["start"], m["goal"], False, False)
        e.reset()
        add = 0.1 * ((e.step(a)["reward"] + 0.7 * 0.0) - 0.0)
        for x in range(2):
            v = 0.0
            for _ in range(counts[x, a]):
                v = v + add
            want[s0, x, a] = v
    assert np.array_equal(agent.to_dense(0).cpu().numpy(), want)
    if agent.hashed:
        assert agent.load.cpu().tolist() == [1] and int(agent.overflow.sum()) == 0
        assert items_np(agent, 0)[0].tolist() == [s0]
    assert int(agent.steps_done[0]) == 2 * 256
    env.close()


# 8. evaluate
@gpu
@pytest.mark.parametrize("storage", ["dense", "hash"])
def test_evaluate(trained, storage):
    need_gpu()
    rs0, _ = restated_run(False, 600)
    sd = trained(False)[4]
    if storage == "dense":
        env, agent, trainer = trained(False)[:3]
        agent.load_state_dict(sd)
    else:  # the same population on hashed tables
        env, agent, trainer = make(nine(False), storage="hash", capacity=64)
        trainer.train(600)
        assert all(torch.equal(agent.to_dense(t), sd["q"][t]) for t in range(24))
    names = ("keys", "vals", "load", "overflow", "gamma") if agent.hashed else ("q", "gamma")
    before = {k: getattr(agent, k).clone() for k in names}
    # continue the shared restatement on a copy of what evaluate reads and advances
    rs = RestatedDQ(nine(False), False, **HP)
    rs.tables = [{k: v.copy() for k, v in t.items()} for t in rs0.tables]
    rs.steps_done, rs.counter = list(rs0.steps_done), rs0.counter
    want = rs.evaluate()
    assert rs.min_gap >= GAP, rs.min_gap
    ucounter = agent.ucounter
    won, rate = trainer.evaluate(new=False)
    assert won.cpu().tolist() == want
    assert rate == sum(want) / 24 and 0 < sum(want)
    assert agent.steps_done.cpu().tolist() == rs.steps_done  # one per acting step
    assert rs.steps_done != rs0.steps_done and agent.ucounter == ucounter
    for k in names:
        assert torch.equal(getattr(agent, k), before[k]), k
    if storage == "dense":
        agent.load_state_dict(sd)  # leave the shared population as the fixture made it
    else:
        env.close()


# 9. checkpoint
@gpu
@pytest.mark.parametrize("storage", ["dense", "hash"])
def test_checkpoint_resumes_bit_exactly(storage):
    need_gpu()
    from mazerl.agents import VectorQAgent
    mazes = nine(False)[:16]
    kw = dict(storage="hash", capacity=64) if storage == "hash" else {}
    env, agent, trainer = make(mazes, regen_won=True, **kw)
    trainer.train(200)
    sd_a, sd_e = agent.state_dict(), env.state_dict()
    assert sd_a["format"] == "mazerl.VectorDoubleQAgent/" + ("2" if agent.hashed else "1")
    assert sd_a["ucounter"] == 200 and sd_a["counter"] == 200
    trainer.train(200)
    env2, agent2, trainer2 = make(mazes, regen_won=True, seed=1, **kw)
    env2.load_state_dict(sd_e)
    agent2.load_state_dict(sd_a)
    assert agent2.ucounter == 200
    trainer2.train(200)
    names = ("keys", "vals", "load", "overflow") if agent.hashed else ("q",)
    for name in names + ("gamma", "steps_done", "wins", "episodes", "cum"):
        assert torch.equal(getattr(agent2, name), getattr(agent, name)), name
    assert agent2.ucounter == agent.ucounter == 400 and agent2.seed == agent.seed
    assert bool(agent.qa.any()) and bool(agent.qb.any()) and int(agent.wins.sum()) > 0
    # each class refuses the other's dictionaries, and the other storage's
    single = VectorQAgent(env, **HP, **kw)
    with pytest.raises(ValueError):
        single.load_state_dict(sd_a)
    with pytest.raises(ValueError):
        agent2.load_state_dict(single.state_dict())
    other = make(mazes, **({} if agent.hashed else dict(storage="hash", capacity=64)))
    with pytest.raises(ValueError):
        other[1].load_state_dict(sd_a)
    for e in (env, env2, other[0]):
        e.close()


# 10. a full table is defined, bounded and counted
@gpu
def test_full_table_drops_and_counts():
    need_gpu()
    rs, log = restated_run(False, 600)
    env, agent, trainer = make(nine(False), storage="hash", capacity=16)
    got = run_logged(trainer, 600)  # completes: every probe loop is bounded by C
    fits = [t for t in range(24) if len(rs.written[t]) <= 16]
    full = [t for t in range(24) if len(rs.written[t]) > 16]
    assert fits and full, (fits, full)
    for g, want in zip(got, zip(*log)):
        assert np.array_equal(g[:, fits].astype(np.int64), np.array(want)[:, fits].astype(np.int64))
    for t in fits:
        (gk, gr), (wk, wr) = items_np(agent, t), written_items(rs, t)
        assert np.array_equal(gk, wk) and np.array_equal(gr, wr), t
    assert_counters(agent, rs, fits)
    load, over = agent.load.cpu().tolist(), agent.overflow.cpu().tolist()
    for t in fits:
        assert load[t] == len(rs.written[t]) and over[t] == 0, t
    for t in full:
        assert load[t] == 16 and over[t] > 0, t
    # a dropped update still counts its get_action, and its episode end still ran
    assert agent.steps_done.cpu().tolist() == [1200] * 24
    assert all(int(agent.episodes[t]) > 0 for t in full)
    env.close()


# 11. refusals
@gpu
def test_refusals():
    need_gpu()
    import mazerl
    from mazerl.agents import VectorDoubleQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env = mazerl.VectorMazeEnv(4, 15, enrich=True, reward64=True)
    with pytest.raises(ValueError, match="enrich=False"):
        VectorDoubleQAgent(env, **HP)
    env.close()
    env = mazerl.VectorMazeEnv(4, 9, enrich=False, reward64=False)
    with pytest.raises(ValueError, match="reward64=True"):
        VectorDoubleQAgent(env, **HP)
    env.close()
    env = mazerl.VectorMazeEnv(4, 9, enrich=False, reward64=True)
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(MemoryError, match="max_bytes"):
        VectorDoubleQAgent(env, max_bytes=4 * 5 * 9 ** 4 * 64 - 1, **HP)
    with pytest.raises(MemoryError, match="max_bytes"):
        VectorDoubleQAgent(env, storage="hash", capacity=64, max_bytes=4 * 64 * 68 + 4 * 12 - 1,
                           **HP)
    assert torch.cuda.mem_get_info()[0] >= free - (1 << 20)  # nothing was allocated
    agent = VectorDoubleQAgent(env, max_bytes=4 * 5 * 9 ** 4 * 64, **HP)
    with pytest.raises(ValueError, match="capacity"):
        VectorDoubleQAgent(env, storage="hash", **HP)
    with pytest.raises(ValueError, match="capacity"):
        VectorDoubleQAgent(env, capacity=64, **HP)
    for bad in (100, 8, 0, 1 << 31):
        with pytest.raises(ValueError, match="power of two"):
            VectorDoubleQAgent(env, storage="hash", capacity=bad, **HP)
    with pytest.raises(ValueError, match="storage"):
        VectorDoubleQAgent(env, storage="sparse", capacity=64, **HP)
    with pytest.raises(ValueError, match="per table"):
        VectorDoubleQAgent(env, learning_rate=[0.1, 0.2], **{k: v for k, v in HP.items()
                                                             if k != "learning_rate"})
    with pytest.raises(ValueError, match="one table id"):
        VectorDoubleQAgent(env, tables=[0, 1], **HP)
    for name in ("lookup", "rehash"):
        with pytest.raises(ValueError, match="hash"):
            getattr(agent, name)(*(([0], [0]) if name == "lookup" else (64,)))
    with pytest.raises(ValueError, match="one per instance"):
        agent.update(coins=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one per instance"):
        agent.update(next_actions=torch.zeros(5, dtype=torch.int32))
    hashed = VectorDoubleQAgent(env, storage="hash", capacity=64,
                                max_bytes=4 * 64 * 68 + 4 * 12, **HP)
    with pytest.raises(MemoryError, match="max_bytes"):
        hashed.rehash(128)
    with pytest.raises(ValueError):
        hashed.rehash(100)
    with pytest.raises(ValueError, match="grow_every"):
        VectorTabularTrainer(env, hashed, grow_every=33)
    VectorTabularTrainer(env, hashed, grow_every=32)
    # the ABI's own refusals, with device pointers
    L = env.lib
    args = [env.obs6.data_ptr(), 4, 9, None, 4, None, agent.q.data_ptr(),
            agent.steps_done.data_ptr(),
            agent.eps_init.data_ptr(), agent.eps_final.data_ptr(), agent.eps_decay.data_ptr(), 0, 0,
            agent.actions.data_ptr(), agent.sidx.data_ptr(), None]
    for pos, bad in ((6, None), (1, 0), (2, 200)):  # a NULL table, n <= 0, max_dim out of range
        a = list(args)
        a[pos] = bad
        assert L.mz_dqtab_act(*a) == -1
        assert L.mz_last_error()
    env.close()
