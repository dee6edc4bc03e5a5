"""VectorQAgent / VectorTabularTrainer (csrc/mz_qtab.hip): a population of tabular Q-learners on
the GPU against a CPU restatement of the reference's QAgent (agents/q_agent.py) and
OffPolicyTrainer.train (lib/trainers/off_policy_trainer.py:28-80) written here: one oracle env per
instance, a dict of np.zeros(4) rows per table keyed by (pos, goal, best_dir), the same Philox
draws, math.exp for epsilon. One instance per table must be equal bit for bit; shared tables are
pinned where the float64 adds commute exactly (disjoint rows; equal addends)."""
import functools
import math
import re

import numpy as np
import pytest

import golden_io as G
import pyoracle as O

SEED = 0x7AB
STREAM = 0x71746162  # MZ_QTAB_STREAM
HP = dict(learning_rate=0.1, initial_epsilon=0.95, epsilon_decay=40.0, final_epsilon=0.05,
          discount_factor=0.7, eta=0.01)
GAP = 1e-9  # no draw may sit this close to epsilon: the device exp may differ from libm by an ulp


@functools.lru_cache(maxsize=None)
def nine(toroidal):
    return [m for m in G.mazes("gen_toroid.npz" if toroidal else "gen_euclid.npz") if m["n"] == 9]


def per_table(v, T):
    v = list(v) if isinstance(v, (list, tuple)) else [v] * T
    assert len(v) == T
    return [float(x) for x in v]


class Restated:
    """The CPU yardstick. table_of None: one table per instance."""

    def __init__(self, mazes, toroidal, table_of=None, seed=SEED, episode_end=True, **hp):
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
        self.seed, self.counter = seed, 0
        self.min_gap = float("inf")
        self.envs, self.goal, self.obs = [None] * self.n, [None] * self.n, [None] * self.n
        self.written = [set() for _ in range(self.n)]
        self.read = [set() for _ in range(self.n)]
        for i, m in enumerate(mazes):
            self.set_maze(i, m["grid"], m["start"], m["goal"])

    def set_maze(self, i, grid, start, goal):
        self.envs[i] = O.Env(grid, start, goal, self.toroidal, False)
        self.goal[i] = tuple(goal)
        self.obs[i] = self.envs[i].reset()

    def key(self, i, o=None):
        o = self.obs[i] if o is None else o
        return (tuple(o["pos"]), self.goal[i], tuple(o["best_dir"]))

    def row(self, t, k):
        return self.tables[t].setdefault(k, np.zeros(4))

    def act(self, active=None):
        before = list(self.steps_done)
        acts = []
        for i in range(self.n):
            if active is not None and not active[i]:
                acts.append(-1)
                continue
            t = self.table_of[i]
            eps = self.ef[t] + (self.ei[t] - self.ef[t]) * math.exp(-1. * before[t] / self.decay[t])
            w = O.philox(self.seed, STREAM ^ (i << 32), self.counter)
            u = (w[0] >> 8) * 2.0 ** -24
            self.min_gap = min(self.min_gap, abs(u - eps))
            self.read[i].add(self.key(i))
            acts.append(w[1] >> 30 if u < eps else int(np.argmax(self.row(t, self.key(i)))))
            self.steps_done[t] += 1
        self.counter += 1
        return acts

    def step(self, actions=None, episode_end=True):
        """One vector step on independent tables (or tables whose instances touch disjoint
        rows); a finished instance replays its maze. Returns (actions, terminated, truncated)."""
        acts = self.act() if actions is None else list(actions)
        term, trunc = [], []
        for i, a in enumerate(acts):
            t = self.table_of[i]
            k = self.key(i)
            o = self.envs[i].step(a)
            k2 = self.key(i, o)
            self.read[i].add(k2)
            self.written[i].add(k)
            r, te, tr = o["reward"], o["terminated"], o["truncated"]
            q = self.row(t, k)
            future = 0.0 if te else float(np.max(self.row(t, k2)))
            td = (r + self.gamma[t] * future) - q[a]
            q[a] = q[a] + self.lr[t] * td
            self.cum[i] += r
            self.obs[i] = o
            if te or tr:
                if episode_end:
                    self.gamma[t] += self.eta[t] if self.cum[i] > 0 else -self.eta[t]
                    self.cum[i] = 0.0
                    self.episodes[t] += 1
                    self.wins[t] += int(te)
                self.obs[i] = self.envs[i].reset()
            term.append(te)
            trunc.append(tr)
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
    rs = Restated(nine(toroidal)[:n], toroidal, **hp)
    log = [rs.step() for _ in range(steps)]
    assert rs.min_gap >= GAP, rs.min_gap  # the precondition of every bit-exact comparison
    return rs, log


def varied_hp(T):
    return dict(learning_rate=[0.05 + 0.01 * t for t in range(T)],
                discount_factor=[0.5 + 0.015 * t for t in range(T)],
                eta=[0.002 * (t % 5) for t in range(T)],
                epsilon_decay=[20.0 + 3.0 * t for t in range(T)])


# ---------------------------------------------------------------------------------------------
# 1. the index (CPU)
def test_state_index_is_injective_on_every_golden_maze():
    from mazerl.agents.vector_q import state_index, table_rows
    rows = table_rows(9)
    assert rows == 5 * 9 ** 4
    rng = np.random.default_rng(5)
    wrapped = set()
    for toroidal in (False, True):
        for m in nine(toroidal):
            e = O.Env(m["grid"], m["start"], m["goal"], toroidal, False)
            seen = {}
            o = e.reset()
            for a in rng.integers(0, 4, 400):
                k = (tuple(o["pos"]), tuple(m["goal"]), tuple(o["best_dir"]))
                s = state_index(9, *k)
                assert 0 <= s < rows
                assert seen.setdefault(s, k) == k  # one row, one key
                if toroidal and max(abs(k[2][0]), abs(k[2][1])) > 1:
                    wrapped.add((k[0][0] in (0, 8), k[0][1] in (0, 8), k[2]))
                o = e.step(int(a))
                if o["terminated"] or o["truncated"]:
                    o = e.reset()
            assert len(set(seen.values())) == len(seen)  # one key, one row
    # wrapped best dirs were seen in both directions on both axes, at rows / columns 0 and 8
    assert {w[2] for w in wrapped} == {(8, 0), (-8, 0), (0, 8), (0, -8)}
    # at one cell the four moves and "none" take five rows, wrapped or not
    for cell in ((0, 0), (8, 8), (0, 8), (4, 4)):
        r, c = cell
        dirs = [(0, 0)] + [(r - (r + dr) % 9, c - (c + dc) % 9)
                           for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1))]
        assert sorted(state_index(9, cell, (2, 2), d) % 5 for d in dirs) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        state_index(9, (9, 0), (1, 1), (0, 0))


# ---------------------------------------------------------------------------------------------
# GPU
torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make(mazes, toroidal=False, tables=None, regen_won=False, seed=SEED, keep_flags=True, **hp):
    import mazerl
    from mazerl.agents.vector_q import VectorQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env = mazerl.VectorMazeEnv(len(mazes), 9, toroidal=toroidal, enrich=False, reward64=True,
                               generate=False)
    env.load_mazes(np.stack([m["grid"] for m in mazes]),
                   np.array([list(m["start"]) + list(m["goal"]) for m in mazes]))
    env.reset()
    agent = VectorQAgent(env, tables=tables, seed=seed, **{**HP, **hp})
    return env, agent, VectorTabularTrainer(env, agent, regen_won=regen_won, keep_flags=keep_flags)


def run_logged(trainer, steps):
    a, te, tr = [], [], []
    for _ in range(steps):
        trainer.vector_step()
        a.append(trainer.agent.actions.clone())
        te.append(trainer.terminated.clone())
        tr.append(trainer.truncated.clone())
    return [torch.stack(x).cpu().numpy() for x in (a, te, tr)]


def assert_log(got, log):
    for name, g, want in zip(("actions", "terminated", "truncated"), got, zip(*log)):
        want = np.array(want)
        bad = np.argwhere(g.astype(np.int64) != want.astype(np.int64))
        assert bad.size == 0, (name, "first difference at (step, instance)", bad[0])


def assert_tables(q, rs, tables=None):
    """q [T, rows, 4] (numpy) holds exactly the restatement's rows; every other row is 0."""
    from mazerl.agents.vector_q import state_index
    for t in (range(rs.T) if tables is None else tables):
        want = np.zeros_like(q[t])
        for k, v in rs.tables[t].items():
            want[state_index(9, *k)] = v
        bad = np.argwhere(q[t] != want)
        assert bad.size == 0, ("table", t, "row", bad[0], q[t][bad[0][0]], want[bad[0][0]])


def assert_agent(agent, rs):
    assert_tables(agent.q.cpu().numpy(), rs)
    assert agent.gamma.cpu().tolist() == rs.gamma
    assert agent.steps_done.cpu().tolist() == rs.steps_done
    assert agent.wins.cpu().tolist() == rs.wins
    assert agent.episodes.cpu().tolist() == rs.episodes


# 2. the reference's own fixture
@gpu
def test_fixture_replay_matches_reference_q_table():
    need_gpu()
    from mazerl.agents.vector_q import state_index
    fx = G.load("agents.npz")
    t = [t for t in G.traces() if t["kind"] == G.KIND_SIMPLE][int(fx["q.trace_index"])]
    env, agent, _ = make([t])  # lr 0.1, gamma 0.7, eta 0.01 (make_golden_agents.py:89)
    for op in t["op"][:600]:
        if op == 4:
            env.reset()
            continue
        agent.act()  # the row acted from; its own action is not taken
        a = torch.tensor([int(op)], dtype=torch.int32, device=env.device)
        env.step(a)
        agent.update(actions=a, episode_end=False)  # QAgent.update alone, as the fixture's loop
    want = np.zeros((agent.rows, 4))
    for k, v in zip(fx["q.keys"], fx["q.values"]):
        x = [int(s) for s in re.findall(r"-?\d+", str(k).replace("int32", ""))]
        assert len(x) == 6, k
        want[state_index(9, x[0:2], x[2:4], x[4:6])] = v
    got = agent.q[0].cpu().numpy()
    assert np.count_nonzero(want.any(1)) > 10
    assert np.array_equal(got, want)
    assert agent.gamma.cpu().tolist() == [0.7]
    env.close()


# 3. independent learners, fixed mazes (and 8: evaluate)
@pytest.fixture(scope="module")
def trained():
    """Per geometry: the GPU population after 600 vector steps on the 24 golden mazes."""
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
    rs, log = restated_run(toroidal, 600)
    env, agent, trainer, got, sd = trained(toroidal)
    assert_log(got, log)
    assert sum(rs.wins) > 100 and sum(rs.episodes) > sum(rs.wins)  # every branch was taken
    assert_tables(sd["q"].cpu().numpy(), rs)
    assert sd["gamma"].cpu().tolist() == rs.gamma
    assert sd["steps_done"].cpu().tolist() == rs.steps_done == [600] * 24
    assert sd["wins"].cpu().tolist() == rs.wins
    assert sd["episodes"].cpu().tolist() == rs.episodes


# 4. per-table hyper-parameters
@gpu
def test_per_table_hyperparameters():
    need_gpu()
    rs, log = restated_run(False, 200, varied=True)
    env, agent, trainer = make(nine(False), **varied_hp(24))
    assert_log(run_logged(trainer, 200), log)
    assert_agent(agent, rs)
    env.close()


# 5. a win gives a new maze
@gpu
def test_win_gives_a_new_maze():
    need_gpu()
    mazes = nine(False)[:16]
    rs = Restated(mazes, False, **HP)
    env, agent, trainer = make(mazes, regen_won=True)
    regenerated = 0
    for step in range(200):
        trainer.vector_step()
        acts, term, trunc = rs.step()
        assert agent.actions.cpu().tolist() == acts, step
        assert trainer.terminated.cpu().tolist() == [int(x) for x in term], step
        assert trainer.truncated.cpu().tolist() == [int(x) for x in trunc], step
        for i in np.flatnonzero(term):
            q = env.query(int(i))
            rs.set_maze(int(i), env.grid(int(i)), (q["start_r"], q["start_c"]),
                        (q["goal_r"], q["goal_c"]))
            regenerated += 1
    assert rs.min_gap >= GAP, rs.min_gap
    assert regenerated > 0  # (the restatement's wins: the new-maze path was taken)
    assert_agent(agent, rs)
    env.close()


# 6. shared table, disjoint rows
@gpu
@pytest.mark.parametrize("toroidal", [False, True])
def test_shared_table_on_disjoint_rows_is_the_union(toroidal):
    """Instances whose rows (read or written over the run) meet nobody else's written rows share
    table 0; the others keep a table each, so every instance keeps its Philox stream. eta = 0
    (one shared gamma would otherwise drift with every instance's episodes) and the shared
    table's decay is scaled by its instances: steps_done advances by that many per step, and
    (k m) / (40 m) rounds like k / 40.
    At least 8 instances must share the table. The 24 euclidean mazes cannot give 8: they have 7
    distinct targets, and every two of them with one target write the row of a common cell next
    to it (checked below: the kept set is one maze per target) — so the bound of 8 is held on
    the 24 toroidal mazes (15 targets), and the euclidean set runs with its 7."""
    need_gpu()
    from mazerl.agents.vector_q import state_index
    mazes = nine(toroidal)
    rs, log = restated_run(toroidal, 300, eta=0.0)
    rows_w = [{state_index(9, *k) for k in rs.written[i]} for i in range(24)]
    rows_r = [{state_index(9, *k) for k in rs.read[i]} for i in range(24)]
    kept = []
    for i in range(24):
        if all(not (rows_w[i] & (rows_w[j] | rows_r[j])) and not (rows_r[i] & rows_w[j])
               for j in kept):
            kept.append(i)
    if toroidal:
        assert len(kept) >= 8, kept
    else:
        assert len(kept) == len({x["goal"] for x in mazes}) == 7, kept
    m = len(kept)
    table_of, decay = [], [40.0 * m]
    for i in range(24):
        table_of.append(0 if i in kept else len(decay))
        if i not in kept:
            decay.append(40.0)
    env, agent, trainer = make(mazes, toroidal, tables=torch.tensor(table_of), eta=0.0,
                               epsilon_decay=decay)
    assert_log(run_logged(trainer, 300), log)
    q = agent.q.cpu().numpy()
    union = np.zeros_like(q[0])
    for i in kept:
        for k, v in rs.tables[i].items():
            s = state_index(9, *k)
            assert not union[s].any() or not v.any()
            union[s] += v
    assert np.array_equal(q[0], union)
    assert int(agent.steps_done[0]) == 300 * m
    assert int(agent.episodes[0]) == sum(rs.episodes[i] for i in kept)
    assert int(agent.wins[0]) == sum(rs.wins[i] for i in kept)
    # the same union from the GPU's own independent run
    env2, agent2, trainer2 = make(mazes, toroidal, eta=0.0)
    trainer2.train(300)
    assert np.array_equal(q[0], agent2.q[kept].sum(0).cpu().numpy())
    env.close()
    env2.close()


# 7. shared table, collisions
@gpu
def test_shared_table_collisions_add():
    need_gpu()
    from mazerl.agents.vector_q import state_index
    m = nine(False)[0]
    rs = Restated([m] * 256, False, table_of=[0] * 256, **HP)
    acts = rs.act()
    assert rs.min_gap >= GAP
    env, agent, trainer = make([m] * 256, tables=1)
    trainer.vector_step()
    assert agent.actions.cpu().tolist() == acts
    counts = np.bincount(acts, minlength=4)
    assert counts.min() > 20  # eps = 0.95: every action is taken many times
    s0 = state_index(9, *rs.key(0))
    want = np.zeros((agent.rows, 4))
    for a in range(4):
        e = O.Env(m["grid"], m["start"], m["goal"], False, False)
        e.reset()
        add = 0.1 * ((e.step(a)["reward"] + 0.7 * 0.0) - 0.0)
        x = 0.0
        for _ in range(counts[a]):
            x = x + add
        want[s0][a] = x
    assert np.array_equal(agent.q[0].cpu().numpy(), want)
    assert int(agent.steps_done[0]) == 256
    env.close()


# 8. evaluate
@gpu
def test_evaluate(trained):
    need_gpu()
    rs0, _ = restated_run(False, 600)
    env, agent, trainer, _, sd = trained(False)
    # continue the shared restatement on a copy of what evaluate reads and advances
    rs = Restated(nine(False), False, **HP)
    rs.tables = [{k: v.copy() for k, v in t.items()} for t in rs0.tables]
    rs.steps_done, rs.counter = list(rs0.steps_done), rs0.counter
    want = rs.evaluate()
    assert rs.min_gap >= GAP, rs.min_gap
    won, rate = trainer.evaluate(new=False)
    assert won.cpu().tolist() == want
    assert rate == sum(want) / 24 and 0 < sum(want)
    assert agent.steps_done.cpu().tolist() == rs.steps_done
    won, rate = trainer.evaluate(new=True)
    assert 0.0 <= rate <= 1.0 and won.shape == (24,)
    assert torch.equal(agent.q, sd["q"])
    assert torch.equal(agent.gamma, sd["gamma"])


# 9. checkpoint
@gpu
def test_checkpoint_resumes_bit_exactly():
    need_gpu()
    mazes = nine(False)[:16]
    env, agent, trainer = make(mazes, regen_won=True)
    trainer.train(50)
    sd_a, sd_e = agent.state_dict(), env.state_dict()
    trainer.train(50)
    env2, agent2, trainer2 = make(mazes, regen_won=True, seed=1)
    env2.load_state_dict(sd_e)
    agent2.load_state_dict(sd_a)
    trainer2.train(50)
    assert torch.equal(agent2.q, agent.q) and bool(agent.q.any())
    assert torch.equal(agent2.gamma, agent.gamma)
    assert torch.equal(agent2.steps_done, agent.steps_done)
    assert torch.equal(agent2.wins, agent.wins) and int(agent.wins.sum()) > 0
    env.close()
    env2.close()


# 10. refusals
@gpu
def test_refusals():
    need_gpu()
    import mazerl
    from mazerl import _native as N
    from mazerl.agents.vector_q import VectorQAgent
    env = mazerl.VectorMazeEnv(4, 15, enrich=True, reward64=True)
    with pytest.raises(ValueError, match="enrich=False"):
        VectorQAgent(env, **HP)
    env.close()
    env = mazerl.VectorMazeEnv(4, 9, enrich=False, reward64=False)
    with pytest.raises(ValueError, match="reward64=True"):
        VectorQAgent(env, **HP)
    env.close()
    env = mazerl.VectorMazeEnv(4, 9, enrich=False, reward64=True)
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(MemoryError, match="max_bytes"):
        VectorQAgent(env, max_bytes=4 * 5 * 9 ** 4 * 32 - 1, **HP)
    assert torch.cuda.mem_get_info()[0] >= free - (1 << 20)  # nothing was allocated
    agent = VectorQAgent(env, max_bytes=4 * 5 * 9 ** 4 * 32, **HP)
    # the ABI's own refusals
    L = env.lib
    rows = N.C.c_int64()
    assert L.mz_qtab_states(4, N.C.byref(rows)) == -1 and L.mz_qtab_states(128, N.C.byref(rows)) == -1
    args = [env.obs6.data_ptr(), 4, 9, None, 4, None, agent.q.data_ptr(), agent.steps_done.data_ptr(),
            agent.eps_init.data_ptr(), agent.eps_final.data_ptr(), agent.eps_decay.data_ptr(), 0, 0,
            agent.actions.data_ptr(), agent.sidx.data_ptr(), None]
    for pos, bad in ((6, None), (1, 0), (2, 200)):  # a NULL table, n <= 0, max_dim out of range
        a = list(args)
        a[pos] = bad
        assert L.mz_qtab_act(*a) == -1
        assert L.mz_last_error()
    env.close()
