"""VectorQAgent(storage="hash") (csrc/mz_qtab.hip, Hashed): the population of tabular Q-learners on
open-addressing hash tables in HBM, against the CPU restatement of tests/test_vector_q.py (shared,
never modified) and against the dense storage. Everything is compared with == on float64 bits."""
import ctypes

import numpy as np
import pytest

import pyoracle as O
from test_vector_q import (GAP, HP, Restated, assert_log, make, need_gpu, nine, restated_run,
                           run_logged, varied_hp)


def reachable_keys(m, toroidal, steps=2000, seed=5):
    """State indices a random walk meets on one golden maze."""
    from mazerl.agents.vector_q import state_index
    e = O.Env(m["grid"], m["start"], m["goal"], toroidal, False)
    o, seen = e.reset(), set()
    for a in np.random.default_rng(seed).integers(0, 4, steps):
        seen.add(state_index(9, tuple(o["pos"]), tuple(m["goal"]), tuple(o["best_dir"])))
        o = e.step(int(a))
        if o["terminated"] or o["truncated"]:
            o = e.reset()
    return seen


# ---------------------------------------------------------------------------------------------
# 1. the hash mirror (CPU)
def test_hash_slot_probe_covers_the_table_and_spreads_the_keys():
    from mazerl.agents.vector_q import hash_slot
    for C in (16, 64, 4096):
        for key in (0, 1, 12345, 5 * 9 ** 4 - 1, 5 * 127 ** 4 - 1):
            s0 = hash_slot(key, C)
            assert 0 <= s0 < C
            assert sorted((s0 + j) % C for j in range(C)) == list(range(C))
    assert hash_slot(1, 16) == 0x9E3779B1 >> 28
    assert hash_slot(3, 1 << 30) == (3 * 0x9E3779B1 % 2 ** 32) >> 2
    for toroidal in (False, True):
        for m in nine(toroidal):
            keys = reachable_keys(m, toroidal)
            assert len(keys) >= 8
            for C in (16, 64, 4096):
                assert len({hash_slot(k, C) for k in keys}) >= min(C, len(keys)) / 2, (C, len(keys))
    for bad in (0, 8, 24, 100, (1 << 30) + 1, 1 << 31):
        with pytest.raises(ValueError):
            hash_slot(1, bad)


# 2. the ABI's argument checks need no GPU
def test_hash_abi_refuses_bad_arguments_without_a_gpu():
    from mazerl import _native as N
    L = N.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 63) & ~63  # a 64-B aligned host address: never dereferenced
    act = [p, 4, 9, None, 4, None, p, p, 64, p, p, p, p, 0, 0, p, p, None]
    upd = [p, 4, 9, None, 4, p, p, 64] + [p] * 14 + [1, None]
    reh = [p, p, 64, p + 1024, p + 1024, 128, 4, p, None]
    look = [p, p, 64, 4, p, p, 4, p, p, None]
    cases = [
        (L.mz_qtab_hash_act, act, {8: (0, 8, 24, 100, -16, (1 << 30) + 1, 1 << 31), 6: (None,),
                                   7: (None,), 1: (0, -1), 2: (200,), 9: (None,)}),
        (L.mz_qtab_hash_update, upd, {7: (0, 8, 48, 1 << 31), 5: (None,), 6: (None,), 1: (-1,),
                                      8: (None,), 9: (None,)}),
        (L.mz_qtab_hash_rehash, reh, {2: (24,), 5: (8, 96), 0: (None,), 1: (None,), 3: (None,),
                                      4: (None,), 6: (0, -1), 7: (None,)}),
        (L.mz_qtab_hash_lookup, look, {2: (63,), 0: (None,), 1: (None,), 6: (-1,), 4: (None,),
                                       7: (None,)}),
    ]
    for fn, good, bads in cases:
        for pos, values in bads.items():
            for v in values:
                a = list(good)
                a[pos] = v
                assert fn(*a) == -1, (fn.__name__, pos, v)
                assert L.mz_last_error()
    look[6] = 0
    assert L.mz_qtab_hash_lookup(*look) == 0  # nothing to look up: no launch, no GPU
    upd[6] = p + 8
    assert L.mz_qtab_hash_update(*upd) == -5  # vals are read 32 B at a time


# ---------------------------------------------------------------------------------------------
# GPU
torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


def make_hash(mazes, toroidal=False, capacity=64, grow_every=0, regen_won=False, **kw):
    """test_vector_q.make with hashed tables (and a trainer that knows grow_every)."""
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env, agent, _ = make(mazes, toroidal, regen_won=regen_won, storage="hash", capacity=capacity,
                         **kw)
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
    return np.array(keys, dtype=np.int64), np.array([rows[k] for k in keys]).reshape(-1, 4)


def items_np(agent, t):
    k, r = agent.items(t)
    return k.cpu().numpy(), r.cpu().numpy()


def assert_items(agent, rs, tables=None):
    for t in (range(rs.T) if tables is None else tables):
        gk, gr = items_np(agent, t)
        wk, wr = written_items(rs, t)
        assert np.array_equal(gk, wk), ("table", t, gk, wk)
        assert np.array_equal(gr, wr), ("table", t)


def assert_hashed_agent(agent, rs):
    assert_items(agent, rs)
    assert agent.gamma.cpu().tolist() == rs.gamma
    assert agent.steps_done.cpu().tolist() == rs.steps_done
    assert agent.wins.cpu().tolist() == rs.wins
    assert agent.episodes.cpu().tolist() == rs.episodes
    assert agent.load.cpu().tolist() == [len(rs.written[t]) for t in range(rs.T)]
    assert int(agent.overflow.sum()) == 0


@pytest.fixture(scope="module")
def trained():
    """Per geometry: the hashed population (capacity 64) after 600 vector steps on the 24
    golden mazes, its log and its state_dict at that point."""
    out = {}

    def get(toroidal):
        if toroidal not in out:
            env, agent, trainer = make_hash(nine(toroidal), toroidal, capacity=64)
            got = run_logged(trainer, 600)
            out[toroidal] = (env, agent, trainer, got, agent.state_dict())
        return out[toroidal]
    yield get
    for env, *_ in out.values():
        env.close()


# 3. one instance per table, at a load factor that forces probing
@gpu
@pytest.mark.parametrize("toroidal", [False, True])
def test_hashed_learners_equal_the_restatement(trained, toroidal):
    need_gpu()
    from mazerl.agents.vector_q import VectorQAgent, hash_slot
    rs, log = restated_run(toroidal, 600)
    env, agent, trainer, got, sd = trained(toroidal)
    assert not hasattr(agent, "q") and agent.storage == "hash" and agent.capacity == 64
    assert_log(got, log)
    fresh = VectorQAgent(env, storage="hash", capacity=64, **HP)
    fresh.load_state_dict(sd)  # (evaluate, in another test, may have advanced the fixture's agent)
    assert_hashed_agent(fresh, rs)
    assert sd["steps_done"].cpu().tolist() == [600] * 24
    assert max(len(w) for w in rs.written) > 64 // 4  # loads above 1/4: chains form
    # q_row and to_dense read the same rows
    t = max(range(24), key=lambda i: len(rs.written[i]))
    for k in list(rs.written[t])[:5]:
        assert fresh.q_row(t, *k).cpu().tolist() == rs.tables[t][k].tolist()
    keys, rows = fresh.items(t)
    dense = fresh.to_dense(t)
    assert torch.equal(dense[keys], rows) and int(dense.ne(0).any(1).sum()) <= keys.numel()
    # absent keys read as the zero row, slot -1
    r, s = fresh.lookup([t, t], [int(keys[0]), 5 * 9 ** 4 - 1])
    assert torch.equal(r[0], rows[0]) and s.cpu().tolist()[1] == -1 and not bool(r[1].any())
    # probing happened: some key sits away from its start slot
    kt = sd["keys"].cpu().numpy()
    away = sum(int(hash_slot(int(k), 64) != slot) for row in kt for slot, k in enumerate(row)
               if k >= 0)
    assert away > 0


# 4. hashed == dense at a size with regeneration
@gpu
def test_hashed_equals_dense_at_21_with_regeneration():
    need_gpu()
    import mazerl
    from mazerl.agents.vector_q import VectorQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    runs = []
    for kw in (dict(storage="dense"), dict(storage="hash", capacity=1024)):
        env = mazerl.VectorMazeEnv(16, 21, enrich=False, reward64=True, seed=0x5EED0021)
        agent = VectorQAgent(env, seed=3, **HP, **kw)
        trainer = VectorTabularTrainer(env, agent, regen_won=True, keep_flags=True)
        runs.append((env, agent, run_logged(trainer, 400)))
    (env_d, dense, log_d), (env_h, hashed, log_h) = runs
    for a, b in zip(log_d, log_h):
        assert np.array_equal(a, b)
    for t in range(16):
        (kd, rd), (kh, rh) = items_np(dense, t), items_np(hashed, t)
        assert np.array_equal(kd, kh[rh.any(1)]) and np.array_equal(rd, rh[rh.any(1)])
        assert len(kh) == int(hashed.load[t]) >= len(kd) > 0
    for name in ("gamma", "steps_done", "wins", "episodes", "cum"):
        assert torch.equal(getattr(dense, name), getattr(hashed, name)), name
    assert int(hashed.overflow.sum()) == 0
    print("wins", int(dense.wins.sum()), "episodes", int(dense.episodes.sum()))
    env_d.close()
    env_h.close()


# 5. per-table hyper-parameters
@gpu
def test_hashed_per_table_hyperparameters():
    need_gpu()
    rs, log = restated_run(False, 200, varied=True)
    env, agent, trainer = make_hash(nine(False), capacity=64, **varied_hp(24))
    assert_log(run_logged(trainer, 200), log)
    assert_hashed_agent(agent, rs)
    env.close()


# 6. shared table, disjoint rows: concurrent inserts of different keys
@gpu
@pytest.mark.parametrize("toroidal", [False, True])
def test_hashed_shared_table_on_disjoint_rows_is_the_union(toroidal):
    """The hashed counterpart of test_shared_table_on_disjoint_rows_is_the_union, with its maze
    selection rule (at least 8 mazes kept on the toroidal set, the 7 targets on the euclidean)."""
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
    env, agent, trainer = make_hash(mazes, toroidal, capacity=1024, tables=torch.tensor(table_of),
                                    eta=0.0, epsilon_decay=decay)
    assert_log(run_logged(trainer, 300), log)
    gk, gr = items_np(agent, 0)
    wk, wr = written_items(rs, 0, instances=kept)
    assert np.array_equal(gk, wk) and np.array_equal(gr, wr)
    assert int(agent.load[0]) == len(set().union(*(rows_w[i] for i in kept))) == len(wk)
    assert int(agent.overflow.sum()) == 0
    assert int(agent.steps_done[0]) == 300 * m
    assert int(agent.episodes[0]) == sum(rs.episodes[i] for i in kept)
    assert int(agent.wins[0]) == sum(rs.wins[i] for i in kept)
    # the same union from the GPU's own independent hashed run
    env2, agent2, trainer2 = make_hash(mazes, toroidal, capacity=1024, eta=0.0)
    trainer2.train(300)
    union = {}
    for i in kept:
        for k, r in zip(*items_np(agent2, i)):
            assert k not in union
            union[int(k)] = r
    assert sorted(union) == gk.tolist()
    assert np.array_equal(np.array([union[k] for k in sorted(union)]), gr)
    env.close()
    env2.close()


# 7. shared table, one key from many lanes: the lanes that lose the claim
@gpu
def test_hashed_shared_table_same_key_from_many_lanes():
    need_gpu()
    from mazerl.agents.vector_q import state_index
    m = nine(False)[0]
    rs = Restated([m] * 256, False, table_of=[0] * 256, **HP)
    acts = rs.act()
    assert rs.min_gap >= GAP
    env, agent, trainer = make_hash([m] * 256, capacity=16, tables=1)
    got = run_logged(trainer, 1)
    assert got[0][0].tolist() == acts
    counts = np.bincount(acts, minlength=4)
    assert counts.min() > 20
    s0 = state_index(9, *rs.key(0))
    want = np.zeros(4)
    for a in range(4):
        e = O.Env(m["grid"], m["start"], m["goal"], False, False)
        e.reset()
        add = 0.1 * ((e.step(a)["reward"] + 0.7 * 0.0) - 0.0)
        x = 0.0
        for _ in range(counts[a]):
            x = x + add
        want[a] = x
    assert agent.load.cpu().tolist() == [1]
    keys, rows = items_np(agent, 0)
    assert keys.tolist() == [s0] and np.array_equal(rows[0], want)
    assert int(agent.steps_done[0]) == 256
    # 19 more steps; the keys written are those of a CPU replay of the logged actions
    more = run_logged(trainer, 19)
    actions = np.concatenate([got[0], more[0]])
    written = set()
    for i in range(256):
        e = O.Env(m["grid"], m["start"], m["goal"], False, False)
        o = e.reset()
        for a in actions[:, i]:
            written.add(state_index(9, tuple(o["pos"]), tuple(m["goal"]), tuple(o["best_dir"])))
            o = e.step(int(a))
            if o["terminated"] or o["truncated"]:
                o = e.reset()
    assert 1 < len(written) <= 16, len(written)  # the table holds them: nothing is dropped
    assert agent.load.cpu().tolist() == [len(written)]
    assert items_np(agent, 0)[0].tolist() == sorted(written)
    assert int(agent.overflow.sum()) == 0
    env.close()


# 8. a full table is defined, bounded and counted
@gpu
@pytest.mark.parametrize("toroidal", [False, True])
def test_full_table_drops_and_counts(toroidal):
    need_gpu()
    rs, log = restated_run(toroidal, 600)
    env, agent, trainer = make_hash(nine(toroidal), toroidal, capacity=16)
    got = run_logged(trainer, 600)  # completes: no probe spins on a full table
    fits = [t for t in range(24) if len(rs.written[t]) <= 16]
    full = [t for t in range(24) if len(rs.written[t]) > 16]
    assert fits and full, (fits, full)
    for g, want in zip(got, zip(*log)):
        assert np.array_equal(g[:, fits].astype(np.int64), np.array(want)[:, fits].astype(np.int64))
    assert_items(agent, rs, fits)
    load, over = agent.load.cpu().tolist(), agent.overflow.cpu().tolist()
    for name in ("gamma", "steps_done", "wins", "episodes"):
        have = getattr(agent, name).cpu().tolist()
        assert [have[t] for t in fits] == [getattr(rs, name)[t] for t in fits], name
    for t in fits:
        assert load[t] == len(rs.written[t]) and over[t] == 0, t
    for t in full:
        assert load[t] == 16 and over[t] > 0, t
    # the episode ends of a full table still ran
    assert agent.steps_done.cpu().tolist() == [600] * 24
    assert all(int(agent.episodes[t]) > 0 for t in full)
    env.close()


# 9. rehash and growth
@gpu
def test_rehash_keeps_the_tables_and_the_run(trained):
    need_gpu()
    rs, log = restated_run(False, 600)
    env, agent, trainer = make_hash(nine(False), capacity=64)
    got = run_logged(trainer, 100)
    before = [items_np(agent, t) for t in range(24)]
    load = agent.load.clone()
    with pytest.raises(ValueError):
        agent.rehash(8)
    with pytest.raises(ValueError):
        agent.rehash(100)
    agent.rehash(256)
    assert agent.capacity == 256 and tuple(agent.keys.shape) == (24, 256)
    assert tuple(agent.vals.shape) == (24, 256, 4)
    for t in range(24):
        k, r = items_np(agent, t)
        assert np.array_equal(k, before[t][0]) and np.array_equal(r, before[t][1])
    assert torch.equal(agent.load, load) and int(agent.overflow.sum()) == 0
    rest = run_logged(trainer, 500)
    assert_log([np.concatenate([a, b]) for a, b in zip(got, rest)], log)
    assert_hashed_agent(agent, rs)
    # test 3's result: the population that stayed at capacity 64
    sd = trained(False)[4]
    for name in ("gamma", "steps_done", "wins", "episodes", "load"):
        assert torch.equal(getattr(agent, name), sd[name]), name
    assert int(agent.load.max()) > 16
    with pytest.raises(ValueError):
        agent.rehash(16)  # below the load
    agent.rehash(1 << int(agent.load.max()).bit_length())  # down, but above the load
    assert agent.capacity < 256
    assert_hashed_agent(agent, rs)
    env.close()


@gpu
@pytest.mark.parametrize("toroidal", [False, True])
def test_growth_from_a_small_capacity_drops_nothing(toroidal):
    need_gpu()
    rs, log = restated_run(toroidal, 600)
    env, agent, trainer = make_hash(nine(toroidal), toroidal, capacity=16, grow_every=8)
    launches = trainer.launches_per_step
    assert_log(run_logged(trainer, 600), log)
    assert_hashed_agent(agent, rs)
    assert agent.capacity >= 64 and int(agent.load.max()) <= agent.capacity // 2
    assert trainer.launches_per_step == launches
    env.close()


# 10. evaluate and checkpoint
@gpu
def test_hashed_evaluate_does_not_insert(trained):
    need_gpu()
    rs0, _ = restated_run(False, 600)
    env, agent, trainer, _, sd = trained(False)
    agent.load_state_dict(sd)
    rs = Restated(nine(False), False, **HP)
    rs.tables = [{k: v.copy() for k, v in t.items()} for t in rs0.tables]
    rs.steps_done, rs.counter = list(rs0.steps_done), rs0.counter
    want = rs.evaluate()
    assert rs.min_gap >= GAP, rs.min_gap
    won, rate = trainer.evaluate(new=False)
    assert won.cpu().tolist() == want
    assert rate == sum(want) / 24 and 0 < sum(want)
    assert agent.steps_done.cpu().tolist() == rs.steps_done
    for name in ("keys", "vals", "load", "overflow", "gamma"):
        assert torch.equal(getattr(agent, name), sd[name]), name
    agent.load_state_dict(sd)  # leave the shared population as the fixture made it


@gpu
def test_hashed_checkpoint_resumes_bit_exactly():
    need_gpu()
    mazes = nine(False)[:16]
    env, agent, trainer = make_hash(mazes, capacity=64, regen_won=True)
    trainer.train(150)
    sd_a, sd_e = agent.state_dict(), env.state_dict()
    assert sd_a["format"] == "mazerl.VectorQAgent/2" and sd_a["capacity"] == 64
    trainer.train(150)
    env2, agent2, trainer2 = make_hash(mazes, capacity=128, regen_won=True, seed=1)
    env2.load_state_dict(sd_e)
    agent2.load_state_dict(sd_a)
    assert agent2.capacity == 64
    trainer2.train(150)
    for name in ("keys", "vals", "load", "overflow", "gamma", "steps_done", "wins", "episodes"):
        assert torch.equal(getattr(agent2, name), getattr(agent, name)), name
    assert int(agent.load.min()) > 0 and int(agent.wins.sum()) > 0
    # dense is format /1, hashed /2, and neither loads the other
    env3, dense, _ = make(mazes, regen_won=True)
    sd_d = dense.state_dict()
    assert sd_d["format"] == "mazerl.VectorQAgent/1" and "keys" not in sd_d
    with pytest.raises(ValueError):
        dense.load_state_dict(sd_a)
    with pytest.raises(ValueError):
        agent2.load_state_dict(sd_d)
    for e in (env, env2, env3):
        e.close()


# 11. the population that did not fit
@gpu
def test_population_at_41_fits_hashed_and_matches_dense():
    """1,024 learners at 41x41: dense tables would take 1,024 x 452 MB; hashed, capacity 4,096,
    they take 151 MB. Instances 0-3 are compared with a 4-instance dense run (1.8 GB): the env
    seeds instance i's first maze with seed + i and its later ones with seed + i + (epoch << 32),
    and the agent draws from Philox(seed, stream ^ (i << 32), counter), so an instance's mazes and
    draws do not depend on how many instances run beside it."""
    need_gpu()
    import mazerl
    from mazerl.agents.vector_q import VectorQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env = mazerl.VectorMazeEnv(1024, 41, enrich=False, reward64=True)
    with pytest.raises(MemoryError, match="max_bytes"):
        VectorQAgent(env, storage="dense", **HP)
    agent = VectorQAgent(env, storage="hash", capacity=4096, **HP)
    assert agent.keys.numel() == 1024 * 4096 and 1024 * 4096 * 36 + 1024 * 12 < 160 << 20
    trainer = VectorTabularTrainer(env, agent, regen_won=True, keep_flags=True)
    got = run_logged(trainer, 300)
    load = agent.load.cpu().numpy()
    assert int(agent.overflow.sum()) == 0
    assert load.min() >= 1 and load.max() <= 300
    assert agent.steps_done.cpu().tolist() == [300] * 1024
    assert bool((agent.episodes >= agent.wins).all())
    env4 = mazerl.VectorMazeEnv(4, 41, enrich=False, reward64=True)
    dense = VectorQAgent(env4, storage="dense", **HP)
    want = run_logged(VectorTabularTrainer(env4, dense, regen_won=True, keep_flags=True), 300)
    for g, w in zip(got, want):
        assert np.array_equal(g[:, :4], w)
    for t in range(4):
        (kd, rd), (kh, rh) = items_np(dense, t), items_np(agent, t)
        assert np.array_equal(kd, kh[rh.any(1)]) and np.array_equal(rd, rh[rh.any(1)])
        assert len(kh) == load[t]
    for name in ("gamma", "wins", "episodes"):
        assert torch.equal(getattr(dense, name), getattr(agent, name)[:4]), name
    env.close()
    env4.close()


# 12. refusals
@gpu
def test_hashed_refusals():
    need_gpu()
    import mazerl
    from mazerl.agents.vector_q import VectorQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env = mazerl.VectorMazeEnv(8, 9, enrich=False, reward64=True)
    with pytest.raises(ValueError, match="capacity"):
        VectorQAgent(env, storage="hash", **HP)
    for bad in (100, 8, 0, 1 << 31):
        with pytest.raises(ValueError, match="power of two"):
            VectorQAgent(env, storage="hash", capacity=bad, **HP)
    with pytest.raises(ValueError, match="storage"):
        VectorQAgent(env, storage="sparse", capacity=64, **HP)
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(MemoryError, match="max_bytes"):
        VectorQAgent(env, storage="hash", capacity=64, max_bytes=8 * 64 * 36 + 8 * 12 - 1, **HP)
    assert torch.cuda.mem_get_info()[0] >= free - (1 << 20)
    agent = VectorQAgent(env, storage="hash", capacity=64, max_bytes=8 * 64 * 36 + 8 * 12, **HP)
    with pytest.raises(MemoryError, match="max_bytes"):
        agent.rehash(128)
    with pytest.raises(ValueError, match="grow_every"):
        VectorTabularTrainer(env, agent, grow_every=33)
    VectorTabularTrainer(env, agent, grow_every=32)
    # shared tables: the bound counts the instances of the fullest-shared table
    shared = VectorQAgent(env, tables=2, storage="hash", capacity=64, **HP)
    with pytest.raises(ValueError, match="grow_every"):
        VectorTabularTrainer(env, shared, grow_every=9)
    VectorTabularTrainer(env, shared, grow_every=8)
    env.close()
