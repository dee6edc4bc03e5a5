"""VectorTabularTrainer's archive, growth, evaluate_explored and checkpoints against the CPU
restatement of test_vector_q.py (one oracle env per instance, the same Philox draws), extended
here by what the reference does with its mazes: `env.mazes` keeps the first maze and every
update_maze() replacement (simple_maze_env.py:34,91), test(n, new=False) replays them
(off_policy_trainer.py:84-119), and the variable-size envs grow by 4 per win up to max_shape, where
the trainer returns (simple_variable_maze_env.py:93-112, off_policy_trainer.py:60-75). As there,
a winner's new maze is read back from the GPU env (the restatement has no generator of its own).
Every comparison is exact."""
import numpy as np
import pytest

from test_vector_q import GAP, Restated, assert_agent, assert_log, make, nine, run_logged

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

SEED = 0x7AB
HP = dict(learning_rate=0.1, initial_epsilon=0.95, epsilon_decay=40.0, final_epsilon=0.05,
          discount_factor=0.7, eta=0.01)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def read_maze(env, i):
    q = env.query(int(i))
    return env.grid(int(i)), (q["start_r"], q["start_c"]), (q["goal_r"], q["goal_c"])


def entry_maze(arch, lin):
    """Entry `lin` of an archive as (grid, start, goal)."""
    from mazerl.archive import unpack_grid, unpack_meta
    n, sr, sc, gr, gc, _ = unpack_meta(arch.meta.view(-1, 2)[lin].cpu().numpy())
    return unpack_grid(arch.bits.view(-1, arch.words)[lin].cpu().numpy(), n, (gr, gc)), (sr, sc), (gr, gc)


def same_maze(a, b):
    return np.array_equal(a[0], b[0]) and tuple(a[1]) == tuple(b[1]) and tuple(a[2]) == tuple(b[2])


def step_both(trainer, rs, history, on_win=None):
    """One vector step of the GPU trainer and of the restatement; a winner's new maze is read
    back from the env and appended to its history. Returns the restatement's flags."""
    env, agent = trainer.env, trainer.agent
    trainer.vector_step()
    acts, term, trunc = rs.step()
    assert agent.actions.cpu().tolist() == acts
    assert trainer.terminated.cpu().tolist() == [int(x) for x in term]
    assert trainer.truncated.cpu().tolist() == [int(x) for x in trunc]
    for i in np.flatnonzero(term):
        if on_win is None or on_win(int(i)):
            mz = read_maze(env, i)
            rs.set_maze(int(i), *mz)
            history[int(i)].append(mz)
    return term


def explored_restated(rs, history, slots):
    """test(n, new=False) as evaluate_explored() plays it: round k on every instance's k-th
    oldest held maze, the others idle; the horizon is the playing instances' largest
    max_steps + 1; afterwards every instance is back on its training maze."""
    held = [h[-slots:] for h in history]
    K = max(len(h) for h in held)
    won = np.zeros((rs.n, K), bool)
    played = np.zeros((rs.n, K), bool)
    for k in range(K):
        active = [k < len(h) for h in held]
        for i in range(rs.n):
            if active[i]:
                rs.set_maze(i, *held[i][k])
            else:
                rs.obs[i] = rs.envs[i].reset()
        played[:, k] = active
        for _ in range(max(rs.envs[i].max_steps for i in range(rs.n) if active[i]) + 1):
            acts = rs.act(active)
            for i, a in enumerate(acts):
                if a < 0:
                    continue
                o = rs.obs[i] = rs.envs[i].step(a)
                won[i, k] |= bool(o["terminated"])
                if o["terminated"] or o["truncated"]:
                    active[i] = False
    for i in range(rs.n):
        rs.set_maze(i, *held[i][-1])
    rs.cum = [0.0] * rs.n
    return won, played


# ---------------------------------------------------------------------------------------------
# 7 and 8: the archive beside the restatement, then evaluate_explored
@pytest.fixture(scope="module")
def explored():
    if not torch.cuda.is_available():
        yield None
        return
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    mazes = nine(False)[:16]
    rs = Restated(mazes, False, **HP)
    env, agent, _ = make(mazes, regen_won=True)
    trainer = VectorTabularTrainer(env, agent, regen_won=True, keep_flags=True, archive=8)
    history = [[(m["grid"], m["start"], m["goal"])] for m in mazes]
    log = []
    for _ in range(200):
        term = step_both(trainer, rs, history)
        log.append((agent.actions.cpu().tolist(), [int(x) for x in term],
                    trainer.truncated.cpu().tolist()))
    yield dict(env=env, agent=agent, trainer=trainer, rs=rs, history=history, log=log,
               mazes=mazes)
    env.close()


@gpu
def test_archive_records_what_env_mazes_would_hold(explored):
    need_gpu()
    x = explored
    rs, arch, history = x["rs"], x["trainer"].archive, x["history"]
    assert rs.min_gap >= GAP, rs.min_gap
    wins = rs.wins  # one table per instance
    assert sum(wins) > 0 and max(len(h) for h in history) >= 3
    assert arch.count.cpu().tolist() == [1 + w for w in wins] == [len(h) for h in history]
    assert arch.held.cpu().tolist() == [min(len(h), 8) for h in history]
    assert arch.dropped.cpu().tolist() == [max(len(h) - 8, 0) for h in history]
    for k in range(8):
        slots = arch.entry_slot(k).cpu().tolist()
        for i, h in enumerate(history):
            kept = h[-8:]
            if k < len(kept):
                assert same_maze(entry_maze(arch, slots[i]), kept[k]), (i, k)
            else:
                assert slots[i] == -1
    # the newest entry is the maze the instance holds now
    newest = arch.newest_slot().cpu().tolist()
    for i in range(16):
        assert same_maze(entry_maze(arch, newest[i]), read_maze(x["env"], i))
    assert_agent(x["agent"], rs)
    # no behaviour change: the same run without an archive takes the same steps to the same tables
    env2, agent2, trainer2 = make(x["mazes"], regen_won=True)
    assert trainer2.archive is None and trainer2.schedule is None
    assert_log(run_logged(trainer2, 200), x["log"])
    assert torch.equal(agent2.q, x["agent"].q)
    assert torch.equal(agent2.gamma, x["agent"].gamma)
    assert x["trainer"].launches_per_step == trainer2.launches_per_step + 1
    env2.close()


@gpu
def test_evaluate_explored_equals_the_restatement(explored):
    need_gpu()
    x = explored
    rs, trainer, agent, env, history = x["rs"], x["trainer"], x["agent"], x["env"], x["history"]
    q_before = agent.q.clone()
    want_won, want_played = explored_restated(rs, history, 8)
    won, played, rate = trainer.evaluate_explored()
    assert rs.min_gap >= GAP, rs.min_gap
    assert np.array_equal(played.cpu().numpy(), want_played)
    assert np.array_equal(won.cpu().numpy(), want_won)
    assert want_played.sum() == sum(min(len(h), 8) for h in history) and want_won.any()
    assert rate == want_won.sum() / want_played.sum()
    assert agent.steps_done.cpu().tolist() == rs.steps_done
    assert torch.equal(agent.q, q_before)  # no updates
    assert not bool(agent.cum.any())
    # the env holds the training mazes again, and training goes on as the restatement's
    for i in range(16):
        assert same_maze(read_maze(env, i), history[i][-1])
    for _ in range(50):
        step_both(trainer, rs, history)
    assert rs.min_gap >= GAP, rs.min_gap
    assert_agent(agent, rs)
    assert trainer.archive.count.cpu().tolist() == [len(h) for h in history]
    env3, _, plain = make(x["mazes"])
    with pytest.raises(ValueError, match="archive="):
        plain.evaluate_explored()
    env3.close()


# ---------------------------------------------------------------------------------------------
# 9. growth
def make_growth(mazes, toroidal, pitch, growth, archive=None, seed=SEED, algorithm=None,
                **agent_kw):
    import mazerl
    from mazerl.agents.vector_q import VectorQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    env = mazerl.VectorMazeEnv(len(mazes), 9, toroidal=toroidal, enrich=False, reward64=True,
                               generate=False, max_dim=pitch)
    env.load_mazes(np.stack([m["grid"] for m in mazes]),
                   np.array([list(m["start"]) + list(m["goal"]) for m in mazes]))
    if algorithm is not None:  # the algorithm of every winner's next maze (per instance)
        env.set_algorithm(torch.tensor(algorithm, dtype=torch.uint8))
    env.reset()
    grow_every = agent_kw.pop("grow_every", 0)
    agent = VectorQAgent(env, seed=seed, **HP, **agent_kw)
    return env, agent, VectorTabularTrainer(env, agent, regen_won=True, keep_flags=True,
                                            archive=archive, growth=growth, grow_every=grow_every)


def assert_tables_at(agent, rs, pitch):
    from mazerl.agents.vector_q import state_index
    for t in range(rs.T):
        got = (agent.to_dense(t) if agent.hashed else agent.q[t]).cpu().numpy()
        want = np.zeros_like(got)
        for k, v in rs.tables[t].items():
            want[state_index(pitch, *k)] = v
        bad = np.argwhere(got != want)
        assert bad.size == 0, ("table", t, "row", bad[0])


GROWTH_STEPS, GROWTH_MIXED_AT = 400, 200


@gpu
def test_growth_equals_the_restatement_under_the_schedules_rule():
    """growth = (9, 17) on 8 golden 9 x 9 mazes, independent dense tables. The step counts were
    chosen on the MI355X from the restatement's own course: after GROWTH_MIXED_AT = 200 vector
    steps it holds instances at 9, 13 and 17 at once, two of them retired (sizes 13, 9, 17, 13, 13,
    13, 13, 17; the last 9 leaves at step 214); by GROWTH_STEPS = 400 retired instances have won
    again on the maze they keep (first at step 320), which must record nothing; instances 0 and 1
    are then still at 13, so no stop comes within these steps (the toroidal case below has one).
    All three are asserted as preconditions."""
    need_gpu()
    mazes = nine(False)[:8]
    steps = GROWTH_STEPS
    rs = Restated(mazes, False, **HP)
    env, agent, trainer = make_growth(mazes, False, 17, (9, 17), archive=4)
    sizes, retired, seen = [9] * 8, [False] * 8, {9}
    history = [[(m["grid"], m["start"], m["goal"])] for m in mazes]
    stopped = None

    def on_win(i):
        if sizes[i] + 4 <= 17:
            sizes[i] += 4
            seen.add(sizes[i])
            return True
        return False
    for step in range(1, steps + 1):
        term = step_both(trainer, rs, history, on_win)
        for i in np.flatnonzero(term):
            retired[i] = retired[i] or sizes[i] >= 17
        if step == GROWTH_MIXED_AT:
            # the precondition: the restatement itself shows every size at once, and a retirement
            print("growth at", step, "sizes", sizes, "retired", retired)
            assert set(sizes) == {9, 13, 17} and any(retired), (sizes, retired)
        if stopped is None and step % 32 == 0 and all(retired):
            stopped = step
        assert trainer.schedule.dim.cpu().tolist() == sizes, step
        assert env.meta()[:, 0].cpu().tolist() == sizes, step
        assert trainer.schedule.retired.cpu().tolist() == retired, step
    assert rs.min_gap >= GAP, rs.min_gap
    print("growth: sizes", sizes, "retired", retired, "wins", rs.wins)
    assert seen == {9, 13, 17} and any(retired)
    assert_tables_at(agent, rs, 17)
    assert agent.gamma.cpu().tolist() == rs.gamma
    assert agent.steps_done.cpu().tolist() == rs.steps_done
    assert agent.wins.cpu().tolist() == rs.wins
    # a retired winner keeps its maze and records nothing: the archive counts the moves only
    assert trainer.archive.count.cpu().tolist() == [len(h) for h in history] == \
        [1 + (s - 9) // 4 for s in sizes]
    assert any(w > (s - 9) // 4 for w, s in zip(rs.wins, sizes))  # (a retired instance won again)
    s = trainer.summary()
    assert s["schedule"]["retired"] == sum(retired) and s["schedule"]["growth"] == [9, 17]
    assert s["schedule"]["instances_per_size"] == {n: sizes.count(n) for n in (9, 13, 17)}
    # the stop: train() checks every 32nd vector step and returns once every instance is retired
    env2, agent2, trainer2 = make_growth(mazes, False, 17, (9, 17))
    trainer2.train(steps)
    # here: never within these steps, since two instances are not retired
    assert stopped is None and retired.count(False) == 2
    assert trainer2.stopped_at is None and trainer.stopped_at is None
    assert trainer2.vector_steps == steps
    assert torch.equal(agent2.q, agent.q)
    env.close()
    env2.close()


TOROID_STEPS = 192


@gpu
def test_toroidal_growth_retires_at_the_first_win_and_stops():
    """growth = (9, 13) on 4 toroidal mazes: the first win moves an instance to 13 and retires
    it. TOROID_STEPS = 192 was chosen on the MI355X: the restatement's last instance wins at step
    114, so the stop comes at the check of step 128 (asserted as a precondition)."""
    need_gpu()
    mazes = nine(True)[:4]
    rs = Restated(mazes, True, **HP)
    env, agent, trainer = make_growth(mazes, True, 13, (9, 13))
    sizes, retired = [9] * 4, [False] * 4
    history = [[None] for _ in mazes]
    stopped = None

    def on_win(i):
        if sizes[i] + 4 <= 13:
            sizes[i] += 4
            return True
        return False
    for step in range(1, TOROID_STEPS + 1):
        term = step_both(trainer, rs, history, on_win)
        for i in np.flatnonzero(term):
            assert sizes[i] == 13
            retired[i] = True
        assert trainer.schedule.dim.cpu().tolist() == sizes, step
        assert trainer.schedule.retired.cpu().tolist() == retired, step
        if step % 32 == 0 and all(retired):
            stopped = step
            break
    assert rs.min_gap >= GAP, rs.min_gap
    assert stopped is not None, (sizes, retired)  # the precondition: every instance won
    assert_tables_at(agent, rs, 13)
    env2, agent2, trainer2 = make_growth(mazes, True, 13, (9, 13))
    trainer2.train(TOROID_STEPS + 64)
    assert trainer2.stopped_at == stopped == trainer2.vector_steps
    assert torch.equal(agent2.q, agent.q)
    trainer2.train(10)  # a stopped trainer stays stopped
    assert trainer2.vector_steps == stopped
    env.close()
    env2.close()


@gpu
def test_hashed_growth_equals_the_dense_run():
    need_gpu()
    mazes = nine(False)[:8]
    env, agent, trainer = make_growth(mazes, False, 17, (9, 17), archive=4)
    envh, agenth, trainerh = make_growth(mazes, False, 17, (9, 17), archive=4, storage="hash",
                                         capacity=64, grow_every=16)
    trainer.train(GROWTH_STEPS)
    trainerh.train(GROWTH_STEPS)
    assert agenth.capacity > 64 and int(agenth.overflow.sum()) == 0
    for t in range(8):
        assert torch.equal(agenth.to_dense(t), agent.q[t]), t
    assert torch.equal(agenth.gamma, agent.gamma) and torch.equal(agenth.wins, agent.wins)
    assert torch.equal(trainerh.schedule.dim, trainer.schedule.dim)
    assert int(trainer.schedule.dim.max()) == 17
    for k in ("bits", "meta", "algo", "count"):
        assert torch.equal(getattr(trainerh.archive, k), getattr(trainer.archive, k)), k
    wh, ph, rh = trainerh.evaluate_explored()
    w, p, r = trainer.evaluate_explored()
    assert torch.equal(wh, w) and torch.equal(ph, p) and rh == r
    env.close()
    envh.close()


@gpu
def test_double_q_takes_the_archive_and_the_growth():
    need_gpu()
    import mazerl
    from mazerl.agents.vector_dq import VectorDoubleQAgent
    from mazerl.trainers.vector_tabular import VectorTabularTrainer
    mazes = nine(False)[:8]
    runs = []
    for _ in range(2):
        env = mazerl.VectorMazeEnv(8, 9, enrich=False, reward64=True, generate=False, max_dim=13)
        env.load_mazes(np.stack([m["grid"] for m in mazes]),
                       np.array([list(m["start"]) + list(m["goal"]) for m in mazes]))
        env.reset()
        agent = VectorDoubleQAgent(env, seed=SEED, **HP)
        tr = VectorTabularTrainer(env, agent, archive=4, growth=(9, 13))
        tr.train(300)
        runs.append((env, agent, tr, tr.evaluate_explored()))
    (e0, a0, t0, x0), (e1, a1, t1, x1) = runs
    assert int(t0.archive.count.sum()) == 8 + int((t0.schedule.dim == 13).sum()) > 8
    assert torch.equal(a0.q, a1.q) and torch.equal(t0.archive.bits, t1.archive.bits)
    assert torch.equal(x0[0], x1[0]) and torch.equal(x0[1], x1[1]) and x0[2] == x1[2]
    assert x0[1].sum() == t0.archive.held.sum()
    with pytest.raises(ValueError, match="regen_won"):
        VectorTabularTrainer(e0, a0, regen_won=False, growth=(9, 13))
    with pytest.raises(ValueError, match="size 9"):
        VectorTabularTrainer(e0, a0, growth=(9, 13))  # (its instances have grown)
    e0.close()
    e1.close()


# ---------------------------------------------------------------------------------------------
# 10. checkpoint
@gpu
def test_checkpoint_resumes_bit_exactly(tmp_path):
    need_gpu()
    from mazerl.archive import MazeArchive
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    mazes = nine(False)[:8]
    path = str(tmp_path / "tabular.pt")
    env, agent, whole = make_growth(mazes, False, 17, (9, 17), archive=4)
    whole.train(250)
    env1, agent1, first = make_growth(mazes, False, 17, (9, 17), archive=4)
    first.train(150)
    save_checkpoint(path, first)
    env2, agent2, resumed = make_growth(mazes, False, 17, (9, 17), archive=4, seed=1)
    load_checkpoint(path, resumed)
    assert resumed.vector_steps == 150
    resumed.train(100)
    assert resumed.vector_steps == whole.vector_steps and resumed.stopped_at == whole.stopped_at
    assert torch.equal(agent2.q, agent.q) and bool(agent.q.any())
    for k in ("gamma", "steps_done", "wins", "episodes", "cum"):
        assert torch.equal(getattr(agent2, k), getattr(agent, k)), k
    for k in ("bits", "meta", "algo", "count", "errors"):
        assert torch.equal(getattr(resumed.archive, k), getattr(whole.archive, k)), k
    assert int(whole.archive.count.sum()) > 8  # (new mazes were recorded on both sides of the save)
    for k in ("dim", "retired", "inst_wins", "total_wins", "new_mazes", "next_dim"):
        assert torch.equal(getattr(resumed.schedule, k), getattr(whole.schedule, k)), k
    a, b = whole.evaluate_explored(), resumed.evaluate_explored()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert bool(a[1].any())
    # an archive saved at another pitch does not load
    env3, agent3, other = make_growth(mazes, False, 13, (9, 13), archive=4)
    with pytest.raises(ValueError, match="pitch"):
        load_checkpoint(path, other)
    with pytest.raises(ValueError, match="pitch"):
        MazeArchive(env3, 4).load_state_dict(whole.archive.state_dict())
    env4, agent4, plain = make_growth(mazes, False, 17, (9, 17))
    with pytest.raises(ValueError, match="archive"):
        load_checkpoint(path, plain)
    for e in (env, env1, env2, env3, env4):
        e.close()


ALGOS3 = [1, 2, 0, 1, 2, 0, 1, 2]  # dfs, prim&kill, r-prim (mazerl.ALGOS ids), per instance


@gpu
def test_checkpoint_keeps_each_instances_algorithm(tmp_path):
    """The winners' next mazes come from the instance's own algorithm (set_algorithm), before and
    after a resume: the resumed run's archive holds the uninterrupted run's algorithm ids and
    mazes. The schedule carries the handle's ids, so its summary counts them too."""
    need_gpu()
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    mazes = nine(False)[:8]
    path = str(tmp_path / "algos.pt")
    kw = dict(archive=4, algorithm=ALGOS3)
    env, agent, whole = make_growth(mazes, False, 17, (9, 17), **kw)
    whole.train(250)
    env1, agent1, first = make_growth(mazes, False, 17, (9, 17), **kw)
    first.train(150)
    save_checkpoint(path, first)
    # the fresh trainer's env holds r-prim everywhere: everything comes from the file
    env2, agent2, resumed = make_growth(mazes, False, 17, (9, 17), archive=4, seed=1)
    load_checkpoint(path, resumed)
    resumed.train(100)
    count = whole.archive.count.cpu()
    # (mazes were built on both sides of the save)
    assert 8 < int(first.archive.count.sum()) < int(count.sum())
    for k in ("bits", "meta", "algo", "count"):
        assert torch.equal(getattr(resumed.archive, k), getattr(whole.archive, k)), k
    assert torch.equal(agent2.q, agent.q)
    # every held entry carries its instance's id, in all three runs
    held = whole.archive.held.cpu().tolist()
    algo = whole.archive.algo.cpu().tolist()
    for i in range(8):
        assert algo[i][:held[i]] == [ALGOS3[i]] * held[i], i
    assert len({ALGOS3[i] for i in range(8) if count[i] >= 2}) >= 2  # (not r-prim alone)
    for tr in (whole, resumed):
        s = tr.summary()["schedule"]
        assert s["instances_per_algorithm"] == {"r-prim": 2, "dfs": 3, "prim&kill": 3}
        moved = [int(c) - 1 for c in count]
        assert s["new_mazes_per_algorithm"] == {
            name: sum(m for m, a in zip(moved, ALGOS3) if a == k)
            for name, k in (("r-prim", 0), ("dfs", 1), ("prim&kill", 2))}
    # the same ids without an archive (the schedule reads them from the handle itself)
    env3, agent3, bare = make_growth(mazes, False, 17, (9, 17), algorithm=ALGOS3)
    assert bare.schedule.algo.cpu().tolist() == ALGOS3
    for e in (env, env1, env2, env3):
        e.close()


@gpu
def test_new_mazes_under_growth_have_the_sizes_reached_and_a_corrupt_entry_is_reported():
    need_gpu()
    mazes = nine(False)[:8]
    env, agent, trainer = make_growth(mazes, False, 17, (9, 17), archive=4)
    trainer.train(GROWTH_MIXED_AT)
    sizes = trainer.schedule.dim.cpu().tolist()
    assert set(sizes) == {9, 13, 17}
    before = [env.grid(i) for i in range(8)]
    won, rate = trainer.evaluate(new=True)
    assert env.meta()[:, 0].cpu().tolist() == sizes and won.shape == (8,)
    assert all(g.shape != env.grid(i).shape or not np.array_equal(g, env.grid(i))
               for i, g in enumerate(before))
    # evaluate_explored() puts the training mazes back, and reports an entry the kernel refuses
    w, p, r = trainer.evaluate_explored()
    for i in range(8):
        assert np.array_equal(env.grid(i), before[i])
    trainer.archive.algo[3, 0] = 7  # a corrupt entry: refused, never loaded
    with pytest.raises(RuntimeError, match="refused"):
        trainer.evaluate_explored()
    assert int(trainer.archive.errors) >= 1
    env.close()
