"""Launch and guard edges of the tabular engine (csrc/mz_qtab.hip) that the other tabular tests do
not reach: they run every bit-exact case in one partial workgroup (<= 24 instances) or in whole
workgroups (1,024). Here 300 instances make two workgroups of 256 lanes, the second with 44, and
shared tables put three tables into every wave of k_qtab_advance, which then takes both of its
branches. No new model: the restatements and helpers are those of test_vector_q.py,
test_vector_qhash.py and test_vector_dq.py.

The restatements' precondition min_gap >= GAP is a condition on the inputs; for these inputs the
smallest gap is 3.0e-5 (Q) and 7.1e-6 (double Q) on both geometries."""
import functools

import numpy as np
import pytest

import test_vector_dq as DQ
import test_vector_q as Q
import test_vector_qhash as QH
from test_vector_q import GAP, HP, assert_log, need_gpu, nine, run_logged

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

N = 300           # 256 + 44 lanes
STEPS = 100       # independent tables
SHARED_STEPS = 50
TABLES = 3        # shared: table_of = i % 3, so every wave mixes three tables


def mazes(toroidal):
    return [nine(toroidal)[i % 24] for i in range(N)]


@functools.lru_cache(maxsize=None)
def restated(agent, toroidal):
    """The restatement of `agent` after STEPS vector steps and its log. Shared by the storages;
    never modified."""
    rs = (Q.Restated if agent == "q" else DQ.RestatedDQ)(mazes(toroidal), toroidal, **HP)
    log = [rs.step() for _ in range(STEPS)]
    assert rs.min_gap >= GAP, rs.min_gap  # the precondition of the bit-exact comparison
    return rs, log


def make(agent, storage, toroidal, tables=None, capacity=64):
    if agent == "dq":
        kw = dict(storage="hash", capacity=capacity) if storage == "hash" else {}
        return DQ.make(mazes(toroidal), toroidal, tables=tables, **kw)
    if storage == "hash":
        return QH.make_hash(mazes(toroidal), toroidal, capacity=capacity, tables=tables)
    return Q.make(mazes(toroidal), toroidal, tables=tables)


@gpu
@pytest.mark.parametrize("toroidal", [False, True], ids=["euclidean", "toroidal"])
@pytest.mark.parametrize("storage", ["dense", "hash"])
@pytest.mark.parametrize("agent", ["q", "dq"])
def test_independent_tables_across_a_ragged_workgroup(agent, storage, toroidal):
    need_gpu()
    rs, log = restated(agent, toroidal)
    env, ag, trainer = make(agent, storage, toroidal)
    assert ag.table_of is None and ag.n == N
    assert_log(run_logged(trainer, STEPS), log)
    if agent == "dq":
        DQ.assert_agent(ag, rs)  # either storage; hashed: load and overflow == 0 as well
    elif storage == "hash":
        QH.assert_hashed_agent(ag, rs)
    else:
        Q.assert_agent(ag, rs)
    if storage == "hash":
        assert int(ag.overflow.sum()) == 0
    env.close()


@gpu
@pytest.mark.parametrize("storage", ["dense", "hash"])
@pytest.mark.parametrize("agent", ["q", "dq"])
def test_shared_tables_mixed_in_every_wave(agent, storage):
    """Shared tables are not bitwise reproducible (their atomic adds arrive in no fixed order), so
    only integer facts are asserted."""
    need_gpu()
    from mazerl.agents.vector_q import state_index
    table_of = np.arange(N) % TABLES
    env, ag, trainer = make(agent, storage, False, tables=torch.tensor(table_of), capacity=1024)
    per_table = N // TABLES
    assert np.bincount(table_of).tolist() == [per_table] * TABLES
    took = np.zeros(TABLES, dtype=np.int64)
    ended = won = 0
    for step in range(SHARED_STEPS):
        obs = env.obs6.cpu().numpy()  # the observation acted from
        trainer.vector_step()
        acts = ag.actions.cpu().numpy()
        assert acts.min() >= 0 and acts.max() <= 3, step
        want = [state_index(9, o[0:2], o[2:4], o[4:6]) for o in obs.astype(np.int64)]
        assert ag.sidx.cpu().tolist() == want, step
        te, tr = trainer.terminated.cpu().numpy() != 0, trainer.truncated.cpu().numpy() != 0
        ended += int((te | tr).sum())
        won += int(te.sum())
        if agent == "dq":
            took += np.bincount(table_of, weights=ag._took.cpu().numpy(),
                                minlength=TABLES).astype(np.int64)
    assert ended > 0
    assert ag.steps_done.cpu().tolist() == (per_table * SHARED_STEPS + took).tolist()
    assert int(ag.episodes.sum()) == ended
    assert int(ag.wins.sum()) == won
    if storage == "hash":
        assert ag.load.cpu().tolist() == (ag.keys >= 0).sum(1).cpu().tolist()
        assert int(ag.load.min()) > 0
        assert int(ag.overflow.sum()) == 0
    env.close()
