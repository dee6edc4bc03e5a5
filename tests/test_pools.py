"""The per-learner explored-maze pools without a GPU: the new symbol of the C ABI and its refusal
of a null handle, MazePoolSet's shapes, counts, refusals and checkpoint checks on host tensors (the
kernel is not involved), a pool of the set read through MazePool's interface, and the refusals
and defaults of the three episodic trainers' command lines, raised before any GPU call."""
import types

import pytest

torch = pytest.importorskip("torch")


def host_env(max_dim=9, num_envs=12, toroidal=False, enrich=False):
    from mazerl import _native
    return types.SimpleNamespace(lib=_native.load(), device=torch.device("cpu"), num_envs=num_envs,
                                 max_dim=max_dim, toroidal=toroidal, enrich=enrich)


def test_the_entry_point_is_declared_and_bound():
    from mazerl import _native
    from test_abi import declared
    assert "mz_archive_push_pools" in declared() and "mz_archive_push_pools" in _native.EXPORTS
    L = _native.load()
    assert len(L.mz_archive_push_pools.argtypes) == 14
    assert len(L.mz_archive_push_pool.argtypes) == 12  # (the single pool's keeps its signature)


def test_push_pools_refuses_a_null_handle_before_any_launch():
    from mazerl import _native
    L = _native.load()
    assert L.mz_archive_push_pools(None, None, 2, 4, 3, 8, 8, 8, 8, 8, 8, 0, 0, None) == -1
    assert L.mz_last_error()


def test_set_shapes_counts_and_refusals():
    from mazerl.archive import MazePoolSet
    env = host_env()
    for groups, cap in ((0, 4), (-1, 4), (5, 4), (24, 4), (3, 0), (3, -2)):
        with pytest.raises(ValueError):
            MazePoolSet(env, groups, cap)
    s = MazePoolSet(env, 3, 7)
    assert (s.groups, s.block, s.capacity, s.pitch, s.words) == (3, 4, 7, 9, 3)
    assert (s.toroidal, s.enrich) == (False, False)
    assert tuple(s.bits.shape) == (21, 3) and tuple(s.meta.shape) == (21, 2)
    for k in ("algo", "owner", "stamp"):
        assert tuple(getattr(s, k).shape) == (21,)
    assert s.algo.dtype == torch.uint8 and s.owner.dtype == s.stamp.dtype == torch.int32
    assert tuple(s.errors.shape) == (1,) and s._count2.data_ptr() % 8 == 0
    for k in ("count", "held", "dropped"):
        v = getattr(s, k)
        assert tuple(v.shape) == (3,) and v.dtype == torch.int32 and not v.any()
    # held / dropped from the counts, on either word of the two-word counters
    for cur in (0, 1):
        s._cur = cur
        s._count2[:, cur] = torch.tensor([5, 7, 2 ** 31 - 1], dtype=torch.int32)
        s._count2[:, cur ^ 1] = 123
        assert s.count.tolist() == [5, 7, 2 ** 31 - 1]
        assert s.held.tolist() == [5, 7, 7] and s.dropped.tolist() == [0, 0, 2 ** 31 - 8]
    with pytest.raises(ValueError):
        s.record(torch.zeros(4, dtype=torch.uint8))  # one flag per instance
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            s.pool(bad)


def test_a_pool_of_the_set_reads_as_a_maze_pool():
    from mazerl.archive import MazePool, MazePoolSet
    s = MazePoolSet(host_env(), 3, 4)
    s.bits.copy_(torch.arange(36, dtype=torch.int32).reshape(12, 3))
    s.owner.copy_(torch.arange(12, dtype=torch.int32) % 4)
    s._cur = 1
    s._count2[:, 1] = torch.tensor([1, 6, 4], dtype=torch.int32)
    v = s.pool(1)
    assert isinstance(v, MazePool) and (v.capacity, v.pitch, v.words) == (4, 9, 3)
    assert (int(v.count), int(v.held), int(v.dropped)) == (6, 4, 2)
    assert torch.equal(v.bits, s.bits[4:8]) and v.bits.data_ptr() == s.bits[4:8].data_ptr()
    assert v.owner.tolist() == [0, 1, 2, 3] and v.errors.data_ptr() == s.errors.data_ptr()
    s._cur = 0  # the view follows the set's counter
    s._count2[1, 0] = 3
    assert (int(v.count), int(v.held), int(v.dropped)) == (3, 3, 0)
    with pytest.raises(TypeError):
        v.record()
    # pool g's checkpoint is a MazePool's: it loads into a pool of a block-sized env
    single = MazePool(host_env(num_envs=4), 4)
    single.load_state_dict(v.state_dict())
    assert int(single.count) == 3 and torch.equal(single.bits, s.bits[4:8])


def test_set_state_dict_checks_before_anything_changes():
    from mazerl.archive import MazePool, MazePoolSet
    env = host_env()
    a = MazePoolSet(env, 3, 4)
    a.bits.copy_(torch.arange(36, dtype=torch.int32).reshape(12, 3))
    a.owner.copy_(torch.arange(12, dtype=torch.int32) % 4)
    a.stamp.copy_(torch.arange(12, dtype=torch.int32) * 3)
    a._cur = 1
    a._count2[:, 1] = torch.tensor([1, 6, 4], dtype=torch.int32)
    sd = a.state_dict()
    assert sd["format"] == "mazerl.MazePoolSet/1" and sd["count"].tolist() == [1, 6, 4]
    assert sd["groups"] == 3 and sd["capacity"] == 4
    b = MazePoolSet(host_env(num_envs=6), 3, 4)  # another env of the same pitch and geometry
    b.load_state_dict(sd)
    assert b.count.tolist() == [1, 6, 4] and b.held.tolist() == [1, 4, 4]
    assert b.dropped.tolist() == [0, 2, 0]
    for k in ("bits", "meta", "algo", "owner", "stamp", "errors"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    # refused: another pitch, capacity, group count, geometry; a MazePool's checkpoint and the
    # reverse; a missing, misshapen or retyped tensor
    others = [MazePoolSet(host_env(max_dim=13), 3, 4), MazePoolSet(env, 3, 5),
              MazePoolSet(env, 4, 3), MazePoolSet(env, 2, 6), MazePoolSet(host_env(toroidal=True), 3, 4),
              MazePoolSet(host_env(enrich=True), 3, 4)]
    for o in others:
        with pytest.raises(ValueError):
            o.load_state_dict(sd)
        assert not o.count.any() and not o.bits.any()
    single = MazePool(env, 12)
    with pytest.raises(ValueError):
        single.load_state_dict(sd)
    c = MazePoolSet(env, 3, 4)
    bad = [single.state_dict(), {"format": "mazerl.MazeArchive/1"}, {}, None,
           {k: v for k, v in sd.items() if k != "owner"},
           dict(sd, bits=sd["bits"][:11]), dict(sd, count=torch.zeros(1, dtype=torch.int32)),
           dict(sd, count=sd["count"].to(torch.int64)), dict(sd, groups=4),
           {k: v for k, v in sd.items() if k != "groups"}]
    for d in bad:
        with pytest.raises(ValueError):
            c.check_state_dict(d)
        with pytest.raises(ValueError):
            c.load_state_dict(d)
    assert not c.count.any() and not c.bits.any() and not c.owner.any()


def test_attach_pool_takes_a_capacity_or_a_pool_of_this_env():
    from mazerl.archive import MazePool, MazePoolSet
    from mazerl.trainers.episodic import attach_pool
    env, other = host_env(), host_env()
    p, s = MazePool(env, 5), MazePoolSet(env, 3, 5)
    assert attach_pool(env, p) is p and attach_pool(env, s, 3) is s
    made = attach_pool(env, 7)
    assert type(made) is MazePool and made.capacity == 7 and made.env is env
    made = attach_pool(env, 7, 4)
    assert type(made) is MazePoolSet and (made.groups, made.capacity) == (4, 7)
    for bad in ((other, p, None), (other, s, 3), (env, s, None), (env, p, 3), (env, s, 4),
                (env, s.pool(0), None), (env, 0, None), (env, 0, 3), (env, 7, 5), (env, "7", None),
                (env, True, None), (env, 7.0, None)):
        with pytest.raises(ValueError):
            attach_pool(*bad)


CLIS = ("train_ppo", "train_reinforce", "train_lstm_dqn")


def _parse(name):
    import importlib
    m = importlib.import_module("mazerl." + name)
    return m, (m.parse_args if name == "train_lstm_dqn" else m.parse)


@pytest.mark.parametrize("name", CLIS)
@pytest.mark.parametrize("argv, match", [
    (["--archive", "-1"], "--archive"),
    (["--archive", "100", "--explored-mazes", "0"], "--explored-mazes"),
    (["--archive", "100", "--explored-mazes", "-5"], "--explored-mazes"),
    (["--explored-mazes", "10"], "needs --archive"),
    (["--archive", "0", "--explored-mazes", "10"], "needs --archive"),
])
def test_the_command_lines_refuse_before_any_gpu_call(name, argv, match, monkeypatch):
    import mazerl.vector_env as ve
    m, _ = _parse(name)
    monkeypatch.setattr(ve.VectorMazeEnv, "__init__",
                        lambda *a, **k: pytest.fail("an env was built before the refusal"))
    if hasattr(m, "init_from_env"):
        monkeypatch.setattr(m, "init_from_env",
                            lambda *a, **k: pytest.fail("the process group before the refusal"))
    for f in ("set_device", "current_device"):
        monkeypatch.setattr(torch.cuda, f,
                            lambda *a, **k: pytest.fail("a GPU call before the refusal"))
    with pytest.raises(ValueError, match=match):
        m.main(argv)
    if name == "train_lstm_dqn":  # and with a population of learners
        with pytest.raises(ValueError, match=match):
            m.main(["--envs", "64", "--learners", "4"] + argv)


@pytest.mark.parametrize("name", CLIS)
def test_the_command_lines_defaults_leave_the_pool_off(name):
    _, parse = _parse(name)
    a = parse([])
    assert a.archive == 0 and a.explored_mazes is None
    a = parse(["--archive", "5000", "--explored-mazes", "64"])
    assert (a.archive, a.explored_mazes) == (5000, 64)
