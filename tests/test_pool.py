"""The explored-maze pool without a GPU: the two new symbols of the C ABI, the workgroup span the
GPU tests size themselves by, MazePool's refusals and checkpoint checks on host tensors (the
kernels are not involved), and the refusals of the mazerl.train entry point, which are raised
before any GPU call."""
import types

import pytest

torch = pytest.importorskip("torch")


def host_env(max_dim=9, num_envs=5, toroidal=False, enrich=True):
    from mazerl import _native
    return types.SimpleNamespace(lib=_native.load(), device=torch.device("cpu"), num_envs=num_envs,
                                 max_dim=max_dim, toroidal=toroidal, enrich=enrich)


def test_the_two_entry_points_are_declared_and_bound():
    from mazerl import _native
    from test_abi import declared
    for f in ("mz_archive_pool_span", "mz_archive_push_pool"):
        assert f in declared() and f in _native.EXPORTS
    L = _native.load()
    assert len(L.mz_archive_pool_span.argtypes) == 1
    assert len(L.mz_archive_push_pool.argtypes) == 12


def test_the_span_is_a_positive_multiple_of_the_wave():
    from mazerl import _native
    from mazerl.archive import pool_span
    s = pool_span()
    assert s > 0 and s % 64 == 0
    assert _native.load().mz_archive_pool_span(None) == -1  # MZ_EINVAL, no GPU involved


def test_push_pool_refuses_a_null_handle_before_any_launch():
    from mazerl import _native
    L = _native.load()
    assert L.mz_archive_push_pool(None, None, 4, 3, 8, 8, 8, 8, 8, 8, 0, None) == -1
    assert L.mz_last_error()


def test_pool_shapes_counts_and_refusals():
    from mazerl.archive import MazePool
    env = host_env()
    for bad in (0, -3):
        with pytest.raises(ValueError):
            MazePool(env, bad)
    p = MazePool(env, 7)
    assert (p.capacity, p.pitch, p.words, p.toroidal, p.enrich) == (7, 9, 3, False, True)
    assert tuple(p.bits.shape) == (7, 3) and tuple(p.meta.shape) == (7, 2)
    for k in ("algo", "owner", "stamp"):
        assert tuple(getattr(p, k).shape) == (7,)
    assert p.algo.dtype == torch.uint8 and p.owner.dtype == p.stamp.dtype == torch.int32
    assert tuple(p.errors.shape) == (1,)
    # held / dropped from the count, on either word of the two-word counter
    for cur in (0, 1):
        p._cur = cur
        for c, held, dropped in ((0, 0, 0), (5, 5, 0), (7, 7, 0), (8, 7, 1), (2 ** 31 - 1, 7, 2 ** 31 - 8)):
            p._count2[cur] = c
            p._count2[cur ^ 1] = 123
            assert (int(p.count), int(p.held), int(p.dropped)) == (c, held, dropped)
    with pytest.raises(ValueError):
        p.record(torch.zeros(4, dtype=torch.uint8))  # one flag per instance


def test_pool_state_dict_checks_before_anything_changes():
    from mazerl.archive import MazePool
    env = host_env()
    a = MazePool(env, 4)
    a.bits.copy_(torch.arange(12, dtype=torch.int32).reshape(4, 3))
    a.owner.copy_(torch.tensor([3, 0, 4, 1], dtype=torch.int32))
    a.stamp.copy_(torch.tensor([0, 0, 6, 9], dtype=torch.int32))
    a._cur = 1
    a._count2[1] = 6
    sd = a.state_dict()
    assert sd["format"] == "mazerl.MazePool/1" and sd["count"].tolist() == [6]
    b = MazePool(host_env(num_envs=2), 4)  # another env of the same pitch and geometry
    b.load_state_dict(sd)
    assert int(b.count) == 6 and int(b.held) == 4 and int(b.dropped) == 2
    for k in ("bits", "meta", "algo", "owner", "stamp", "errors"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    # refused: another pitch, capacity, geometry, format; a missing, misshapen or retyped tensor
    others = [MazePool(host_env(max_dim=13), 4), MazePool(env, 5),
              MazePool(host_env(toroidal=True), 4), MazePool(host_env(enrich=False), 4)]
    for o in others:
        with pytest.raises(ValueError):
            o.load_state_dict(sd)
        assert int(o.count) == 0 and not o.bits.any()
    c = MazePool(env, 4)
    bad = [{"format": "mazerl.MazeArchive/1"}, {}, None,
           {k: v for k, v in sd.items() if k != "owner"},
           dict(sd, bits=sd["bits"][:3]), dict(sd, count=torch.zeros(2, dtype=torch.int32)),
           dict(sd, stamp=sd["stamp"].to(torch.int64)), dict(sd, capacity=5),
           {k: v for k, v in sd.items() if k != "pitch"}]
    for d in bad:
        with pytest.raises(ValueError):
            c.check_state_dict(d)
        with pytest.raises(ValueError):
            c.load_state_dict(d)
    assert int(c.count) == 0 and not c.bits.any() and not c.owner.any()


@pytest.mark.parametrize("argv, match", [
    (["--archive", "-1"], "--archive"),
    (["--archive", "100", "--explored-mazes", "0"], "--explored-mazes"),
    (["--archive", "100", "--explored-mazes", "-5"], "--explored-mazes"),
    (["--explored-mazes", "10"], "needs --archive"),
    (["--archive", "0", "--explored-mazes", "10"], "needs --archive"),
])
def test_train_refuses_before_any_gpu_call(argv, match, monkeypatch):
    from mazerl import train
    import mazerl.vector_env as ve
    monkeypatch.setattr(ve.VectorMazeEnv, "__init__",
                        lambda *a, **k: pytest.fail("an env was built before the refusal"))
    monkeypatch.setattr(train, "init_from_env",
                        lambda *a, **k: pytest.fail("the process group before the refusal"))
    monkeypatch.setattr(torch.cuda, "set_device",
                        lambda *a, **k: pytest.fail("a GPU call before the refusal"))
    with pytest.raises(ValueError, match=match):
        train.main(argv)


def test_train_defaults_leave_the_pool_off():
    from mazerl import train
    a = train.parse([])
    assert a.archive == 0 and a.explored_mazes is None
    a = train.parse(["--archive", "5000", "--explored-mazes", "64"])
    assert (a.archive, a.explored_mazes) == (5000, 64)
