"""The explored-maze archive without a GPU: the bit layout of an entry (mazerl.archive.pack_grid /
unpack_grid, the pure numpy mirror of csrc/mz_archive.hip), the ring arithmetic of MazeArchive on
host tensors, the three new symbols of the C ABI, and the refusals of the train_tabular entry
point, which are raised before any GPU call."""
import types

import numpy as np
import pytest

import golden_io as G

SIZES = {"gen_euclid.npz": (9, 15, 21, 41, 81), "gen_toroid.npz": (9, 17, 21, 29, 41)}


def golden(name):
    return [m for m in G.mazes(name) if m["n"] in SIZES[name]]


# 1. the bit layout
@pytest.mark.parametrize("name", sorted(SIZES))
def test_pack_and_unpack_reproduce_every_golden_maze(name):
    from mazerl.archive import archive_words, pack_grid, unpack_grid
    mazes = golden(name)
    assert {m["n"] for m in mazes} == set(SIZES[name])
    for m in mazes:
        n, g = m["n"], m["grid"]
        for P in (n, n + 4):
            bits = pack_grid(g, P)
            W = archive_words(P)
            assert W == (P * P + 31) // 32
            assert bits.dtype == np.int32 and bits.shape == (W,)
            assert np.array_equal(unpack_grid(bits, n, m["goal"]), g)
            # bit (r n + c) & 31 of word (r n + c) >> 5, the maze's own n whatever the pitch
            u = bits.view(np.uint32)
            for r, c in ((0, 0), m["start"], m["goal"], (n - 1, n - 1), (n // 2, n // 2 + 1)):
                i = r * n + c
                assert (int(u[i >> 5]) >> (i & 31)) & 1 == int(g[r, c] != 0)
            # nothing past n n: the rest of the last used word and every later word
            used = (n * n + 31) // 32
            assert not u[used:].any()
            if (n * n) % 32:
                assert int(u[used - 1]) >> ((n * n) % 32) == 0
            assert int(sum(bin(int(x)).count("1") for x in u)) == int((g != 0).sum())


def test_one_bit_in_the_last_used_word():
    """15 x 15 = 7 * 32 + 1 and 81 x 81 = 205 * 32 + 1 cells: the last used word holds exactly
    one cell, the corner (n - 1, n - 1) — a wall in every euclidean maze, so the edge is made
    visible with an all-open grid."""
    from mazerl.archive import pack_grid, unpack_grid
    for n in (15, 81):
        assert (n * n) % 32 == 1
        g = np.ones((n, n), np.uint8)
        for P in (n, n + 4):
            u = pack_grid(g, P).view(np.uint32)
            used = (n * n + 31) // 32
            assert int(u[used - 1]) == 1 and not u[used:].any()
            assert (u[:used - 1] == 0xFFFFFFFF).all()
            assert np.array_equal(unpack_grid(u.view(np.int32), n), g)
        m = [x for x in G.mazes("gen_euclid.npz") if x["n"] == n][0]
        assert int(pack_grid(m["grid"]).view(np.uint32)[(n * n) // 32]) == int(m["grid"][-1, -1] != 0)
    with pytest.raises(ValueError):
        pack_grid(np.ones((9, 9), np.uint8), 7)
    with pytest.raises(ValueError):
        unpack_grid(np.zeros(2, np.int32), 9)


def test_archive_words_refusals():
    from mazerl.archive import archive_words
    assert archive_words(5) == 1 and archive_words(127) == 505
    for bad in (4, 128):
        with pytest.raises(ValueError):
            archive_words(bad)


# 2. header and bindings
def test_the_three_entry_points_are_declared_and_bound():
    from mazerl import _native
    from test_abi import declared
    for f in ("mz_archive_words", "mz_archive_push", "mz_archive_load"):
        assert f in declared() and f in _native.EXPORTS
    L = _native.load()
    assert len(L.mz_archive_push.argtypes) == 9 and len(L.mz_archive_load.argtypes) == 10


# the ring arithmetic, on host tensors (the kernels are not involved)
def test_ring_counts_and_entry_slots():
    torch = pytest.importorskip("torch")
    from mazerl import _native
    from mazerl.archive import MazeArchive
    env = types.SimpleNamespace(lib=_native.load(), device=torch.device("cpu"), num_envs=5,
                                max_dim=9)
    a = MazeArchive(env, 3)
    assert a.words == 3 and tuple(a.bits.shape) == (5, 3, 3) and tuple(a.meta.shape) == (5, 3, 2)
    counts = [0, 1, 3, 4, 8]
    a.count.copy_(torch.tensor(counts, dtype=torch.int32))
    assert a.held.tolist() == [0, 1, 3, 3, 3]
    assert a.dropped.tolist() == [0, 0, 0, 1, 5]
    for k in range(4):
        want = []
        for i, c in enumerate(counts):
            pushes = list(range(max(c - 3, 0), c))  # the push numbers still held, oldest first
            want.append(i * 3 + pushes[k] % 3 if k < len(pushes) else -1)
        assert a.entry_slot(k).tolist() == want, k
    assert a.newest_slot().tolist() == [-1, 3, 8, 9, 13]
    with pytest.raises(ValueError):
        a.entry_slot(-1)
    with pytest.raises(ValueError):
        MazeArchive(env, 0)
    # checkpoints: the same geometry round-trips, another pitch / ring / population is refused
    sd = a.state_dict()
    b = MazeArchive(env, 3)
    b.load_state_dict(sd)
    assert b.count.tolist() == counts
    other = types.SimpleNamespace(lib=env.lib, device=env.device, num_envs=5, max_dim=13)
    for bad in (MazeArchive(other, 3), MazeArchive(env, 4)):
        with pytest.raises(ValueError):
            bad.load_state_dict(sd)
    with pytest.raises(ValueError):
        b.load_state_dict({"format": "something else"})


# 3. the entry point
@pytest.mark.parametrize("argv, match", [
    (["--dim", "10"], "odd"),
    (["--growth", "9", "16"], "odd"),
    (["--growth", "8", "17"], "odd"),
    (["--growth", "17", "9"], "START <= MAX"),
    (["--growth", "9", "17", "--dim", "9"], "exclude"),
    (["--dim", "129"], "odd, in"),
    (["--storage", "hash"], "needs --capacity"),
    (["--storage", "hash", "--capacity", "1000"], "power of two"),
    (["--capacity", "1024"], "belong to --storage hash"),
    (["--grow-every", "8"], "belong to --storage hash"),
    (["--envs", "0"], "--envs"),
    (["--steps", "0"], "--steps"),
    (["--archive-slots", "0"], "--archive-slots"),
    (["--envs", "4", "--tables", "5"], "--tables"),
])
def test_train_tabular_refuses_before_any_gpu_call(argv, match, monkeypatch):
    from mazerl import train_tabular
    # main() must raise out of parse(): VectorMazeEnv is never reached (it is not even imported)
    import mazerl.vector_env as ve
    monkeypatch.setattr(ve.VectorMazeEnv, "__init__",
                        lambda *a, **k: pytest.fail("an env was built before the refusal"))
    with pytest.raises(ValueError, match=match):
        train_tabular.main(argv)


def test_train_tabular_defaults():
    from mazerl import train_tabular
    a = train_tabular.parse(["--growth", "9", "17", "--agent", "dq"])
    assert (a.start, a.max_dim, a.eps_decay, a.agent) == (9, 17, float(17 * 17 // 2), "dq")
    a = train_tabular.parse([])
    assert (a.start, a.max_dim, a.growth, a.storage) == (9, 9, None, "dense")
