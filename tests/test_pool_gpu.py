"""mz_archive_push_pool on the GPU (csrc/mz_archive.hip, mazerl.archive.MazePool): the pool holds,
in call order and within a call in ascending instance id, exactly the host view of each flagged
instance (env.grid / query / meta) with its owner and stamp — across workgroups, for mixed sizes,
on the odd-word and the long-maze paths, for calls issued back to back, and never at or past its
capacity; it reads back through mz_archive_load as mz_load_mazes builds the same mazes. Every
comparison is exact."""
import numpy as np
import pytest

import golden_io as G

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def by_size(toroidal):
    out = {}
    for m in G.mazes("gen_toroid.npz" if toroidal else "gen_euclid.npz"):
        out.setdefault(m["n"], []).append(m)
    return out


def make_env(mazes, pitch, toroidal=False, enrich=False, algos=None, generate_dim=None):
    """One instance per maze (None: the instance keeps the maze generate_dim generated)."""
    import mazerl
    dims = [m["n"] for m in mazes if m is not None]
    env = mazerl.VectorMazeEnv(len(mazes), generate_dim or dims[0], toroidal=toroidal, enrich=enrich,
                               max_dim=pitch, reward64=True, generate=generate_dim is not None)
    for n in sorted(set(dims)):
        ids = [i for i, m in enumerate(mazes) if m is not None and m["n"] == n]
        env.load_mazes(np.stack([mazes[i]["grid"] for i in ids]),
                       np.array([list(mazes[i]["start"]) + list(mazes[i]["goal"]) for i in ids]),
                       env_ids=ids)
    if algos is not None:
        env.set_algorithm(torch.tensor(algos, dtype=torch.uint8))
    env.reset()
    return env


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


def host_table(env, pitch, algos):
    """host_entry of every instance as arrays: bits [B, W], meta uint32 [B, 2], algo [B]."""
    ent = [host_entry(env, i, pitch, algos[i]) for i in range(env.num_envs)]
    return (np.stack([e[0] for e in ent]), np.array([e[1] for e in ent], np.uint32),
            np.array([e[2] for e in ent], np.uint8))


def pool_host(p, rows=None):
    rows = p.bits.shape[0] if rows is None else rows
    return dict(bits=p.bits[:rows].cpu().numpy(),
                meta=p.meta[:rows].cpu().numpy().view(np.uint32),
                algo=p.algo[:rows].cpu().numpy(), owner=p.owner[:rows].cpu().numpy(),
                stamp=p.stamp[:rows].cpu().numpy())


def assert_pool(p, table, owners, stamps):
    """The pool's first len(owners) entries are the table rows of `owners`, stamped `stamps`;
    every later row is still zero."""
    n = len(owners)
    h = pool_host(p)
    idx = np.asarray(owners, np.int64)
    assert np.array_equal(h["owner"][:n], idx.astype(np.int32))
    assert np.array_equal(h["stamp"][:n], np.asarray(stamps, np.int32))
    assert np.array_equal(h["bits"][:n], table[0][idx])
    assert np.array_equal(h["meta"][:n], table[1][idx])
    assert np.array_equal(h["algo"][:n], table[2][idx])
    for k, v in h.items():
        assert not v[n:].any(), k


@pytest.fixture(scope="module")
def big():
    """B = 2 span + 1 instances of generated 9 x 9 mazes (pitch 9: 3 words, entries that are not
    8-byte aligned), algorithm ids i % 3, and their host table — shared, never changed."""
    need_gpu()
    from mazerl.archive import pool_span
    span = pool_span()
    B = 2 * span + 1
    algos = [i % 3 for i in range(B)]
    env = make_env([None] * B, 9, algos=algos, generate_dim=9)
    table = host_table(env, 9, algos)
    assert len({t.tobytes() for t in table[0]}) > B // 4  # the mazes differ
    yield env, table, span, B
    env.close()


def flag_patterns(B, span):
    g = torch.Generator().manual_seed(0xF1A6)
    rnd = (torch.rand(B, generator=g) < 1.0 / 3.0).to(torch.uint8)
    assert 0.28 < float(rnd.float().mean()) < 0.39 and int(rnd[:span].sum()) not in (0, span)

    def only(i):
        f = torch.zeros(B, dtype=torch.uint8)
        f[i] = 1
        return f
    return [torch.zeros(B, dtype=torch.uint8), torch.ones(B, dtype=torch.uint8), None, only(0),
            only(span), only(B - 1), rnd, 3 * rnd]  # (any nonzero byte is a flag)


def run_sequence(env, B, span, check=None):
    from mazerl.archive import MazePool
    pats = flag_patterns(B, span)
    p = MazePool(env, sum(B if f is None else int((f != 0).sum()) for f in pats) + 5)
    owners, stamps = [], []
    for k, f in enumerate(pats):
        p.record(f, stamp=10 + k)
        ids = list(range(B)) if f is None else torch.nonzero(f).reshape(-1).tolist()
        owners += ids
        stamps += [10 + k] * len(ids)
        if check is not None:
            assert int(p.count) == int(p.held) == len(owners) and int(p.dropped) == 0
            check(p, owners, stamps)
    return p


# 1. order and content across workgroups
@gpu
def test_order_and_content_across_workgroups(big):
    env, table, span, B = big
    p = run_sequence(env, B, span, lambda p, o, s: assert_pool(p, table, o, s))
    assert int(p.count) == p.capacity - 5


# 5. repeatability
@gpu
def test_the_sequence_is_repeatable_to_the_bit(big):
    env, table, span, B = big
    a, b = run_sequence(env, B, span), run_sequence(env, B, span)
    for k in ("bits", "meta", "algo", "owner", "stamp"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.count, b.count) and int(a.count) > 2 * B + 3  # (two whole calls)


# 2. mixed sizes and the long-maze path
@gpu
@pytest.mark.parametrize("toroidal, sizes, pitch, B", [(False, (9, 15, 21), 21, 65),
                                                       (True, (9, 17, 21), 21, 65),
                                                       (False, (81,), 81, 3)])
def test_mixed_sizes_and_the_long_maze_path(toroidal, sizes, pitch, B):
    need_gpu()
    from mazerl.archive import MazePool, archive_words
    pool = by_size(toroidal)
    mz = [pool[sizes[i % len(sizes)]][(i // len(sizes)) % len(pool[sizes[0]])] for i in range(B)]
    algos = [(i + 2) % 3 for i in range(B)]
    env = make_env(mz, pitch, toroidal, algos=algos)
    assert {env.query(i)["n"] for i in range(B)} == set(sizes)
    table = host_table(env, pitch, algos)
    p = MazePool(env, 3 * B)
    assert p.words == archive_words(pitch) and (pitch != 81 or p.words == 206)
    flags = torch.tensor([(i * 7 + 3) % 5 < 2 or i == B - 1 for i in range(B)])
    some = torch.nonzero(flags).reshape(-1).tolist()
    p.record(flags, stamp=4)
    p.record(None, stamp=5)
    assert_pool(p, table, some + list(range(B)), [4] * len(some) + [5] * B)
    assert int(p.count) == len(some) + B
    # bits past N N of every entry are 0 (a 9 x 9 maze under pitch 21 leaves 11 words)
    h = pool_host(p, int(p.count))
    for row, m in zip(h["bits"], h["meta"]):
        n = int(m[0]) & 0xFF
        used = (n * n + 31) // 32
        u = row.view(np.uint32)
        assert not u[used:].any() and ((n * n) % 32 == 0 or int(u[used - 1]) >> ((n * n) % 32) == 0)
    # the ABI's refusals, before any launch: a wrong row length, no capacity, a null array, a
    # misaligned counter
    L = env.lib
    args = [env._h, None, p.capacity, p.words, p.bits.data_ptr(), p.meta.data_ptr(),
            p.algo.data_ptr(), p.owner.data_ptr(), p.stamp.data_ptr(), p._count2.data_ptr(), 0, None]
    for pos, bad in ((3, p.words + 1), (2, 0), (2, -1), (4, None), (7, None), (8, None), (9, None),
                     (9, p._count2.data_ptr() + 2)):
        x = list(args)
        x[pos] = bad
        assert L.mz_archive_push_pool(*x) == -1 and L.mz_last_error()
    assert_pool(p, table, some + list(range(B)), [4] * len(some) + [5] * B)
    env.close()


# 3. back-to-back calls
@gpu
def test_back_to_back_calls_behave_as_sequential_calls(big):
    env, table, span, B = big
    from mazerl.archive import MazePool
    g = torch.Generator().manual_seed(77)
    fl = [(torch.rand(B, generator=g) < d).to(torch.uint8).to(env.device) for d in (0.5, 0.02, 0.9)]
    p = MazePool(env, 2 * B)
    torch.cuda.synchronize()
    for k, f in enumerate(fl):  # nothing between the three launches
        p.record(f, stamp=k + 1)
    torch.cuda.synchronize()
    ids = [torch.nonzero(f).reshape(-1).tolist() for f in fl]
    assert all(len(i) > 0 for i in ids)
    assert int(p.count) == sum(len(i) for i in ids)
    assert_pool(p, table, ids[0] + ids[1] + ids[2],
                [1] * len(ids[0]) + [2] * len(ids[1]) + [3] * len(ids[2]))


# 4. capacity
@gpu
def test_nothing_at_or_past_the_capacity_is_written(big):
    env, table, span, B = big
    from mazerl.archive import MazePool
    first = [3, span - 1, span, span + 7, 2 * span, 5, 64, 63, 1000, 2047]
    first = sorted(set(i for i in first if i < B))
    cap = len(first) + span + span // 2  # the all-instances call crosses it at instance 1.5 span
    p = MazePool(env, cap)
    S32, S8 = 0x5A5A5A5A, 0xA5
    back = {}
    for k in ("bits", "meta", "algo", "owner", "stamp"):
        t = getattr(p, k)
        big_t = torch.full((cap + 8,) + tuple(t.shape[1:]), S8 if t.dtype == torch.uint8 else S32,
                           dtype=t.dtype, device=t.device)
        back[k] = big_t
        setattr(p, k, big_t[:cap])
        assert getattr(p, k).data_ptr() == big_t.data_ptr()
    f = torch.zeros(B, dtype=torch.uint8)
    f[first] = 1
    p.record(f, stamp=1)
    p.record(None, stamp=2)
    assert (int(p.count), int(p.held), int(p.dropped)) == (len(first) + B, cap, len(first) + B - cap)
    owners = first + list(range(cap - len(first)))
    assert owners[-1] == span + span // 2 - 1
    stamps = [1] * len(first) + [2] * (cap - len(first))
    assert_pool(p, table, owners, stamps)  # (cap rows: all of them are entries)

    def guards_intact():
        for k, t in back.items():
            want = S8 if t.dtype == torch.uint8 else S32
            assert bool((t[cap:] == want).all()), k
    guards_intact()
    before = {k: t.clone() for k, t in back.items()}
    p.record(f, stamp=3)
    p.record(None, stamp=4)
    p.record(torch.zeros(B, dtype=torch.uint8), stamp=5)
    assert int(p.count) == 2 * (len(first) + B) and int(p.held) == cap
    for k, t in back.items():
        assert torch.equal(t, before[k]), k
    guards_intact()
    # the count saturates and does not wrap
    p._count2.fill_(2 ** 31 - 10)
    p.record(None, stamp=6)
    assert int(p.count) == 2 ** 31 - 1 and int(p.held) == cap
    for k, t in back.items():
        assert torch.equal(t, before[k]), k


# 6. load
def assert_same_envs(x, y, ids=None):
    ids = range(x.num_envs) if ids is None else ids
    mx, my = x.meta().cpu(), y.meta().cpu()
    for i in ids:
        assert np.array_equal(x.grid(i), y.grid(i)), i
        assert x.query(i) == y.query(i), i
        assert mx[i].tolist() == my[i].tolist(), i


@gpu
@pytest.mark.parametrize("toroidal, sizes", [(False, (9, 15, 21)), (True, (9, 17, 21))])
def test_load_equals_load_mazes_and_refuses_a_corrupted_entry(toroidal, sizes):
    need_gpu()
    from mazerl.archive import MazePool
    pool = by_size(toroidal)
    n = 7
    src = [pool[sizes[i % len(sizes)]][i // len(sizes)] for i in range(n)]
    algos = [(i + 1) % 3 for i in range(n)]
    A = make_env(src, 21, toroidal, algos=algos)
    p = MazePool(A, 2 * n)
    p.record(torch.tensor([1, 0, 1, 1, 0, 1, 1]), stamp=1)  # entries 0..4 = instances 0 2 3 5 6
    p.record(None, stamp=2)                                  # entries 5..11 = instances 0..6
    assert p.owner[:12].tolist() == [0, 2, 3, 5, 6, 0, 1, 2, 3, 4, 5, 6]
    # target t takes entry slot[t]; entry 3 (instance 5's maze) is corrupted, target 2 left alone
    slot = [6, 1, -1, 3, 11, 9, 2]
    inst = [1, 2, None, 5, 6, 4, 3]
    p.algo[3] = 7
    gd = sizes[0]
    B = make_env([None] * n, 21, toroidal, generate_dim=gd)
    C = make_env([src[i] if (i is not None and t != 3) else None for t, i in enumerate(inst)], 21,
                 toroidal, generate_dim=gd)
    kept = {t: B.grid(t).copy() for t in (2, 3)}
    p.load(B, torch.tensor(slot))
    B.reset()
    assert int(p.errors) == 1
    assert_same_envs(B, C)  # (the generated mazes of targets 2 and 3 come from the same seed)
    for t in (2, 3):
        assert np.array_equal(B.grid(t), kept[t])
    # the algorithm id travels with the entry: B pushed again holds A's entries
    back = MazePool(B, n)
    back.record()
    for t, i in enumerate(inst):
        if i is not None and t != 3:
            j = slot[t]
            assert torch.equal(back.bits[t], p.bits[j]) and torch.equal(back.meta[t], p.meta[j])
            assert int(back.algo[t]) == algos[i] and int(back.owner[t]) == t
    for e in (A, B, C):
        e.close()


# 7. round trip
@gpu
def test_to_mazes_and_a_state_dict_round_trip():
    need_gpu()
    from mazerl.archive import MazePool
    from mazerl.trainers.vector_trainer import snapshot_mazes
    pool = by_size(True)
    mz = [pool[(9, 17, 21)[i % 3]][i // 3] for i in range(6)]
    env = make_env(mz, 21, toroidal=True)
    p = MazePool(env, 9)
    p.record(torch.tensor([0, 1, 0, 0, 1, 1]), stamp=3)
    p.record(None, stamp=8)  # 9 offered, 9 held; one more call is dropped whole
    p.record(None, stamp=9)
    assert (int(p.count), int(p.held), int(p.dropped)) == (15, 9, 6)
    order = [1, 4, 5, 0, 1, 2, 3, 4, 5]
    got, want = p.to_mazes(), snapshot_mazes(env, order)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    for g, w in zip(p.to_mazes(2, 4), snapshot_mazes(env, order[2:6])):
        assert np.array_equal(g, w)
    assert len(p.to_mazes(9)[2]) == 0
    for bad in ((0, 10), (9, 1), (-1, 2)):
        with pytest.raises(ValueError):
            p.to_mazes(*bad)
    other = make_env([None] * 2, 21, toroidal=True, generate_dim=9)
    q = MazePool(other, 9)
    q.record(None, stamp=1)  # (its counter stands on the other word)
    q.load_state_dict(p.state_dict())
    for k in ("bits", "meta", "algo", "owner", "stamp", "errors"):
        assert torch.equal(getattr(p, k), getattr(q, k)), k
    assert (int(q.count), int(q.held), int(q.dropped)) == (15, 9, 6)
    for g, w in zip(q.to_mazes(), want):
        assert np.array_equal(g, w)
    q.record(None, stamp=2)  # and goes on counting from there
    assert int(q.count) == 17 and torch.equal(p.bits, q.bits) and torch.equal(p.stamp, q.stamp)
    small = make_env([None], 9, generate_dim=9)
    with pytest.raises(ValueError):
        MazePool(small, 9).load_state_dict(p.state_dict())
    for e in (env, other, small):
        e.close()
