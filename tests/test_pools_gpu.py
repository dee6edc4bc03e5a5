"""mz_archive_push_pools on the GPU (csrc/mz_archive.hip, mazerl.archive.MazePoolSet): the B
instances of a handle are G groups of b, and pool g holds, in call order and within a call in
ascending instance id, exactly the host view of each flagged instance of group g (env.grid /
query / meta) with its id within the group and the call's stamp — for groups smaller than, equal
to and larger than the workgroup span, for group starts that are no multiple of 16, for calls
issued back to back, and never at or past a pool's capacity. With one group it is
mz_archive_push_pool bit for bit. Every comparison is exact."""
import numpy as np
import pytest

from test_pool_gpu import (assert_same_envs, by_size, flag_patterns, host_table, make_env,
                           need_gpu)

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
KEYS = ("bits", "meta", "algo", "owner", "stamp")

# (G, b) with S = pool_span(): one group across workgroups (= the single pool), groups across
# workgroups with an unaligned second start, b = span, many groups inside one span with starts
# that are no multiples of 16, one instance per group
CASES = {"1x(2S+1)": lambda S: (1, 2 * S + 1), "2x(S+1)": lambda S: (2, S + 1),
         "3xS": lambda S: (3, S), "7x5": lambda S: (7, 5), "64x1": lambda S: (64, 1)}
case = pytest.mark.parametrize("name", list(CASES))


@pytest.fixture(scope="module")
def handles():
    """name -> (env, host table, G, b, span): generated 9 x 9 mazes at pitch 9 (3 words: entries
    that are not 8-byte aligned), algorithm ids i % 3 — built on first use, shared, never changed."""
    need_gpu()
    from mazerl.archive import pool_span
    span, made = pool_span(), {}

    def get(name):
        if name not in made:
            G, b = CASES[name](span)
            algos = [i % 3 for i in range(G * b)]
            env = make_env([None] * (G * b), 9, algos=algos, generate_dim=9)
            table = host_table(env, 9, algos)
            assert len({t.tobytes() for t in table[0]}) > min(G * b, 64) // 4  # the mazes differ
            made[name] = (env, table, G, b, span)
        return made[name]
    yield get
    for h in made.values():
        h[0].close()


def patterns(B, span, G, b):
    """test_pool_gpu.flag_patterns (its own where B exceeds a span, the same kinds below it) and
    one pattern that flags all of one group and none of its neighbours."""
    if B > span:
        pats = flag_patterns(B, span)
    else:
        g = torch.Generator().manual_seed(0xF1A6)
        rnd = (torch.rand(B, generator=g) < 1.0 / 3.0).to(torch.uint8)
        assert 0 < int(rnd.sum()) < B

        def only(i):
            f = torch.zeros(B, dtype=torch.uint8)
            f[i] = 1
            return f
        pats = [torch.zeros(B, dtype=torch.uint8), torch.ones(B, dtype=torch.uint8), None, only(0),
                only(B // 2), only(B - 1), rnd, 3 * rnd]
    return pats + [one_group(B, G, b, G // 2)]


def one_group(B, G, b, g):
    f = torch.zeros(B, dtype=torch.uint8)
    f[g * b:(g + 1) * b] = 1
    return f


class Model:
    """What the pools must hold: per group the (id within the group, stamp) of its entries."""

    def __init__(self, G, b, C):
        self.G, self.b, self.C = G, b, C
        self.entries = [[] for _ in range(G)]
        self.count = [0] * G

    def push(self, flags, stamp):
        f = np.ones(self.G * self.b, bool) if flags is None else (flags.cpu().numpy() != 0)
        for g in range(self.G):
            ids = np.nonzero(f[g * self.b:(g + 1) * self.b])[0].tolist()
            room = self.C - len(self.entries[g])
            self.entries[g] += [(i, stamp) for i in ids[:max(room, 0)]]
            self.count[g] = min(self.count[g] + len(ids), 2 ** 31 - 1)


def set_host(s):
    h = {k: getattr(s, k).cpu().numpy() for k in KEYS}
    h["meta"] = h["meta"].view(np.uint32)
    return h


def assert_set(s, table, model):
    """Pool g's first entries are the table rows of the model's instances of group g, with their
    local ids and stamps; every later row of every pool is still zero; the counts agree."""
    G, b, C = model.G, model.b, model.C
    h = set_host(s)
    rows, inst, owner, stamp = [], [], [], []
    for g, ent in enumerate(model.entries):
        assert len(ent) <= C
        rows += [g * C + k for k in range(len(ent))]
        inst += [g * b + i for i, _ in ent]
        owner += [i for i, _ in ent]
        stamp += [st for _, st in ent]
    rows, inst = np.asarray(rows, np.int64), np.asarray(inst, np.int64)
    assert np.array_equal(h["owner"][rows], np.asarray(owner, np.int32))
    assert np.array_equal(h["stamp"][rows], np.asarray(stamp, np.int32))
    assert np.array_equal(h["bits"][rows], table[0][inst])
    assert np.array_equal(h["meta"][rows], table[1][inst])
    assert np.array_equal(h["algo"][rows], table[2][inst])
    free = np.ones(G * C, bool)
    free[rows] = False
    for k, v in h.items():
        assert not v[free].any(), k
    assert s.count.tolist() == model.count
    assert s.held.tolist() == [min(c, C) for c in model.count]
    assert s.dropped.tolist() == [max(c - C, 0) for c in model.count]


def run_sequence(env, G, b, span, check=None):
    from mazerl.archive import MazePoolSet
    B = G * b
    pats = patterns(B, span, G, b)
    C = sum(b if f is None else int((f != 0).sum()) for f in pats) + 3  # (no pool can overflow)
    s, model = MazePoolSet(env, G, C), Model(G, b, C)
    for k, f in enumerate(pats):
        s.record(f, stamp=10 + k)
        model.push(f, 10 + k)
        if check is not None:
            check(s, model)
    return s, model


# 1. order, content and owner per group
@gpu
@case
def test_order_content_and_owner_per_group(handles, name):
    env, table, G, b, span = handles(name)
    s, model = run_sequence(env, G, b, span, lambda s, m: assert_set(s, table, m))
    assert sum(model.count) > 2 * G * b and not any(s.dropped.tolist())
    assert int(s.owner.max()) == b - 1  # the id within the group, not the instance id


# 2. one group is the single pool
@gpu
def test_one_group_is_the_single_pool_bit_for_bit(handles):
    from mazerl.archive import MazePool, MazePoolSet
    env, table, G, b, span = handles("1x(2S+1)")
    pats = patterns(b, span, 1, b)
    C = sum(b if f is None else int((f != 0).sum()) for f in pats) - span // 2  # (and it overflows)
    s, p = MazePoolSet(env, 1, C), MazePool(env, C)
    for k, f in enumerate(pats):
        s.record(f, stamp=k)
        p.record(f, stamp=k)
        assert int(s.count[0]) == int(p.count)
    for key in KEYS:
        assert torch.equal(getattr(s, key), getattr(p, key)), key
    assert int(p.dropped) == span // 2 == int(s.dropped[0]) and int(s.held[0]) == C
    v = s.pool(0)
    for key in KEYS:
        assert torch.equal(getattr(v, key), getattr(p, key)), key
    assert int(v.count) == int(p.count)


# 3. repeatability
@gpu
@case
def test_the_sequence_is_repeatable_to_the_bit(handles, name):
    env, table, G, b, span = handles(name)
    (x, _), (y, _) = run_sequence(env, G, b, span), run_sequence(env, G, b, span)
    for k in KEYS:
        assert torch.equal(getattr(x, k), getattr(y, k)), k
    assert torch.equal(x.count, y.count) and int(x.count.min()) >= 2 * b  # (two whole calls)


# 4. back-to-back calls
@gpu
@case
def test_back_to_back_calls_behave_as_sequential_calls(handles, name):
    from mazerl.archive import MazePoolSet
    env, table, G, b, span = handles(name)
    B = G * b
    g = torch.Generator().manual_seed(77)
    fl = [(torch.rand(B, generator=g) < d).to(torch.uint8).to(env.device) for d in (0.5, 0.1, 0.9)]
    fl.append(one_group(B, G, b, G - 1).to(env.device))
    assert all(int(f.sum()) > 0 for f in fl)
    s, model = MazePoolSet(env, G, 4 * b), Model(G, b, 4 * b)
    torch.cuda.synchronize()
    for k, f in enumerate(fl):  # nothing between the launches
        s.record(f, stamp=k + 1)
    torch.cuda.synchronize()
    for k, f in enumerate(fl):
        model.push(f, k + 1)
    assert_set(s, table, model)


# 5. capacity: exactly one group overflows, in the middle of a call where a call can
@gpu
@case
def test_nothing_at_or_past_a_pools_capacity_is_written(handles, name):
    """Group gx is flagged alone twice, then every instance once: gx is offered 3 b entries, the
    others b. C = 2 b + b // 2, so the last call crosses gx's capacity at its instance b // 2 (for
    b = 1 the whole third entry is dropped) and no other pool is full. The arrays sit in front of
    guard rows; gx is the middle group (the row past its pool is its neighbour's entry 0) and the
    last one (the row past its pool is the first guard row)."""
    from mazerl.archive import MazePoolSet
    env, table, G, b, span = handles(name)
    B, C = G * b, 2 * b + b // 2
    S32, S8 = 0x5A5A5A5A, 0xA5
    for gx in sorted({G // 2, G - 1}):
        s, model = MazePoolSet(env, G, C), Model(G, b, C)
        back = {}
        for k in KEYS:
            t = getattr(s, k)
            wide = torch.full((G * C + 8,) + tuple(t.shape[1:]), S8 if t.dtype == torch.uint8 else S32,
                              dtype=t.dtype, device=t.device)
            wide[:G * C] = 0
            back[k] = wide
            setattr(s, k, wide[:G * C])
            assert getattr(s, k).data_ptr() == wide.data_ptr()

        def guards_intact():
            for k, t in back.items():
                assert bool((t[G * C:] == (S8 if t.dtype == torch.uint8 else S32)).all()), k
        f = one_group(B, G, b, gx)
        for stamp, flags in ((1, f), (2, f), (3, None)):
            s.record(flags, stamp=stamp)
            model.push(flags, stamp)
        assert_set(s, table, model)  # (also: every row past a pool's last entry is still zero)
        want = [b] * G
        want[gx] = 3 * b
        assert s.count.tolist() == want and int(s.held[gx]) == C
        assert s.dropped.tolist() == [3 * b - C if g == gx else 0 for g in range(G)]
        assert model.entries[gx][-1] == ((b // 2 - 1, 3) if b > 1 else (0, 2))
        guards_intact()
        # a full pool takes nothing more, the others go on; the count saturates and does not wrap
        before = {k: t[gx * C:(gx + 1) * C].clone() for k, t in back.items()}
        s.record(f, stamp=4)
        s.record(None, stamp=5)
        model.push(f, 4)
        model.push(None, 5)
        assert_set(s, table, model)
        s._count2[gx].fill_(2 ** 31 - 2)
        s.record(None, stamp=6)
        assert int(s.count[gx]) == 2 ** 31 - 1 and int(s.held[gx]) == C
        for k, t in back.items():
            assert torch.equal(t[gx * C:(gx + 1) * C], before[k]), k
        guards_intact()


# 6. mixed sizes, the long-maze path and the ABI's refusals
@gpu
@pytest.mark.parametrize("toroidal, sizes, pitch, G, b", [(False, (9, 15, 21), 21, 6, 11),
                                                          (True, (9, 17, 21), 21, 6, 11),
                                                          (False, (81,), 81, 3, 1)])
def test_mixed_sizes_and_the_long_maze_path(toroidal, sizes, pitch, G, b):
    need_gpu()
    from mazerl.archive import MazePoolSet, archive_words
    pool, B = by_size(toroidal), G * b
    mz = [pool[sizes[i % len(sizes)]][(i // len(sizes)) % len(pool[sizes[0]])] for i in range(B)]
    algos = [(i + 2) % 3 for i in range(B)]
    env = make_env(mz, pitch, toroidal, algos=algos)
    assert {env.query(i)["n"] for i in range(B)} == set(sizes)
    table = host_table(env, pitch, algos)
    C = 3 * b
    s, model = MazePoolSet(env, G, C), Model(G, b, C)
    assert s.words == archive_words(pitch) and (pitch != 81 or s.words == 206)
    flags = torch.tensor([(i * 7 + 3) % 5 < 2 or i == B - 1 for i in range(B)]).to(torch.uint8)
    for stamp, f in ((4, flags), (5, None)):
        s.record(f, stamp=stamp)
        model.push(f, stamp)
    assert_set(s, table, model)
    # bits past N N of every entry are 0 (a 9 x 9 maze under pitch 21 leaves 11 words)
    h = set_host(s)
    for g in range(G):
        for k in range(len(model.entries[g])):
            row, m = h["bits"][g * C + k], h["meta"][g * C + k]
            n = int(m[0]) & 0xFF
            used = (n * n + 31) // 32
            u = row.view(np.uint32)
            assert not u[used:].any()
            assert (n * n) % 32 == 0 or int(u[used - 1]) >> ((n * n) % 32) == 0
    # the ABI's refusals, before any launch: no groups, groups that do not divide B, no capacity, a
    # wrong row length, a null array, a counter that is not 8-byte aligned, a parity out of range
    L = env.lib
    args = [env._h, None, G, C, s.words, s.bits.data_ptr(), s.meta.data_ptr(), s.algo.data_ptr(),
            s.owner.data_ptr(), s.stamp.data_ptr(), s._count2.data_ptr(), s._cur, 0, None]
    for pos, bad in ((2, 0), (2, -1), (2, B + 1), (2, 4 if B % 4 else 5), (3, 0), (3, -1),
                     (4, s.words + 1), (5, None), (6, None), (7, None), (8, None), (9, None),
                     (10, None), (10, s._count2.data_ptr() + 4), (11, 2), (11, -1)):
        x = list(args)
        x[pos] = bad
        assert L.mz_archive_push_pools(*x) == -1 and L.mz_last_error(), (pos, bad)
    torch.cuda.synchronize()
    assert_set(s, table, model)
    env.close()


# 7. load: rows of different pools into one env
@gpu
@pytest.mark.parametrize("toroidal, sizes", [(False, (9, 15, 21)), (True, (9, 17, 21))])
def test_load_of_rows_from_different_pools_equals_load_mazes(toroidal, sizes):
    need_gpu()
    from mazerl.archive import MazePoolSet
    pool = by_size(toroidal)
    G, b, C = 4, 2, 3
    src = [pool[sizes[i % len(sizes)]][i // len(sizes)] for i in range(G * b)]
    algos = [(i + 1) % 3 for i in range(G * b)]
    A = make_env(src, 21, toroidal, algos=algos)
    s = MazePoolSet(A, G, C)
    s.record(torch.tensor([1, 0, 0, 1, 1, 1, 0, 0]), stamp=1)  # pools: [0], [1], [0, 1], []
    s.record(None, stamp=2)                                     # then instances 0, 1 of each
    assert s.held.tolist() == [3, 3, 3, 2]
    assert s.owner.tolist() == [0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 0]
    # target t takes linear row g C + k; target 3 is left alone
    rows = [3 * C + 1, 0, 2 * C + 0, -1, 1 * C + 2, 2 * C + 2, 0 * C + 2]
    inst = [7, 0, 4, None, 3, 4, 1]  # the instances of A those rows hold
    gd = sizes[0]
    T = make_env([None] * len(rows), 21, toroidal, generate_dim=gd)
    W = make_env([None if i is None else src[i] for i in inst], 21, toroidal, generate_dim=gd)
    s.load(T, torch.tensor(rows))
    T.reset()
    assert int(s.errors) == 0
    assert_same_envs(T, W)  # (target 3's generated maze comes from the same seed)
    # one pool through its view: the view's slots are the pool's own entry numbers
    V = make_env([None] * 3, 21, toroidal, generate_dim=gd)
    s.pool(2).load(V, torch.tensor([2, 0, 1]))
    V.reset()
    W2 = make_env([src[4], src[4], src[5]], 21, toroidal)
    assert_same_envs(V, W2)
    for e in (A, T, W, V, W2):
        e.close()


# 8. round trip
@gpu
def test_to_mazes_and_a_state_dict_round_trip():
    need_gpu()
    from mazerl.archive import MazePool, MazePoolSet
    from mazerl.trainers.vector_trainer import snapshot_mazes
    pool = by_size(True)
    mz = [pool[(9, 17, 21)[i % 3]][i // 3] for i in range(6)]
    env = make_env(mz, 21, toroidal=True)
    s = MazePoolSet(env, 2, 5)
    s.record(torch.tensor([0, 1, 0, 0, 1, 1]), stamp=3)
    s.record(None, stamp=8)
    s.record(None, stamp=9)  # pool 0: 1 + 3 + 3 offered, 5 held; pool 1: 2 + 3 + 3, 5 held
    assert (s.count.tolist(), s.held.tolist(), s.dropped.tolist()) == ([7, 8], [5, 5], [2, 3])
    order = [[1, 0, 1, 2, 0], [4, 5, 3, 4, 5]]
    for g in (0, 1):
        got, want = s.pool(g).to_mazes(), snapshot_mazes(env, order[g])
        for x, w in zip(got, want):
            assert x.dtype == w.dtype and np.array_equal(x, w)
        for x, w in zip(s.pool(g).to_mazes(1, 3), snapshot_mazes(env, order[g][1:4])):
            assert np.array_equal(x, w)
    other = make_env([None] * 4, 21, toroidal=True, generate_dim=9)
    q = MazePoolSet(other, 2, 5)
    q.record(None, stamp=1)  # (its counters stand on the other word)
    q.load_state_dict(s.state_dict())
    for k in KEYS + ("errors",):
        assert torch.equal(getattr(s, k), getattr(q, k)), k
    assert (q.count.tolist(), q.held.tolist(), q.dropped.tolist()) == ([7, 8], [5, 5], [2, 3])
    q.record(None, stamp=2)  # and goes on counting from there
    assert q.count.tolist() == [9, 10] and torch.equal(s.bits, q.bits)
    # pool g of the set is the MazePool of a b-instance env: its checkpoint loads into one
    small = make_env(mz[3:], 21, toroidal=True)
    p = MazePool(small, 5)
    p.record(torch.tensor([0, 1, 1]), stamp=3)
    p.record(None, stamp=8)
    p.record(None, stamp=9)
    v = s.pool(1)
    for k in KEYS:
        assert torch.equal(getattr(v, k), getattr(p, k)), k
    assert int(v.count) == int(p.count) == 8
    with pytest.raises(ValueError):
        MazePoolSet(other, 4, 5).load_state_dict(s.state_dict())
    for e in (env, other, small):
        e.close()
