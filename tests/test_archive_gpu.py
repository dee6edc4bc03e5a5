"""csrc/mz_archive.hip on the GPU: mz_archive_push against the host view of each instance
(env.grid / query / meta), mz_archive_load against mz_load_mazes of the same golden mazes, bit for
bit, the refusals of the load's memory contract, and MazeArchive.to_mazes. Every comparison is
exact."""
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
    """What the archive must hold for instance i, from the host accessors alone."""
    from mazerl.archive import pack_grid
    q, g = env.query(i), env.grid(i)
    n = q["n"]
    maxs = int(env.meta()[i, 5])
    m0 = n | n << 8 | q["start_r"] << 16 | q["start_c"] << 24
    m1 = q["goal_r"] | q["goal_c"] << 8 | maxs << 16
    assert q["max_steps"] == maxs
    return pack_grid(g, pitch), (m0, m1), algo


def assert_entry(arch_host, lin, want):
    bits, meta, algo = arch_host
    wb, wm, wa = want
    assert np.array_equal(bits[lin], wb), lin
    assert tuple(int(x) & 0xFFFFFFFF for x in meta[lin]) == wm, lin
    assert int(algo[lin]) == wa, lin


def host_view(a):
    return (a.bits.view(-1, a.words).cpu().numpy(), a.meta.view(-1, 2).cpu().numpy(),
            a.algo.view(-1).cpu().numpy())


# 4. push equals the host view
@gpu
@pytest.mark.parametrize("toroidal, sizes, pitch, B", [(False, (9, 15, 21), 21, 65),
                                                       (True, (9, 17, 21), 21, 65),
                                                       (False, (81,), 81, 1)])
def test_push_equals_the_host_view(toroidal, sizes, pitch, B):
    need_gpu()
    from mazerl.archive import MazeArchive, archive_words
    pool = by_size(toroidal)

    def pick(shift):
        return [pool[sizes[(i + shift) % len(sizes)]][(i // len(sizes) + shift) % len(pool[sizes[0]])]
                for i in range(B)]
    algos = [i % 3 for i in range(B)]
    env = make_env(pick(0), pitch, toroidal, algos=algos)
    assert {env.query(i)["n"] for i in range(B)} == set(sizes)
    a = MazeArchive(env, 3)
    assert a.words == archive_words(pitch)
    flags = torch.tensor([(i * 7 + 3) % 5 < 2 or i == B - 1 for i in range(B)])
    assert B == 1 or 0.3 < float(flags.float().mean()) < 0.7
    a.record(flags)
    hv = host_view(a)
    for i in range(B):
        for s in range(3):
            lin = i * 3 + s
            if flags[i] and s == 0:
                assert_entry(hv, lin, host_entry(env, i, pitch, algos[i]))
            else:  # untouched
                assert not hv[0][lin].any() and not hv[1][lin].any() and hv[2][lin] == 0
    assert a.count.cpu().tolist() == [int(f) for f in flags]
    # bits past N N of every stored entry are 0 (a 9 x 9 maze under pitch 21 leaves 11 words)
    for i in np.flatnonzero(flags.numpy()):
        n = env.query(int(i))["n"]
        u = hv[0][int(i) * 3].view(np.uint32)
        used = (n * n + 31) // 32
        assert not u[used:].any() and ((n * n) % 32 == 0 or int(u[used - 1]) >> ((n * n) % 32) == 0)

    # the ring wraps: slots = 2, three pushes with the mazes changed in between
    r = MazeArchive(env, 2)
    want = [[] for _ in range(B)]
    for push in range(3):
        if push:
            mz = pick(push)
            for n in sizes:
                ids = [i for i in range(B) if mz[i]["n"] == n]
                if ids:
                    env.load_mazes(np.stack([mz[i]["grid"] for i in ids]),
                                   np.array([list(mz[i]["start"]) + list(mz[i]["goal"]) for i in ids]),
                                   env_ids=ids)
            env.reset()
        f = None if push == 1 else torch.tensor([(i + push) % 3 != 1 for i in range(B)])
        r.record(f)
        for i in range(B):
            if f is None or bool(f[i]):
                want[i].append(host_entry(env, i, pitch, algos[i]))
    counts = [len(w) for w in want]
    assert r.count.cpu().tolist() == counts and max(counts) == 3
    assert r.held.cpu().tolist() == [min(c, 2) for c in counts]
    assert r.dropped.cpu().tolist() == [max(c - 2, 0) for c in counts]
    hv = host_view(r)
    for k in range(3):
        slots = r.entry_slot(k).cpu().tolist()
        for i in range(B):
            kept = want[i][-2:]
            if k < len(kept):
                assert i * 2 <= slots[i] < i * 2 + 2
                assert_entry(hv, slots[i], kept[k])
            else:
                assert slots[i] == -1
    newest = r.newest_slot().cpu().tolist()
    for i in range(B):
        assert_entry(hv, newest[i], want[i][-1])
    # the ABI's refusals: a wrong row length, no slots
    L = env.lib
    args = [env._h, None, 2, r.words, r.bits.data_ptr(), r.meta.data_ptr(), r.algo.data_ptr(),
            r.count.data_ptr(), None]
    for pos, bad in ((3, r.words + 1), (2, 0), (4, None)):
        x = list(args)
        x[pos] = bad
        assert L.mz_archive_push(*x) == -1 and L.mz_last_error()
    assert r.count.cpu().tolist() == counts
    env.close()


# 5. load equals mz_load_mazes
OUTPUTS = ("obs6", "reward64", "terminated", "truncated", "pos", "best_dir")


def trajectory(env, steps, seed=11):
    """The env's outputs under one fixed pseudo-random action sequence, reset_done() after each
    step: {name: [steps, ...]} on the host."""
    names = OUTPUTS + (("window_bits",) if env.window_bits is not None else ())
    g = torch.Generator().manual_seed(seed)
    acts = torch.randint(0, 4, (steps, env.num_envs), generator=g, dtype=torch.int32).to(env.device)
    rec = {k: [] for k in names}
    for t in range(steps):
        env.step(acts[t])
        for k in names:
            rec[k].append(getattr(env, k).clone())
        env.reset_done()
    return {k: torch.stack(v).cpu() for k, v in rec.items()}


def assert_same_envs(x, y, ids=None):
    ids = range(x.num_envs) if ids is None else ids
    mx, my = x.meta().cpu(), y.meta().cpu()
    for i in ids:
        assert np.array_equal(x.grid(i), y.grid(i)), i
        assert x.query(i) == y.query(i), i
        assert mx[i].tolist() == my[i].tolist(), i


def assert_same_trajectories(x, y):
    steps = int(max(x.meta()[:, 5].max(), y.meta()[:, 5].max())) + 2
    tx, ty = trajectory(x, steps), trajectory(y, steps)
    for k in tx:
        bad = (tx[k] != ty[k]).nonzero()
        assert bad.numel() == 0, (k, "first difference at (step, instance, ...)", bad[0].tolist())
    assert bool(tx["terminated"].any()) or bool(tx["truncated"].any())  # episodes ended and restarted


@gpu
@pytest.mark.parametrize("toroidal, enrich, sizes", [(False, False, (9, 15, 21)),
                                                     (False, True, (15, 21)),
                                                     (True, False, (9, 17, 21)),
                                                     (True, True, (9, 17, 21))])
def test_load_equals_load_mazes(toroidal, enrich, sizes):
    need_gpu()
    from mazerl.archive import MazeArchive
    pool = by_size(toroidal)
    n = 7
    src_mazes = [pool[sizes[i % len(sizes)]][i // len(sizes)] for i in range(n)]
    algos = [(i + 1) % 3 for i in range(n)]
    A = make_env(src_mazes, 21, toroidal, enrich, algos=algos)
    arch = MazeArchive(A, 1)
    arch.record()
    # target perm[j] takes the maze of A's instance j; target 4 (j = 2) is left alone
    perm = [3, 0, 4, 6, 1, 5, 2]
    slot = [j if perm[j] != 4 else -1 for j in range(n)]
    gd = sizes[0]
    B = make_env([None] * n, 21, toroidal, enrich, generate_dim=gd)
    C = make_env([src_mazes[perm.index(t)] if t != 4 else None for t in range(n)], 21, toroidal,
                 enrich, generate_dim=gd)
    kept = B.grid(4).copy()
    arch.load(B, torch.tensor(slot), env_ids=torch.tensor(perm))
    B.reset()
    assert int(arch.errors) == 0
    assert_same_envs(B, C)
    assert np.array_equal(B.grid(4), kept)
    want_steps = {m["n"]: m["max_steps"] for m in src_mazes}
    for j, t in enumerate(perm):
        if t != 4:  # max_steps is the fixture's own value (the reference's set_max_steps)
            assert B.query(t)["max_steps"] == src_mazes[j]["max_steps"], (t, want_steps)
    # the algorithm id travels with the entry: B pushed again holds A's entries
    back = MazeArchive(B, 1)
    back.record()
    for j, t in enumerate(perm):
        if t != 4:
            assert torch.equal(back.bits[t, 0], arch.bits[j, 0])
            assert torch.equal(back.meta[t, 0], arch.meta[j, 0])
            assert int(back.algo[t, 0]) == algos[j]
    assert_same_trajectories(B, C)
    for e in (A, B, C):
        e.close()


@gpu
def test_load_into_a_single_instance_and_from_another_pitch():
    need_gpu()
    from mazerl.archive import MazeArchive
    pool = by_size(False)
    m = pool[15][0]
    A = make_env([pool[9][0], m], 17)  # the archive's pitch is 17: rows of 10 words
    arch = MazeArchive(A, 2)
    arch.record()
    B = make_env([None], 21, generate_dim=9)  # B = 1, a larger pitch
    C = make_env([m], 21)
    arch.load(B, arch.entry_slot(0)[1:2])
    B.reset()
    assert int(arch.errors) == 0
    assert_same_envs(B, C)
    assert_same_trajectories(B, C)
    # a handle whose pitch cannot hold the entry refuses it and stays as it was
    D = make_env([None], 9, generate_dim=9)
    before = D.grid(0).copy()
    arch.load(D, arch.entry_slot(0)[1:2])
    D.reset()
    assert int(arch.errors) == 1 and np.array_equal(D.grid(0), before)
    for e in (A, B, C, D):
        e.close()


# 6. the memory contract
@gpu
def test_bad_entries_are_refused_and_leave_their_targets_untouched():
    """Hand-made bad entries beside good ones in one launch, each breaking exactly one rule of
    the load. The entries with a bad N are all-open squares of that N with start (1, 1) and goal
    (2, 2) — inside every N here, both bits set — and the same construction at N = 11 is a good
    entry of this launch, so only the rule on N refuses them; the source archive's pitch is 25, so
    N = P + 2 = 23 fits the source rows and fails the destination's pitch alone. The other three
    are recorded entries with one field changed. This test runs refusals only: every bad entry
    must be rejected by the kernel's own checks before any store."""
    need_gpu()
    from mazerl.archive import MazeArchive, pack_grid
    pool = by_size(False)
    P, n = 21, 8
    held = [pool[15][i] for i in range(n)]       # what the targets hold
    loaded = [pool[(9, 15, 21)[i % 3]][4 + i // 3] for i in range(n)]  # what the archive holds
    A = make_env(loaded, 25, algos=[1] * n)
    arch = MazeArchive(A, 1)
    arch.record()
    assert arch.words == 20
    meta = arch.meta.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    algo = arch.algo.cpu().numpy()

    def open_square(i, N):
        arch.bits[i, 0] = torch.from_numpy(pack_grid(np.ones((N, N), np.uint8), 25))
        meta[i, 0, 0] = N | N << 8 | 1 << 16 | 1 << 24
        meta[i, 0, 1] = 2 | 2 << 8
    open_square(0, 10)                                # N even
    open_square(1, P + 2)                             # N = P + 2
    open_square(2, 3)                                 # N = 3
    open_square(6, 11)                                # the control: the same square at a good N
    m0 = int(meta[3, 0, 0])
    meta[3, 0, 0] = m0 & 0xFFFF                       # the start on a wall, (0, 0)
    assert loaded[3]["grid"][0, 0] == 0
    m1 = int(meta[4, 0, 1])
    meta[4, 0, 1] = (m1 & ~0xFF) | (int(meta[4, 0, 0]) & 0xFF)  # goal row = N
    algo[5, 0] = 7                                    # algorithm id 7
    bad, good = [0, 1, 2, 3, 4, 5], [6, 7]
    arch.meta.copy_(torch.from_numpy(meta.astype(np.uint32).view(np.int32)))
    arch.algo.copy_(torch.from_numpy(algo))
    square = np.ones((11, 11), np.uint8)
    square[2, 2] = 2
    loaded[6] = dict(n=11, grid=square, start=(1, 1), goal=(2, 2))
    T = make_env(held, P)
    twin = make_env([held[i] if i in bad else loaded[i] for i in range(n)], P)
    arch.load(T, arch.entry_slot(0))
    T.reset()
    assert int(arch.errors) == len(bad)
    assert_same_envs(T, twin)
    for i in bad:
        assert np.array_equal(T.grid(i), held[i]["grid"])
    for i in good:
        assert np.array_equal(T.grid(i), loaded[i]["grid"])
    assert_same_trajectories(T, twin)
    # an instance id outside the handle is refused as well
    arch.errors.zero_()
    arch.load(T, arch.entry_slot(0)[6:8], env_ids=torch.tensor([n, -1]))
    T.reset()
    twin.reset()
    assert int(arch.errors) == 2
    assert_same_envs(T, twin)
    for e in (A, T, twin):
        e.close()


# 11. to_mazes
@gpu
def test_to_mazes_is_the_snapshot_and_loads_into_an_enrich_env():
    need_gpu()
    import mazerl
    from mazerl.archive import MazeArchive
    from mazerl.trainers.vector_trainer import load_selected, snapshot_mazes
    pool = by_size(True)
    mz = [pool[(9, 17, 21)[i % 3]][i // 3] for i in range(6)]
    env = make_env(mz, 21, toroidal=True)
    arch = MazeArchive(env, 2)
    arch.record()
    env.load_mazes(np.stack([pool[9][5]["grid"]]), np.array([list(pool[9][5]["start"]) +
                                                              list(pool[9][5]["goal"])]), env_ids=[1])
    env.reset()
    arch.record(torch.tensor([0, 1, 0, 0, 0, 0]))
    got = arch.to_mazes()
    want = snapshot_mazes(env, range(6))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    sub = arch.to_mazes(ids=[4, 1])
    for g, w in zip(sub, snapshot_mazes(env, [4, 1])):
        assert np.array_equal(g, w)
    assert len(arch.to_mazes(entry="all")[2]) == 7 and len(arch.to_mazes(entry=1)[2]) == 1
    assert np.array_equal(arch.to_mazes(ids=[1], entry=0)[0][0, :17, :17], mz[1]["grid"])
    env2 = mazerl.VectorMazeEnv(6, 9, toroidal=True, enrich=True, max_dim=21, generate=False)
    load_selected(env2, got)
    for i in range(6):
        assert np.array_equal(env2.grid(i), env.grid(i))
        assert env2.query(i) == env.query(i)
    env.close()
    env2.close()
