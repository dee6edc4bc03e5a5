"""Best-of-C mazes on the GPU for the vectorised trainers: the reference hands
its agent the easiest of six candidates by McClendon difficulty for every new maze
(BaseMazeEnv.generate_maze, base_maze_env.py:78-97; toroidal_maze_env.py:40-54, scored on the
bordered maze) — the env's first maze and every win's update_maze (off_policy_trainer.py:202,
ppo_trainer.py:96). Here both the initial mazes (mz_generate_best) and a maze bank's refilled
slots (mz_bank_create_ex, candidates = 6) are chosen by k_mcclendon + k_cand_select inside the
launch sequence, and checked against best_of_mazes — the same candidates scored with the host's
glibc log, argmin = the reference's first minimum (tests/test_greedy_rows.py pins best_of_mazes
to the host restatement, which tests/test_difficulty.py pins to the reference's values)."""
import numpy as np
import pytest
import torch

from test_bank import Solver

pytestmark = pytest.mark.gpu


def bank_key(seed, bank, algo, di=0):
    """mz_bank_fill's Philox key of a (bank, algorithm, size index) block."""
    return (seed ^ ((3 * bank + algo + 1) << 56) ^ (di << 48)) & 0xFFFFFFFFFFFFFFFF


def assert_bank_block(env, bank, algo, dim, di, slots, seed, epoch, toroidal=False):
    from mazerl.trainers.vector_trainer import best_of_mazes
    from mazerl.vector_env import ALGOS
    a = ALGOS[algo]
    key = (bank_key(seed, bank, a, di) + (epoch << 32)) & 0xFFFFFFFFFFFFFFFF
    grids, sg, _ = best_of_mazes(len(slots), dim, algo, seed=key, device="cuda:0", candidates=6,
                                 toroidal=toroidal)
    for k, j in enumerate(slots):
        g, info = env.bank_slot(bank, algo, dim, j)
        assert np.array_equal(g, grids[k, :dim, :dim]), (bank, algo, dim, j)
        assert info == tuple(int(x) for x in sg[k]), (bank, algo, dim, j)


def test_generate_best_matches_best_of_mazes():
    """VectorMazeEnv(candidates=6): instance e holds best_of_mazes' maze e (candidate c of maze e
    = Philox seed + 6 e + c), euclidean 21 x 21 and 81 x 81 (the headline's size)."""
    from mazerl import VectorMazeEnv
    from mazerl.trainers.vector_trainer import best_of_mazes
    for n, dim, algo in ((24, 21, "dfs"), (12, 81, "r-prim"), (12, 41, "prim&kill")):
        env = VectorMazeEnv(n, dim, enrich=True, device="cuda:0", seed=0x5EED0077, algorithm=algo,
                            done_list=False, candidates=6)
        grids, sg, _ = best_of_mazes(n, dim, algo, seed=0x5EED0077, device="cuda:0", candidates=6)
        for e in range(n):
            q = env.query(e)
            assert np.array_equal(env.grid(e), grids[e]), (dim, e)
            assert (q["start_r"], q["start_c"], q["goal_r"], q["goal_c"]) == tuple(sg[e])
            assert (q["r"], q["c"]) == (q["start_r"], q["start_c"]) and q["steps"] == 0
        st = env.select_stats()
        assert st["groups"] == n and st["unresolved"] == 0 and st["near_ties"] == 0
        env.close()


def test_generate_best_variable_size_toroidal_make_env():
    """make_env(candidates=6) over toroidal sizes (config 5's variable-size envs): instance i of
    size dims[i % 3] holds best_of_mazes' maze i (scored as the bordered maze)."""
    from mazerl.trainers.vector_trainer import best_of_mazes, make_env
    n, dims = 18, [17, 21, 29]
    env = make_env(n, dims, toroidal=True, algorithm="prim&kill", seed=0x5EED0100,
                   device="cuda:0", done_list=False, candidates=6)
    grids, sg, sizes = best_of_mazes(n, dims, "prim&kill", seed=0x5EED0100, device="cuda:0",
                                     candidates=6, toroidal=True)
    for e in range(n):
        m = int(sizes[e])
        q = env.query(e)
        assert q["n"] == m
        assert np.array_equal(env.grid(e), grids[e, :m, :m]), e
        assert (q["start_r"], q["start_c"], q["goal_r"], q["goal_c"]) == tuple(sg[e])
    assert env.select_stats()["unresolved"] == 0
    env.close()


def test_best_of_bank_first_fill_matches_best_of_mazes():
    """enable_bank(candidates=6): slot j of every (bank, algorithm) block's first fill is
    best_of_mazes' maze j for the block's Philox key (the candidates a C = 1 bank would build for
    slots 6 j .. 6 j + 5)."""
    from mazerl import VectorMazeEnv
    B, K, dim, seed = 32, 10, 21, 0xBA4C0011
    env = VectorMazeEnv(B, dim, enrich=True, device="cuda:0", seed=7, algorithm="r-prim",
                        done_list=False)
    env.enable_bank(slots=K, swap_every=10 ** 9, algorithms=["r-prim", "dfs", "prim&kill"],
                    seed=seed, candidates=6)
    torch.cuda.synchronize()
    for bank in (0, 1):
        for algo in ("r-prim", "dfs", "prim&kill"):
            assert_bank_block(env, bank, algo, dim, 0, range(K), seed, 0)
    st = env.select_stats()
    assert st["groups"] == 2 * 3 * K and st["unresolved"] == 0 and st["near_ties"] == 0
    env.close()


def test_best_of_bank_refill_rebuilds_consumed_slots_only():
    """A refill (epoch 1) rebuilds exactly the consumed slots [0, used) as best-of-6 mazes of the
    epoch-1 keys (the difficulty launch and the selection read the consumed count on the device)
    and leaves the others; winners receive the slots in instance order."""
    from mazerl import VectorMazeEnv
    from mazerl.vector_env import _ptr
    import mazerl._native as N
    B, K, dim, seed = 48, 40, 15, 0xBA4C0022
    env = VectorMazeEnv(B, dim, enrich=True, device="cuda:0", seed=9, algorithm="dfs",
                        done_list=False)
    env.enable_bank(slots=K, swap_every=10 ** 9, algorithms=["dfs"], seed=seed, candidates=6)
    torch.cuda.synchronize()
    before = [env.bank_slot(0, "dfs", dim, j) for j in range(K)]
    solver = Solver(env)
    used = 0
    for _ in range(400):
        env.step(solver.actions())
        env.reset_done(regen_won=True)
        used = int(env.bank_consumed()[1])
        if used >= 3:
            break
    assert 0 < used < K
    N.check(env.lib.mz_bank_fill(env._h, 0, seed, env._stream()))
    torch.cuda.synchronize()
    assert_bank_block(env, 0, "dfs", dim, 0, range(used), seed, 1)
    for j in range(used, K):
        g, info = env.bank_slot(0, "dfs", dim, j)
        assert np.array_equal(g, before[j][0]) and info == before[j][1]
    assert int(env.bank_consumed()[1]) == 0
    env.close()


def test_best_of_bank_multi_size_toroidal():
    """A toroidal bank over several sizes with best-of-6 slots (config 5's variable-size envs):
    size index di keys its slots with di << 48 and scores the bordered mazes."""
    from mazerl.trainers.vector_trainer import make_env
    dims, K, seed = [17, 25], 6, 0xBA4C0033
    env = make_env(16, dims, toroidal=True, algorithm="r-prim", seed=5, device="cuda:0",
                   done_list=False)
    env.enable_bank(slots=K, swap_every=10 ** 9, algorithms=["r-prim"], seed=seed, dims=dims,
                    candidates=6)
    torch.cuda.synchronize()
    for di, dim in enumerate(dims):
        assert_bank_block(env, 0, "r-prim", dim, di, range(K), seed, 0, toroidal=True)
    env.close()


def test_best_of_bank_rejects_bad_candidates():
    from mazerl import VectorMazeEnv, _native as N
    env = VectorMazeEnv(8, 21, enrich=True, device="cuda:0", seed=1)
    arr = (N.C.c_int32 * 1)(21)
    assert env.lib.mz_bank_create_ex(env._h, 4, arr, 1, 1, 0) != 0
    assert env.lib.mz_bank_create_ex(env._h, 4, arr, 1, 1, 65) != 0
    assert env.lib.mz_generate_best(env._h, None, 8, None, 0, 21, 1, 0, None) != 0
    assert env.lib.mz_bank_create_ex(env._h, 4, arr, 1, 1, 6) == 0
    env.close()
    big = VectorMazeEnv(4, 101, enrich=True, device="cuda:0", seed=1, generate=False)
    arr = (N.C.c_int32 * 1)(101)
    assert big.lib.mz_bank_create_ex(big._h, 4, arr, 1, 1, 6) == -2  # beyond the LDS plan
    assert big.lib.mz_bank_create_ex(big._h, 4, arr, 1, 1, 1) == 0   # one candidate: no scoring
    big.close()


# ---- the screen -> exact -> host pipeline (mz_screen.hip, k_cand_pick, k_cand_select) ---------
def _gen(n, dim, algo, seed, dbg):
    from mazerl import VectorMazeEnv
    env = VectorMazeEnv(n, dim, enrich=True, device="cuda:0", seed=seed, generate=False,
                        done_list=False)
    env.set_debug(dbg)
    env.select_stats(reset=True)
    env.generate(algorithm=algo, dim=dim, seed=seed, candidates=6)
    torch.cuda.synchronize()
    return env


def test_screen_decides_and_matches_exact_path():
    """The screen's picks == every group through the order-exact kernel (debug flag 1) == the
    host-log argmin of best_of_mazes; without the flag no group needs the exact kernel."""
    from mazerl.trainers.vector_trainer import best_of_mazes
    for n, dim, algo in ((40, 81, "r-prim"), (40, 81, "dfs"), (40, 41, "prim&kill")):
        seed = 0x5C2EE0 + dim
        a = _gen(n, dim, algo, seed, 0)
        b = _gen(n, dim, algo, seed, 1)
        grids, sg, _ = best_of_mazes(n, dim, algo, seed=seed, device="cuda:0", candidates=6)
        for e in range(n):
            assert np.array_equal(a.grid(e), grids[e]) and np.array_equal(b.grid(e), grids[e]), e
            qa, qb = a.query(e), b.query(e)
            assert qa == qb and (qa["start_r"], qa["start_c"], qa["goal_r"], qa["goal_c"]) == tuple(sg[e])
        sa, sb = a.select_stats(), b.select_stats()
        assert sa["groups"] == n and sa["exact"] == 0 and sa["unresolved"] == 0, sa
        assert sb["groups"] == n and sb["exact"] == n and sb["unresolved"] == 0, sb
        a.close()
        b.close()


def test_screen_cannot_decide_identical_candidates_exact_path_keeps_the_first():
    """All six candidates of a group from one seed (debug flag 4): equal difficulties, which no
    bound can separate — the group goes to the exact kernel, whose first-minimum rule keeps
    candidate 0 (the reference replaces only on a strict `<`): the maze of seed + 6 e."""
    from mazerl import VectorMazeEnv
    n, dim, seed = 24, 41, 0x71A5
    env = _gen(n, dim, "r-prim", seed, 4)
    ref = VectorMazeEnv(6 * n, dim, enrich=True, device="cuda:0", seed=seed, algorithm="r-prim",
                        done_list=False)
    for e in range(n):
        assert np.array_equal(env.grid(e), ref.grid(6 * e)), e
    st = env.select_stats()
    assert st["exact"] == n and st["unresolved"] == 0 and st["near_ties"] == 0, st
    env.close()
    ref.close()


def test_declined_candidates_are_scored_on_the_host():
    """Candidates the exact kernel declines (forced for every even-numbered one, debug flags
    1 | 2) are scored by the host restatement inside the stream: the selection is still the
    first minimum over all six (best_of_mazes), none unresolved."""
    from mazerl.trainers.vector_trainer import best_of_mazes
    n, dim, seed = 30, 33, 0xDEC1
    env = _gen(n, dim, "dfs", seed, 3)
    grids, sg, _ = best_of_mazes(n, dim, "dfs", seed=seed, device="cuda:0", candidates=6)
    for e in range(n):
        assert np.array_equal(env.grid(e), grids[e]), e
    st = env.select_stats()
    assert st["exact"] == n and st["host_scored"] == 3 * n and st["unresolved"] == 0, st
    env.close()


def test_bank_slots_with_host_scored_candidates():
    """A best-of-6 bank whose refill has its even candidates declined (host-scored): every slot
    equals the reference's first minimum over the six candidates (best_of_mazes)."""
    from mazerl import VectorMazeEnv
    B, K, dim, seed = 32, 12, 21, 0xBA4C0044
    env = VectorMazeEnv(B, dim, enrich=True, device="cuda:0", seed=3, algorithm="r-prim",
                        done_list=False)
    env.set_debug(3)
    env.select_stats(reset=True)
    env.enable_bank(slots=K, swap_every=10 ** 9, algorithms=["r-prim", "prim&kill"], seed=seed,
                    candidates=6)
    torch.cuda.synchronize()
    for algo in ("r-prim", "prim&kill"):
        assert_bank_block(env, 0, algo, dim, 0, range(K), seed, 0)
        assert_bank_block(env, 1, algo, dim, 0, range(K), seed, 0)
    st = env.select_stats()
    assert st["groups"] == 4 * K and st["host_scored"] == 4 * K * 3 and st["unresolved"] == 0, st
    env.close()


# ---- past the caps: kXCap = 256 groups for the order-exact kernel, kHCap = 256 declined candidates
# for the host restatement per run (mz_api.hip). What the code promises there: a group past kXCap
# keeps the screen's pick and is counted unresolved; a group with a declined candidate past kHCap
# picks among its scored candidates and is counted unresolved. Never a stale or foreign maze.
def _marker(dim):
    """A recognisable maze no generator makes: one corridor down column 1 and along the last row."""
    g = np.zeros((dim, dim), np.uint8)
    g[1:dim - 1, 1] = 1
    g[dim - 2, 1:dim - 1] = 1
    g[dim - 2, dim - 2] = 2
    return g, (1, 1, dim - 2, dim - 2)


def _gen_over_marker(n, dim, algo, seed, dbg):
    """_gen, every instance holding the marker maze before the best-of-6 generation."""
    from mazerl import VectorMazeEnv
    env = VectorMazeEnv(n, dim, enrich=True, device="cuda:0", seed=seed, generate=False,
                        done_list=False)
    g, sg = _marker(dim)
    env.load_mazes(np.repeat(g[None], n, 0), np.repeat(np.array([sg], np.int32), n, 0))
    assert np.array_equal(env.grid(n - 1), g)
    env.set_debug(dbg)
    env.select_stats(reset=True)
    env.generate(algorithm=algo, dim=dim, seed=seed, candidates=6)
    torch.cuda.synchronize()
    return env


class Candidates:
    """Candidate c of group e = instance 6 e + c of a plain env with the same seed."""

    def __init__(self, n, dim, algo, seed, toroidal=False):
        from mazerl import VectorMazeEnv
        self.env = VectorMazeEnv(6 * n, dim, enrich=True, device="cuda:0", seed=seed,
                                 algorithm=algo, done_list=False, toroidal=toroidal)
        self.toroidal = toroidal

    def maze(self, e, c):
        q = self.env.query(6 * e + c)
        return self.env.grid(6 * e + c), (q["start_r"], q["start_c"], q["goal_r"], q["goal_c"])

    def which(self, e, grid, sg):
        """The candidates of group e equal to (grid, sg)."""
        out = []
        for c in range(6):
            g, s = self.maze(e, c)
            if np.array_equal(g, grid) and tuple(s) == tuple(sg):
                out.append(c)
        return out

    def host_difficulties(self, e):
        from mazerl import difficulty as D
        fn = D.toroidal_difficulty if self.toroidal else D.maze_difficulty
        return [fn(g, s[:2], s[2:]) for g, s in (self.maze(e, c) for c in range(6))]


def _held(env, e):
    q = env.query(e)
    return env.grid(e), (q["start_r"], q["start_c"], q["goal_r"], q["goal_c"])


def test_more_groups_than_the_exact_kernel_takes_keep_the_screens_pick():
    """300 groups, every one sent to the order-exact kernel (debug flag 1): 256 go through it, 44
    keep the screen's pick, counted unresolved — one of the group's own six candidates, its host
    difficulty within the screen's bound ceiling (a relative 2^-30, tests/test_screen_gpu.py) of
    the group's minimum."""
    from mazerl.trainers.vector_trainer import best_of_mazes
    n, dim, seed = 300, 21, 0x0CA9E1
    env = _gen_over_marker(n, dim, "dfs", seed, 1)
    st = env.select_stats()
    assert st["groups"] == 300 and st["exact"] == 256 and st["unresolved"] == 44, st
    grids, sg, _ = best_of_mazes(n, dim, "dfs", seed=seed, device="cuda:0", candidates=6)
    cand = Candidates(n, dim, "dfs", seed)
    other = 0
    for e in range(n):
        g, s = _held(env, e)
        if np.array_equal(g, grids[e]) and s == tuple(sg[e]):
            continue
        other += 1  # not the first minimum: only a group past the cap may differ
        cs = cand.which(e, g, s)
        assert cs, e  # a stale or foreign maze
        d = cand.host_difficulties(e)
        assert abs(d[cs[0]] - min(d)) <= 2.0 ** -30 * abs(min(d)), (e, cs, d)
    assert other <= 44, other
    env.close()
    cand.env.close()


def _check_host_cap(held, n_groups, unresolved, grids, sg, cand):
    equal = 0
    for e in range(n_groups):
        g, s = held(e)
        assert cand.which(e, g, s), e  # one of its own six: no stale or foreign maze
        equal += int(np.array_equal(g, grids[e][:g.shape[0], :g.shape[1]]) and tuple(s) == tuple(sg[e]))
    assert equal >= n_groups - unresolved, (equal, unresolved)


def test_more_declined_candidates_than_the_host_takes():
    """100 groups through the exact kernel with every even candidate declined (debug flags 1 | 2):
    300 declined candidates, 256 host slots. The 44 left without a score lie in 15 .. 44 groups,
    counted unresolved; those pick among their scored candidates, every other group is the first
    minimum."""
    from mazerl.trainers.vector_trainer import best_of_mazes
    n, dim, seed = 100, 21, 0x0CA9E2
    env = _gen_over_marker(n, dim, "dfs", seed, 3)
    st = env.select_stats()
    assert st["groups"] == n and st["exact"] == n and st["host_scored"] == 256, st
    assert 15 <= st["unresolved"] <= 44, st
    grids, sg, _ = best_of_mazes(n, dim, "dfs", seed=seed, device="cuda:0", candidates=6)
    cand = Candidates(n, dim, "dfs", seed)
    _check_host_cap(lambda e: _held(env, e), n, st["unresolved"], grids, sg, cand)
    env.close()
    cand.env.close()


def test_more_declined_candidates_than_the_host_takes_toroidal_bank():
    """A toroidal best-of-6 bank block of 100 slots at 17 squares (every candidate through the
    exact kernel) with the even candidates declined (debug flag 2): 300 declined candidates per
    block against 256 host slots, for each of the two banks' fills."""
    from mazerl import VectorMazeEnv
    from mazerl.trainers.vector_trainer import best_of_mazes
    from mazerl.vector_env import ALGOS
    B, K, dim, seed = 16, 100, 17, 0xBA4C0055
    env = VectorMazeEnv(B, dim, enrich=True, device="cuda:0", seed=3, algorithm="dfs",
                        done_list=False, toroidal=True)
    env.set_debug(2)
    env.select_stats(reset=True)
    env.enable_bank(slots=K, swap_every=10 ** 9, algorithms=["dfs"], seed=seed, candidates=6)
    torch.cuda.synchronize()
    st = env.select_stats()
    assert st["groups"] == 2 * K and st["host_scored"] == 2 * 256, st
    assert 2 * 15 <= st["unresolved"] <= 2 * 44, st
    equal = 0
    for bank in (0, 1):
        key = bank_key(seed, bank, ALGOS["dfs"])
        grids, sg, _ = best_of_mazes(K, dim, "dfs", seed=key, device="cuda:0", candidates=6,
                                     toroidal=True)
        cand = Candidates(K, dim, "dfs", key, toroidal=True)
        for j in range(K):
            g, info = env.bank_slot(bank, "dfs", dim, j)
            assert cand.which(j, g, info), (bank, j)
            equal += int(np.array_equal(g, grids[j, :dim, :dim]) and info == tuple(int(x) for x in sg[j]))
        cand.env.close()
    assert equal >= 2 * K - st["unresolved"], (equal, st)
    env.close()


def test_generate_best_second_chunk():
    """mz_generate_best works in chunks of 49,152 / C groups: 8,200 groups of 6 at 15 squares put
    groups 8,192 .. 8,199 into a second chunk — instance e still holds the first minimum of
    candidates 6 e .. 6 e + 5 (checked on groups 8,190 .. 8,199, across the chunk boundary)."""
    from mazerl import VectorMazeEnv, difficulty as D
    n, dim, seed = 8200, 15, 0x0CA9E3
    env = VectorMazeEnv(n, dim, enrich=True, device="cuda:0", seed=seed, algorithm="dfs",
                        done_list=False, candidates=6)
    st = env.select_stats()
    assert st["groups"] == n and st["unresolved"] == 0, st
    cand = Candidates(n, dim, "dfs", seed)
    lo = 8190
    ids = np.arange(6 * lo, 6 * n, dtype=np.int32)
    d = D.difficulty_batch(cand.env, ids).reshape(n - lo, 6)
    for k, e in enumerate(range(lo, n)):
        g, s = cand.maze(e, int(d[k].argmin()))
        hg, hs = _held(env, e)
        assert np.array_equal(hg, g) and hs == s, e
    env.close()
    cand.env.close()
