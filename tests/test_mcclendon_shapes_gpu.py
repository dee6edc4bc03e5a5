"""The GPU McClendon kernels on hand-built tree mazes (tests/golden/shapes.npz: the reference's
ComplexityEvaluation values of the mazes of tests/maze_shapes.py, maze_complexity_evaluation.py:
310-329). Every other fixture came out of the reference's three generators, whose mazes reach only
part of k_mcclendon's case analysis (csrc/mz_mcclendon.hip); these reach the rest: one corridor that
is the whole graph, hallway views holding half of the graph (iterated in G's node order instead of
the set table's), hallway sizes across the thread / lane / wave paths and the set tables' resize
points, every reason for leaving a maze to the host, trees off the odd lattice, and a toroidal
handle's one-wave BFS through thousands of levels (a 79-square serpentine and spiral).

The mazes the order-exact kernel has to score itself (shape_cases.must_score, from the maze and
oracle/mcclendon.py alone) must come back with status 0 and bit-exact; any other maze may be left
to the host (status 2) but never scored wrongly; the Python wrapper, host fallback included, equals
the reference on every maze.
"""
import math

import numpy as np
import pytest

import maze_shapes as S
import shape_cases as SC

pytestmark = pytest.mark.gpu

SENT_F = 0x7FF8DEADBEEF0001  # a NaN payload: compared as bits
SENT_I = -0x5A5A5A5B
GUARD = 64


@pytest.fixture(scope="module")
def mods():
    import torch
    from mazerl import VectorMazeEnv, difficulty
    from mazerl import _native as N
    return torch, VectorMazeEnv, difficulty, N


def _load(mods, ms, toroidal=False):
    """One handle holding ms, loaded per size (a load sets N = the grid size)."""
    _, VectorMazeEnv, _, _ = mods
    dim = max(m["n"] for m in ms)
    env = VectorMazeEnv(len(ms), dim, enrich=True, device="cuda:0", generate=False,
                        toroidal=toroidal, done_list=False)
    for n in sorted({m["n"] for m in ms}):
        ids = [k for k, m in enumerate(ms) if m["n"] == n]
        grids = np.stack([ms[k]["grid"] for k in ids]).astype(np.uint8)
        sg = np.array([ms[k]["start"] + ms[k]["goal"] for k in ids], np.int32)
        env.load_mazes(grids, sg, env_ids=np.array(ids, np.int32))
    return env


class Guarded:
    """rows x width elements between guards, all sentinel: the kernel's out / status argument."""

    def __init__(self, torch, rows, width, dtype, sent):
        self.rows, self.width = rows, width
        self.it = torch.int64 if dtype == torch.float64 else torch.int32
        self.sent = sent
        self.t = torch.full((GUARD + rows * width + GUARD,), sent, dtype=self.it, device="cuda:0")
        self.esz = 8 if dtype == torch.float64 else 4
        self.np = np.float64 if dtype == torch.float64 else np.int32

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.esz

    def bits(self):
        return self.t.cpu().numpy()

    def body(self):
        b = self.bits()[GUARD:GUARD + self.rows * self.width]
        return np.ascontiguousarray(b).view(self.np).reshape(self.rows, self.width)

    def untouched_outside(self, rows):
        """Guards and body rows >= rows still hold the sentinel."""
        b = self.bits().copy()
        b[GUARD:GUARD + rows * self.width] = self.sent
        return bool((b == self.sent).all())


def _raw(mods, env, ids=None, spare=3, fn="mz_difficulty_batch"):
    """(out [n, 2], status [n]) of the raw entry point; guards and `spare` rows past n checked."""
    torch, _, _, N = mods
    n = env.num_envs if ids is None else len(ids)
    out = Guarded(torch, n + spare, 2, torch.float64, SENT_F)
    st = Guarded(torch, n + spare, 1, torch.int32, SENT_I)
    idt = None if ids is None else torch.as_tensor(np.asarray(ids, np.int32), device=env.device)
    N.check(getattr(N.load(), fn)(env._h, None if idt is None else idt.data_ptr(), n, out.ptr,
                                  st.ptr, env._stream()))
    torch.cuda.synchronize()
    assert out.untouched_outside(n) and st.untouched_outside(n), fn
    o, s = out.body()[:n], st.body()[:n, 0]
    assert (s != SENT_I).all() and (o.view(np.int64) != SENT_F).all(), fn  # every listed row written
    return o, s


def _loadable(m):
    return m["n"] % 2 == 1  # mz_load_mazes refuses even sizes (check_dim)


@pytest.fixture(scope="module")
def eu(mods):
    """Every odd-sized fixture maze in one euclidean handle of pitch 81, scored once."""
    ms = [m for m in SC.mazes() if _loadable(m)]
    assert len(ms) >= 150 and max(m["n"] for m in ms) == 81
    env = _load(mods, ms)
    pw, st = _raw(mods, env)
    yield dict(ms=ms, env=env, pw=pw, st=st)
    env.close()


def _check_raw(ms, pw, st, where):
    """4a: must-score mazes status 0; a scored maze equals the reference bit for bit; a finite
    reference value never meets status 1 / 3; a NaN row never a finite product under status 0."""
    declined = {}
    for k, m in enumerate(ms):
        tag = (where, m["index"], m["family"], m["n"], int(st[k]))
        if not SC.finite(m):
            assert not (st[k] == 0 and math.isfinite(pw[k, 0])), tag
            continue
        assert st[k] in (0, 2), tag
        if SC.must_score(m["index"]):
            assert st[k] == 0, tag + (SC.facts(m["index"]),)
        if st[k] == 0:
            assert math.log(pw[k, 0]) == m["difficulty"], tag + (math.log(pw[k, 0]), m["difficulty"])
            assert math.log(pw[k, 1]) == m["complexity"], tag + (math.log(pw[k, 1]), m["complexity"])
        else:
            assert pw[k, 0] == 0.0 and pw[k, 1] == 0.0, tag
            declined.setdefault(m["family"], []).append(m["index"])
    print(where, "left to the host:", declined)
    return declined


def _check_wrapper(D, env, ms, st):
    """4b: difficulty_batch (kernel + host fallback) == the reference on every finite row; a row
    on which the reference raises is never scored by the kernel, and the wrapper raises too."""
    fin = [k for k, m in enumerate(ms) if SC.finite(m)]
    d, c = D.difficulty_batch(env, np.array(fin, np.int32), complexity=True)
    for i, k in enumerate(fin):
        m = ms[k]
        assert d[i] == m["difficulty"] and c[i] == m["complexity"], \
            (m["index"], m["family"], m["n"], int(st[k]), d[i], m["difficulty"])
    nan = [k for k, m in enumerate(ms) if not SC.finite(m)]
    assert nan and (st[nan] != 0).all(), st[nan]
    for k in nan[:2] + nan[-2:]:
        with pytest.raises(ValueError):
            D.difficulty_batch(env, np.array([fin[0], k], np.int32))


def test_raw_status_and_products_match_the_reference(eu):
    ms = eu["ms"]
    must = sum(SC.finite(m) and SC.must_score(m["index"]) for m in ms)
    assert 3 * must >= 2 * len(ms)
    declined = _check_raw(ms, eu["pw"], eu["st"], "euclidean")
    # the reasons phase A / B document do decline: a straight goal square inside a corridor, a
    # solution whose points are all junctions, an open border square
    for k, m in enumerate(ms):
        f = SC.facts(m["index"])
        if SC.finite(m) and (f["goal_straight"] or f["all_junctions"] or f["open_border"]):
            assert eu["st"][k] == 2, (m["index"], m["family"], f)
    assert declined


def test_wrapper_with_host_fallback_matches_the_reference(mods, eu):
    _, _, D, _ = mods
    _check_wrapper(D, eu["env"], eu["ms"], eu["st"])


def test_even_sizes_are_refused_at_load(mods):
    _, VectorMazeEnv, _, _ = mods
    ms = [m for m in SC.mazes() if not _loadable(m)]
    assert ms
    env = VectorMazeEnv(2, 81, enrich=True, device="cuda:0", generate=False, done_list=False)
    for m in ms[:2]:
        with pytest.raises(Exception, match="even maze dim"):
            env.load_mazes(m["grid"][None], np.array([m["start"] + m["goal"]], np.int32))
    env.close()


def test_toroidal_handle_scores_the_cropped_mazes(mods):
    """The fixture's bordered mazes of >= 19 squares with their wall ring cropped off, in a
    toroidal handle: the kernel scores the bordered maze again (its distance field from the
    one-wave BFS: ~3,100 levels on the 79-square serpentine) — the same rule and equalities."""
    _, _, D, _ = mods
    src = [m for m in SC.mazes() if _loadable(m) and m["n"] >= 19 and m["family"] != "border"]
    ms = [dict(m, grid=m["grid"][1:-1, 1:-1], n=m["n"] - 2,
               start=(m["start"][0] - 1, m["start"][1] - 1),
               goal=(m["goal"][0] - 1, m["goal"][1] - 1)) for m in src]
    big = {m["family"] for m in ms if m["n"] == 79}
    assert {"serpentine", "spiral"} <= big and len(ms) >= 90
    env = _load(mods, ms, toroidal=True)
    pw, st = _raw(mods, env)
    _check_raw(ms, pw, st, "toroidal")
    _check_wrapper(D, env, ms, st)
    env.close()


def screen_takes(m):
    """What mz_screen.hip and k_compact_from_handle (mz_env.hip) document as the screen's input,
    from the maze itself: an odd-lattice maze (no open square at an even-even position or on the
    border, start and goal cells) whose cells form a spanning tree of the whole lattice, the goal
    a dead end (find_random_position keeps one-neighbour squares)."""
    g, n = m["grid"], m["n"]
    if not S.on_odd_lattice(g) or S.open_border(g) or n >= 128:
        return False
    if not all(x % 2 == 1 for x in m["start"] + m["goal"]):
        return False
    W = (n - 1) // 2
    if int((g[1::2, 1::2] != 0).sum()) != W * W:
        return False
    return S.degree(g, *m["goal"]) == 1


def test_screen_within_its_bound_of_the_reference(mods, eu):
    _, _, D, _ = mods
    ms = eu["ms"]
    p, e, st = D.screen_batch(eu["env"])
    taken, emax = 0, {}
    for k, m in enumerate(ms):
        tag = (m["index"], m["family"], m["n"], int(st[k]))
        assert st[k] in (0, 2), tag
        if screen_takes(m) and SC.finite(m):
            assert st[k] == 0, tag
            taken += 1
        if st[k] != 0:
            continue
        assert SC.finite(m), tag  # d = 0 between neighbouring points: declined
        assert e[k] > 0 and math.isfinite(e[k]), tag
        dref = m["difficulty"]
        assert abs(math.log(p[k]) - dref) <= 1.01 * e[k] + 4 * math.ulp(dref), \
            tag + (math.log(p[k]), dref, e[k])
        emax[m["family"]] = max(emax.get(m["family"], 0.0), float(e[k]))
    print("screen: largest e per family:", {f: f"{v:.3e}" for f, v in sorted(emax.items())})
    fams = {m["family"] for k, m in enumerate(ms) if st[k] == 0}
    assert taken >= 40 and {"serpentine", "spiral", "comb", "binary", "kruskal", "wilson"} <= fams


def test_subset_ids_write_their_rows_only(mods, eu):
    """A list naming a declined maze between two scored ones (and one maze twice): out[i] and
    status[i] belong to ids[i]; the rows past the list and the guards keep their bits — on both
    the order-exact kernel and the screen."""
    ms, st, pw = eu["ms"], eu["st"], eu["pw"]
    dec = [k for k in range(len(ms)) if st[k] == 2 and SC.finite(ms[k])]
    ok = [k for k in range(len(ms)) if st[k] == 0 and SC.finite(ms[k])]
    assert dec and len(ok) > 10
    ids = [ok[3], dec[0], ok[-1], dec[-1], ok[3], ok[7]]
    o, s = _raw(mods, eu["env"], ids, spare=5)
    assert np.array_equal(s, st[ids]) and np.array_equal(o.view(np.int64), pw[ids].view(np.int64))
    o1, s1 = _raw(mods, eu["env"], None, spare=0, fn="mz_screen_batch")
    o2, s2 = _raw(mods, eu["env"], ids, spare=5, fn="mz_screen_batch")
    assert np.array_equal(s2, s1[ids])
    for i, k in enumerate(ids):  # the screen's sums are atomic: equal within both bounds
        assert abs(o2[i, 0] - o1[k, 0]) <= (o2[i, 1] + o1[k, 1]) * o1[k, 0], (i, k)
