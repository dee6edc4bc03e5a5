"""Hand-built tree mazes for the McClendon difficulty checks (pure numpy, no GPU).

Every maze the difficulty code was pinned on before came out of the reference's three generators
(r-prim, dfs, prim&kill). The builders here make trees those generators do not: each turns a tree
over the W x W cell lattice (cell (r, c) = square (2 r + 1, 2 c + 1), a link opens the square in
between) into a bordered (2 W + 1)^2 grid, 0 = wall, 1 = open, the goal square holding 2 (the
convention of tests/golden/mcclendon.npz), plus start and goal squares.

cases() is the deterministic list tests/golden/make_golden_shapes.py scores with the reference
and stores in tests/golden/shapes.npz; tests/test_difficulty_shapes.py asserts that cases() still
regenerates exactly the stored grids.

Families (FAMILIES gives the ids stored in the fixture):
  serpentine  boustrophedon: one corridor through every cell;
  spiral      one corridor winding inward;
  comb        a spine along row 0 with a straight tooth down every column;
  zigzag      a spine down column 0 whose teeth are unit square waves: a tooth with k corners is a
              hallway of k + 1 nodes next to one junction, so the hallway sizes are chosen freely;
  zigzag_side the same with dead-end stubs hung on the teeth: hallways between two junctions;
  binary      each cell links north or west (random.Random(seed)): long border corridors;
  kruskal     a uniformly shuffled Kruskal tree;
  wilson      a uniform spanning tree (loop-erased random walks);
  adjacent    start and goal one passage apart on a Kruskal tree;
  shifted     one of the above moved one square down and right, off the odd lattice: with one
              extra wall row and column at the top-left (even N), or one on every side (odd N,
              the cells on even coordinates) — still a tree inside a wall ring;
  border      a Kruskal tree with one more open square on the grid's border, a leaf next to a cell;
  staircase   a corridor of unit steps in which every open square is a corner: neighbouring points
              lie d = 0 apart and the reference divides by zero.
"""
import random

import numpy as np

FAMILIES = ["serpentine", "spiral", "comb", "zigzag", "zigzag_side", "binary", "kruskal", "wilson",
            "adjacent", "shifted", "staircase", "border"]


# ---- cell trees -----------------------------------------------------------------------------
def _links(path):
    return list(zip(path, path[1:]))


def serpentine_path(W):
    return [(r, c) for r in range(W) for c in (range(W) if r % 2 == 0 else range(W - 1, -1, -1))]


def spiral_path(W):
    seen, path = set(), []
    r, c, dr, dc = 0, 0, 0, 1
    for _ in range(W * W):
        path.append((r, c))
        seen.add((r, c))
        nr, nc = r + dr, c + dc
        if not (0 <= nr < W and 0 <= nc < W) or (nr, nc) in seen:
            dr, dc = dc, -dr  # turn right
            nr, nc = r + dr, c + dc
        r, c = nr, nc
    return path


def comb_links(W):
    out = [((0, c), (0, c + 1)) for c in range(W - 1)]
    for c in range(W):
        out += [((r, c), (r + 1, c)) for r in range(W - 1)]
    return out


def tooth_cells(r, W):
    """The unit square wave of the two-row band r, r + 1 over columns 1 .. W - 1: every cell of it
    but the last one used is a corner."""
    out = []
    for c in range(1, W):
        out += [(r, c), (r + 1, c)] if c % 2 == 1 else [(r + 1, c), (r, c)]
    return out


def zigzag_links(W, corners, stubs=()):
    """Spine down column 0; tooth t leaves the spine at row band * t (band = 2 rows, 3 with stubs)
    and has corners[t] corners. stubs[t] lists positions along tooth t (cells of the band's lower
    row: p % 4 in (1, 2)) that get a one-cell dead end below them, which makes them junctions."""
    band = 3 if stubs else 2
    assert band * (len(corners) - 1) + band - 1 < W
    out = [((r, 0), (r + 1, 0)) for r in range(W - 1)]
    ends = []
    for t, k in enumerate(corners):
        cells = tooth_cells(band * t, W)
        assert 0 <= k < len(cells)
        tooth = [(band * t, 0)] + cells[:k + 1]
        out += _links(tooth)
        ends.append(tooth[-1])
        for p in (stubs[t] if stubs else ()):
            r, c = cells[p]
            assert p < k and r == band * t + 1
            out.append(((r, c), (r + 1, c)))
    return out, ends


def binary_links(W, seed):
    rng = random.Random(seed)
    out = []
    for r in range(W):
        for c in range(W):
            if r == 0 and c == 0:
                continue
            north = c == 0 or (r > 0 and rng.random() < 0.5)
            out.append(((r, c), (r - 1, c) if north else (r, c - 1)))
    return out


def kruskal_links(W, seed):
    rng = random.Random(seed)
    edges = [((r, c), (r, c + 1)) for r in range(W) for c in range(W - 1)]
    edges += [((r, c), (r + 1, c)) for r in range(W - 1) for c in range(W)]
    rng.shuffle(edges)
    root = {(r, c): (r, c) for r in range(W) for c in range(W)}

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    out = []
    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            root[ra] = rb
            out.append((a, b))
    return out


def wilson_links(W, seed):
    rng = random.Random(seed)
    cells = [(r, c) for r in range(W) for c in range(W)]
    in_tree = {cells[0]}
    out = []
    for s in cells:
        if s in in_tree:
            continue
        nxt, x = {}, s
        while x not in in_tree:  # the walk's last exit from each cell is its loop-erased step
            r, c = x
            nb = [(r + dr, c + dc) for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1))
                  if 0 <= r + dr < W and 0 <= c + dc < W]
            nxt[x] = rng.choice(nb)
            x = nxt[x]
        x = s
        while x not in in_tree:
            in_tree.add(x)
            out.append((x, nxt[x]))
            x = nxt[x]
    return out


# ---- grids ----------------------------------------------------------------------------------
def grid_of(W, links, start, goal, pad=0):
    """(grid, start square, goal square) of a cell tree. pad 1: one extra wall row and column at
    the top-left; pad 2: one on every side. Both move the cells to even coordinates."""
    n = 2 * W + 1
    g = np.zeros((n, n), np.uint8)
    for (r0, c0), (r1, c1) in links:
        assert abs(r0 - r1) + abs(c0 - c1) == 1
        g[2 * r0 + 1, 2 * c0 + 1] = g[2 * r1 + 1, 2 * c1 + 1] = g[r0 + r1 + 1, c0 + c1 + 1] = 1
    o = 1 if pad else 0
    s = (2 * start[0] + 1 + o, 2 * start[1] + 1 + o)
    t = (2 * goal[0] + 1 + o, 2 * goal[1] + 1 + o)
    if pad:
        g = np.pad(g, ((1, pad - 1), (1, pad - 1)))
    assert g[s] == 1 and g[t] == 1 and s != t
    g[t] = 2
    return g, s, t


def staircase_grid(n):
    g = np.zeros((n, n), np.uint8)
    for k in range(1, n - 2):
        g[k, k] = g[k, k + 1] = 1
    g[n - 2, n - 2] = 2
    return g, (1, 1), (n - 2, n - 2)


def _corner_ids(path):
    return [i for i in range(1, len(path) - 1)
            if path[i - 1][0] != path[i + 1][0] and path[i - 1][1] != path[i + 1][1]]


def _straight_ids(path):
    cs = set(_corner_ids(path))
    return [i for i in range(1, len(path) - 1) if i not in cs]


def _dead_ends(W, links):
    deg = {}
    for a, b in links:
        deg[a] = deg.get(a, 0) + 1
        deg[b] = deg.get(b, 0) + 1
    return sorted(x for x, d in deg.items() if d == 1)


def _pick(xs, frac):
    return xs[min(len(xs) - 1, int(frac * len(xs)))]


SIZES = {15: 7, 21: 10, 41: 20, 81: 40}  # squares -> cells per side


def cases():
    """The fixture's mazes, in order: dicts of family, name, n, grid, start, goal."""
    out = []

    def add(family, name, W, links, start, goal, pad=0):
        g, s, t = grid_of(W, links, start, goal, pad)
        out.append(dict(family=family, name=name, n=g.shape[0], grid=g, start=s, goal=t))

    # one corridor: ends, reversed, goal at a corner / on a straight cell, both inside
    for fam, mk in (("serpentine", serpentine_path), ("spiral", spiral_path)):
        for n, W in SIZES.items():
            p = mk(W)
            co, stt = _corner_ids(p), _straight_ids(p)
            L = _links(p)
            add(fam, f"{n}-ends", W, L, p[0], p[-1])
            if n == 81:
                add(fam, f"{n}-goal-corner-quarter", W, L, p[0], p[_pick(co, 0.25)])
                continue
            add(fam, f"{n}-reversed", W, L, p[-1], p[0])
            add(fam, f"{n}-goal-corner-quarter", W, L, p[0], p[_pick(co, 0.25)])
            add(fam, f"{n}-goal-corner-late", W, L, p[0], p[_pick(co, 0.8)])
            add(fam, f"{n}-goal-straight", W, L, p[0], p[_pick(stt, 0.5)])
            add(fam, f"{n}-inside-corners", W, L, p[_pick(co, 0.3)], p[_pick(co, 0.7)])
            if n <= 21:
                add(fam, f"{n}-start-straight-goal-end", W, L, p[_pick(stt, 0.4)], p[-1])
    # comb
    for n, W in SIZES.items():
        L = comb_links(W)
        add("comb", f"{n}-tips", W, L, (W - 1, 0), (W - 1, W - 1))
        if n == 81:
            continue
        add("comb", f"{n}-inner-tips", W, L, (W - 1, 2), (W - 1, W - 3))
        add("comb", f"{n}-spine-ends", W, L, (0, 0), (0, W - 1))
        add("comb", f"{n}-spine-inside", W, L, (0, 1), (0, W - 2))
        add("comb", f"{n}-tip-to-spine-end", W, L, (W - 1, W // 2), (0, 0))
    # zig-zag teeth: corners per tooth sweep the hallway sizes (nodes = corners + 1, + 1 junction)
    zz = [(15, (0, 1, 2)), (15, (3, 7, 11)), (15, (11, 5, 0)),
          (21, (1, 2, 3, 4, 5)), (21, (9, 11, 13, 15, 17)), (21, (12, 13, 14, 16, 17)),
          (41, tuple(range(0, 10))), (41, tuple(range(10, 20))), (41, tuple(range(20, 30))),
          (41, tuple(range(28, 38))), (41, (37, 1, 30, 2, 18, 3, 12, 13, 14, 4)),
          (81, tuple(range(27, 47))), (81, tuple(range(39, 78, 2))), (81, tuple(range(58, 78)))]
    for n, ks in zz:
        W = SIZES[n]
        L, ends = zigzag_links(W, ks)
        tag = f"{n}-k{ks[0]}-{ks[-1]}"
        add("zigzag", tag + "-spine", W, L, (0, 0), (W - 1, 0))
        if n <= 41:
            add("zigzag", tag + "-tooth-to-tooth", W, L, ends[0], ends[-1])
            add("zigzag", tag + "-tooth-to-spine", W, L, ends[len(ends) // 2], (W - 1, 0))
    zs = [(15, (5, 9), ((1,), (2, 6))), (21, (7, 12, 17), ((5,), (1, 9), (6, 13))),
          (41, (9, 15, 21, 27, 33, 37), ((1,), (6,), (2, 13), (14,), (5, 21), (17, 30))),
          (41, (4, 8, 12, 16, 20, 24), ((1,), (2,), (5, 9), (6,), (1, 14), (10, 18))),
          (81, tuple(range(20, 46, 2)), tuple((4 * (t % 4) + 1, 4 * (t % 4) + 10) for t in range(13)))]
    for n, ks, st in zs:
        W = SIZES[n]
        L, ends = zigzag_links(W, ks, st)
        tag = f"{n}-k{ks[0]}-{ks[-1]}"
        add("zigzag_side", tag + "-spine", W, L, (0, 0), (W - 1, 0))
        if n <= 41:
            add("zigzag_side", tag + "-tooth-to-tooth", W, L, ends[0], ends[-1])
    # random trees: binary, Kruskal, Wilson
    for fid, (fam, mk) in enumerate((("binary", binary_links), ("kruskal", kruskal_links),
                                     ("wilson", wilson_links))):
        for n, W in SIZES.items():
            for k in range(1 if n == 81 else 3 if n == 41 else 4):
                seed = 1000 * fid + 10 * n + k
                L = mk(W, seed)
                de = _dead_ends(W, L)
                rng = random.Random(seed ^ 0x5A)
                if k % 2 == 0:
                    s, t = (0, 0), (W - 1, W - 1)
                    if fam == "binary":  # (0, 0) .. a far dead end; the corner cell is a corner
                        t = de[-1]
                else:
                    s, t = rng.sample(de, 2)
                add(fam, f"{n}-seed{seed}", W, L, s, t)
    # start one passage from the goal
    for n, W in SIZES.items():
        for k in range(1 if n == 81 else 2):
            seed = 7000 + 10 * n + k
            L = kruskal_links(W, seed)
            a, b = random.Random(seed).choice(L)
            add("adjacent", f"{n}-seed{seed}", W, L, a, b)
    # off the odd lattice: pad 1 -> even N, pad 2 -> odd N, the cells on even coordinates
    for base, W in ((13, 6), (15, 7), (19, 9), (39, 19), (79, 39)):
        sp, se = spiral_path(W), serpentine_path(W)
        zk = tuple(range(0, W // 2))
        zl, _ = zigzag_links(W, zk)
        trees = [("spiral", _links(sp), sp[0], sp[-1]), ("serpentine", _links(se), se[0], se[-1]),
                 ("comb", comb_links(W), (W - 1, 0), (W - 1, W - 1)),
                 ("zigzag", zl, (0, 0), (W - 1, 0)),
                 ("kruskal", kruskal_links(W, 8000 + base), (0, 0), (W - 1, W - 1)),
                 ("wilson", wilson_links(W, 8500 + base), (0, 0), (W - 1, W - 1)),
                 ("binary", binary_links(W, 8700 + base), (0, 0), (W - 1, W - 1))]
        if base == 79:
            trees = trees[:2] + trees[4:5]
        for nm, L, s, t in trees:
            if base >= 15 and nm in ("spiral", "kruskal", "zigzag"):
                add("shifted", f"{base + 1}-{nm}", W, L, s, t, pad=1)
            if base != 15:
                add("shifted", f"{base + 2}-{nm}", W, L, s, t, pad=2)
    # one open leaf on the border: top, left, bottom, right
    for n, side in ((15, 0), (15, 1), (21, 2), (21, 3), (41, 0), (81, 2)):
        W = SIZES[n]
        g, s, t = grid_of(W, kruskal_links(W, 9000 + n + side), (0, 0), (W - 1, W - 1))
        k = 2 * (W // 2) + 1
        g[[(0, k), (k, 0), (n - 1, k), (k, n - 1)][side]] = 1
        out.append(dict(family="border", name=f"{n}-side{side}", n=n, grid=g, start=s, goal=t))
    # ... and the start on that leaf: the reference's neighbour count then indexes past the grid
    # (row / column -1 wraps to the far side, row / column N raises IndexError)
    for side in range(4):
        n, W = 15, 7
        g, s, t = grid_of(W, kruskal_links(W, 9100 + side), (0, 0), (W - 1, W - 2))
        s = [(0, 7), (7, 0), (n - 1, 7), (7, n - 1)][side]
        g[s] = 1
        out.append(dict(family="border", name=f"{n}-start-side{side}", n=n, grid=g, start=s, goal=t))
    # every open square a corner
    for n in (15, 21, 41, 81):
        g, s, t = staircase_grid(n)
        out.append(dict(family="staircase", name=f"{n}", n=n, grid=g, start=s, goal=t))
    return out


# ---- the classes the GPU tests sort the mazes into (computed from the maze alone) -----------
def degree(grid, r, c):
    n = grid.shape[0]
    return sum(1 for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1))
               if 0 <= r + dr < n and 0 <= c + dc < n and grid[r + dr, c + dc] != 0)


def goal_is_straight(grid, goal):
    r, c = goal
    if degree(grid, r, c) != 2:
        return False
    return bool((grid[r - 1, c] and grid[r + 1, c]) or (grid[r, c - 1] and grid[r, c + 1]))


def open_border(grid):
    return bool(grid[0].any() or grid[-1].any() or grid[:, 0].any() or grid[:, -1].any())


def on_odd_lattice(grid):
    """Odd size, every open square with an even coordinate a passage between two odd-odd cells
    (what the reference's generators make)."""
    n = grid.shape[0]
    if n % 2 == 0:
        return False
    o = grid != 0
    if o[0::2, 0::2].any():
        return False
    return True
