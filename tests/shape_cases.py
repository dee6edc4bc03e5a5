"""The hand-built maze fixture (tests/golden/shapes.npz, made by tests/golden/make_golden_shapes.py
from tests/maze_shapes.py) and the classes its tests sort the mazes into. The classes come from
the maze and oracle/mcclendon.py alone, never from what a kernel reports."""
import functools
import math
import os
import sys

import golden_io as G
import maze_shapes as S

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")

# The order-exact kernel keeps a hallway's CPython set tables in wave registers, 128 slots at the
# most. CPython's set_merge sizes the copy of a 64-entry set to 256 slots, so a 128-slot table
# holds at most 63 entries; a hallway view (the hallway's nodes plus its adjacent split points) of
# <= 48 nodes stays under that bound with a margin.
VIEW_CAP = 48


@functools.lru_cache(maxsize=None)
def mazes():
    z = G.load("shapes.npz")
    out = []
    for i in range(len(z["n"])):
        n = int(z["n"][i])
        out.append(dict(index=i, family=S.FAMILIES[int(z["family"][i])], n=n,
                        grid=z["grid"][i, :n, :n].copy(),
                        start=tuple(int(x) for x in z["start"][i]),
                        goal=tuple(int(x) for x in z["goal"][i]),
                        difficulty=float(z["difficulty"][i]), complexity=float(z["complexity"][i])))
    return out


def oracle():
    if ORACLE not in sys.path:
        sys.path.insert(0, ORACLE)
    import mcclendon
    return mcclendon


@functools.lru_cache(maxsize=None)
def facts(index):
    """What decides a maze's class: goal_straight, all_junctions (every solution point a
    junction), open_border, view (the largest hallway view's node count), odd_lattice, and
    nodes / half_view (the graph's size; a hallway view holding at least half of it)."""
    M = oracle()
    m = mazes()[index]
    g = m["grid"]
    try:
        built, halls = M._build(g, m["start"], m["goal"])
        nodes, s_nodes = len(built[0].adj), built[6]
    except IndexError:  # a start on the bottom / right border: the reference raises as well
        nodes, s_nodes, halls = 0, [m["start"]], []
    view = max((len(mem) for _, mem in halls), default=0)
    return dict(goal_straight=S.goal_is_straight(g, m["goal"]),
                all_junctions=all(S.degree(g, r, c) == 3 for r, c in s_nodes),
                open_border=S.open_border(g), view=view, odd_lattice=S.on_odd_lattice(g),
                nodes=nodes, half_view=any(2 * len(mem) >= nodes for _, mem in halls),
                views=sorted(len(mem) for _, mem in halls))


def must_score(index):
    """The mazes the order-exact kernel has to score itself (status 0)."""
    f = facts(index)
    return (not f["goal_straight"] and not f["all_junctions"] and not f["open_border"]
            and f["view"] <= VIEW_CAP)


def finite(m):
    return not math.isnan(m["difficulty"])
