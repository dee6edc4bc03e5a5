#!/usr/bin/env python3
"""Fixtures for the convolutional autoencoder from the reference's own code: with random.seed(SEED)
the 8 dataset tensors of lib/maze_generation.py generate_collection_of_mazes((15, 15), 8, ...) with
the grids and start / goal points gen_maze drew for them, the state_dict key names, shapes and
values of a seeded lib/models/convolutional_autoencoder.py CAE(3, 32), and that module's output for
the 8 tensors.

The reference's loss needs pytorch_msssim, which is not installed where the fixtures are made, so
no loss value is recorded: the loss is pinned by its definition (tests/cae_model.py).

Test infrastructure only (build container). Writes tests/golden/cae.npz (data only).
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20270
ALGOS = ["r-prim", "prim&kill", "dfs"]


def main(ref):
    sys.path.insert(0, HERE)
    import _refstubs
    _refstubs.install()
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from lib import maze_generation as MG
    from lib.models.convolutional_autoencoder import CAE

    drawn = []
    gen_maze = MG.gen_maze

    def recording(shape, algorithm="dfs"):
        start, goal, maze = gen_maze(shape, algorithm)
        drawn.append((algorithm, start, goal, [row[:] for row in maze]))
        return start, goal, maze

    MG.gen_maze = recording
    random.seed(SEED)
    tensors = MG.generate_collection_of_mazes((15, 15), 8, ALGOS)
    MG.gen_maze = gen_maze
    x = torch.stack(tensors).numpy().astype(np.uint8)
    grids, sg, algo = [], [], []
    k = 0
    for t in tensors:  # the draw each kept tensor came from (duplicates are skipped in order)
        while True:
            a, s, g, m = drawn[k]
            k += 1
            mt = torch.tensor(m)
            nv = (mt != 0).int()
            nv[s[0]][s[1]] = 0
            if torch.equal(torch.stack([(mt == 0).int(), (mt == 1).int(), nv]), t):
                grids.append(np.array(m, dtype=np.uint8))
                sg.append([s[0], s[1], g[0], g[1]])
                algo.append(a)
                break
    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    net = CAE(3, 32)
    sd = net.state_dict()
    out = {f"sd.{k}": v.detach().numpy().copy() for k, v in sd.items()}
    out["names"] = np.array(list(sd.keys()))
    with torch.no_grad():
        y = net(torch.from_numpy(x).float())
    out.update(x=x, grids=np.stack(grids), start_goal=np.array(sg, dtype=np.int32),
               algo=np.array(algo), y=y.numpy().copy(), seed=np.int64(SEED))
    path = os.path.join(HERE, "cae.npz")
    np.savez_compressed(path, **out)
    print("tensors", x.shape, "draws", len(drawn), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_cae.py <path to the reference checkout>")
    main(sys.argv[1])
