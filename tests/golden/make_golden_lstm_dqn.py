#!/usr/bin/env python3
"""Fixtures for the recurrent DQN from the reference's own network: agents/lstm_dqn_agent.py's
DQN(6, 4, 32) seeded, its state_dict, three input batches [batch, seq, 6] (batch / seq = 1 / 1,
3 / 7, 5 / 20) and the q values its forward returns from zero state.

The forward is recorded in a process with MKL_CBWR=COMPATIBLE, ATEN_CPU_CAPABILITY=default and one
thread (PINNED, the settings tests/test_lstm_dqn.py runs the drop-in under): MKL chooses its sgemm
by the CPU, and the last bit of a q value with it.

Test infrastructure only (build container). Writes tests/golden/lstm_dqn.npz (data only).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (3, 7), (5, 20)]
SEED = 20261
PINNED = {"MKL_CBWR": "COMPATIBLE", "ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1",
          "MKL_NUM_THREADS": "1"}


def main(ref):
    sys.path.insert(0, HERE)
    import _refstubs
    _refstubs.install()
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from agents import lstm_dqn_agent
    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    net = lstm_dqn_agent.DQN(6, 4, 32, torch.device("cpu"))
    out = {f"sd.{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()}
    out["names"] = np.array(list(net.state_dict().keys()))
    rng = np.random.default_rng(4243)
    for j, (b, s) in enumerate(SHAPES):
        x = rng.random((b, s, 6)).astype(np.float32)
        net.reset_hidden_state(b)
        with torch.no_grad():
            q = net(torch.from_numpy(x))
        out[f"x{j}"] = x
        out[f"q{j}"] = q.numpy().copy()
    path = os.path.join(HERE, "lstm_dqn.npz")
    np.savez_compressed(path, **out)
    print("shapes", SHAPES, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_lstm_dqn.py <path to the reference checkout>")
    if any(os.environ.get(k) != v for k, v in PINNED.items()):  # set before torch loads: a child
        import subprocess
        sys.exit(subprocess.run([sys.executable] + sys.argv, env=dict(os.environ, **PINNED)).returncode)
    main(sys.argv[1])
