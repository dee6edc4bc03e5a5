#!/usr/bin/env python3
"""Fixtures for REINFORCE from the reference's own code: agents/rf_agent.py:10-129 driven the way
lib/trainers/value_based_trainer.py:39-89 drives it (select_action per step with the squeeze(0)
of both log-prob outputs, get_returns, optimize_model, scheduler_step) on a small PolicyNetwork
over consecutive synthetic episodes, the cosine schedule past T_max, and get_returns on a pool of
reward sequences.

Test infrastructure only (build container). Writes tests/golden/reinforce.npz (data only).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
EP_LENS = [2, 5, 17, 64]
POOL_LENS = [1, 2, 3, 63, 64, 65, 256, 257, 1000]
LR, GAMMA, SEED = 1e-3, 0.99, 20260


def pack_windows(w):
    """[n, 3, 15, 15] 0/1 -> int32 [n, 22]: element j of the flattened window is bit j % 32 of
    word j // 32 (the env's window_bits layout)."""
    n = w.shape[0]
    flat = np.zeros((n, 22 * 32), np.uint64)
    flat[:, :675] = w.reshape(n, 675).astype(np.uint64)
    words = (flat.reshape(n, 22, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return words.astype(np.uint32).view(np.int32)


def rewards(rng, n):
    r = (rng.random(n) - 0.5).tolist()
    r[-1] = 1.0  # a "win"
    return r


def main(ref):
    sys.path.insert(0, HERE)
    import _refstubs
    _refstubs.install()
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    from agents import rf_agent
    torch.set_num_threads(1)
    out = {}
    rng = np.random.default_rng(4242)

    torch.manual_seed(SEED)
    net = rf_agent.PolicyNetwork(3, 6, 4, 4, hidden_dim=8)
    agent = rf_agent.RFAgent.__new__(rf_agent.RFAgent)
    agent.lr, agent.gamma, agent.device = LR, GAMMA, torch.device("cpu")
    agent.policy_net = net
    net.train()
    agent.optimizer = torch.optim.AdamW(net.parameters(), LR)
    agent.lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(agent.optimizer, T_max=200,
                                                                    eta_min=1e-5)
    names = [k for k, _ in net.named_parameters()]
    out["names"] = np.array(names)
    for k, p in net.named_parameters():
        out[f"init.{k}"] = p.detach().numpy().copy()
    out["ep.lens"] = np.array(EP_LENS, np.int64)
    out["lr"], out["gamma"] = np.float64(LR), np.float64(GAMMA)
    for e, T in enumerate(EP_LENS):
        s6 = rng.random((T, 6)).astype(np.float32)
        win = rng.integers(0, 2, (T, 3, 15, 15)).astype(np.float32)
        rs = rewards(rng, T)
        acts, lps, logps = [], [], []
        for t in range(T):
            state = (torch.from_numpy(s6[t:t + 1]), torch.from_numpy(win[t:t + 1]))
            a, lp, logp = agent.select_action(state)
            acts.append(a)
            lps.append(lp.squeeze(0))
            logps.append(logp.squeeze(0))
        ret = agent.get_returns(rs)
        agent.optimize_model(lps, logps, ret)
        agent.scheduler_step()
        out[f"ep{e}.obs6"] = s6
        out[f"ep{e}.bits"] = pack_windows(win)
        out[f"ep{e}.actions"] = np.array(acts, np.int64)
        out[f"ep{e}.rewards"] = np.array(rs, np.float64)
        out[f"ep{e}.returns"] = ret.numpy().copy()
        out[f"ep{e}.lr_after"] = np.float64(agent.optimizer.param_groups[0]["lr"])
        for k, p in net.named_parameters():
            out[f"ep{e}.grad.{k}"] = p.grad.detach().numpy().copy()
            out[f"ep{e}.param.{k}"] = p.detach().numpy().copy()
    lrs = []
    for _ in range(450):
        agent.scheduler_step()
        lrs.append(agent.optimizer.param_groups[0]["lr"])
    out["sched.first_step"] = np.int64(len(EP_LENS) + 1)  # scheduler steps taken at lrs[0]
    out["sched.lr"] = np.array(lrs, np.float64)

    rew, rets = [], []
    for n in POOL_LENS:
        rs = rewards(rng, n)
        rew.append(np.array(rs, np.float64))
        if n > 1:  # (a 1-step episode's returns are NaN: lengths and rewards only)
            rets.append(agent.get_returns(rs).numpy().astype(np.float32))
    out["pool.lens"] = np.array(POOL_LENS, np.int64)
    out["pool.rewards"] = np.concatenate(rew)
    out["pool.returns"] = np.concatenate(rets)
    path = os.path.join(HERE, "reinforce.npz")
    np.savez_compressed(path, **out)
    print("episodes", EP_LENS, "lr", out["sched.lr"][:2], "bytes", os.path.getsize(path))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_reinforce.py <path to the reference checkout>")
    main(sys.argv[1])
