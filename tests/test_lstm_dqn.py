"""The recurrent DQN off the GPU: the drop-in DQN against the reference network's recorded
state_dict and q values (tests/golden/lstm_dqn.npz), the float64 model (tests/drqn_model.py)
against both and against torch's float64 autograd, the eps schedule, and the single-env DQNAgent's
episode memory."""
import math
import random

import numpy as np
import pytest
import torch

import drqn_model as M
import golden_io as G

SHAPES = [(1, 1), (3, 7), (5, 20)]


@pytest.fixture(scope="module")
def fx():
    return G.load("lstm_dqn.npz")


def _sd(fx, dtype=torch.float32):
    return {k: torch.from_numpy(fx[f"sd.{k}"]).to(dtype) for k in M.KEYS}


def _net(fx, dtype=torch.float32):
    from mazerl.agents.lstm_dqn_agent import DQN
    net = DQN(6, 4, 32, torch.device("cpu")).to(dtype)
    net.load_state_dict(_sd(fx, dtype))
    return net


PINNED = {"MKL_CBWR": "COMPATIBLE", "ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1",
          "MKL_NUM_THREADS": "1"}
CHILD = """
import sys
import numpy as np, torch
import golden_io as G
from mazerl.agents.lstm_dqn_agent import DQN
torch.set_num_threads(1)
fx = G.load("lstm_dqn.npz")
net = DQN(6, 4, 32, torch.device("cpu"))
net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd.")})
out = {}
for j in range(3):
    x = torch.from_numpy(fx[f"x{j}"])
    net.reset_hidden_state(x.shape[0])
    with torch.no_grad():
        out[f"q{j}"] = net(x).numpy()
np.savez(sys.argv[1], **out)
"""


def test_dropin_loads_the_reference_state_dict_and_returns_its_bits(fx, tmp_path):
    """The same torch ops give the same bits only on the same CPU code path: MKL picks its sgemm
    by the CPU it runs on, and on another CPU one of the four q values of the 1 / 1 batch came out
    one ulp away. So the fixture is recorded, and the drop-in run here, in a process of its own
    with MKL's run-to-run-and-CPU-to-CPU reproducible mode (MKL_CBWR=COMPATIBLE) and ATen's
    baseline kernels (ATEN_CPU_CAPABILITY=default), single-threaded; both have to be set before
    torch loads, hence the child process. The comparison is bit for bit."""
    import os
    import subprocess
    import sys
    out = str(tmp_path / "q.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path), **PINNED)
    r = subprocess.run([sys.executable, "-c", CHILD, out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.load(out)
    for j, (b, s) in enumerate(SHAPES):
        assert got[f"q{j}"].shape == (b, 4)
        assert np.array_equal(got[f"q{j}"], fx[f"q{j}"]), (j, got[f"q{j}"], fx[f"q{j}"])


def test_dropin_keys_state_and_unroll(fx):
    assert [str(k) for k in fx["names"]] == list(M.KEYS)
    net = _net(fx)
    assert list(net.state_dict().keys()) == list(M.KEYS)
    for j, (b, s) in enumerate(SHAPES):
        x = torch.from_numpy(fx[f"x{j}"])
        assert tuple(x.shape) == (b, s, 6)
        net.reset_hidden_state(b)
        with torch.no_grad():
            q = net(x)
        assert tuple(net.hidden_state.shape) == (b, 32) and tuple(net.cell_state.shape) == (b, 32)
        with torch.no_grad():  # unroll(): every step's q (the same ops), the carried state untouched
            h0 = net.hidden_state.clone()
            qs = net.unroll(x)
        assert torch.equal(qs[:, -1], q) and torch.equal(h0, net.hidden_state)


def test_model_agrees_with_the_recorded_q_values(fx):
    """float64 model vs the reference's float32 forward. A gate pre-activation is 40 roundings on
    sum |terms| <= 1 + 38 / sqrt(32) < 8 (|w| <= 1 / sqrt(32), |x|, |h| <= 1), i.e. < 40 * 8 u;
    the nonlinearities' slopes are <= 1, c grows by at most that per step and h' by as much again,
    over up to 20 steps: 20 * 2 * 320 u, and the head adds 33 roundings on sum |terms| < 7."""
    P = M.as_f64({k: fx[f"sd.{k}"] for k in M.KEYS})
    u = 2.0 ** -24
    for j, (b, s) in enumerate(SHAPES):
        q = M.forward(P, fx[f"x{j}"].astype(np.float64))
        bound = (s * 2 * 320 + 33 * 7) * u
        assert np.abs(q - fx[f"q{j}"]).max() <= bound, (j, np.abs(q - fx[f"q{j}"]).max(), bound)


def _episodes(rng, lens, terms):
    return [dict(x=rng.random((n + 1, 6)), a=rng.integers(0, 4, n), r=rng.random(n) - 0.5,
                 term=bool(t)) for n, t in zip(lens, terms)]


def test_model_gradient_agrees_with_torch_float64_autograd(fx):
    from mazerl.agents.lstm_dqn_agent import td_loss
    rng = np.random.default_rng(7)
    src = _net(fx, torch.float64)
    tgt = _net(fx, torch.float64)
    with torch.no_grad():
        for p in tgt.parameters():
            p.add_(torch.from_numpy(rng.normal(0, 0.05, tuple(p.shape))))
    eps = _episodes(rng, [1, 2, 7, 20], [1, 0, 1, 0])
    P = M.as_f64({k: v.detach().numpy() for k, v in src.state_dict().items()})
    Pt = M.as_f64({k: v.detach().numpy() for k, v in tgt.state_dict().items()})
    out = M.td_loss(P, Pt, eps, 0.99)
    loss = td_loss(src, tgt, [(torch.from_numpy(e["x"]), torch.from_numpy(e["a"]),
                               torch.from_numpy(e["r"]), e["term"]) for e in eps], 0.99)
    loss.backward()
    assert abs(out["loss"] - loss.item()) <= 1e-10 * abs(loss.item())
    for k, p in src.named_parameters():
        g = p.grad.numpy()
        assert np.abs(out["grads"][k] - g).max() <= 1e-10 * np.abs(g).max(), k


def test_batch_gradient_is_the_weighted_sum_of_episode_gradients(fx):
    rng = np.random.default_rng(8)
    P = M.as_f64({k: fx[f"sd.{k}"] for k in M.KEYS})
    eps = _episodes(rng, [3, 5, 2], [1, 0, 0])
    whole = M.td_loss(P, P, eps, 0.9)
    parts = [M.td_loss(P, P, [e], 0.9, weight=1.0 / 10) for e in eps]
    for k in M.KEYS:
        s = sum(p["grads"][k] for p in parts)
        assert np.abs(s - whole["grads"][k]).max() <= 1e-14 * max(1.0, np.abs(s).max())


class _Env:
    class action_space:
        n = 4

    def reset(self):
        return {"agent": np.zeros(2, np.float32), "target": np.ones(2, np.float32),
                "best dir": np.zeros(2, np.float32)}, {}


def _agent(**kw):
    from mazerl.agents.lstm_dqn_agent import DQNAgent
    args = dict(learning_rate=1e-3, starting_epsilon=0.9, final_epsilon=0.05, epsilon_decay=50.0,
                discount_factor=0.99, batch_size=3, memory_size=5, target_update_frequency=4,
                device=torch.device("cpu"))
    args.update(kw)
    return DQNAgent(_Env(), **args)


def test_epsilon_schedule_and_update_steps_done():
    from mazerl.agents.lstm_dqn_agent import epsilon_at
    random.seed(3)
    torch.manual_seed(3)
    ag = _agent()
    assert ag.epsilon() == 0.9
    for k in range(11):
        assert ag.epsilon() == 0.05 + 0.85 * math.exp(-1.0 * k / 50.0) == epsilon_at(k, 0.9, 0.05, 50.0)
        a = ag.get_action(torch.rand(6))
        assert tuple(a.shape) == (1, 1) and a.dtype == torch.long and 0 <= int(a) < 4
    assert ag.steps_done == 11
    ag.update_steps_done()
    assert ag.steps_done == 5
    # explore_actions=2 reproduces the reference's randrange(2)
    ag2 = _agent(starting_epsilon=1.0, final_epsilon=1.0, explore_actions=2)
    assert {int(ag2.get_action(torch.rand(6))) for _ in range(64)} == {0, 1}


def test_agent_stores_whole_episodes_and_waits_for_a_batch():
    random.seed(4)
    torch.manual_seed(4)
    ag = _agent()
    rng = np.random.default_rng(4)
    before = [p.detach().clone() for p in ag.source_net.parameters()]
    for ep, n in enumerate([2, 4, 3]):
        xs = rng.random((n + 1, 6)).astype(np.float32)
        for t in range(n):
            a = ag.get_action(torch.from_numpy(xs[t]))
            if t == 0:  # the state restarted from zero: h is one step from zero
                h, c = ag.source_net.lstm_cell(torch.from_numpy(xs[0:1]))
                assert torch.equal(ag.source_net.hidden_state, h.detach())
            last = t == n - 1
            nxt = None if (last and ep != 1) else torch.from_numpy(xs[t + 1])
            ag.memorize(last, torch.from_numpy(xs[t]), int(a), 0.25 * t, nxt)
            assert len(ag.memory) == ep + (1 if last else 0)
            if len(ag.memory) < 3:
                assert ag.optimize_model() is None
        x, a_, r, term = ag.memory[-1]
        assert tuple(x.shape) == (n + 1, 6) and tuple(a_.shape) == (n,) and r.dtype == torch.float32
        assert np.array_equal(x[:n].numpy(), xs[:n]) and term == (ep != 1)
        if ep == 1:
            assert np.array_equal(x[n].numpy(), xs[n])  # truncated: x_n kept for the bootstrap
    assert all(torch.equal(b, p) for b, p in zip(before, ag.source_net.parameters()))
    loss = ag.optimize_model()
    assert loss is not None and math.isfinite(loss)
    assert any(not torch.equal(b, p) for b, p in zip(before, ag.source_net.parameters()))
    ag.update_target()
    for k, v in ag.source_net.state_dict().items():
        assert torch.equal(v, ag.target_net.state_dict()[k])
    assert ag.has_to_update(8) and not ag.has_to_update(9)
    ag.scheduler_step()
    assert ag.optimizer.param_groups[0]["lr"] == pytest.approx(
        1e-6 + (1e-3 - 1e-6) * (1 + math.cos(math.pi / 30)) / 2, rel=1e-12)
