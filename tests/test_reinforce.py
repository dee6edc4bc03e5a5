"""REINFORCE on the CPU (mazerl/agents/rf_agent.py) against the reference's own run recorded in
tests/golden/reinforce.npz (make_golden_reinforce.py: agents/rf_agent.py driven as
lib/trainers/value_based_trainer.py drives it, four consecutive episodes of 2, 5, 17 and 64 steps
on PolicyNetwork(3, 6, 4, 4, hidden_dim=8)), and the three C entry points' argument checks.
No GPU is needed."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden_io as G
from mazerl.agents.rf_agent import (PolicyNetwork, _expand_bits, cosine_lr, get_returns,
                                    reinforce_loss)


@pytest.fixture(scope="module")
def fx():
    return G.load("reinforce.npz")


def fixture_net(fx, device="cpu"):
    net = PolicyNetwork(3, 6, 4, 4, hidden_dim=8)
    sd = {str(k): torch.from_numpy(fx[f"init.{k}"]) for k in fx["names"]}
    net.load_state_dict(sd)  # strict: the reference's names, every one of them
    return net.to(device)


def test_policy_network_takes_the_reference_state_dict(fx):
    net = fixture_net(fx)
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in fx["names"]]
    for k, p in net.named_parameters():
        assert np.array_equal(p.detach().numpy(), fx[f"init.{k}"]), k
    assert sum(p.numel() for p in PolicyNetwork(3, 6, 4, 32).parameters()) == 2_140_548


def test_packed_windows_expand_to_the_f32_window():
    w = torch.randint(0, 2, (5, 3, 15, 15), generator=torch.Generator().manual_seed(1))
    flat = torch.zeros(5, 22 * 32, dtype=torch.int64)
    flat[:, :675] = w.reshape(5, 675)
    words = (flat.view(5, 22, 32) << torch.arange(32)).sum(2)
    bits = torch.where(words >= 2**31, words - 2**32, words).to(torch.int32)
    assert torch.equal(_expand_bits(bits, 3), w.float())
    net = PolicyNetwork(3, 6, 4, 4, hidden_dim=8)
    s6 = torch.rand(5, 6)
    assert torch.equal(net((s6, bits)), net((s6, w.float())))


def test_four_episodes_reproduce_the_reference(fx):
    """reinforce_loss + clip_grad_norm_(1.0) + torch AdamW + cosine_lr on the recorded states and
    actions: the returns, the clipped gradients, the parameters after each step and the lr."""
    net = fixture_net(fx)
    lr0, gamma = float(fx["lr"]), float(fx["gamma"])
    opt = torch.optim.AdamW(net.parameters(), lr0)
    for e, T in enumerate(int(n) for n in fx["ep.lens"]):
        ret = get_returns(fx[f"ep{e}.rewards"].tolist(), gamma)
        torch.testing.assert_close(ret, torch.from_numpy(fx[f"ep{e}.returns"]), rtol=1e-5, atol=2e-6)
        s6 = torch.from_numpy(fx[f"ep{e}.obs6"])
        bits = torch.from_numpy(fx[f"ep{e}.bits"])
        act = torch.from_numpy(fx[f"ep{e}.actions"])
        assert s6.shape == (T, 6) and bits.shape == (T, 22) and bits.dtype == torch.int32
        for g in opt.param_groups:
            g["lr"] = cosine_lr(e, lr0)
        loss = reinforce_loss(net((s6, bits)), act, ret - ret.mean())
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        for k, p in net.named_parameters():
            ref = torch.from_numpy(fx[f"ep{e}.grad.{k}"])
            torch.testing.assert_close(p.grad, ref, rtol=1e-4, atol=1e-6 * float(ref.abs().max()),
                                       msg=lambda m, k=k, e=e: f"episode {e} grad {k}: {m}")
        opt.step()
        for k, p in net.named_parameters():
            torch.testing.assert_close(p.detach(), torch.from_numpy(fx[f"ep{e}.param.{k}"]),
                                       rtol=1e-5, atol=1e-5,
                                       msg=lambda m, k=k, e=e: f"episode {e} param {k}: {m}")
        assert abs(cosine_lr(e + 1, lr0) - float(fx[f"ep{e}.lr_after"])) <= 1e-12


def test_cosine_lr_follows_the_scheduler_past_t_max(fx):
    k0, lrs = int(fx["sched.first_step"]), fx["sched.lr"]
    assert len(lrs) == 450 and k0 + 449 > 2 * 200
    for j, ref in enumerate(lrs):
        assert abs(cosine_lr(k0 + j, float(fx["lr"])) - float(ref)) <= 1e-12, k0 + j
    assert cosine_lr(200, 1e-3) == pytest.approx(1e-5, abs=1e-15)
    assert cosine_lr(300, 1e-3) > cosine_lr(200, 1e-3)  # the reference runs on: the lr rises again


def test_get_returns_matches_the_pool(fx):
    lens = [int(n) for n in fx["pool.lens"]]
    assert lens == [1, 2, 3, 63, 64, 65, 256, 257, 1000]
    ro, po = 0, 0
    for n in lens:
        r = fx["pool.rewards"][ro:ro + n].tolist()
        ro += n
        out = get_returns(r, float(fx["gamma"]))
        if n == 1:
            assert out.shape == (1,) and math.isnan(float(out[0]))
            continue
        torch.testing.assert_close(out, torch.from_numpy(fx["pool.returns"][po:po + n]),
                                   rtol=1e-5, atol=2e-6)
        po += n
    assert po == len(fx["pool.returns"])
    assert torch.equal(get_returns([0.0, 0.0, 0.0], 0.99), torch.zeros(3))  # constant: zeros, not NaN


# ---- the C entry points refuse bad arguments before any GPU call ------------------------------
P = 0x10000  # an aligned non-null address; never dereferenced: every call is refused or empty
ACT = ["logits", "ldl", "tau", "obs6", "bits", "B", "L", "seed", "counter", "t", "rec_s6", "rec_w",
       "rec_a", "act_out", "stream"]
FIN = ["rec_r", "rec_s6", "rec_w", "rec_a", "B", "L", "fin_id", "fin_off", "fin_len", "fin_count",
       "gamma", "cap", "p_s6", "p_w", "p_a", "p_adv", "p_len", "episodes", "stream"]
HEAD = ["logits", "ldl", "action", "adv", "len", "episodes", "b", "tau", "coef", "loss", "dlogits",
        "ldg", "stream"]
SCALARS = dict(ldl=4, ldg=4, tau=2.0, B=0, L=8, b=0, seed=1, counter=0, gamma=0.99, cap=16,
               coef=0.01, stream=None)


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def _call(lib, fn, names, **over):
    a = {k: SCALARS.get(k, P) for k in names}
    a.update(over)
    return getattr(lib, fn)(*[a[k] for k in names])


def _refused(lib, rc):
    assert rc != 0
    assert lib.mz_last_error()  # a text for the caller
    return lib.mz_last_error().decode()


@pytest.mark.parametrize("fn,names,count", [("mz_rf_act", ACT, "B"), ("mz_rf_finish", FIN, "B"),
                                            ("mz_rf_head_loss", HEAD, "b")])
def test_entry_points_refuse_bad_arguments(lib, fn, names, count):
    assert _call(lib, fn, names) == 0  # the well-formed empty call: each refusal has one cause
    for k in names:
        if k not in SCALARS:
            assert "null" in _refused(lib, _call(lib, fn, names, **{k: None})), k
    _refused(lib, _call(lib, fn, names, **{count: -1}))
    if "L" in names:
        _refused(lib, _call(lib, fn, names, L=-1))
    if "tau" in names:
        for tau in (0.0, -2.0, float("nan")):
            assert "temperature" in _refused(lib, _call(lib, fn, names, tau=tau))
    for k in ("ldl", "ldg"):
        if k in names:
            assert "stride" in _refused(lib, _call(lib, fn, names, **{k: 3}))
    if "cap" in names:
        _refused(lib, _call(lib, fn, names, cap=-1))
    assert _call(lib, fn, names) == 0


def test_trainer_refuses_cpu_device_and_plain_envs():
    from mazerl.trainers.reinforce_trainer import VectorReinforceTrainer
    full = SimpleNamespace(window_bits=object(), reward64=object())
    with pytest.raises(RuntimeError, match="GPU"):
        VectorReinforceTrainer(full, "cpu")
    for env in (SimpleNamespace(window_bits=None, reward64=object()),
                SimpleNamespace(window_bits=object(), reward64=None)):
        with pytest.raises(ValueError, match="window_bits=True, reward64=True"):
            VectorReinforceTrainer(env, "cuda")


class _OneObsEnv:
    """What RFAgent's constructor reads of an env: the action count and one observation."""
    action_space = SimpleNamespace(n=4)

    def reset(self):
        return {"agent": np.zeros(2, np.float32), "target": np.zeros(2, np.float32),
                "best dir": np.zeros(2, np.float32), "window": torch.zeros(3, 15, 15)}, {}


def test_drop_in_agent_steps_as_reinforce_loss(fx):
    """RFAgent driven as ValueBasedTrainer.train drives the reference's (select_action per step,
    squeeze(0) of both outputs, get_returns, optimize_model, scheduler_step) == the same episode
    through reinforce_loss + clip + AdamW, which the fixture pins to the reference."""
    import copy
    from mazerl.agents.rf_agent import RFAgent
    torch.manual_seed(5)
    agent = RFAgent(_OneObsEnv(), 1e-3, 0.99, torch.device("cpu"))
    assert sum(p.numel() for p in agent.policy_net.parameters()) == 2_140_548
    assert agent.get_probs((torch.zeros(1, 6), torch.zeros(1, 3, 15, 15))).shape == (1, 4)
    ref = copy.deepcopy(agent.policy_net)
    opt = torch.optim.AdamW(ref.parameters(), 1e-3)
    T = 17
    s6 = torch.from_numpy(fx["ep2.obs6"])
    win = _expand_bits(torch.from_numpy(fx["ep2.bits"]), 3)
    rewards = fx["ep2.rewards"].tolist()
    acts, lps, logps = [], [], []
    for t in range(T):
        a, lp, logp = agent.select_action((s6[t:t + 1], win[t:t + 1]))
        assert isinstance(a, int) and lp.shape == () and logp.shape == (1, 4)
        assert float(lp) == pytest.approx(float(logp[0, a]))
        acts.append(a)
        lps.append(lp.squeeze(0))
        logps.append(logp.squeeze(0))
    ret = agent.get_returns(rewards)
    agent.optimize_model(lps, logps, ret)
    agent.scheduler_step()
    assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(cosine_lr(1, 1e-3), abs=1e-12)
    loss = reinforce_loss(ref((s6, win)), torch.tensor(acts), ret - ret.mean())
    loss.backward()
    torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
    opt.step()
    for (k, p), q in zip(agent.policy_net.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-6 * float(q.grad.abs().max()),
                                   msg=lambda m, k=k: f"grad {k}: {m}")
        # AdamW's first step is lr g / (|g| + 1e-8): only where |g| is well above 1e-8 is it
        # insensitive to the two summation orders of the entropy mean
        firm = q.grad.abs() > 1e-6
        assert bool(firm.any()), k
        torch.testing.assert_close(p.detach()[firm], q.detach()[firm], rtol=1e-5, atol=1e-5,
                                   msg=lambda m, k=k: f"param {k}: {m}")


def test_drop_in_agent_is_exported():
    from mazerl import agents
    from mazerl.agents.rf_agent import RFAgent
    assert agents.RFAgent is RFAgent and agents.PolicyNetwork is PolicyNetwork
    for m in ("get_probs", "select_action", "get_returns", "optimize_model", "scheduler_step"):
        assert callable(getattr(RFAgent, m))
