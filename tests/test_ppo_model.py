"""tests/ppo_model.py anchored on the CPU, before tests/test_ppo_exact.py holds a kernel to it:
against the recorded reference outputs, against the package's own torch expressions in float64
(with autograd), and against a plain restatement of do_episode's bookkeeping. The caps on what
the GPU tests may leave out are checked here for the model alone, on the same cases."""
from collections import deque

import numpy as np
import pytest
import torch

import golden_io as G
import ppo_cases as K
import ppo_model as M


def _close(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=2e-6, equal_nan=True)


def test_finish_matches_recorded_reference_outputs():
    """calculate_returns / calculate_advantages of the reference on 12 recorded episodes
    (tests/golden/agents.npz "ppo.pool.*"), at the tolerance tests/test_ppo_gpu.py gives the
    kernel against the same fixture; the 1-step episodes are NaN there and left out."""
    fx = G.load("agents.npz")
    lens = [int(n) for n in fx["ppo.pool.lens"]]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    gamma = float(fx["ppo.pool.gamma"])
    seen = 0
    for k, n in enumerate(lens):
        sl = slice(off[k], off[k + 1])
        if n == 1:
            assert np.isnan(fx["ppo.pool.returns"][sl]).all()
            continue
        R, A, _ = M.finish(fx["ppo.pool.rewards"][sl], fx["ppo.pool.values"][sl], gamma)
        _close(R, fx["ppo.pool.returns"][sl])
        _close(A, fx["ppo.pool.advantages"][sl])
        seen += 1
    assert seen >= 8


@pytest.mark.parametrize("name,gamma", K.FINISH_LISTS)
def test_finish_matches_package_on_the_gpu_tests_episodes(name, gamma):
    """The model against mazerl.agents.ppo.calculate_returns / calculate_advantages (float32
    torch on the CPU) on every episode the GPU test lists, rtol 1e-5 / atol 2e-6.

    That tolerance is about float32 reductions, and it has a reach: rounding the mean of the
    returns to float32 moves every normalised return by up to u |mean| / std (u = 2^-24), so two
    correct evaluations can differ by a few times that. Past |mean| / std = 16 (3 u 16 = 2.9e-6 >
    atol) the package's float32 result is no yardstick: the 3-step episode with rewards (-0.05,
    -0.05, -1), |mean| / std = 26, has the model 1.0e-6 and torch 2.0e-6 from the float64
    evaluation of the same float32 returns, 3.0e-6 apart. Such episodes (the grid-stride list
    draws some 50 among its 2,100 of 2 to 4 steps; none in the other lists) are held to that float64 evaluation
    instead, at the same tolerance."""
    from mazerl.agents.ppo import calculate_advantages, calculate_returns
    c = K.finish_list(name, gamma)
    model = K.finish_model(name, gamma)
    unclear = stiff = 0
    for (i, n), (R, A, clear) in zip(zip(c["ids"], c["lens"]), model):
        rew, val = c["rec_r"][i, :n], c["rec_v"][i, :n]
        ret = calculate_returns([float(x) for x in rew], gamma)
        adv = calculate_advantages(ret, torch.from_numpy(val))
        assert ret.dtype == torch.float32
        acc, out = 0.0, []
        for x in rew[::-1]:
            acc = float(x) + acc * gamma
            out.insert(0, acc)
        o = np.array(out, np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            cond = abs(o.mean()) / o.std(ddof=1)
            if cond > 16:
                stiff += 1
                Rn = (o - o.mean()) / o.std(ddof=1)
                a = Rn - val
                _close(R, Rn)
                _close(A, (a - a.mean()) / (a.std(ddof=1) + 1e-8))
            else:
                _close(R, ret.numpy())
                _close(A, adv.numpy())
        unclear += not clear
    print(f"{name} gamma {gamma}: {len(model)} episodes, {unclear} not clear,"
          f" {stiff} with |mean| / std > 16")
    assert unclear <= 2  # the GPU test's cap; a condition on the seed
    assert name == "stride" or stiff == 0
    if name == "edge":
        assert np.isnan(model[0][0]).all() and np.isnan(model[0][1]).all()  # zero variance


def test_finish_flags_a_statistic_on_a_rounding_midpoint():
    f = np.float32(1.25)
    mid = (float(f) + float(np.nextafter(f, np.float32(2)))) / 2
    assert M._near_midpoint(mid, 1.0) and M._near_midpoint(mid * (1 + 2.0 ** -45), 1.0)
    assert not M._near_midpoint(float(f), 1.0) and not M._near_midpoint(mid * (1 + 2.0 ** -30), 1.0)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("mode", K.HEAD_MODES)
@pytest.mark.parametrize("b", K.HEAD_BS)
def test_head_matches_float64_autograd(b, mode):
    c = K.head_case(b, mode)
    m = c["model"]
    total, dlogits, dvalue = K.torch_head(c, torch.float64)
    ok = m["clear"]
    left = int((~ok).sum())
    r = (abs(m["total"] - total) / abs(total), _rel(m["dlogits"][ok], dlogits[ok]) if ok.any() else 0.0,
         _rel(m["dvalue"], dvalue))
    print(f"b {b} {mode}: rel err loss {r[0]:.2e} dlogits {r[1]:.2e} dvalue {r[2]:.2e};"
          f" columns not clear {left}")
    assert max(r) <= 1e-12
    assert left <= b // 100  # the GPU test's cap (1 % of the columns); a condition on the seed
    r_ =np.exp(m["lp_new"][None, :] - c["lp_old"][:, None].astype(np.float64))
    frac = float(((r_ >= 0.7) & (r_ <= 1.3)).mean())
    if b >= 37:
        # both activations of the clip (b = 37: three of its columns are the saturated rows')
        assert (0.8 < frac < 1.0) if mode == "inside" else (0.0 < frac < 0.4), frac


def _torch_pair(lp_new, lp_old, adv, clip):
    ln = torch.tensor(lp_new, dtype=torch.float64, requires_grad=True)
    lo = torch.tensor(lp_old, dtype=torch.float64).reshape(-1, 1)
    a = torch.tensor(adv, dtype=torch.float64)
    ratio = (ln - lo).exp()
    s = torch.min(ratio * a, torch.clamp(ratio, min=1 - clip, max=1 + clip) * a)
    s.sum().backward()
    return s.sum(0).detach().numpy(), ln.grad.numpy()  # part, adv * dsum


@pytest.mark.parametrize("b", [1, 2, 37, 257])
def test_pair_ties_and_inclusive_boundaries_match_autograd(b):
    """r = exp(0) = 1 for every pair. clip 0: 1 - clip == r == 1 + clip, a tie on an inclusive
    boundary, w = 1. clip 0.3 with zero advantages: s1 == s2 == 0 with r inside, w = 1."""
    rng = np.random.default_rng(b)
    lp = np.full(b, np.float32(-0.8125))
    adv = (rng.integers(-256, 257, b) / 64.0).astype(np.float32)
    for clip, a in ((0.0, adv), (0.3, np.zeros(b, np.float32)), (0.3, adv)):
        part, dsum, clear = M.pair(lp, lp, a, clip)
        tp, tg = _torch_pair(lp, lp, a, clip)
        assert clear.all()
        assert np.array_equal(part, tp) and np.array_equal(a.astype(np.float64) * dsum, tg)
        assert np.array_equal(part, b * a.astype(np.float64)) and np.array_equal(dsum, np.full(b, float(b)))
    # the same tie under a negative advantage
    part, dsum, _ = M.pair(np.zeros(1), np.zeros(1), np.array([-1.0]), 0.0)
    assert part[0] == -1.0 and dsum[0] == 1.0


def test_pair_flags_ratios_next_to_a_boundary():
    lp_old = np.zeros(3)
    lp_new = np.log(np.array([0.7 * (1 + 2.0 ** -20), 1.0, 1.3 * (1 - 2.0 ** -17)]))
    assert list(M.pair(lp_new, lp_old, np.ones(3), 0.3)[2]) == [False, True, True]


def test_act_matches_torch_float64_and_inverse_cdf():
    for B in K.ACT_BS:
        c = K.act_case(B)
        m = c["model"]
        z = torch.tensor(c["logits"], dtype=torch.float64)
        p = torch.softmax(z, dim=-1)
        assert _rel(m["p"], p.numpy()) <= 1e-14
        lp = torch.log_softmax(z, dim=-1).numpy()
        assert np.abs(m["logp"] - lp).max() <= 1e-13 * max(1.0, np.abs(lp).max())
        r = c["u24"] / 2.0 ** 24
        cdf = np.cumsum(m["p"], axis=1)
        a = m["action"]
        ar = np.arange(B)
        assert np.all(r < cdf[ar, a]) and np.all((a == 0) | (r >= cdf[ar, np.maximum(a - 1, 0)]))
        assert np.all(m["allowed"][ar, a]) and np.all(m["allowed"][m["clear"]].sum(1) == 1)
        left = int((~m["clear"]).sum())
        print(f"B {B}: rows not clear {left}; actions {np.bincount(a, minlength=4).tolist()}")
        assert left <= 2  # the GPU test's cap; a condition on the seed
        assert (c["u24"] >= 0).all() and (c["u24"] < 2 ** 24).all()
    big = K.act_case(4099)
    assert len(set(big["u24"].tolist())) > 4000  # a stream per instance, not one draw repeated


def test_act_flags_a_uniform_next_to_a_boundary():
    """Equal logits: boundaries at 1/4, 1/2, 3/4. r = 1/4 exactly belongs to action 1 (r < c is
    strict) and is not clear; the action across the boundary is allowed there and nowhere else."""
    z = np.zeros((4, 4), np.float32)
    m = M.act(z, [2 ** 22, 2 ** 22 - 20, 2 ** 22 + 2 ** 6, 3 * 2 ** 22 - 1])
    assert list(m["action"]) == [1, 0, 1, 2] and list(m["clear"]) == [False, True, True, False]
    assert m["allowed"].tolist() == [[True, True, False, False], [True, False, False, False],
                                     [False, True, False, False], [False, False, True, True]]


def test_scan_matches_do_episode_bookkeeping():
    """The per-instance bookkeeping of PPOAgent.do_episode / PPOTrainer.train restated with one
    deque per instance: append the reward; on done count the episode (a win if terminated), drop a
    1-step episode, else hand the episode to the pool in instance order; start over."""
    B, L, steps = 300, 50, 9
    rng = np.random.default_rng(42)
    eps = [deque() for _ in range(B)]
    t = np.zeros(B, np.int32)
    fill, total, stats = 17, 1000, [5, 4, 3, 0]
    pool_rows, episodes, wins, short = fill, stats[0], stats[1], stats[2]
    rec_r = np.full((B, L), np.nan)
    for _ in range(steps):
        term = (rng.random(B) < 0.2).astype(np.uint8)
        trunc = (rng.random(B) < 0.2).astype(np.uint8)
        rew = rng.choice(K.REWARDS, B)
        out = M.scan(t, term, trunc, rew, L, fill, total, stats)
        for i, ti, r in out["rec"]:
            rec_r[i, ti] = r
        listed = []
        for i in range(B):
            eps[i].append(rew[i])
            if term[i] or trunc[i]:
                episodes += 1
                wins += int(term[i])
                if len(eps[i]) >= 2:
                    listed.append((i, pool_rows, len(eps[i])))
                    assert list(rec_r[i, :len(eps[i])]) == list(eps[i])
                    pool_rows += len(eps[i])
                else:
                    short += 1
                eps[i].clear()
        assert list(zip(out["fin_id"], out["fin_off"], out["fin_len"])) == listed
        assert out["fin_count"] == len(listed)
        assert list(out["t"]) == [len(e) for e in eps]
        assert out["fill"] == pool_rows and out["total"] == total + pool_rows - fill
        assert out["stats"] == [episodes, wins, short, 0]
        t, fill, total, stats = out["t"], out["fill"], out["total"], out["stats"]
    assert short > 3 + 3 and episodes > short  # 1-step episodes occurred, and longer ones
    # an unfinished episode that reaches L: counted, t held at L - 1, nothing listed
    out = M.scan([L - 1, L - 1, 0], [0, 1, 1], [0, 1, 0], [0.5, 1.0, -1.0], L, 0, 0, [0, 0, 0, 0])
    assert list(out["t"]) == [L - 1, 0, 0] and out["stats"] == [2, 2, 1, 1]
    assert out["fin_id"] == [1] and out["fin_len"] == [L] and out["fin_off"] == [0]
    assert out["rec"] == [(0, L - 1, 0.5), (1, L - 1, 1.0), (2, 0, -1.0)]


@pytest.mark.parametrize("B", K.SCAN_BS)
def test_scan_cases_reach_every_branch(B):
    """The GPU test's scan patterns, through the model alone: over the two calls of the mixed
    pattern 1-step drops, full-length episodes and record overflows all occur (B >= 64)."""
    t = K.scan_t0(B, "mix")
    st = dict(K.SCAN_STATE0)
    full = 0
    for call in (0, 1):
        term, trunc, rew = K.scan_step(B, "mix", call)
        out = M.scan(t, term, trunc, rew, K.SCAN_L, st["fill"], st["total"], st["stats"])
        full += sum(n == K.SCAN_L for n in out["fin_len"])
        t, st = out["t"], dict(fill=out["fill"], total=out["total"], stats=out["stats"])
    if B >= 64:
        s0 = K.SCAN_STATE0["stats"]
        assert st["stats"][2] > s0[2] and st["stats"][3] > s0[3] and full > 0
        assert ((term != 0) & (trunc != 0)).any()
