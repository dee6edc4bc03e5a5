"""Prioritized replay windows off the GPU: the integer sampler of tests/drqn_prio_model.py (strata,
proportionality, uniformity over the memory's windows at alpha = 0, a dominating mass, more
positions than mass), the mass rule, the weighted loss against torch's float64 autograd of
window_td_loss(weights=w), and the refusals of the constructor, the command line and the three
entry points, none of which needs a device."""
import ctypes as C
from collections import deque

import numpy as np
import pytest
import torch

import drqn_model as M
import drqn_prio_model as PM
import drqn_window_model as W

ONE = PM.ONE
H, L = 32, 8
EINVAL = -1


def _memory(masses, T, lens):
    prio = np.array(masses, np.int64) * 1
    assert prio.shape[1] == W.windows_in(L, T)
    for row, n in zip(prio, lens):  # a mass wherever the episode has a window, none elsewhere
        nw = W.windows_in(n, T)
        assert (row[:nw] > 0).all() and (row[nw:] == 0).all()
    return prio, np.array(lens, np.int32)


def _chi2_p(counts, probs):
    from scipy.stats import chi2
    counts, probs = np.asarray(counts, np.float64), np.asarray(probs, np.float64)
    exp = counts.sum() * probs
    stat = float(((counts - exp) ** 2 / exp).sum())
    return stat, chi2.sf(stat, len(counts) - 1)


# ---- the sampler --------------------------------------------------------------------------------
def test_every_draw_lies_in_its_stratum_and_its_window_holds_it():
    prio, lens = _memory([[1 * ONE, 2 * ONE], [3 * ONE, 0], [4 * ONE, 5 * ONE]], 4, [8, 4, 7])
    flat = [int(v) for v in prio.ravel()]
    S = sum(flat)
    for E in (1, 3, 7, 65):
        for counter in range(20):
            s = PM.sample(prio, lens, 5, counter, E, 4, 4, 0.6)
            for e in range(E):
                lo, hi, t = s["lo"][e], s["hi"][e], s["t"][e]
                assert (lo, hi) == (e * S // E, (e + 1) * S // E)
                assert lo <= t < hi
                i = s["slot"][e] * 2 + (s["b"][e] + s["k"][e]) // 4
                assert sum(flat[:i]) <= t < sum(flat[:i]) + flat[i] and flat[i] == s["mass"][e]
                n = lens[s["slot"][e]]
                st = s["b"][e] + s["k"][e]
                assert s["n"][e] == n and s["b"][e] == max(0, st - 4)
                assert s["m"][e] == min(4, n - st) >= 1
            assert np.array_equal(s["off"], np.concatenate([[0], np.cumsum(np.array(s["m"]) + 2)[:-1]]))
            assert s["tot"] == (sum(s["m"]) + 2 * E, sum(s["m"]))


def test_draws_are_proportional_to_mass():
    """Masses (1, 2, 3, 0, 4, 5) 2^20 over three slots, E = 7, 7,150 update counts: 50,050 draws
    against mass / S, chi-square on 4 degrees of freedom at 1e-6."""
    prio, lens = _memory([[1 * ONE, 2 * ONE], [3 * ONE, 0], [4 * ONE, 5 * ONE]], 4, [8, 4, 8])
    counts = np.zeros(6, np.int64)
    for counter in range(7150):
        s = PM.sample(prio, lens, 9, counter, 7, 4, 0, 0.0)
        for slot, b, k in zip(s["slot"], s["b"], s["k"]):
            counts[slot * 2 + (b + k) // 4] += 1
    assert counts.sum() == 50050 and counts[3] == 0
    stat, p = _chi2_p(counts[[0, 1, 2, 4, 5]], np.array([1, 2, 3, 4, 5]) / 15)
    print(f"chi-square {stat:.2f} on 4 dof, p {p:.3f}, counts {counts.tolist()}")
    assert p > 1e-6, counts.tolist()


def test_alpha_zero_is_uniform_over_the_memorys_windows():
    """Every filled window at mass 2^20 (what alpha = 0 writes and what entry gives): episodes of
    1, 2, 5 and 8 steps at T = 1 have 1, 2, 5 and 8 windows, and each of the 16 windows is drawn
    equally often, so a step of the 1-step episode is trained on as often as one of the 8-step
    episode. Departure 8 draws each episode equally often: 8 times as often per step."""
    lens = [1, 2, 5, 8]
    prio = np.zeros((4, 8), np.int64)
    for row, n in zip(prio, lens):
        row[:n] = PM.mass_of(np.float32([0.3, 2.0]), 0.0, 0.9, 1e-3)
    assert prio.max() == ONE
    counts = np.zeros((4, 8), np.int64)
    for counter in range(3200):
        s = PM.sample(prio, np.array(lens), 3, counter, 5, 1, 0, 0.4)
        assert (s["isw"] == 1.0).all()  # equal masses: no correction
        for slot, b, k in zip(s["slot"], s["b"], s["k"]):
            counts[slot, b + k] += 1
    filled = prio > 0
    assert counts[~filled].sum() == 0
    stat, p = _chi2_p(counts[filled], np.full(16, 1 / 16))
    per_step = [counts[i, :n].sum() / n for i, n in enumerate(lens)]
    print(f"chi-square {stat:.2f} on 15 dof, p {p:.3f}; draws per step of each episode {per_step}")
    assert p > 1e-6
    assert max(per_step) / min(per_step) < 1.2


def test_a_dominating_mass_takes_nearly_every_draw():
    prio = np.array([[1, 1], [PM.CEIL, 1], [1, 0]], np.int64)
    lens = np.array([2, 2, 1])
    hits = total = 0
    for counter in range(200):
        s = PM.sample(prio, lens, 1, counter, 8, 1, 0, 0.6)
        hits += sum(1 for slot, b, k in zip(s["slot"], s["b"], s["k"]) if (slot, b + k) == (1, 0))
        total += 8
        # the rare small window gets the full weight, the dominating one a tiny weight
        for v, w in zip(s["mass"], s["isw"]):
            assert w == (1.0 if v == min(s["mass"]) else (min(s["mass"]) / v) ** 0.6)
    assert hits >= 0.999 * total, (hits, total)


def test_more_positions_than_mass_still_gives_valid_windows():
    prio = np.array([[1, 0, 0], [0, 0, 0], [1, 1, 0]], np.int64)  # S = 3 < E
    lens = np.array([2, 0, 4])
    for E in (4, 7, 65):
        s = PM.sample(prio, lens, 2, 11, E, 2, 2, 1.0)
        assert all(v == 1 for v in s["mass"]) and all(m >= 1 for m in s["m"])
        assert all(lo <= t and (t < hi or hi == lo) for lo, hi, t in zip(s["lo"], s["hi"], s["t"]))
        assert 1 not in s["slot"]


def test_the_draw_is_keyed_by_seed_counter_and_position():
    words = {(s, c, e): PM.draw(s, c, e) for s in (1, 2) for c in (0, 1) for e in (0, 1)}
    assert len(set(words.values())) == 8
    assert PM.draw(1, 1, 1) == words[(1, 1, 1)] and all(0 <= w < 2 ** 64 for w in words.values())


# ---- entry and the mass rule --------------------------------------------------------------------
def test_entry_follows_the_ring_like_a_deque():
    cap, T, B = 5, 3, 9
    Wn = W.windows_in(L, T)
    prio, psum = np.full((cap, Wn), -7, np.int64), np.full(cap, -7, np.int64)
    dq, total, pm = deque(maxlen=cap), 0, ONE
    plan = [[(0, 2), (3, 8)], [(1, 3), (2, 4), (5, 8), (7, 1)],
            [(i, 1 + (i * 3) % 8) for i in range(7)]]  # the last: more episodes than slots
    for step, fin in enumerate(plan):
        pm += step * 12345
        PM.store(prio, psum, pm, total % cap, fin, B, L, T)
        for _, n in fin:
            dq.append((n, pm))
        total += len(fin)
        for j, (n, v) in enumerate(dq):
            slot = (total - len(dq) + j) % cap
            nw = W.windows_in(n, T)
            assert (prio[slot, :nw] == v).all() and (prio[slot, nw:] == 0).all()
            assert psum[slot] == nw * v
    assert (prio >= 0).all()  # seven episodes into five slots: every slot written


def test_the_mass_rule():
    a = np.float32([0.5, 0.25, 1.0])
    pr = 0.9 * 1.0 + (1.0 - 0.9) * ((0.5 + 0.25 + 1.0) / 3)
    assert PM.mass_of(a, 0.9, 0.9, 1e-3) == round((pr + 1e-3) ** 0.9 * ONE)
    assert PM.mass_of(a, 0.0, 0.9, 1e-3) == ONE           # alpha = 0: exactly priority 1
    assert PM.mass_of(np.float32([0.0]), 2.0, 0.9, 1e-3) == 1          # (1e-6 2^20 rounds to 1)
    assert PM.mass_of(np.float32([0.0]), 6.0, 0.9, 1e-3) == 1          # clamped from below
    assert PM.mass_of(np.float32([1e6]), 0.9, 0.9, 1e-3) == PM.CEIL    # clamped from above
    assert PM.mass_of(np.float32([np.inf]), 0.9, 0.9, 1e-3) == PM.CEIL
    assert PM.mass_of(np.float32([np.nan, 1.0]), 0.9, 0.9, 1e-3) == PM.CEIL
    prio, psum = np.array([[5, 6, 0], [7, 0, 0]], np.int64), np.array([11, 7], np.int64)
    masses, pm = PM.update(prio, psum, 9, [0, 0, 1], [1, 1, 0], [a, a, np.float32([0.0])], 0.9, 0.9,
                           1e-3)
    assert masses[0] == masses[1] and prio[0, 1] == masses[0] and prio[1, 0] == masses[2]
    assert psum.tolist() == [5 + masses[0], masses[2]] and pm == max(9, *masses)


# ---- the weighted loss --------------------------------------------------------------------------
def _net(seed, dtype=torch.float64):
    from mazerl.agents.lstm_dqn_agent import DQN
    torch.manual_seed(seed)
    return DQN(6, 4, 32, torch.device("cpu")).to(dtype)


def _f64(net):
    return M.as_f64({k: v.detach().numpy() for k, v in net.state_dict().items()})


def _batch(rng, T, K):
    ws = []
    for n, term in zip([1, T, T + 1, 3 * T + 2, T, T + 1], [1, 1, 1, 0, 0, 0]):
        ep = dict(x=rng.random((n + 1, 6)), a=rng.integers(0, 4, n), r=rng.random(n) - 0.5,
                  term=bool(term))
        sn = rng.random((W.windows_in(n, T), 64)) - 0.5
        ws += [W.window_of(ep, T, K, j, sn) for j in range(W.windows_in(n, T))]
    return ws


@pytest.mark.parametrize("T,K", [(1, 0), (3, 3), (8, 0)])
def test_weighted_model_gradient_agrees_with_torch_float64_autograd(T, K):
    from mazerl.agents.lstm_dqn_agent import window_td_loss
    rng = np.random.default_rng(21 + T)
    src, tgt = _net(1), _net(2)
    P, Pt = _f64(src), _f64(tgt)
    ws = _batch(rng, T, K)
    ws = ws + ws[:2]  # sampling is with replacement: a window may come twice
    wts = rng.random(len(ws)) ** 2 + 1e-3
    wts[0] = 1.0
    out = PM.weighted_td_loss(P, Pt, ws, 0.99, wts)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)  # noqa: E731
    tws = [(t(w["x"]), torch.from_numpy(np.asarray(w["a"])), t(w["r"]), t(w["h0"]), t(w["c0"]),
            w["k"], w["term"]) for w in ws]
    loss = window_td_loss(src, tgt, tws, 0.99, weights=torch.from_numpy(wts))
    loss.backward()
    assert abs(out["loss"] - loss.item()) <= 1e-10 * abs(loss.item())
    for k, p in src.named_parameters():
        g = p.grad.numpy()
        assert np.abs(out["grads"][k] - g).max() <= 1e-10 * np.abs(g).max(), (T, K, k)
    # every weight 1: the unweighted model, operation for operation
    one = PM.weighted_td_loss(P, Pt, ws, 0.99, np.ones(len(ws)))
    plain = W.window_td_loss(P, Pt, ws, 0.99)
    assert one["loss"] == plain["loss"]
    for k in M.KEYS:
        assert np.array_equal(one["grads"][k], plain["grads"][k]), k
    # and torch's weights=None is its weights = 1
    for p in src.parameters():
        p.grad = None
    a = window_td_loss(src, tgt, tws, 0.99)
    b = window_td_loss(src, tgt, tws, 0.99, weights=torch.ones(len(ws), dtype=torch.float64))
    assert a.item() == b.item()


# ---- refusals, none of which needs a device -----------------------------------------------------
class _Env:
    num_envs, max_dim, toroidal = 12, 9, False


def test_constructor_refuses_priority_arguments_that_break_the_rules():
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer as Tr
    for kw in (dict(priority_alpha=0.9),                                  # no window
               dict(window=4, priority_alpha=-0.1), dict(window=4, priority_alpha=float("nan")),
               dict(window=4, priority_alpha=float("inf")), dict(window=4, priority_alpha="0.9"),
               dict(window=4, priority_alpha=0.9, priority_beta=-1.0),
               dict(window=4, priority_alpha=0.9, priority_beta=(0.4, 1.0)),
               dict(window=4, priority_alpha=0.9, priority_beta=(0.4, 1.0, 0)),
               dict(window=4, priority_alpha=0.9, priority_beta=(0.4, -1.0, 10)),
               dict(window=4, priority_alpha=0.9, priority_beta=(0.4, 1.0, 2.5)),
               dict(window=4, priority_alpha=0.9, priority_eta=1.5),
               dict(window=4, priority_alpha=0.9, priority_eta=-0.1),
               dict(window=4, priority_alpha=0.9, priority_eps=0.0),
               dict(window=4, priority_alpha=0.9, priority_eps=float("inf"))):
        with pytest.raises(ValueError, match="priority_alpha"):
            Tr(_Env(), "cuda", **kw)


def test_command_line_takes_the_priority_flags():
    from mazerl.train_lstm_dqn import parse_args
    a = parse_args(["--envs", "64", "--window", "4", "--burn-in", "4", "--priority-alpha", "0.9"])
    assert (a.priority_alpha, a.priority_beta, a.priority_eta, a.priority_eps) == (0.9, 0.6, 0.9, 1e-3)
    a = parse_args(["--envs", "64", "--window", "4", "--priority-alpha", "0", "--priority-beta",
                    "0.4,1,5000", "--priority-eta", "0.5", "--priority-eps", "0.01"])
    assert (a.priority_alpha, a.priority_beta, a.priority_eta, a.priority_eps) == \
        (0.0, (0.4, 1.0, 5000), 0.5, 0.01)
    assert parse_args(["--envs", "64", "--window", "4"]).priority_alpha is None
    for argv in (["--priority-alpha", "0.9"],                              # no --window
                 ["--window", "4", "--priority-alpha", "-1"],
                 ["--window", "4", "--priority-alpha", "0.9", "--priority-beta", "0.4,1"],
                 ["--window", "4", "--priority-alpha", "0.9", "--priority-eta", "2"],
                 ["--window", "4", "--priority-alpha", "0.9", "--priority-eps", "0"],
                 ["--window", "4", "--priority-beta", "0.5"],              # no --priority-alpha
                 ["--window", "4", "--learners", "2", "--priority-alpha", "0.9"]):
        with pytest.raises(SystemExit):
            parse_args(["--envs", "64"] + argv)


def test_entry_points_refuse_bad_arguments():
    from mazerl import _native as N
    lib = N.load()
    buf = (C.c_uint64 * 64)()  # any non-null address: a refusal comes before any use of it
    p = C.addressof(buf)
    store = lambda hid=H, B=4, Lr=L, T=3, cap=5, fin=p, prio=p, psum=p, pmax=p, ring=p: \
        lib.mz_drqn_prio_store(hid, B, Lr, T, fin, p, p, cap, prio, psum, pmax, ring, None)  # noqa: E731
    sample = lambda hid=H, E=4, Lr=L, T=3, K=3, cap=5, lens=p, prio=p, psum=p, wdir=p, isw=p, \
        beta=0.6: lib.mz_drqn_prio_sample(1, 2, hid, E, Lr, T, K, cap, lens, prio, psum, wdir, p, p,  # noqa: E731
                                          isw, beta, None)
    update = lambda hid=H, E=4, Lr=L, T=3, cap=5, wdir=p, qa=p, d=p, isw=p, alpha=0.9, eta=0.9, \
        eps=1e-3, prio=p, pmax=p: lib.mz_drqn_prio_update(  # noqa: E731
            hid, E, Lr, T, cap, wdir, p, p, qa, p, d, p, isw, alpha, eta, eps, prio, p, pmax, None)
    nan, inf = float("nan"), float("inf")
    bad = [
        lambda: store(hid=16), lambda: store(B=0), lambda: store(Lr=0), lambda: store(T=0),
        lambda: store(cap=0), lambda: store(fin=None), lambda: store(prio=None),
        lambda: store(psum=None), lambda: store(pmax=None), lambda: store(ring=None),
        lambda: store(cap=2 ** 33, T=8),                          # capacity W 2^30 >= 2^63
        lambda: sample(hid=8), lambda: sample(E=0), lambda: sample(Lr=0), lambda: sample(T=0),
        lambda: sample(K=-3), lambda: sample(K=4), lambda: sample(cap=0), lambda: sample(lens=None),
        lambda: sample(prio=None), lambda: sample(psum=None), lambda: sample(wdir=None),
        lambda: sample(isw=None), lambda: sample(beta=-0.1), lambda: sample(beta=nan),
        lambda: sample(beta=inf), lambda: sample(cap=2 ** 31, E=4, T=8, K=0),
        lambda: update(hid=16), lambda: update(E=0), lambda: update(Lr=0), lambda: update(T=0),
        lambda: update(cap=0), lambda: update(wdir=None), lambda: update(qa=None),
        lambda: update(d=None), lambda: update(isw=None), lambda: update(prio=None),
        lambda: update(pmax=None), lambda: update(alpha=-1.0), lambda: update(alpha=nan),
        lambda: update(alpha=inf), lambda: update(eta=-0.1), lambda: update(eta=1.1),
        lambda: update(eta=nan), lambda: update(eps=0.0), lambda: update(eps=-1.0),
        lambda: update(eps=nan), lambda: update(eps=inf), lambda: update(cap=2 ** 29, E=8, T=4),
    ]
    for k, f in enumerate(bad):
        assert f() == EINVAL, k
        with pytest.raises(ValueError):
            N.check(f())
    # the bound is checked before the pointers: 20,000 slots x 161 windows x E = 256 passes it
    # (what refuses is the null pointer), 2^33 does not
    assert lib.mz_drqn_prio_sample(1, 2, H, 256, 6440, 40, 40, 20000, None, p, p, p, p, p, p, 0.6,
                                   None) == EINVAL
    assert b"null pointer" in lib.mz_last_error()
    assert lib.mz_drqn_prio_sample(1, 2, H, 4, L, 8, 0, 2 ** 31, None, p, p, p, p, p, p, 0.6,
                                   None) == EINVAL
    assert b"63 bits" in lib.mz_last_error()
