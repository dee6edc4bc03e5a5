"""The replay-window loss off the GPU: the float64 model (tests/drqn_window_model.py) against
torch's float64 autograd and against drqn_model.td_loss, the burn-in's zero gradient, and the
torch float32 window_td_loss (agents/lstm_dqn_agent.py) against the model."""
import numpy as np
import torch

import drqn_model as M
import drqn_window_model as W


def _net(seed, dtype=torch.float32):
    from mazerl.agents.lstm_dqn_agent import DQN
    torch.manual_seed(seed)
    return DQN(6, 4, 32, torch.device("cpu")).to(dtype)


def _f64(net):
    return M.as_f64({k: v.detach().numpy() for k, v in net.state_dict().items()})


def _episodes(rng, lens, terms, dtype=np.float64):
    return [dict(x=rng.random((n + 1, 6)).astype(dtype), a=rng.integers(0, 4, n),
                 r=(rng.random(n) - 0.5).astype(dtype), term=bool(t)) for n, t in zip(lens, terms)]


def _snaps(rng, n, T, dtype=np.float64):
    return (rng.random((W.windows_in(n, T), 64)) - 0.5).astype(dtype)


def _torch_windows(ws, dtype):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    return [(t(w["x"]), torch.from_numpy(np.asarray(w["a"])), t(w["r"]), t(w["h0"]), t(w["c0"]),
             w["k"], w["term"]) for w in ws]


def _batch(rng, T, K, dtype=np.float64):
    """Every window of episodes whose lengths cover n = 1, T, T + 1 and a long one, both ends."""
    lens = [1, T, T + 1, 3 * T + 2, T, T + 1]
    eps = _episodes(rng, lens, [1, 1, 1, 0, 0, 0], dtype)
    ws = []
    for e in eps:
        n = len(e["a"])
        sn = _snaps(rng, n, T, dtype)
        ws += [W.window_of(e, T, K, j, sn) for j in range(W.windows_in(n, T))]
    return ws


def test_model_gradient_agrees_with_torch_float64_autograd():
    from mazerl.agents.lstm_dqn_agent import window_td_loss
    rng = np.random.default_rng(11)
    src, tgt = _net(1, torch.float64), _net(2, torch.float64)
    P, Pt = _f64(src), _f64(tgt)
    for T, K in [(1, 0), (1, 2), (3, 0), (3, 3), (3, 6), (8, 8)]:
        ws = _batch(rng, T, K)
        assert any(w["k"] == K for w in ws) and any(w["term"] for w in ws)
        out = W.window_td_loss(P, Pt, ws, 0.99)
        for p in src.parameters():
            p.grad = None
        loss = window_td_loss(src, tgt, _torch_windows(ws, torch.float64), 0.99)
        loss.backward()
        assert abs(out["loss"] - loss.item()) <= 1e-10 * abs(loss.item())
        for k, p in src.named_parameters():
            g = p.grad.numpy()
            assert np.abs(out["grads"][k] - g).max() <= 1e-10 * np.abs(g).max(), (T, K, k)


def test_one_window_per_whole_episode_is_the_episode_loss_exactly():
    rng = np.random.default_rng(12)
    P, Pt = _f64(_net(3)), _f64(_net(4))
    eps = _episodes(rng, [1, 2, 7, 8], [1, 0, 1, 0])
    whole = M.td_loss(P, Pt, eps, 0.9)
    out = W.window_td_loss(P, Pt, [W.window_of(e, 8, 0, 0) for e in eps], 0.9)
    assert out["loss"] == whole["loss"]
    for a, b in zip(out["qa"] + out["y"], whole["qa"] + whole["y"]):
        assert np.array_equal(a, b)
    for k in M.KEYS:
        assert np.array_equal(out["grads"][k], whole["grads"][k]), k


def test_burn_in_steps_receive_no_gradient():
    """The model: a window with K > 0 has exactly the gradient of the K = 0 window that starts
    from the state the burn-in produced. torch: the loss has no gradient w.r.t. the burn-in's
    inputs or the initial state, and one w.r.t. the training steps' inputs."""
    from mazerl.agents.lstm_dqn_agent import window_td_loss
    rng = np.random.default_rng(13)
    src, tgt = _net(5, torch.float64), _net(6, torch.float64)
    P, Pt = _f64(src), _f64(tgt)
    ep = _episodes(rng, [11], [1])[0]
    w = W.window_of(ep, 3, 6, 3, _snaps(rng, 11, 3))
    assert (w["b"], w["k"], w["m"], w["term"]) == (3, 6, 2, True)
    out = W.window_td_loss(P, Pt, [w], 0.9)
    h, c = out["entry"][0]
    cut = dict(w, x=w["x"][w["k"]:], h0=h, c0=c, k=0)
    # (the target's own burn-in is folded into y: feed the cut window the same targets)
    q, cache, _, _ = W.unroll_from(P, np.asarray(cut["x"][:2], np.float64), h, c)
    qa = q[np.arange(2), w["a"]]
    assert np.array_equal(qa, out["qa"][0])
    g = M.bptt(P, cache, w["a"], 2.0 / 2 * (qa - out["y"][0]))
    for k in M.KEYS:
        assert np.array_equal(g[k], out["grads"][k]), k
    tw = _torch_windows([w], torch.float64)[0]
    x, h0, c0 = (t.clone().requires_grad_(True) for t in (tw[0], tw[3], tw[4]))
    window_td_loss(src, tgt, [(x, tw[1], tw[2], h0, c0) + tw[5:]], 0.9).backward()
    assert h0.grad is None and c0.grad is None
    assert bool((x.grad[:6] == 0).all()) and bool((x.grad[6:8] != 0).any())
    assert bool((x.grad[8:] == 0).all())  # x_{s+m} only feeds the target


def test_torch_float32_loss_agrees_with_the_model_to_counted_rounding():
    """float32 torch vs the model, counted as test_lstm_dqn does for the forward: |w| <= 1 /
    sqrt(32), |x|, |h0|, |c0| <= 1, so a gate pre-activation is 40 roundings on sum |terms| < 8
    (320 u), the slopes are <= 1 and c and h' each take that once per step: e_q(n) = (n 2 320 +
    33 7) u after n steps. y = r + gamma max Q' adds 2 roundings on |r| + |Q'| < 2 to e_q(k + m +
    1). A residual d is off by e_d = e_q + e_y, d^2 by 2 |d| e_d + e_d^2 + u d^2, and the mean
    over sum m steps adds (sum m + 1) u relative."""
    from mazerl.agents.lstm_dqn_agent import window_td_loss
    rng = np.random.default_rng(14)
    u = 2.0 ** -24
    src, tgt = _net(7), _net(8)
    for net in (src, tgt):
        assert all(float(p.detach().abs().max()) <= 1 / np.sqrt(32) for p in net.parameters())
    P, Pt = _f64(src), _f64(tgt)
    for T, K in [(1, 1), (3, 0), (3, 6), (8, 8)]:
        ws = _batch(rng, T, K, np.float32)
        out = W.window_td_loss(P, Pt, ws, 0.99)
        tws = _torch_windows(ws, torch.float32)
        worst, steps, err = 0.0, sum(w["m"] for w in ws), 0.0
        with torch.no_grad():
            for w, tw, mq, my in zip(ws, tws, out["qa"], out["y"]):
                x, a, r, h0, c0, k, term = tw
                m = a.shape[0]
                q = src.unroll_from(x[None, :k + m], h0[None], c0[None])[0][0, k:]
                qa = q.gather(1, a[:, None]).squeeze(1).numpy()
                e_q = ((k + m) * 2 * 320 + 33 * 7) * u
                e_y = ((k + m + 1) * 2 * 320 + 33 * 7) * u + 2 * 2 * u
                assert np.abs(qa - mq).max() <= e_q, (T, K, np.abs(qa - mq).max(), e_q)
                y = r + np.float32(0.99) * tgt.unroll_from(x[None], h0[None],
                                                           c0[None])[0][0, k + 1:].max(dim=1)[0]
                if term:
                    y[m - 1] = r[m - 1]
                assert np.abs(y.numpy() - my).max() <= e_y, (T, K)
                d = np.abs(mq - my)
                e_d = e_q + e_y
                err += float((2 * d * e_d + e_d ** 2 + u * d ** 2).sum())
                worst = max(worst, float(np.abs(qa - mq).max() / e_q))
        loss = window_td_loss(src, tgt, tws, 0.99).item()
        bound = err / steps + (steps + 1) * u * out["loss"]
        print(f"T {T} K {K}: q error / bound {worst:.3f}, loss error / bound "
              f"{abs(loss - out['loss']) / bound:.3f}")
        assert abs(loss - out["loss"]) <= bound, (T, K, loss, out["loss"], bound)
