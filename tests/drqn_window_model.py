"""Float64 numpy model of the recurrent DQN's replay windows (VectorRecurrentDQNTrainer departures
7-9: windows of T steps, stored state, K burn-in steps), built on drqn_model's cell, head and bptt.

A window is a dict: x [k + m + 1, 6] (the observations of steps b .. s + m), a [m], r [m] (the m
training steps s .. s + m - 1), h0 / c0 [32] (the state both nets start from at step b), k (the
burn-in steps s - b) and term (the last training step is the last step of a terminated episode)."""
import numpy as np

import drqn_model as M

H = M.H


def unroll_from(P, xs, h0, c0):
    """xs [T, 6] from the state (h0, c0) [32] -> q [T, 4], the per-step cache for drqn_model.bptt
    and the state after the last step. With zero state this is drqn_model.unroll, op for op."""
    h, c = np.asarray(h0, np.float64)[None], np.asarray(c0, np.float64)[None]
    qs, cache = [], []
    for t in range(xs.shape[0]):
        h1, c1, gates = M.cell(P, xs[t:t + 1], h, c)
        cache.append((xs[t], h[0], c[0], h1[0], c1[0]) + tuple(g[0] for g in gates))
        qs.append(M.head(P, h1)[0])
        h, c = h1, c1
    return np.array(qs).reshape(-1, 4), cache, h[0], c[0]


def windows_in(n, T):
    return (n - 1) // T + 1


def window_of(ep, T, K, j, snaps=None):
    """Window j of episode ep (drqn_model's dict). snaps [ceil(n / T), 64] = (h, c) per window
    start, row 0 unused; None: every window starts from zero state."""
    n = len(ep["a"])
    s = j * T
    assert 0 <= s < n and K % T == 0
    m, b = min(T, n - s), max(0, s - K)
    st = np.zeros(2 * H) if snaps is None or b == 0 else np.asarray(snaps[b // T], np.float64)
    return dict(x=np.asarray(ep["x"])[b:s + m + 1], a=np.asarray(ep["a"])[s:s + m],
                r=np.asarray(ep["r"])[s:s + m], h0=st[:H], c0=st[H:], k=s - b,
                term=bool(ep["term"]) and s + m == n, b=b, s=s, m=m)


def window_td_loss(P, Pt, windows, gamma, weight=None):
    """-> dict(qa, y: lists of [m] arrays per window, entry: list of (h, c) entering step s, loss,
    grads). loss = sum (Q_t[a_t] - y_t)^2 / sum m; the burn-in steps only advance the state, and
    the gradient stops at the state that enters step s."""
    steps = sum(len(w["a"]) for w in windows)
    wt = 1.0 / steps if weight is None else weight
    out = {"qa": [], "y": [], "entry": [], "loss": 0.0,
           "grads": {k: np.zeros_like(P[k]) for k in M.KEYS}}
    for w in windows:
        k, m = w["k"], len(w["a"])
        x, a, r = np.asarray(w["x"], np.float64), np.asarray(w["a"]), np.asarray(w["r"], np.float64)
        _, _, h, c = unroll_from(P, x[:k], w["h0"], w["c0"])
        q, cache, _, _ = unroll_from(P, x[k:k + m], h, c)
        qt, _, _, _ = unroll_from(Pt, x, w["h0"], w["c0"])
        y = r + gamma * qt[k + 1:].max(axis=1)
        if w["term"]:
            y[m - 1] = r[m - 1]
        qa = q[np.arange(m), a]
        out["qa"].append(qa)
        out["y"].append(y)
        out["entry"].append((h, c))
        out["loss"] += wt * float(((qa - y) ** 2).sum())
        g = M.bptt(P, cache, a, 2.0 * wt * (qa - y))
        for key in M.KEYS:
            out["grads"][key] += g[key]
    return out
