"""Float64 numpy restatement of the recurrent DQN (nn.LSTMCell(6, 32) + nn.Linear(32, 4), gate order
i, f, g, o): the cell, the head, the episode-batch TD loss of VectorRecurrentDQNTrainer and its
gradient by back-propagation through time. The GPU kernels and the torch drop-in are held to it.

Parameters are a dict keyed like the net's state_dict (KEYS), float64 arrays. An episode is a dict
x [n + 1, 6], a [n], r [n], term (bool)."""
import numpy as np

KEYS = ("lstm_cell.weight_ih", "lstm_cell.weight_hh", "lstm_cell.bias_ih", "lstm_cell.bias_hh",
        "fc.weight", "fc.bias")
H = 32


def as_f64(sd):
    return {k: np.asarray(sd[k], dtype=np.float64) for k in KEYS}


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def cell(P, x, h, c):
    """One step for rows x [m, 6], h / c [m, 32] -> (h', c', gates (i, f, g, o))."""
    z = (P[KEYS[2]] + P[KEYS[3]]) + x @ P[KEYS[0]].T + h @ P[KEYS[1]].T
    i, f, o = sigmoid(z[:, :H]), sigmoid(z[:, H:2 * H]), sigmoid(z[:, 3 * H:])
    g = np.tanh(z[:, 2 * H:3 * H])
    c1 = f * c + i * g
    return o * np.tanh(c1), c1, (i, f, g, o)


def head(P, h):
    return h @ P[KEYS[4]].T + P[KEYS[5]]


def forward(P, x):
    """The reference's DQN.forward: x [batch, seq, 6] from zero state -> q of the last step."""
    h = c = np.zeros((x.shape[0], H))
    for t in range(x.shape[1]):
        h, c, _ = cell(P, x[:, t], h, c)
    return head(P, h)


def unroll(P, xs):
    """xs [T, 6] from zero state -> q [T, 4] and the per-step cache for bptt()."""
    h = c = np.zeros((1, H))
    qs, cache = [], []
    for t in range(xs.shape[0]):
        h1, c1, gates = cell(P, xs[t:t + 1], h, c)
        cache.append((xs[t], h[0], c[0], h1[0], c1[0]) + tuple(g[0] for g in gates))
        qs.append(head(P, h1)[0])
        h, c = h1, c1
    return np.array(qs), cache


def bptt(P, cache, a, dq):
    """Gradient of sum_t dq[t] * Q_t[a[t]] w.r.t. the six parameters."""
    G = {k: np.zeros_like(P[k]) for k in KEYS}
    dh_n = np.zeros(H)
    dc_n = np.zeros(H)
    for t in range(len(cache) - 1, -1, -1):
        x, hp, cp, h1, c1, i, f, g, o = cache[t]
        G[KEYS[4]][a[t]] += dq[t] * h1
        G[KEYS[5]][a[t]] += dq[t]
        dh = dh_n + dq[t] * P[KEYS[4]][a[t]]
        tc = np.tanh(c1)
        dc = dc_n + dh * o * (1.0 - tc * tc)
        dz = np.concatenate([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g),
                             dh * tc * o * (1 - o)])
        G[KEYS[0]] += np.outer(dz, x)
        G[KEYS[1]] += np.outer(dz, hp)
        G[KEYS[2]] += dz
        G[KEYS[3]] += dz
        dh_n = P[KEYS[1]].T @ dz
        dc_n = dc * f
    return G


def td_loss(P, Pt, episodes, gamma, weight=None):
    """-> dict(qa, y: lists of [n] arrays per episode, loss, grads). loss = mean over all sum n
    steps of (Q_t[a_t] - y_t)^2, y_t = r_t + gamma max_a Q'_{t+1}[a] (r_t alone at the last step of
    a terminated episode), no gradient through y. weight: 1 / sum n by default."""
    steps = sum(len(e["a"]) for e in episodes)
    w = 1.0 / steps if weight is None else weight
    out = {"qa": [], "y": [], "loss": 0.0, "grads": {k: np.zeros_like(P[k]) for k in KEYS}}
    for e in episodes:
        n = len(e["a"])
        x, a, r = np.asarray(e["x"], np.float64), np.asarray(e["a"]), np.asarray(e["r"], np.float64)
        q, cache = unroll(P, x[:n])
        qt, _ = unroll(Pt, x)
        y = r + gamma * qt[1:].max(axis=1)
        if e["term"]:
            y[n - 1] = r[n - 1]
        qa = q[np.arange(n), a]
        out["qa"].append(qa)
        out["y"].append(y)
        out["loss"] += w * float(((qa - y) ** 2).sum())
        g = bptt(P, cache, a, 2.0 * w * (qa - y))
        for k in KEYS:
            out["grads"][k] += g[k]
    return out
