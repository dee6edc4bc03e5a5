"""Integer and float64 model of the recurrent DQN's prioritized replay windows
(VectorRecurrentDQNTrainer departures 10-12; csrc/mz_drqn.hip k_drqn_prio_store / _sample /
_update), numpy and Python ints only.

A mass is an int in [0, 2^30]: a fixed-point priority with 20 fractional bits, 0 = no such window.
mem_prio is an int array [capacity][W], W = ceil(L / T); psum[slot] its row sums. Every sum is a
Python int, so the sampler here is exact: the kernel must give the same windows bit for bit."""
import math

import numpy as np

import drqn_window_model as W

FRAC = 20
ONE = 1 << FRAC
CEIL = 1 << 30
PRIO_STREAM = 0x64727170  # MZ_DRQN_PRIO_STREAM (csrc/mz_common.h)
M64 = (1 << 64) - 1


def draw(seed, counter, e):
    """The 64-bit word of batch position e: (r0 << 32) | r1 of philox(seed, {stream ^ e << 32,
    counter})."""
    import pyoracle as O
    r = O.philox(seed & M64, PRIO_STREAM ^ (e << 32), counter & M64)
    return (r[0] << 32) | r[1]


# ---- departure 10: entry ------------------------------------------------------------------------
def store(mem_prio, psum, prio_max, head, fin, B, L, T):
    """The listed episodes fin = [(instance, n), ...] enter at prio_max by k_drqn_store's slot
    rule and validity tests. mem_prio / psum are changed in place; returns the slots written."""
    cap = mem_prio.shape[0]
    first = max(0, len(fin) - cap)
    out = []
    for k in range(first, len(fin)):
        i, n = fin[k]
        if i < 0 or i >= B or n < 1 or n > L or head < 0 or head >= cap:
            continue
        slot = (head + k) % cap
        nw = W.windows_in(n, T)
        mem_prio[slot] = 0
        mem_prio[slot, :nw] = prio_max
        psum[slot] = nw * prio_max
        out.append(slot)
    return out


# ---- departure 11: sampling ---------------------------------------------------------------------
def locate(masses, t):
    """The index i of the flat int sequence `masses` with prefix(i) <= t < prefix(i) + masses[i]."""
    pre = 0
    for i, v in enumerate(masses):
        if pre <= t < pre + v:
            return i
        pre += v
    raise ValueError("t beyond the masses")


def sample(mem_prio, mem_len, seed, counter, E, T, K, beta, words=None):
    """-> dict of int arrays slot, n, b, k, m, off [E], tot (rows, steps), mass [E], the strata
    lo / hi and the draws t [E] (Python ints), and isw [E] float64 (round it to float32 to compare
    with the device). words: the 64-bit draws (default: the Philox stream)."""
    flat = [int(v) for v in np.asarray(mem_prio).ravel()]
    Wn = np.asarray(mem_prio).shape[1]
    S = sum(flat)
    out = {k: [] for k in ("slot", "n", "b", "k", "m", "mass", "lo", "hi", "t")}
    for e in range(E):
        lo, hi = e * S // E, (e + 1) * S // E
        r = draw(seed, counter, e) if words is None else words[e]
        t = lo + ((r * (hi - lo)) >> 64)
        i = locate(flat, t)
        slot, j = divmod(i, Wn)
        n = int(mem_len[slot])
        assert 0 <= j < W.windows_in(n, T), (slot, j, n)
        s = j * T
        b = max(0, s - K)
        for key, v in zip(out, (slot, n, b, s - b, min(T, n - s), flat[i], lo, hi, t)):
            out[key].append(v)
    m = np.array(out["m"], np.int64)
    out["off"] = np.concatenate([[0], np.cumsum(m + 2)[:-1]]).astype(np.int64)
    out["tot"] = (int((m + 2).sum()), int(m.sum()))
    mmin = min(out["mass"])
    out["isw"] = np.array([math.pow(mmin / v, beta) for v in out["mass"]], np.float64)
    return out


# ---- departure 12: the new masses and the weighted loss -------------------------------------------
def mass_of(a, alpha, eta, eps):
    """a: the window's |Q_t[a_t] - y_t| as float32, in time order."""
    a = np.asarray(a, np.float32)
    mx = float(a.max())
    s = 0.0
    for v in a:
        s += float(v)
    pr = eta * mx + (1.0 - eta) * (s / len(a))
    q = 1.0 if alpha == 0 else math.pow(pr + eps, alpha)
    v = q * ONE
    if not v < CEIL:  # (a NaN too)
        return CEIL
    return max(1, int(round(v)))  # round(): to nearest, ties to even, as llrint


def update(mem_prio, psum, prio_max, slots, js, resid, alpha, eta, eps):
    """resid[e]: window e's float32 |qa - y|. Changes mem_prio / psum in place; returns (the
    masses written, the new prio_max)."""
    masses = [mass_of(a, alpha, eta, eps) for a in resid]
    for slot, j, v in zip(slots, js, masses):
        mem_prio[slot, j] = v
    for slot in set(slots):
        psum[slot] = int(mem_prio[slot].astype(object).sum())
    return masses, max([prio_max] + masses)


def weighted_td_loss(P, Pt, windows, gamma, weights):
    """drqn_window_model.window_td_loss with window e's terms scaled by weights[e]: loss =
    sum_e w_e sum_t (Q_t[a_t] - y_t)^2 / sum m, and its gradient. With every weight 1.0 this is
    window_td_loss's arithmetic, operation for operation."""
    steps = sum(len(w["a"]) for w in windows)
    out = {"qa": [], "y": [], "entry": [], "loss": 0.0, "grads": None}
    for w, we in zip(windows, weights):
        o = W.window_td_loss(P, Pt, [w], gamma, weight=float(we) / steps)
        for k in ("qa", "y", "entry"):
            out[k] += o[k]
        out["loss"] += o["loss"]
        if out["grads"] is None:
            out["grads"] = {k: np.zeros_like(v) for k, v in o["grads"].items()}
        for k in out["grads"]:
            out["grads"][k] += o["grads"][k]
    return out
