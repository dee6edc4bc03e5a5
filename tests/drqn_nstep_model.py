"""Models of the recurrent DQN's double-Q targets and n-step returns (VectorRecurrentDQNTrainer
departures 13-14), on top of drqn_model and drqn_window_model.

A span is drqn_window_model's window dict (x [k + m + 1, 6], a [m], r [m], h0 / c0, k, term = the
last training step is the last step of a terminated episode); a whole episode is the window T = L,
K = 0, j = 0. Rows 0 .. m of a span are the steps s .. s + m: m training steps and the step after.

  returns_exact   the returns kernel's float32 arithmetic, bit for bit: fmaf rounds the exact
                  a b + c once (Fraction arithmetic), max follows fmaxf (a NaN operand is ignored,
                  +0 above -0), the loss term is the float64 sum of squares in time order;
  nstep_td_loss   the float64 model of the whole update: qa, y, loss, the six gradients, the source
                  net's first argmax per row and its top-two gap;
  torch_nstep     the same in torch float32 on the CPU (the reference error of the project's bound).
"""
from fractions import Fraction

import numpy as np

import drqn_model as M
import drqn_window_model as W

F32 = np.float32


def round_f32(x):
    """The exact rational x rounded once to float32 (nearest, ties to even)."""
    if x == 0:
        return F32(0.0)
    # float(Fraction) rounds once to float64; a second rounding to float32 could double-round, so
    # round by hand: scale so that the integer part holds 24 bits
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = 0
    while x >= 1 << 24:
        x /= 2
        e += 1
    while x < 1 << 23:
        x *= 2
        e -= 1
    if e < -149:  # subnormal: fewer bits
        x /= 1 << (-149 - e)
        e = -149
    n, rem = divmod(x.numerator, x.denominator)
    half = Fraction(rem, x.denominator)
    if half > Fraction(1, 2) or (half == Fraction(1, 2) and n % 2):
        n += 1
    return F32(sign * float(n) * 2.0 ** e)  # (n <= 2^24 and the scale are exact in float64)


def fmaf32(a, b, c):
    """fmaf in float32: a b + c rounded once. NaN and infinities by numpy's rules; an exact zero
    result takes IEEE's sign (the sum of two zeros of unlike sign is +0)."""
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        prod_neg = bool(np.signbit(a)) != bool(np.signbit(b))
        if float(a) * float(b) == 0.0 and float(c) == 0.0:  # zero + zero
            return F32(-0.0) if prod_neg and np.signbit(c) else F32(0.0)
        return F32(0.0)  # exact cancellation of nonzero terms: +0 (round to nearest)
    return round_f32(exact)


def fmaxf32(a, b):
    """fmaxf: a NaN operand is ignored; +0 is above -0."""
    if np.isnan(a):
        return F32(b)
    if np.isnan(b):
        return F32(a)
    if a == b:
        return F32(b) if np.signbit(a) else F32(a)
    return F32(a) if a > b else F32(b)


def max4(v):
    return fmaxf32(fmaxf32(v[0], v[1]), fmaxf32(v[2], v[3]))


def first_argmax(v):
    """The acting kernel's rule: the first maximum in action order; a NaN row selects 0."""
    a = 0
    for k in range(1, 4):
        if v[k] > v[a]:
            a = k
    return a


def returns_exact(r, qa, q4, sel, N, gamma, term, steps):
    """One span: r [m], qa [m], q4 [m + 1, 4] (float32), sel [m + 1] ints or None, term = no
    bootstrap at row m, steps = the batch's training steps. -> y [m], d [m] (float32), the span's
    loss term (float64)."""
    m = len(r)
    gamma = F32(gamma)
    inv = F32(1.0 / float(steps))
    y, d = np.zeros(m, F32), np.zeros(m, F32)
    sq = np.float64(0.0)
    with np.errstate(invalid="ignore"):
        for i in range(m):
            u = i + min(N, m - i)
            acc = F32(r[u - 1])
            if not (u == m and term):
                boot = max4(q4[u]) if sel is None else F32(q4[u][int(sel[u]) & 3])
                acc = fmaf32(gamma, boot, acc)
            for j in range(u - 2, i - 1, -1):
                acc = fmaf32(gamma, acc, r[j])
            dd = F32(F32(qa[i]) - acc)
            y[i] = acc
            d[i] = F32(F32(F32(2.0) * dd) * inv)
            sq = sq + np.float64(dd) * np.float64(dd)
    return y, d, sq


def episode_span(ep):
    """A whole episode (drqn_model's dict) as a span from zero state."""
    return W.window_of(ep, len(ep["a"]), 0, 0)


def _targets(r, boot, N, gamma, term):
    m = len(r)
    y = np.zeros(m, boot.dtype)
    for i in range(m):
        u = i + min(N, m - i)
        acc = r[u - 1] if (u == m and term) else r[u - 1] + gamma * boot[u]
        for j in range(u - 2, i - 1, -1):
            acc = r[j] + gamma * acc
        y[i] = acc
    return y


def nstep_td_loss(P, Pt, spans, gamma, double_q, N, weight=None, given=None):
    """-> dict(qa, y: lists of [m] arrays per span, sel, gap: lists of [m + 1] (the source net's
    first argmax and top-two gap at steps s .. s + m), loss, grads). The selection is a constant of
    the loss; the source's extra step carries no loss term and no gradient. given: a selection per
    span to bootstrap from in place of the model's own (sel and gap stay the model's)."""
    steps = sum(len(w["a"]) for w in spans)
    wt = 1.0 / steps if weight is None else weight
    out = {"qa": [], "y": [], "sel": [], "gap": [], "loss": 0.0,
           "grads": {k: np.zeros_like(P[k]) for k in M.KEYS}}
    for w in spans:
        k, m = w["k"], len(w["a"])
        x, a, r = np.asarray(w["x"], np.float64), np.asarray(w["a"]), np.asarray(w["r"], np.float64)
        _, _, h, c = W.unroll_from(P, x[:k], w["h0"], w["c0"])
        q, cache, h, c = W.unroll_from(P, x[k:k + m], h, c)
        qx, _, _, _ = W.unroll_from(P, x[k + m:k + m + 1], h, c)
        qs = np.concatenate([q, qx])
        qt = W.unroll_from(Pt, x, w["h0"], w["c0"])[0][k:]
        sel = np.array([first_argmax(v) for v in qs])
        top = np.sort(qs, axis=1)
        use = sel if given is None else np.asarray(given[len(out["qa"])])
        boot = qt[np.arange(m + 1), use] if double_q else qt.max(axis=1)
        y = _targets(r, boot, N, gamma, w["term"])
        qa = q[np.arange(m), a]
        out["qa"].append(qa)
        out["y"].append(y)
        out["sel"].append(sel)
        out["gap"].append(top[:, 3] - top[:, 2])
        out["loss"] += wt * float(((qa - y) ** 2).sum())
        g = M.bptt(P, cache, a, 2.0 * wt * (qa - y))
        for key in M.KEYS:
            out["grads"][key] += g[key]
    return out


def torch_nstep(src, tgt, spans, gamma, double_q, N, given=None):
    """nstep_td_loss in torch float32 on the CPU with autograd (src, tgt: lstm_dqn_agent.DQN).
    -> dict(qa, y: concatenated float32 arrays, sel: list of [m + 1], loss, grads)."""
    import torch
    t32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32))  # noqa: E731
    for p in src.parameters():
        p.grad = None
    total, steps, qas, ys, sels = 0.0, 0, [], [], []
    for w in spans:
        k, m = w["k"], len(w["a"])
        x, a, r = t32(w["x"]), torch.from_numpy(np.asarray(w["a"])), t32(w["r"])
        h0, c0 = t32(w["h0"])[None], t32(w["c0"])[None]
        h, c = h0, c0
        with torch.no_grad():
            if k:
                _, h, c = src.unroll_from(x[None, :k], h, c)
        q, h1, c1 = src.unroll_from(x[None, k:k + m], h, c)
        q = q[0]
        with torch.no_grad():
            qx = src.unroll_from(x[None, k + m:k + m + 1], h1, c1)[0][0]
            qs = torch.cat([q.detach(), qx])
            sel = np.array([first_argmax(v) for v in qs.numpy()])
            qt = tgt.unroll_from(x[None], h0, c0)[0][0, k:]
            use = torch.from_numpy(np.asarray(sel if given is None else given[len(sels)]))
            boot = qt[torch.arange(m + 1), use.long()] if double_q else qt.max(dim=1)[0]
            y = t32(_targets(r.numpy(), boot.numpy(), N, np.float32(gamma), w["term"]))
        qa = q.gather(1, a[:, None]).squeeze(1)
        total = total + ((qa - y) ** 2).sum()
        steps += m
        qas.append(qa.detach().numpy())
        ys.append(y.numpy())
        sels.append(sel)
    loss = total / steps
    loss.backward()
    return dict(qa=np.concatenate(qas), y=np.concatenate(ys), sel=sels, loss=loss.item(),
                grads={k: p.grad.numpy().copy() for k, p in src.named_parameters()})
