"""Exact and float64 models of the PPO device path (csrc/mz_ppo.hip, k_pair_surrogate of
csrc/mz_optim.hip), numpy only. tests/test_ppo_model.py anchors them to the package's torch
expressions and to the recorded reference outputs; tests/test_ppo_exact.py holds the kernels to them.

scan    integer model of mz_ppo_scan (include/mazerl.h): every output is exact.
finish  mz_ppo_finish's documented arithmetic per episode: the recurrence in float64, every
        statistic from an exact sum (math.fsum) rounded once to float32, the normalisations in
        float32. The kernel adds the same float64 terms in another order; its statistic can round to
        another float32 only when the exact one lies next to a rounding midpoint, which `clear`
        reports (a mean whose sum is exact in every order is exempt: there is nothing to differ).
act     float64 softmax / log-prob and the inverse-CDF action of a 24-bit uniform.
pair    the [b, b] clipped surrogate with torch's gradient routing, float64.
head    mz_ppo_head_loss in float64 with its gradients written out.
"""
import math

import numpy as np

PPO_STREAM = 0x70706f21          # MZ_PPO_STREAM (csrc/mz_common.h)
ENT_EPS = float(np.float32(1e-8))  # the kernel's epsilon is the float32 constant
MID_GUARD = 2.0 ** -40           # finish: distance to a float32 rounding midpoint, times the scale
CDF_GUARD = 2.0 ** -20           # act: distance of the uniform to a cumulative boundary
CLIP_GUARD = 2.0 ** -18          # pair: relative distance of a ratio to a clip boundary


def uniform24(seed, counter, B):
    """The 24-bit integers behind k_ppo_act's uniforms, instance by instance."""
    import pyoracle as O
    return np.array([O.philox(seed, PPO_STREAM ^ (i << 32), counter)[0] >> 8 for i in range(B)],
                    np.int64)


# ---- scan ---------------------------------------------------------------------------------------
def scan(t, term, trunc, reward64, L, fill, total, stats):
    """One mz_ppo_scan call. Returns a dict: t (new), rec (list of (i, t, reward) written to
    rec_r), fin_id / fin_off / fin_len (lists, instance order), fin_count, fill, total, stats."""
    t = np.array(t, np.int64)
    stats = [int(s) for s in stats]
    rec, fin_id, fin_off, fin_len = [], [], [], []
    off = int(fill)
    for i in range(len(t)):
        ti = int(t[i])
        if 0 <= ti < L:
            rec.append((i, ti, float(reward64[i])))
        ti += 1
        if term[i] or trunc[i]:
            stats[0] += 1
            stats[1] += 1 if term[i] else 0
            if ti >= 2:
                fin_id.append(i)
                fin_off.append(off)
                fin_len.append(ti)
                off += ti
            else:
                stats[2] += 1
            ti = 0
        elif ti >= L:
            stats[3] += 1
            ti = L - 1
        t[i] = ti
    return dict(t=t.astype(np.int32), rec=rec, fin_id=fin_id, fin_off=fin_off, fin_len=fin_len,
                fin_count=len(fin_id), fill=off, total=int(total) + off - int(fill), stats=stats)


# ---- finish -------------------------------------------------------------------------------------
def _near_midpoint(x, scale):
    """x (float64) within MID_GUARD * scale of the midpoint of two neighbouring float32 values."""
    if not (math.isfinite(x) and math.isfinite(scale)):
        return False
    f = np.float32(x)
    for side in (np.float32(-np.inf), np.float32(np.inf)):
        g = np.nextafter(f, side)
        if np.isfinite(g) and abs(x - (float(f) + float(g)) / 2) <= MID_GUARD * scale:
            return True
    return False


def _mean_std32(x32):
    """mean and unbiased std of float32 values from exact sums, the second moment about the
    unrounded float64 mean; each rounded to float32. Also: whether either sits on a midpoint
    (scale: the largest |x| for the mean, the largest |x - mean| for the std)."""
    x = x32.astype(np.float64)
    n = len(x)
    mean = math.fsum(x) / n
    d = x - mean
    with np.errstate(invalid="ignore", divide="ignore"):
        std = math.sqrt(math.fsum(d * d) / (n - 1))
    near = _near_midpoint(std, float(np.abs(d).max()))
    if not _sum_is_exact_in_any_order(x32):
        near = near or _near_midpoint(mean, float(np.abs(x).max()))
    return np.float32(mean), np.float32(std), near


def _sum_is_exact_in_any_order(x32):
    """Every x is a multiple of q, the smallest float32 spacing among them, and n max|x| <
    2^52 q: each partial sum of any order is a multiple of q below 2^53 q, a float64 exactly.
    The kernel's sum is then the exact one and its mean this model's, bit for bit, wherever it
    lies. (Short episodes: the mean of two float32 values is a float32 midpoint more often than
    not, and both sides round that tie alike.)"""
    nz = np.abs(x32[x32 != 0])
    if not len(nz) or not np.isfinite(nz).all():
        return True
    return len(x32) * float(nz.max()) < 2.0 ** 52 * float(np.spacing(nz).min())


def finish(rewards, values, gamma):
    """One episode (n >= 2). rewards float64 [n], values float32 [n] -> (returns f32 [n],
    advantages f32 [n], clear)."""
    r = np.asarray(rewards, np.float64)
    v = np.asarray(values, np.float32)
    n = len(r)
    g = np.float64(gamma)
    R = np.empty(n, np.float32)
    acc = np.float64(0.0)
    for t in range(n - 1, -1, -1):
        acc = r[t] + acc * g
        R[t] = np.float32(acc)
    with np.errstate(invalid="ignore", divide="ignore"):
        m32, s32, near1 = _mean_std32(R)
        Rn = (R - m32) / s32
        A = Rn - v
        am32, as32, near2 = _mean_std32(A) if np.isfinite(A).all() else (np.float32("nan"),) * 2 + (False,)
        adv = (A - am32) / (as32 + np.float32(1e-8))
    assert Rn.dtype == np.float32 and adv.dtype == np.float32
    return Rn, adv, not (near1 or near2)


# ---- act ----------------------------------------------------------------------------------------
def act(logits, u24):
    """logits [B, 4] (float32 values), u24 [B] -> dict: p, logp [B, 4] float64, action [B],
    clear [B], allowed [B, 4] (the actions within CDF_GUARD of the uniform: the one drawn, and on a
    row that is not clear its neighbour across the boundary)."""
    z = np.asarray(logits, np.float64)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(axis=1, keepdims=True)
    p = e / S
    logp = z - m - np.log(S)
    r = np.asarray(u24, np.float64) / 2.0 ** 24
    c = np.cumsum(p, axis=1)
    below = r[:, None] < c
    action = np.where(below.any(axis=1), below.argmax(axis=1), 3)
    clear = (np.abs(r[:, None] - c) > CDF_GUARD).all(axis=1)
    lo = np.concatenate([np.zeros((len(r), 1)), c[:, :3]], axis=1)
    allowed = (r[:, None] >= lo - CDF_GUARD) & (r[:, None] < c + CDF_GUARD)
    allowed[np.arange(len(r)), action] = True
    return dict(p=p, logp=logp, action=action.astype(np.int64), clear=clear, allowed=allowed)


# ---- pair surrogate -----------------------------------------------------------------------------
def pair(lp_new, lp_old, adv, clip):
    """part [b], dsum [b] float64 and clear [b]; element (j, i) pairs lp_old[j] with lp_new[i]."""
    ln, lo_, a = (np.asarray(x, np.float64).reshape(-1) for x in (lp_new, lp_old, adv))
    lo, hi = 1.0 - clip, 1.0 + clip
    r = np.exp(ln[None, :] - lo_[:, None])
    s1 = r * a[None, :]
    s2 = np.clip(r, lo, hi) * a[None, :]
    inside = ((r >= lo) & (r <= hi)).astype(np.float64)
    w = np.where(s1 == s2, 0.5 + 0.5 * inside, np.where(s1 < s2, 1.0, inside))
    part = np.minimum(s1, s2).sum(axis=0)
    dsum = (r * w).sum(axis=0)
    near = np.zeros(r.shape, bool)
    for edge in (lo, hi):
        near |= (np.abs(r - edge) <= CLIP_GUARD * edge) & (r != edge)
    return part, dsum, ~near.any(axis=0)


# ---- head loss ----------------------------------------------------------------------------------
def head(logits, value, action, lp_old, adv, ret, coef, clip):
    """mz_ppo_head_loss in float64. logits [b, 4], the rest [b]; coef the float32 device scalar.
    Returns dict: total, dlogits [b, 4], dvalue [b], lp_new, ent, part, dsum, clear [b]."""
    z = np.asarray(logits, np.float64)
    v, ret, a64 = (np.asarray(x, np.float64).reshape(-1) for x in (value, ret, adv))
    act_ = np.asarray(action, np.int64).reshape(-1)
    b = z.shape[0]
    ar = np.arange(b)
    coef = float(np.float32(coef))
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    S = e.sum(axis=1, keepdims=True)
    p = e / S
    lsm = z - m - np.log(S)
    lp_new = lsm[ar, act_]
    lg = np.log(p + ENT_EPS)
    ent = -(p * lg).sum(axis=1)
    part, dsum, clear = pair(lp_new, lp_old, a64, clip)
    total = -(part.sum() / (b * b) + coef * ent.mean()) + 0.5 * np.mean((v - ret) ** 2)
    dlp = -a64 * dsum / (b * b)
    onehot = np.zeros((b, 4))
    onehot[ar, act_] = 1.0
    g = -(lg + p / (p + ENT_EPS))                      # d entropy / d p_k
    dent = p * (g - (p * g).sum(axis=1, keepdims=True))  # d entropy / d z_k
    dlogits = dlp[:, None] * (onehot - p) - (coef / b) * dent
    dvalue = (v - ret) / b
    return dict(total=float(total), dlogits=dlogits, dvalue=dvalue, lp_new=lp_new, ent=ent,
                part=part, dsum=dsum, clear=clear)
