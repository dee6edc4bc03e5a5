"""Plain float64 models of the learner's hand-written update stages (numpy only, no native code):

  head_forward / head_backward   the Q head + loss of csrc/mz_trainer.hip (k_head_loss, k_loss_sum,
                                 k_head_loss_bwd + the column sum): the second hidden layer's
                                 activation, fc3, the TD error of optimize_model and mse_loss(mean)
  q_loss_forward / q_loss_backward  the same loss from given Q rows (k_q_loss_fwd / k_q_loss_bwd)
  adamw_step                     the per-element update of csrc/mz_optim.hip's header comment

They state the operation, not the kernels' loops. Inputs are f32 arrays widened to f64; the
constants are the f32 values the kernels hold (slope f32(0.01), f32(gamma), norm f32(2 / b); AdamW's
scalars formed in double, cast to f32, widened), so a model and its kernel differ by the kernel's
f32 roundings alone. Special values follow torch: argmax takes the first maximum and the first
NaN, max propagates NaN, ReLU is clamp_min (NaN propagates) with threshold_backward as its
gradient, LeakyReLU's gradient is z > 0 ? g : g * slope. tests/test_learner_model.py pins every
model to torch float64 autograd / torch.optim.AdamW on the CPU."""
import numpy as np

SLOPE = np.float64(np.float32(0.01))
U32 = 2.0 ** -24  # unit roundoff of f32


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def act_forward(z, act):
    """act 0: LeakyReLU(0.01); act 1: ReLU as clamp_min(z, 0) (NaN propagates)."""
    z = _f64(z)
    if act == 0:
        return np.where(z > 0, z, z * SLOPE)
    return np.where(np.isnan(z), z, np.maximum(z, 0.0))


def act_backward(z, g, act):
    """leaky_relu_backward: z > 0 ? g : g * slope; threshold_backward: z <= 0 ? 0 : g."""
    z, g = _f64(z), _f64(g)
    if act == 0:
        return np.where(z > 0, g, g * SLOPE)
    return np.where(z <= 0, 0.0, g)


def _linear(h, w, bias):
    """q[i,k] = sum_j h[i,j] w[k,j] + bias[k] and mag[i,k] = sum_j |h||w| + |bias| (products formed
    element by element: inf * 0 and NaN behave as IEEE says, whatever a BLAS would do)."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = (h[:, None, :] * w[None, :, :]).sum(-1) + bias[None, :]
        mag = (np.abs(h)[:, None, :] * np.abs(w)[None, :, :]).sum(-1) + np.abs(bias)[None, :]
    return q, mag


def _td(q_sa, q_next, q_tgt, reward, gamma, dbl):
    """V(s') = q_tgt[argmax q_next] (first maximum / first NaN) or max q_tgt (NaN propagates);
    diff = Q(s,a) - (V * gamma + r)."""
    g32 = np.float64(np.float32(gamma))
    rows = np.arange(q_tgt.shape[0])
    if dbl:
        choice = np.argmax(q_next, axis=1)  # numpy: first maximum, first NaN — as torch.argmax
        v = q_tgt[rows, choice]
    else:
        choice = np.argmax(q_tgt, axis=1)
        v = np.max(q_tgt, axis=1)  # propagates NaN
    with np.errstate(invalid="ignore", over="ignore"):
        diff = q_sa - (v * g32 + reward)
        loss = np.mean(diff * diff)
    return choice, v, diff, loss


def head_forward(z2s, w3s, b3s, z2t, w3t, b3t, action, reward, gamma, b, act, dbl):
    """z2s [>= b (2b when dbl), H], z2t [>= b, H]: pre-activations of the source rows (s, then s'
    when dbl) and of the target's s' rows. Returns a dict: q_s, q_n, q_t [b, 4] (q_n None unless
    dbl), their magnitude sums mag_s, mag_n, mag_t, choice [b] (the argmax column: of q_n when
    dbl, else of q_t), v [b], diff [b], loss."""
    z2s, z2t = _f64(z2s), _f64(z2t)
    w3s, b3s, w3t, b3t = _f64(w3s), _f64(b3s), _f64(w3t), _f64(b3t)
    action = np.asarray(action, dtype=np.int64)[:b]
    reward = _f64(reward)[:b]
    q_s, mag_s = _linear(act_forward(z2s[:b], act), w3s, b3s)
    q_t, mag_t = _linear(act_forward(z2t[:b], act), w3t, b3t)
    q_n = mag_n = None
    if dbl:
        q_n, mag_n = _linear(act_forward(z2s[b:2 * b], act), w3s, b3s)
    choice, v, diff, loss = _td(q_s[np.arange(b), action], q_n, q_t, reward, gamma, dbl)
    return dict(q_s=q_s, q_n=q_n, q_t=q_t, mag_s=mag_s, mag_n=mag_n, mag_t=mag_t, choice=choice,
                v=v, diff=diff, loss=loss)


def head_tolerances(fw, action, reward, gamma, H, dbl):
    """The derived f32 bounds of tests/test_head_loss_exact.py from a head_forward() result:
    tol_q = (ceil(H / 64) + 10) u mag per Q value; per row tol_diff = tol_q(s, a) + gamma
    tol_q(v) + 3 u (|q| + |gamma v| + |r|); and near[i]: the float64 top-two gap of the row the
    choice is made on is <= 2 max_k tol_q (kernel and model might then pick different columns)."""
    b = fw["diff"].shape[0]
    rows = np.arange(b)
    a = np.asarray(action, dtype=np.int64)[:b]
    g32 = np.float64(np.float32(gamma))
    n = (-(-H // 64) + 10) * U32
    tq_s, tq_t = n * fw["mag_s"], n * fw["mag_t"]
    near = np.zeros(b, dtype=bool)  # (DQN's max is continuous in the row: no choice to miss)
    if dbl:
        top = np.sort(fw["q_n"], axis=1)
        near = (top[:, 3] - top[:, 2]) <= 2.0 * (n * fw["mag_n"]).max(axis=1)
    q_sa, v = fw["q_s"][rows, a], fw["v"]
    # DQN's max over the target's row: whichever column wins, its value is within the largest tol
    tv = tq_t[rows, fw["choice"]] if dbl else tq_t.max(axis=1)
    tol_diff = tq_s[rows, a] + g32 * tv + 3 * U32 * (np.abs(q_sa) + np.abs(g32 * v) +
                                                    np.abs(_f64(reward)[:b]))
    return tol_diff, near


def head_backward(gradient, diff, action, b, z2s, w3s, act, mags=False):
    """From the upstream gradient of the loss and the per-row diff: g_i = diff_i * norm * gradient,
    dz2[i,j] = act'(z2[i,j]) applied to g_i * W3[a_i,j]; dW3[k,j] = sum_{a_i = k} g_i act(z2[i,j]);
    db3[k] = sum_{a_i = k} g_i. mags: also sum_i |t_i| of the two sums (for the tolerances)."""
    z = _f64(z2s)[:b]
    w = _f64(w3s)
    a = np.asarray(action, dtype=np.int64)[:b]
    norm = np.float64(np.float32(2.0 / b))
    with np.errstate(invalid="ignore", over="ignore"):
        g = _f64(diff)[:b] * norm * np.float64(gradient)
        dz2 = act_backward(z, g[:, None] * w[a], act)
        t = g[:, None] * act_forward(z, act)
        H = z.shape[1]
        dW, db = np.zeros((4, H)), np.zeros(4)
        aW, ab = np.zeros((4, H)), np.zeros(4)
        for k in range(4):
            sel = a == k
            dW[k], db[k] = t[sel].sum(0), g[sel].sum()
            aW[k], ab[k] = np.abs(t[sel]).sum(0), np.abs(g[sel]).sum()
    return (dz2, dW, db, aW, ab) if mags else (dz2, dW, db)


def q_loss_forward(q, q_next, q_tgt, action, reward, gamma, b):
    """The loss from Q rows: q [>= b, 4], q_next [b, 4] or None (DQN), q_tgt [b, 4]."""
    q, q_tgt = _f64(q)[:b], _f64(q_tgt)[:b]
    a = np.asarray(action, dtype=np.int64)[:b]
    qn = None if q_next is None else _f64(q_next)[:b]
    choice, v, diff, loss = _td(q[np.arange(b), a], qn, q_tgt, _f64(reward)[:b], gamma,
                                qn is not None)
    return dict(choice=choice, v=v, diff=diff, loss=loss)


def q_loss_backward(gradient, diff, action, b, rows):
    """dq [rows, 4]: diff_i * norm * gradient at column a_i of row i < b, zero elsewhere."""
    norm = np.float64(np.float32(2.0 / b))
    dq = np.zeros((rows, 4))
    with np.errstate(invalid="ignore", over="ignore"):
        dq[np.arange(b), np.asarray(action, dtype=np.int64)[:b]] = \
            _f64(diff)[:b] * norm * np.float64(gradient)
    return dq


def adamw_scalars(lr, step, b1, b2, eps, wd):
    """The per-step scalars as the kernel's first lines form them: in double from the f32 lr and
    the step count after this step, then cast to f32 (and widened again)."""
    f = lambda x: np.float64(np.float32(x))  # noqa: E731
    lr = np.float64(np.float32(lr))
    t = np.float64(np.float32(np.float32(step) + np.float32(1.0)))
    bc1 = 1.0 - np.power(np.float64(b1), t)
    return dict(step_size=f(lr / bc1), bc2_sqrt=f(np.sqrt(1.0 - np.power(np.float64(b2), t))),
                decay=f(1.0 - lr * np.float64(wd)), w1=f(1.0 - np.float64(b1)), b2=f(b2),
                w2=f(1.0 - np.float64(b2)), eps=f(eps))


def adamw_step(p, g, m, v, lr, step, b1, b2, eps, wd, clamp, gscale):
    """One step from `step` completed steps (the kernel reads t = step + 1):
         g = clamp(g * grad_scale, -c, c)        NaN propagates
         p = p * (1 - lr * wd)
         m = m + (1 - b1) * (g - m)
         v = v * b2 + (1 - b2) * g * g
         p = p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    Returns (p', m', v', g_clamped) in float64."""
    s = adamw_scalars(lr, step, b1, b2, eps, wd)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    c = np.float64(np.float32(clamp))
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.clip(g * np.float64(np.float32(gscale)), -c, c)  # np.clip propagates NaN
        p = p * s["decay"]
        m = m + s["w1"] * (g - m)
        v = v * s["b2"] + s["w2"] * (g * g)
        denom = np.sqrt(v) / s["bc2_sqrt"] + s["eps"]
        p = p - s["step_size"] * (m / denom)
    return p, m, v, g
