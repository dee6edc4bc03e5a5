"""Deterministic inputs for the Q-loss parity fixtures (shared by tests/golden/make_golden_learner.py
and tests/test_learner.py), the packed-window layout, and the random and hand-made head + loss
inputs of tests/test_head_loss_exact.py / tests/test_learner_model.py. Pure data generation — no
reference code."""
import numpy as np
import torch

REWARDS = [1.0, 0.45, -0.55, -1.0, -0.18126924692201818, -0.13929202357494222, -0.05]
CASES = {  # name: (variant, h_channels, hidden_dim, n, gamma, lr, train_mode)
    "dqn_small": ("dqn", 4, 8, 8, 0.7, 1e-3, False),
    "ddqn_small": ("ddqn", 4, 8, 8, 0.7, 1e-3, False),
    "ddqn_small_dropout": ("ddqn", 4, 8, 8, 0.7, 1e-3, True),
    "dqn_full": ("dqn", 32, 1024, 16, 0.7, 1e-3, False),
    "ddqn_full": ("ddqn", 32, 1024, 16, 0.7, 1e-3, False),
}


def fill_params(net, seed):
    """Overwrite every parameter (sorted by name) from one seeded generator."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(net.named_parameters()):
            fan = p[0].numel() if p.dim() > 1 else p.numel()
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / np.sqrt(max(1, fan)))


def make_batch(n, seed):
    rng = np.random.default_rng(seed)
    s6 = rng.random((n, 6)).astype(np.float32)
    w = rng.integers(0, 2, (n, 3, 15, 15)).astype(np.float32)
    a = rng.integers(0, 4, n).astype(np.int64)
    r = rng.choice(REWARDS, n).astype(np.float64)
    s6n = rng.random((n, 6)).astype(np.float32)
    wn = rng.integers(0, 2, (n, 3, 15, 15)).astype(np.float32)
    return s6, w, a, r, s6n, wn


def pack_windows(w):
    """[n, 3, 15, 15] of 0 / 1 -> packed int32 [n, 22] (element j = bit j % 32 of word j // 32:
    the replay's storage, what the HIP stem reads)."""
    x = torch.as_tensor(np.asarray(w)).reshape(len(w), -1).to(torch.int64)
    x = torch.cat((x, x.new_zeros(x.shape[0], 22 * 32 - x.shape[1])), 1).view(-1, 22, 32)
    words = (x << torch.arange(32)).sum(-1)
    return (words - ((words >> 31) << 32)).to(torch.int32)  # two's complement of bit 31


def head_case(H, b, act, missing_action=None):
    """Random head + loss inputs (f32 / int64 numpy): z2 ~ N(0, 1) for the source's [2b, H] stacked
    rows and the target's [b, H]; W3, b3 uniform in +-1/sqrt(H); actions cover all four values
    (but `missing_action`, which then never occurs); rewards from REWARDS."""
    rng = np.random.default_rng(1000 * H + 10 * b + act)
    z2s = rng.standard_normal((2 * b, H)).astype(np.float32)
    z2t = rng.standard_normal((b, H)).astype(np.float32)
    k = 1.0 / np.sqrt(H)
    w3s, w3t = (rng.uniform(-k, k, (4, H)).astype(np.float32) for _ in range(2))
    b3s, b3t = (rng.uniform(-k, k, 4).astype(np.float32) for _ in range(2))
    action = rng.integers(0, 4, b).astype(np.int64)
    action[:4] = np.arange(4)[:b]
    if missing_action is not None:
        action[action == missing_action] = (missing_action + 1) % 4
    reward = rng.choice(REWARDS, b).astype(np.float32)
    return dict(H=H, b=b, act=act, z2s=z2s, w3s=w3s, b3s=b3s, z2t=z2t, w3t=w3t, b3t=b3t,
                action=action, reward=reward, gamma=0.7)


def special_head_cases():
    """Hand-made head + loss inputs whose every f32 operation but the last of a chain is exact
    (small dyadic values, gamma 0.5, b = 4 so norm = 0.5): the kernels' finite results are then the
    float64 model's rounded once. Each case: dict(name, H, b, act, dbl, z2s [2b, H], w3s, b3s, z2t
    [b, H], w3t, b3t, action, reward, gamma[, choice]) in f32 / int64 numpy arrays."""
    nan, inf = float("nan"), float("inf")
    f = lambda x: np.array(x, dtype=np.float32)  # noqa: E731
    out = []

    def eye(H, cols):  # W3[k] = unit vector of column cols[k]
        w = np.zeros((4, H), np.float32)
        for k, c in enumerate(cols):
            w[k, c] = 1.0
        return w

    def rows(H, spec):  # rows from {column: value} dicts
        z = np.zeros((len(spec), H), np.float32)
        for i, d in enumerate(spec):
            for c, v in d.items():
                z[i, c] = v
        return z
    H = 8
    # DDQN ties: q_n columns 1 and 2 are bit-equal everywhere (same weights and bias); row 0 ties
    # 1 == 2, row 1 ties 0 == 1 == 2, row 2 has a unique maximum 3, row 3 ties 0 == 3 above 1 == 2.
    # The target's columns 1 and 2 differ by 1 (its bias), so diff shows which one was taken.
    s_rows = [{0: 1, 1: 2, 3: 3}, {0: 2, 1: 1}, {1: 4, 3: 1}, {0: 3, 3: 2}]
    n_rows = [{0: 1, 1: 3}, {0: 2, 1: 2, 3: 1}, {1: 1, 3: 5}, {0: 4, 1: 1, 3: 4}]
    for act in (0, 1):
        out.append(dict(name=f"ties-act{act}", H=H, b=4, act=act, dbl=1,
                        z2s=rows(H, s_rows + n_rows), w3s=eye(H, [0, 1, 1, 3]),
                        b3s=f([0.5, 0.5, 0.5, 0.5]), z2t=rows(H, n_rows), w3t=eye(H, [0, 1, 1, 3]),
                        b3t=f([0, 0, 1, 0]), action=np.array([0, 1, 2, 3]),
                        reward=f([1.0, -1.0, 0.5, -0.5]), gamma=0.5, choice=[1, 0, 3, 0]))
    # zeros of both signs, one negative entry per row (LeakyReLU scales it, ReLU drops it), and in
    # the second group a NaN row, then +inf / -inf rows (inf * 0 = NaN in the other Q columns)
    # (row i takes action i; the one negative entry of a row is the only nonzero term of its
    # Q(s,a), so LeakyReLU's inexact slope meets one rounding only; s' / target rows are >= 0)
    zs = [{0: 0.0, 1: 3.0, 2: -0.0, 5: -2.0}, {0: -0.0, 1: -4.0, 3: 0.0}, {0: 1.0, 2: -0.0, 3: 0.0,
          6: -1.0}, {0: 0.5, 5: -0.0, 7: 0.0}]
    zn = [{1: -0.0, 2: 1.0}, {0: 2.0, 3: 0.0, 5: 4.0}, {2: -0.0, 6: 4.0, 7: 2.0}, {0: 0.0, 5: -0.0}]
    w_mix = np.zeros((4, H), np.float32)
    w_mix[0, [0, 2, 5]] = [1, 1, 1]
    w_mix[1, [1, 3]] = [2, -1]
    w_mix[2, [2, 6, 3]] = [-1, 1, 0.5]
    w_mix[3, [0, 5, 7]] = [4, 1, 0.25]
    for act in (0, 1):
        for dbl in (0, 1):
            base = dict(H=H, b=4, act=act, dbl=dbl, w3s=w_mix, b3s=f([0, 0, 0, 0]),
                        w3t=w_mix[::-1].copy(), b3t=f([1, 0, 0, 0]), action=np.array([0, 1, 2, 3]),
                        reward=f([0.5, -1.0, 1.0, 0.25]), gamma=0.5)
            out.append(dict(base, name=f"zeros-act{act}-dbl{dbl}", z2s=rows(H, zs + zn),
                            z2t=rows(H, zn)))
            bad = [dict(d) for d in zs]
            bad[1][3] = nan
            out.append(dict(base, name=f"nan-act{act}-dbl{dbl}", z2s=rows(H, bad + zn),
                            z2t=rows(H, zn)))
            bad = [dict(d) for d in zs]
            bad[2][6] = inf
            badn = [dict(d) for d in zn]
            badn[0][1] = inf
            badn[3][7] = -inf
            out.append(dict(base, name=f"inf-act{act}-dbl{dbl}", z2s=rows(H, bad + badn),
                            z2t=rows(H, zn)))
    # NaN in fc3's bias: whole Q columns are NaN, the first of them wins every argmax
    for act in (0, 1):
        out.append(dict(name=f"bias-nan-act{act}", H=H, b=4, act=act, dbl=1, z2s=rows(H, zs + zn),
                        w3s=w_mix, b3s=f([0, nan, 0, nan]), z2t=rows(H, zn), w3t=eye(H, [0, 1, 2, 3]),
                        b3t=f([0, 1, 2, 3]), action=np.array([0, 1, 2, 3]),
                        reward=f([0.5, -1.0, 1.0, 0.25]), gamma=0.5, choice=[1, 1, 1, 1]))
    # the Q rows of test_fused_q_loss_propagates_nan_like_torch as z2 rows under an identity W3
    # (H = 4). A NaN entry of z2 reaches all four Q columns (NaN * 0), so those rows arrive all-NaN.
    q = [[1., 2., 3., 4.], [0.5, nan, 0.1, 0.2], [1., 1., 1., 1.], [2., 0., 0., 0.]]
    qn = [[0., nan, 5., nan], [1., 2., 3., 4.], [nan, 0., 0., 0.], [3., 1., 9., 2.]]
    qt = [[1., nan, 3., 4.], [1., nan, 0., 0.], [5., 6., 7., 8.], [1., 2., 3., nan]]
    for act in (0, 1):
        for dbl in (0, 1):
            out.append(dict(name=f"qrows-act{act}-dbl{dbl}", H=4, b=4, act=act, dbl=dbl,
                            z2s=f(q + qn), w3s=eye(4, [0, 1, 2, 3]), b3s=f([0, 0, 0, 0]), z2t=f(qt),
                            w3t=eye(4, [0, 1, 2, 3]), b3t=f([0, 0, 0, 0]),
                            action=np.array([0, 2, 1, 3]), reward=f([0.5, -0.05, 1.0, 0.45]),
                            gamma=0.5))
    return out


def param_stats(net, grads=False):
    out = {}
    for name, p in sorted(net.named_parameters()):
        t = p.grad if grads else p.data
        out[name] = (float(t.double().sum()), float(t.double().abs().sum()))
    return out
