"""tests/stem_model.py anchored before the GPU tests (tests/test_stem_exact.py) trust it: against
the torch float64 pipeline of tests/test_stem.py with autograd, against that file's mask
generator, and against itself (ordered float32 backward vs the float64 sum; every mutation must
show). CPU only.

Bounds (u = 2^-24, gamma_k = k u / (1 - k u)), none taken from an output:
  forward   model v64 vs torch float64: the model multiplies by 0.01f and by the float32 scale,
            torch by 0.01 and 1 / (1 - p) in float64: each within u / 2 relative -> u |v|
            (+ 1e-12 for float64 rounding); model float32 feat vs v64: 3 u |v| (three roundings:
            a, x 0.01f, x scale).
  backward  backward64 (float32 terms gc = (g * scale) * 0.01f) vs torch float64 autograd: two
            float32 roundings and the two constants per term -> gamma_4 sum |gc|.
  ordered   float32 backward vs backward64: any order of float32 additions over N leaves is within
            gamma_(N-1) sum |gc|, N <= 49 n per output.
"""
import functools

import numpy as np
import pytest
import torch

import stem_model as S
import test_stem as T

KEY, SALT = (0x5A17 << 32) | 0x9ABCDEF1, 0x3C6EF372


@functools.lru_cache(maxsize=None)
def _bits(n, density):
    return S.edge_windows(n, 7, density)


class _Net:
    """what test_stem._torch_stem reads: net.conv[0], float64"""

    def __init__(self, w, b):
        c = torch.nn.Conv2d(3, 32, 3, padding=1).double()
        with torch.no_grad():
            c.weight.copy_(torch.from_numpy(w.astype(np.float64)).view(32, 3, 3, 3))
            c.bias.copy_(torch.from_numpy(b.astype(np.float64)))
        self.conv = [c]


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_model_matches_torch_float64_on_decided_windows(scale, p):
    n = 96
    bits = _bits(128, 0.5)[:n]
    w, b = S.qnet_conv(scale)
    d = S.forward_detail(bits, w, b, p, KEY, SALT)
    net = _Net(w, b)
    win = torch.from_numpy(S.window(bits).astype(np.float64))
    keep = torch.from_numpy(S.keep_masks(n, KEY, SALT, p).astype(np.float64)) if p else None
    pf = float(np.float32(p))
    ft = T._torch_stem(net, torch.zeros(n, 6, dtype=torch.float64), win, keep, pf)
    ref = ft.detach().numpy()[:, :S.FEAT]
    dec = ~d["undecided"]
    idx = (d["code"] & 3).astype(np.int64)[:, :, None]
    v64 = np.take_along_axis(d["v64"], idx, 2)[:, :, 0]
    e_v = np.take_along_axis(d["e_v"], idx, 2)[:, :, 0]
    assert dec.mean() > 0.999
    assert np.all(np.abs(ref - v64)[dec] <= (S.U * np.abs(v64) + 1e-12)[dec])
    assert np.all(np.abs(d["feat"].astype(np.float64) - v64) <= 3 * S.U * np.abs(v64))
    assert np.all(3 * S.U * np.abs(v64) <= e_v + 1e-300)
    # backward, on the rows whose every window is decided (torch routes by its own float64 max)
    rows = np.flatnonzero(dec.all(1))
    assert len(rows) >= n // 2
    g = np.zeros((n, S.FEAT), np.float32)
    g[rows] = np.random.default_rng(3).standard_normal((len(rows), S.FEAT)).astype(np.float32)
    gt = torch.autograd.grad((ft[:, :S.FEAT] * torch.from_numpy(g.astype(np.float64))).sum(),
                             [net.conv[0].weight, net.conv[0].bias])
    dw64, db64, asum = S.backward64(bits, d["code"], g, S.FEAT, n, d["scale"])
    tol = S.gamma(4) * asum + 1e-12
    assert np.all(np.abs(gt[0].numpy().reshape(32, 27) - dw64) <= tol[:, :27])
    assert np.all(np.abs(gt[1].numpy() - db64) <= tol[:, 27])
    assert np.abs(dw64).max() > 1.0


def test_keep_masks_are_test_stem_masks_and_share_qact_rules():
    """The same bits as tests/test_stem.py's generator, keys with a non-zero high half included.
    The acting forward (tests/qact_model.py) draws from another generator (an xorshift stream per
    row and channel pair), so its masks are not these; what the two share is the lowbias32 hash
    and the threshold rule, and those must agree."""
    import qact_model as Q
    for n, key, salt, p in ((5, 0x123456789AB, 7, 0.2), (3, (0xFFFFFFFF << 32) | 0xFFFFFFFE, 0xFFFFFFFF, 0.2),
                            (4, 0, 0, 0.5), (2, KEY, SALT, 0.999995), (2, KEY, SALT, 2.0 ** -18)):
        ours = S.keep_masks(n, key, salt, p)
        assert np.array_equal(ours, T._masks(n, key, salt, p) > 0), (key, salt, p)
    assert S.keep_masks(2, KEY, SALT, 2.0 ** -18).all()
    assert not S.keep_masks(2, KEY, SALT, 0.999995)[:, :, :14, :14].any()
    # rows are independent of n (the GPU tests evaluate the model in row blocks)
    assert np.array_equal(S.keep4(3, KEY, SALT, 0.2, row0=16386), S.keep4(16389, KEY, SALT, 0.2)[16386:])
    x = np.arange(0, 2 ** 32, 65521, dtype=np.uint64)
    assert np.array_equal(S._hash32(x), Q._lowbias32(x))
    for p in (0.0, 0.2, 0.5, 2.0 ** -18, 2.0 ** -17, 0.999995, 13107 / 65536):
        assert S.drop_thresh(p) == (Q.drop_thresh(p) if p > 0 else 0)
    assert (S.drop_thresh(0.2), S.drop_thresh(2.0 ** -18), S.drop_thresh(0.999995)) == (13107, 0, 65536)
    assert S.drop_scale(2.0 ** -18) == 1.0 and S.drop_scale(0.2) == np.float32(1.25)


@pytest.mark.parametrize("n", [65, 449])
def test_ordered_float32_backward_is_within_the_order_free_bound(n):
    bits = _bits(512, 0.5)[:n]
    w, b = S.qnet_conv(3.0)
    _, code, _ = S.forward(bits[:64], w, b, 0.2, KEY, SALT)
    code = np.concatenate([code] * 8)[:n]  # any valid code bytes do: the backward takes them as data
    g = np.random.default_rng(5).standard_normal((n, S.FEAT)).astype(np.float32)
    scale = S.drop_scale(0.2)
    dw, db, part = S.backward(bits, code, g, S.FEAT, n, scale)
    dw64, db64, asum = S.backward64(bits, code, g, S.FEAT, n, scale)
    assert part.shape == (S.chunks_of(n), 32, 28) and dw.dtype == np.float32
    bound = S.gamma(49 * n) * asum
    assert np.all(np.abs(dw - dw64) <= bound[:, :27]) and np.all(np.abs(db - db64) <= bound[:, 27])
    assert np.abs(dw - dw64).max() > 0  # the order is felt: a float32 sum, not the float64 one
    # the chunks are summed in ascending order from 0.0f
    s = np.zeros((32, 28), np.float32)
    for c in range(part.shape[0]):
        s = s + part[c]
    assert np.array_equal(s[:, :27], dw) and np.array_equal(s[:, 27], db)


def test_every_mutation_changes_the_model():
    bits = _bits(128, 0.5)
    for w, b in (S.dyadic_weights(2), S.qnet_conv(3.0)):
        feat, code, _ = S.forward(bits, w, b, 0.2, KEY, SALT)
        for m in S.FWD_MUTATIONS:
            f2, c2, _ = S.forward(bits, w, b, 0.2, KEY, SALT, mutate=m)
            assert not np.array_equal(code, c2), m
        # only the mask rule shows in the features (the other two move the argmax among equals)
        assert not np.array_equal(feat, S.forward(bits, w, b, 0.2, KEY, SALT, mutate="thresh_gt")[0])
    g = np.random.default_rng(1).standard_normal((128, S.FEAT)).astype(np.float32)
    dw, db, part = S.backward(bits, code, g, S.FEAT, 128, S.drop_scale(0.2))
    for m, n in (("cls2_no_slope", 128), ("bwd_limit_row", 64), ("bwd_limit_row", 128)):
        d2 = S.backward(bits[:n], code[:n], g[:n], S.FEAT, n, S.drop_scale(0.2), mutate=m)
        d0 = S.backward(bits[:n], code[:n], g[:n], S.FEAT, n, S.drop_scale(0.2))
        assert not np.array_equal(d0[0], d2[0]) and not np.array_equal(d0[1], d2[1]), m
    # reduce_no_tail: visible at every chunk count that is no multiple of 8 (7, 9, 17; not 8)
    n = 9 * 64
    bb, cc, gg = (np.concatenate([x] * 5)[:n] for x in (bits, code, g))
    for k in (7, 8, 9):
        d0 = S.backward(bb, cc, gg, S.FEAT, k * 64, 1.0)
        d2 = S.backward(bb, cc, gg, S.FEAT, k * 64, 1.0, mutate="reduce_no_tail")
        assert np.array_equal(d0[0], d2[0]) == (k == 8), k


def test_a_draw_equal_to_the_threshold_is_kept():
    """thresh_gt differs from the kernel's rule only on draws equal to thresh: the shared dropout
    case must hold some (or no test could tell the two rules apart)."""
    u = S.draws(128, KEY, SALT)
    assert (u == S.drop_thresh(0.2)).sum() >= 4


TIER_B = [(dens, scale, p) for dens in (0.5, 0.08) for scale in (1.0, 3.0) for p in (0.0, 0.2)]


@pytest.mark.parametrize("density,scale,p", TIER_B)
def test_tier_b_inputs_leave_at_most_one_window_in_a_thousand_undecided(density, scale, p):
    bits = _bits(512, density)
    w, b = S.qnet_conv(scale)
    _, _, und = S.forward(bits, w, b, p, KEY, SALT)
    print(f"density {density} x{scale} p {p}: undecided {und.sum()} of {und.size} ({100 * und.mean():.4f}%)")
    assert und.mean() <= 1e-3


def test_tier_a_weights_are_exact_in_float32():
    """Every partial sum of the dyadic weights is a multiple of 2^-6 below 2^5 (exact in float32
    in any order), and the windows produce ties in bulk: equal maxima from different patches."""
    w, b = S.dyadic_weights(2)
    assert np.array_equal(w * 64, np.round(w * 64)) and np.abs(w).max() <= 1 and np.abs(b).max() <= 1
    assert not (np.signbit(b) & (b == 0)).any()  # no -0 bias: the sign of a zero sum would depend on the order
    d = S.forward_detail(_bits(128, 0.5), w, b, 0.2, KEY, SALT)
    assert np.array_equal(d["a64"], d["a64"].astype(np.float32).astype(np.float64))
    v = d["v32"]
    ties = (v == v.max(2, keepdims=True)).sum(2) > 1
    print(f"tier A: {ties.sum()} of {ties.size} windows with an exact tie for the maximum")
    assert ties.mean() > 0.02
    assert (d["code"] >> 2 == 0).any() and (d["code"] >> 2 == 2).any()
