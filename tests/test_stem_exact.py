"""The learner's conv stem (csrc/mz_stem.hip: k_stem_fwd, k_stem_bwd, k_stem_reduce) through the
C ABI (mz_stem_forward, mz_stem_backward, mz_stem_backward_ex, mz_stem_workspace_floats) against
tests/stem_model.py, at the sizes where the launches change path: the forward's groups of 4 rows
and its 4,096-workgroup cap, the backward's chunks of 64 rows, the reduce's groups of 8 chunks
and its tail.

Bounds, none taken from a kernel's output (tests/stem_model.py derives them):
  tier A    dyadic weights: feat bit-equal, code byte-equal, every window compared.
  tier B    real weights: decided windows code-equal and feat within e_v; an undecided window
            names one of the model's candidates, with the exact keep bit, feat within that
            candidate's e_v (at most 0.1% of the windows: tests/test_stem_model.py).
  backward  dw, db and the partial workspace bit-equal to the ordered float32 model.

Memory: every output buffer is filled with a sentinel, padded to its pitch, given rows past n and
wrapped in guards (tests/test_ppo_exact.py's Buf); whatever the contract does not write must
still hold the sentinel. gfeat's pad columns hold NaN sentinels. Inputs are exactly n rows
between guards; every index handed to a kernel is inside its buffers."""
import functools

import numpy as np
import pytest
import torch

import stem_model as S
from test_ppo_exact import DEV, Buf, _dev, _lib, _stream

pytestmark = pytest.mark.gpu
KEY, SALT = (0x5A17 << 32) | 0x9ABCDEF1, 0x3C6EF372  # the counter's high half is not zero
P_TINY, P_ALL = 2.0 ** -18, 0.999995  # thresh 0 (nothing can drop) and 65,536 (everything drops)
EXTRA = 2  # rows allocated past n in every output: must keep their sentinel
IN_DIM = S.FEAT + 6


@functools.lru_cache(maxsize=None)
def _bits(n, density=0.5):
    return S.edge_windows(n, 7, density)


@functools.lru_cache(maxsize=None)
def _weights(tier):
    return S.dyadic_weights(2) if tier == "A" else S.qnet_conv(float(tier[1:]))


def _obs(n):
    return np.random.default_rng(11).uniform(-1, 1, (n, 6)).astype(np.float32)


def _forward(bits, n, w, b, p, ld, want_code, key=KEY, salt=SALT, rng=True):
    """mz_stem_forward on the first n rows -> rc, feat Buf, code Buf (or None), obs6, rng Buf."""
    N, L = _lib()
    obs = _obs(n)
    din = [Buf(np.uint32, n, S.WW, data=bits[:n].view(np.uint32)), Buf(np.float32, n, 6, data=obs),
           Buf(np.float32, 32, 27, data=w), Buf(np.float32, 32, data=b)]
    feat = Buf(np.float32, n + EXTRA, IN_DIM, ld=max(ld, IN_DIM))
    code = Buf(np.uint8, n + EXTRA, S.FEAT) if want_code else None
    ctr = Buf(np.int64, 1, data=[key])
    rc = L.mz_stem_forward(din[0].ptr, din[1].ptr, n, din[2].ptr, din[3].ptr, p,
                           ctr.ptr if rng else None, salt, feat.ptr, ld,
                           code.ptr if want_code else None, _stream())
    torch.cuda.synchronize()
    assert all(x.same() for x in din) and ctr.same()  # inputs and the counter are only read
    return rc, feat, code, obs


def _rows_mask(n, width):
    m = np.zeros((n + EXTRA, width), bool)
    m[:n] = True
    return m


def _pad_rows(x, width, dtype):
    out = np.zeros((x.shape[0] + EXTRA, width), dtype)
    out[:x.shape[0]] = x
    return out


def _backward(bits, code, g, ld, n, p, mode):
    """mz_stem_backward (mode "plain") / _ex with a NULL ("null") or a real ("counter") counter
    -> rc, dw, db, partial Bufs, counter Buf. g: [n, 1568]; pad columns hold NaN sentinels."""
    N, L = _lib()
    din = [Buf(np.uint32, n, S.WW, data=bits[:n].view(np.uint32)),
           Buf(np.uint8, n, S.FEAT, data=code[:n]), Buf(np.float32, n, S.FEAT, ld=max(ld, S.FEAT), data=g[:n])]
    wsn = L.mz_stem_workspace_floats(n)
    assert wsn == S.chunks_of(n) * 32 * 28
    part = Buf(np.float32, wsn)
    dw, db = Buf(np.float32, 32, 27), Buf(np.float32, 32)
    ctr = Buf(np.int64, 1, data=[KEY])
    args = (din[0].ptr, din[1].ptr, din[2].ptr, ld, n, p, part.ptr, dw.ptr, db.ptr)
    if mode == "plain":
        rc = L.mz_stem_backward(*args, _stream())
    else:
        rc = L.mz_stem_backward_ex(*args, ctr.ptr if mode == "counter" else None, _stream())
    torch.cuda.synchronize()
    assert all(x.same() for x in din)
    return rc, dw, db, part, ctr


def _check_backward(tag, bits, code, g, ld, n, p, mode):
    rc, dw, db, part, ctr = _backward(bits, code, g, ld, n, p, mode)
    assert rc == 0
    mdw, mdb, mpart = S.backward(bits, code, g, S.FEAT, n, S.drop_scale(p))
    bad = int((part.host().view(np.int32) != mpart.reshape(-1, 1).view(np.int32)).sum()) if n else 0
    print(f"  {tag}: n {n} chunks {S.chunks_of(n)} ld {ld} p {p:g} {mode}: partials differing {bad},"
          f" max |dw| {np.abs(mdw).max():.3g}")
    assert part.same(mpart), "partials"
    assert dw.same(mdw) and db.same(mdb), "dw / db"
    assert ctr.same([KEY + 1] if mode == "counter" else None), "counter"


# ---- tier A: everything bit-equal ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_a(p):
    return S.forward_lean(_bits(128), *_weights("A"), p, KEY, SALT)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65])
def test_forward_dyadic_is_bit_equal(n):
    """All four (DROP, CODE) instantiations, feat at both pitches; p = 2^-18 must be the stem
    without dropout, p = 0.999995 must drop everything (idx 0, class 0, a zero feature)."""
    w, b = _weights("A")
    bits = _bits(128)
    for p, ld, want_code in ((0.0, 1574, True), (0.0, 1600, False), (0.2, 1600, True),
                             (0.2, 1574, False), (P_TINY, 1574, True), (P_ALL, 1600, True)):
        mf, mc = _model_a(p)
        rc, feat, code, obs = _forward(bits, n, w, b, p, ld, want_code)
        assert rc == 0
        exp = _pad_rows(np.concatenate([mf[:n], obs], 1), IN_DIM, np.float32)
        got = feat.host()[:n, :S.FEAT]
        print(f"  n {n} p {p:g} ld {ld} code {want_code}: feat bits differing"
              f" {int((got.view(np.int32) != mf[:n].view(np.int32)).sum())} of {n * S.FEAT}")
        assert feat.same(exp, _rows_mask(n, IN_DIM)), (p, ld)  # bit-equal; pads, rows >= n, guards
        if want_code:
            assert code.same(_pad_rows(mc[:n], S.FEAT, np.uint8), _rows_mask(n, S.FEAT)), (p, ld)
        if p == P_TINY:
            assert np.array_equal(mf.view(np.int32), _model_a(0.0)[0].view(np.int32))
        if p == P_ALL and n:
            assert not code.host()[:n].any() and not got.any()  # +-0 everywhere
        if p == 0.0 and n >= 4:  # garbage in the pad bits 675..703 (row 2) changes nothing (row 3)
            assert np.array_equal(got[2].view(np.int32), got[3].view(np.int32))
            assert not want_code or np.array_equal(code.host()[2], code.host()[3])


def test_forward_past_the_workgroup_cap():
    """n = 16,389: 4,098 groups of 4 rows on the 4,096 workgroups the launch is capped at, so
    workgroups 0 and 1 take a second group (rows 16,384..16,388); dropout and code on, tier A.
    The model runs in blocks of 512 rows (the windows repeat with that period, the draws do not);
    everything is compared on the device, pads, rows past n and guards included."""
    n, blk, ld = 16389, 512, 1600
    w, b = _weights("A")
    base = _bits(512)
    bits = np.concatenate([base] * (n // blk + 1))[:n]
    rc, feat, code, obs = _forward(bits, n, w, b, 0.2, ld, True)
    assert rc == 0
    tables = S._conv_tables(base, w, b)
    ef = torch.from_numpy(feat.init.copy()).to(DEV)
    ec = torch.from_numpy(code.init.copy()).to(DEV)
    G = 64  # test_ppo_exact.GUARD
    efb = ef[G:G + (n + EXTRA) * ld].view(n + EXTRA, ld)
    ecb = ec[G:G + (n + EXTRA) * S.FEAT].view(n + EXTRA, S.FEAT)
    for r0 in range(0, n, blk):
        m = min(blk, n - r0)
        tb = tables if m == blk else S._conv_tables(base[:m], w, b)
        mf, mc = S.forward_lean(base[:m], w, b, 0.2, KEY, SALT, row0=r0, tables=tb)
        efb[r0:r0 + m, :S.FEAT] = _dev(mf.view(np.int32))
        ecb[r0:r0 + m] = _dev(mc)
    efb[:n, S.FEAT:IN_DIM] = _dev(obs.view(np.int32))
    dfeat = int((feat.t != ef).sum())
    dcode = int((code.t != ec).sum())
    tail = int((feat.t[G:].view(-1)[16384 * ld:n * ld] != ef[G:].view(-1)[16384 * ld:n * ld]).sum())
    print(f"  n {n}: feat words differing {dfeat} (rows >= 16384: {tail}), code bytes differing {dcode}")
    assert dfeat == 0 and dcode == 0


# ---- tier B: real weights ------------------------------------------------------------------------
TIER_B = [(dens, scale, p) for dens in (0.5, 0.08) for scale in (1.0, 3.0) for p in (0.0, 0.2)]


@pytest.mark.parametrize("density,scale,p", TIER_B)
def test_forward_real_weights_within_the_derived_bound(density, scale, p):
    n = 512
    bits = _bits(n, density)
    w, b = _weights(f"B{scale}")
    d = S.forward_detail(bits, w, b, p, KEY, SALT)
    rc, feat, code, obs = _forward(bits, n, w, b, p, 1574, True)
    assert rc == 0
    assert feat.untouched_outside(_rows_mask(n, IN_DIM)) and code.untouched_outside(_rows_mask(n, S.FEAT))
    assert np.array_equal(feat.host()[:n, S.FEAT:].view(np.int32), obs.view(np.int32))
    kf, kc = feat.host()[:n, :S.FEAT].astype(np.float64), code.host()[:n]
    kidx, kcls = (kc & 3).astype(np.int64)[:, :, None], kc >> 2
    at = lambda x: np.take_along_axis(x, kidx, 2)[:, :, 0]  # noqa: E731
    und = d["undecided"]
    err, e_v = np.abs(kf - at(d["v64"])), at(d["e_v"])
    ratio = np.where(e_v > 0, err / np.where(e_v > 0, e_v, 1), 0)
    print(f"  density {density} x{scale} p {p}: windows {und.size} undecided {und.sum()}"
          f" ({100 * und.mean():.4f}%) code mismatches on decided {(kc != d['code'])[~und].sum()}"
          f" on undecided {(kc != d['code'])[und].sum()} largest e_k/e_v {ratio.max():.4f}"
          f" (decided {ratio[~und].max():.4f})")
    assert np.array_equal(kc[~und], d["code"][~und])            # decided: the model's byte
    assert (kc <= 11).all() and at(d["cand"]).all()             # any window: one of the candidates
    assert np.array_equal(kcls == 0, ~at(d["keep"]))            # the keep bit is an integer: exact
    sure = at(d["sure"])
    assert np.array_equal(kc[sure], at(d["codes4"])[sure])      # class certain: that position's byte
    assert np.all(err <= e_v)                                   # feat within e_v of the named position
    assert und.mean() <= 1e-3


# ---- backward on its own -------------------------------------------------------------------------
def _codes(n, kind):
    rng = np.random.default_rng(17)
    if kind == "twelve":  # all twelve valid bytes; some rows of class 0 only
        c = (rng.integers(0, 4, (n, S.FEAT)) | (rng.integers(0, 3, (n, S.FEAT)) << 2)).astype(np.uint8)
        c[1::7] &= 3
        return c
    c = S.forward_lean(_bits(128), *_weights("B3.0"), 0.2, KEY, SALT)[1]
    return np.concatenate([c] * (n // 128 + 1))[:n]


def _g(n):
    return np.random.default_rng(23).standard_normal((n, S.FEAT)).astype(np.float32)


def _many_bits(n):
    return np.concatenate([_bits(512)] * (n // 512 + 1))[:n]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 448, 449, 513, 1025])
def test_backward_is_the_ordered_float32_model(n):
    """Chunk counts 0, 1, 2, 7, 8, 9, 17: the reduce's unrolled groups of 8 and its tail. n = 0:
    dw / db zeroed, the counter advanced, nothing else written. gfeat at its three pitches."""
    bits, g = _many_bits(max(n, 1)), _g(n)
    for kind, ld, p, mode in (("twelve", 1568, 0.2, "plain"), ("model", 1574, 0.0, "counter"),
                              ("twelve", 1600, P_TINY, "null"), ("model", 1568, 0.2, "counter")):
        _check_backward(kind, bits, _codes(n, kind), g, ld, n, p, mode)


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_backward_integer_gradients_equal_the_integer_sum(p):
    """Order-independent: g a multiple of 4 (x 1.25 at p = 0.2: still an integer), classes 0 / 1
    only, so every partial sum is an integer below 2^24 and the float32 result is THE sum."""
    n = 449
    rng = np.random.default_rng(29)
    bits = _many_bits(n)
    code = (rng.integers(0, 4, (n, S.FEAT)) | (rng.integers(0, 2, (n, S.FEAT)) << 2)).astype(np.uint8)
    gi = 4 * rng.integers(-8, 9, (n, S.FEAT))
    rc, dw, db, part, _ = _backward(bits, code, gi.astype(np.float32), 1574, n, p, "plain")
    assert rc == 0
    gc = np.where(code >> 2 == 1, gi * 5 // 4 if p else gi, 0)
    pw = S.patch_words(bits)
    q = np.arange(S.FEAT) % 49
    sel = pw[np.arange(n)[:, None], 2 * (q // 7) + ((code >> 1) & 1), 2 * (q % 7) + (code & 1)]
    gc3, sel3 = gc.reshape(n, 32, 49), sel.reshape(n, 32, 49).astype(np.int64)
    idw = np.stack([(gc3 * ((sel3 >> k) & 1)).sum((0, 2)) for k in range(27)], 1)
    idb = gc3.sum((0, 2))
    assert np.abs(gc).sum() < 2 ** 24
    print(f"  p {p}: max |dw| {np.abs(idw).max()} max |db| {np.abs(idb).max()}")
    assert dw.same(idw.astype(np.float32)) and db.same(idb.astype(np.float32))


# ---- end to end ----------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2, P_TINY])
def test_forward_then_backward_on_the_kernels_own_code(p):
    """Real weights; the backward model is fed the code bytes the kernel wrote, so no window is
    excused, and the gradients must be bit-equal. p = 2^-18: forward and backward both run the
    stem without dropout (scale 1)."""
    n = 193
    bits = _bits(512)[:n]
    w, b = _weights("B3.0")
    rc, feat, code, _ = _forward(bits, n, w, b, p, 1574, True)
    assert rc == 0
    kc = code.host()[:n]
    mf, mc, und = S.forward(bits, w, b, p, KEY, SALT)
    assert np.array_equal(kc[~und], mc[~und])
    _check_backward("own code", bits, kc, _g(n), 1574, n, p, "counter")


# ---- refusals ------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    n = 5
    w, b = _weights("A")
    bits = _bits(128)
    for p, ld, rng in ((0.0, 1573, True), (0.0, 1568, True), (-0.1, 1574, True), (1.0, 1574, True),
                       (float("nan"), 1574, True), (0.2, 1574, False), (P_TINY, 1574, False)):
        rc, feat, code, _ = _forward(bits, n, w, b, p, ld, True, rng=rng)
        assert rc == -1, (p, ld, rng)  # MZ_EINVAL
        assert feat.same() and code.same(), (p, ld, rng)
    code, g = _codes(n, "twelve"), _g(n)
    for p, ld in ((0.0, 1567), (0.2, 0), (-0.1, 1568), (1.0, 1568), (float("nan"), 1574)):
        for mode in ("plain", "counter"):
            rc, dw, db, part, ctr = _backward(bits, code, g, ld, n, p, mode)
            assert rc == -1, (p, ld, mode)
            assert dw.same() and db.same() and part.same() and ctr.same(), (p, ld, mode)
