"""An exact CPU model of the learner's conv stem (csrc/mz_stem.hip: k_stem_fwd, k_stem_bwd,
k_stem_reduce), its dropout masks and the windows the CPU and GPU tests share. CPU only: numpy
on the host, no library call.

Forward. The window is binary, so a conv output is b[c] + the sum of the weights whose patch bit
is set. `conv_exact` evaluates that once per DISTINCT 27-bit patch word in float64 (identical
patches give identical values, as they do in the kernel, whose MFMA chain sees only the patch
word), together with the magnitude |b| + sum bit_k |w_k| every rounding bound is stated in.
LeakyReLU, dropout and the 2x2 max then follow the kernel operation for operation in float32:
a > 0 ? a : a * 0.01f, (x * keep) * scale, the first strict maximum in (0,0) (0,1) (1,0) (1,1)
order from -inf, code byte idx | cls << 2 (cls 0 dropped, 1 kept and a > 0, 2 kept and a <= 0).

Two tiers of weights:
  A  dyadic: weights and bias multiples of 2^-6 in [-1, 1]. Every partial sum of at most 28 such
     terms is a multiple of 2^-6 below 2^5: exact in float32 in ANY order, the MFMA's included.
     The kernel's feat must equal the model's bit for bit, its code byte for byte.
  B  real weights. With u = 2^-24 and gamma_k = k u / (1 - k u), a float32 sum of 28 terms in any
     order (each addition rounded once, fused or not) is within
         e_a = gamma_28 (|b| + sum bit_k |w_k|)
     of the exact sum, and the two float32 products that follow (x 0.01f, x scale) move the
     feature by at most 2 u |v| more (+ second-order terms; 3 u |v| covers them):
         e_v = scale e_a + 3 u |v|,         v the float64 value of the feature position
     (a dropped position is +-0 exactly: e_v = 0). A position can be the pool's maximum when
     v + e_v >= max_s (v_s - e_v,s). Positions with the same patch word and the same keep bit
     hold the same float32 value in the kernel, so of such a group only the lowest index can win
     (strict >). A window is DECIDED when one candidate is left and, if it is kept, its
     |a| > e_a (its gradient class is then certain too).

Backward. The build uses -ffp-contract=off, and every addition of k_stem_bwd / k_stem_reduce is
written out in the source, so the float32 result is a fixed function of the inputs:
`backward` repeats it addition for addition — per (chunk of 64 rows, channel) thread tid's
items i = tid + 256 u, u = 0..12, then the xor butterfly 32, 16, .., 1 over each wave's 64 lanes,
then ((r0 + r1) + r2) + r3 over the 4 waves, then the chunks in ascending order from 0.0f — and
returns the [chunks][32][28] partials too. `backward64` sums the same float32 terms gc in
float64 (no order).

MUTATIONS: defects a rework of the kernels could plausibly have; each must change the model's
output on the shared cases (tests/test_stem_model.py) and, applied to the kernels, fail a GPU
test (tests/test_stem_exact.py):
  last_max        the pool keeps the LAST maximum (v >= m)
  thresh_gt       kept iff u > thresh (a draw equal to thresh dropped)
  code_yx_swap    the argmax's y and x bits swapped in the code byte
  cls2_no_slope   the backward forgets the 0.01 of class 2 (kept, a <= 0)
  reduce_no_tail  k_stem_reduce drops the chunks after its last full group of 8
  bwd_limit_row   k_stem_bwd's item limit one chunk row short: i < (CHUNK - 1) * NPOOL
"""
import numpy as np

FEAT, NPOOL, NACC, CHUNK, WW = 1568, 49, 28, 64, 22
U = 2.0 ** -24
MUTATIONS = ("last_max", "thresh_gt", "code_yx_swap", "cls2_no_slope", "reduce_no_tail",
             "bwd_limit_row")
FWD_MUTATIONS, BWD_MUTATIONS = MUTATIONS[:3], MUTATIONS[3:]
SLOPE = np.float32(0.01)
M32 = np.uint64(0xFFFFFFFF)


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


# ---- windows ------------------------------------------------------------------------------------
def pack(win, pad_garbage=None):
    """bool [n, 3, 15, 15] (or [n, 675]) -> int32 [n, 22]; rows listed in pad_garbage get the pad
    bits 675..703 of word 21 set."""
    w = np.asarray(win).reshape(len(win), 675)
    padded = np.zeros((w.shape[0], 704), np.uint64)
    padded[:, :675] = w
    if pad_garbage is not None:
        padded[np.asarray(pad_garbage, int), 675:] = 1
    words = (padded.reshape(-1, WW, 32) << np.arange(32, dtype=np.uint64)).sum(2)
    return np.ascontiguousarray(words.astype(np.uint32).view(np.int32))


def window(bits):
    """int32 / uint32 [n, 22] -> uint8 [n, 3, 15, 15]; pad bits 675..703 ignored."""
    b = np.ascontiguousarray(np.asarray(bits)).view(np.uint32).reshape(-1, WW)
    i = np.arange(675)
    return ((b[:, i // 32] >> (i % 32).astype(np.uint32)) & 1).astype(np.uint8).reshape(-1, 3, 15, 15)


def patch_words(bits):
    """uint32 [n, 15, 15]: bit k = ch*9 + ky*3 + kx (torch's weight order) of the word at (y, x)
    is window[ch][y + ky - 1][x + kx - 1], 0 outside the window (zero padding)."""
    w = window(bits)
    p = np.zeros((w.shape[0], 3, 17, 17), np.uint32)
    p[:, :, 1:16, 1:16] = w
    pw = np.zeros((w.shape[0], 15, 15), np.uint32)
    for ch in range(3):
        for ky in range(3):
            for kx in range(3):
                pw |= p[:, ch, ky:ky + 15, kx:kx + 15] << np.uint32(ch * 9 + ky * 3 + kx)
    return pw


def pool_order(x):
    """[n, 15, 15, ...] per conv position -> [n, 49, 4, ...]: pooled q = 7 py + px, 2x2 position
    r = 2 dy + dx (row and column 14 are never pooled)."""
    x = x[:, :14, :14]
    s = x.shape
    x = x.reshape(s[0], 7, 2, 7, 2, *s[3:])
    x = np.moveaxis(x, 2, 3)  # n, py, px, dy, dx
    return x.reshape(s[0], NPOOL, 4, *s[3:])


def edge_windows(n, seed, density=0.5):
    """int32 [n, 22], n >= 64. Random windows at `density`, and from row 0 on: all-zero, all-one,
    row 3 with garbage in the pad bits 675..703 (row 2), row 3, then a single bit at each corner
    and edge midpoint of each channel (24 rows: the conv's zero padding), then a window of
    identical 2x2 tiles and one of full rows (identical patches inside a pool window: ties)."""
    assert n >= 64
    rng = np.random.default_rng(seed)
    w = rng.random((n, 3, 15, 15)) < density
    w[0], w[1] = False, True
    w[2] = w[3]
    k = 4
    for ch in range(3):
        for y, x in ((0, 0), (0, 14), (14, 0), (14, 14), (0, 7), (7, 0), (14, 7), (7, 14)):
            w[k] = False
            w[k, ch, y, x] = True
            k += 1
    yy, xx = np.meshgrid(np.arange(15), np.arange(15), indexing="ij")
    w[k] = (yy % 2 == 0) & (xx % 2 == 1)
    w[k + 1] = (yy % 4 < 2)
    return pack(w, pad_garbage=[2])


def dyadic_weights(seed):
    """Tier A: w [32, 27], b [32] float32, multiples of 2^-6 in [-1, 1]; a few equal and opposite
    weights and zero biases so that different patches tie and sums hit exactly 0."""
    rng = np.random.default_rng(seed)
    w = (rng.integers(-64, 65, (32, 27)) / 64.0).astype(np.float32)
    b = (rng.integers(-64, 65, 32) / 64.0).astype(np.float32)
    w[0, :] = np.float32(0.25)          # every patch with the same popcount ties
    w[1, 1::2] = -w[1, 0:26:2]          # sums cancel to exactly 0
    b[1] = 0.0
    w[2, :] = 0.0                       # a constant channel: all four positions tie
    w[3, :] = -np.abs(w[3, :])          # all a <= b: class 2 wherever b <= 0
    b[3] = 0.0
    return w, b


# ---- the conv, exactly --------------------------------------------------------------------------
def _conv_tables(bits, w, b):
    """inv int [n, 15, 15] into the distinct patch words, a_tab / mag_tab float64 [words, 32]."""
    w64 = np.asarray(w, np.float64).reshape(32, 27)
    b64 = np.asarray(b, np.float64).reshape(32)
    pw = patch_words(bits)
    words, inv = np.unique(pw, return_inverse=True)
    on = ((words[:, None] >> np.arange(27, dtype=np.uint32)) & 1).astype(np.float64)  # [W, 27]
    a = on @ w64.T + b64  # one row per distinct word: identical patches, identical values
    mag = on @ np.abs(w64).T + np.abs(b64)
    return pw, inv.reshape(pw.shape), a, mag


def conv_exact(bits, w, b):
    """a, mag: float64 [n, 32, 15, 15]. a = b[c] + sum_k bit_k w[c][k], evaluated once per distinct
    patch word; mag = |b[c]| + sum_k bit_k |w[c][k]|."""
    _, inv, a, mag = _conv_tables(bits, w, b)
    return np.moveaxis(a[inv], 3, 1), np.moveaxis(mag[inv], 3, 1)


# ---- dropout masks ------------------------------------------------------------------------------
def _hash32(x):  # lowbias32 (Wellons)
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def drop_thresh(p):
    """floor(p * 65536 + 0.5) in float32, as the launch computes it."""
    p = np.float32(p)
    return int(p * np.float32(65536.0) + np.float32(0.5)) if p > 0 else 0


def drop_scale(p):
    """1 / (1 - p) (float64 division, rounded to float32) when something can be dropped, else 1."""
    return np.float32(1.0 / (1.0 - float(np.float32(p)))) if drop_thresh(p) else np.float32(1.0)


def draws(n, key, salt, row0=0):
    """The 16-bit draws, uint32 [n, 1568, 4] (feature j = c*49 + q, 2x2 position r), of rows
    row0 .. row0 + n for the 64-bit counter value `key`."""
    key, salt = int(key) & ((1 << 64) - 1), int(salt) & 0xFFFFFFFF
    k0 = np.uint64((key & 0xFFFFFFFF) ^ ((salt * 0x9E3779B9) & 0xFFFFFFFF))
    k1 = np.uint64(((key >> 32) + int(_hash32(np.array([salt]))[0])) & 0xFFFFFFFF)
    nn = np.arange(row0, row0 + n, dtype=np.uint64)[:, None]
    j = np.arange(FEAT, dtype=np.uint64)[None, :]
    gid = (np.uint64(2) * (nn * np.uint64(FEAT) + j)) & M32  # uint32 arithmetic in the kernel
    h0 = _hash32((_hash32(gid ^ k0) + k1) & M32)
    h1 = _hash32((_hash32(((gid + np.uint64(1)) & M32) ^ k0) + k1) & M32)
    u = np.stack([h0 & np.uint64(0xFFFF), h0 >> np.uint64(16), h1 & np.uint64(0xFFFF),
                  h1 >> np.uint64(16)], axis=2)
    return u.astype(np.uint32)


def keep4(n, key, salt, p, row0=0, mutate=None):
    """bool [n, 1568, 4]: kept iff the draw >= thresh."""
    u = draws(n, key, salt, row0)
    t = drop_thresh(p)
    return u > t if mutate == "thresh_gt" else u >= t


def keep_masks(n, key, salt, p):
    """bool [n, 32, 15, 15] in window layout (row and column 14, never pooled: True)."""
    k4 = keep4(n, key, salt, p).reshape(n, 32, 7, 7, 2, 2)
    keep = np.ones((n, 32, 15, 15), bool)
    keep[:, :, :14, :14] = np.moveaxis(k4, 4, 3).reshape(n, 32, 14, 14)
    return keep


# ---- forward ------------------------------------------------------------------------------------
def forward_detail(bits, w, b, p=0.0, key=0, salt=0, row0=0, mutate=None, detail=True,
                   tables=None):
    """The model: feat (float32 [n, 1568]), code (uint8 [n, 1568]) and, with `detail`, everything
    the tier-B checks need, per feature j = c*49 + q and 2x2 position r ([n, 1568, 4]):
      a64, e_a   the exact conv value and its float32 any-order bound
      keep       the keep bits (all True without dropout)
      v32        the float32 value the max runs over;  v64 the same chain in float64;  e_v
      codes4     the code byte position r would get (uint8)
      cand       the positions that can win;  sure: the position's gradient class is certain
      undecided  bool [n, 1568] (module docstring)"""
    assert mutate is None or mutate in FWD_MUTATIONS
    bits = np.asarray(bits)
    n = bits.shape[0]
    pw, inv, a_tab, mag_tab = tables or _conv_tables(bits, w, b)
    inv4 = pool_order(inv)  # [n, 49, 4]

    def pooled(tab):  # [words, 32] -> [n, 1568, 4]
        return tab[inv4].transpose(0, 3, 1, 2).reshape(n, FEAT, 4)

    thresh, scale = drop_thresh(p), drop_scale(p)
    drop = thresh > 0
    keep = keep4(n, key, salt, p, row0, mutate) if drop else np.ones((n, FEAT, 4), bool)
    a32 = pooled(a_tab.astype(np.float32))
    lk = np.where(a32 > 0, a32, a32 * SLOPE)
    v32 = (lk * keep.astype(np.float32)) * scale if drop else lk
    cls4 = np.where(keep, np.where(a32 > 0, 1, 2), 0).astype(np.uint8)
    # the kernel's scan
    m = np.full((n, FEAT), -np.inf, np.float32)
    idx = np.zeros((n, FEAT), np.uint8)
    for r in range(4):
        win = v32[:, :, r] >= m if mutate == "last_max" else v32[:, :, r] > m
        m = np.where(win, v32[:, :, r], m)
        idx = np.where(win, np.uint8(r), idx)
    cls = np.take_along_axis(cls4, idx[:, :, None].astype(np.int64), 2)[:, :, 0]
    pos = np.arange(4, dtype=np.uint8)
    if mutate == "code_yx_swap":
        idx, pos = ((idx & 1) << 1) | (idx >> 1), np.array([0, 2, 1, 3], np.uint8)
    code = (idx | (cls << 2)).astype(np.uint8)
    if not detail:
        return dict(feat=m, code=code, scale=scale)
    codes4 = (pos[None, None, :] | (cls4 << 2)).astype(np.uint8)
    a64, e_a = pooled(a_tab), gamma(28) * pooled(mag_tab)
    lk64 = np.where(a64 > 0, a64, a64 * float(SLOPE))
    v64 = lk64 * keep * float(scale) if drop else lk64
    e_v = np.where(keep, float(scale) * e_a + 3 * U * np.abs(v64), 0.0)
    pw4 = np.broadcast_to(pool_order(pw)[:, None], (n, 32, NPOOL, 4)).reshape(n, FEAT, 4)
    # candidates
    cand = v64 + e_v >= (v64 - e_v).max(2, keepdims=True)
    same = lambda x, r, s: x[:, :, r] == x[:, :, s]  # noqa: E731
    for r in range(1, 4):
        for s in range(r):  # an earlier position with the same kernel value shadows r
            twin = same(keep, r, s) & (same(pw4, r, s) | ~keep[:, :, r])
            cand[:, :, r] &= ~(twin & cand[:, :, s])
    sure = ~keep | (np.abs(a64) > e_a)  # the position's gradient class is certain
    first = cand.argmax(2)[:, :, None]
    undecided = (cand.sum(2) != 1) | ~np.take_along_axis(sure, first, 2)[:, :, 0]
    return dict(a64=a64, e_a=e_a, keep=keep, v32=v32, v64=v64, e_v=e_v, codes4=codes4, cand=cand,
                sure=sure, feat=m, code=code, undecided=undecided, scale=scale)


def forward(bits, w, b, p=0.0, key=0, salt=0, row0=0, mutate=None):
    """feat float32 [n, 1568], code uint8 [n, 1568], undecided bool [n, 1568]."""
    d = forward_detail(bits, w, b, p, key, salt, row0, mutate)
    return d["feat"], d["code"], d["undecided"]


def forward_lean(bits, w, b, p=0.0, key=0, salt=0, row0=0, mutate=None, tables=None):
    """feat, code only (no bounds): for many rows. tables: _conv_tables(bits, w, b), when the same
    windows are evaluated again as other rows (other dropout draws)."""
    d = forward_detail(bits, w, b, p, key, salt, row0, mutate, detail=False, tables=tables)
    return d["feat"], d["code"]


def qnet_conv(scale=1.0, seed=11):
    """Tier B: the conv weights [32, 27] / bias [32] of a freshly initialised QNet, x scale."""
    import torch
    from mazerl.agents.nets import QNet
    torch.manual_seed(seed)
    conv = QNet(variant="ddqn").conv[0]
    s = np.float32(scale)
    return (conv.weight.detach().numpy().reshape(32, 27) * s).astype(np.float32), \
        (conv.bias.detach().numpy() * s).astype(np.float32)


# ---- backward -----------------------------------------------------------------------------------
def chunks_of(n):
    return (n + CHUNK - 1) // CHUNK


def _terms(bits, code, g, ld, n, scale, mutate=None):
    """gc float32 [n, 1568] (0 where class 0) and sel uint32 [n, 1568]: the patch word at the
    code's argmax position with bit 27 (the bias) set, 0 where class 0."""
    code = np.asarray(code, np.uint8).reshape(-1, FEAT)[:n].astype(np.uint32)
    g = np.asarray(g, np.float32).reshape(-1, ld)[:n, :FEAT]
    cls = code >> 2
    gs = g * np.float32(scale)
    gc = np.where(cls == 1, gs, gs if mutate == "cls2_no_slope" else gs * SLOPE).astype(np.float32)
    gc = np.where(cls == 0, np.float32(0), gc)
    pw = patch_words(np.asarray(bits)[:n])
    q = np.arange(FEAT) % NPOOL
    y = 2 * (q // 7)[None, :] + ((code >> 1) & 1)
    x = 2 * (q % 7)[None, :] + (code & 1)
    sel = pw[np.arange(n)[:, None], y, x] | np.uint32(1 << 27)
    return gc, np.where(cls == 0, np.uint32(0), sel)


def backward(bits, code, g, ld, n, scale, mutate=None):
    """dw float32 [32, 27], db float32 [32], partial float32 [chunks, 32, 28]: the kernels'
    additions in the kernels' order."""
    assert mutate is None or mutate in BWD_MUTATIONS
    ch_n = chunks_of(n)
    partial = np.zeros((ch_n, 32, NACC), np.float32)
    if n > 0:
        gc, sel = _terms(bits, code, g, ld, n, scale, mutate)
    items = 13 * 256  # i = tid + 256 u; the real ones are i < 64 * 49 = 3,136
    limit = (CHUNK - 1) * NPOOL if mutate == "bwd_limit_row" else CHUNK * NPOOL
    kbit = np.arange(NACC, dtype=np.uint32)
    for c0 in range(ch_n):
        r0, r1 = c0 * CHUNK, min(n, (c0 + 1) * CHUNK)
        gci = np.zeros((32, items), np.float32)
        seli = np.zeros((32, items), np.uint32)
        m = min((r1 - r0) * NPOOL, limit)
        # item i = s*49 + q of channel c is feature c*49 + q of row r0 + s
        gci[:, :(r1 - r0) * NPOOL] = gc[r0:r1].reshape(r1 - r0, 32, NPOOL).transpose(1, 0, 2).reshape(32, -1)
        seli[:, :(r1 - r0) * NPOOL] = sel[r0:r1].reshape(r1 - r0, 32, NPOOL).transpose(1, 0, 2).reshape(32, -1)
        gci[:, m:], seli[:, m:] = 0, 0
        gci, seli = gci.reshape(32, 13, 256), seli.reshape(32, 13, 256)
        acc = np.zeros((32, 256, NACC), np.float32)
        for u in range(13):  # +0.0f where the bit is off: the identity (acc is never -0)
            on = ((seli[:, u, :, None] >> kbit) & 1).astype(bool)
            acc = acc + np.where(on, gci[:, u, :, None], np.float32(0))
        v = acc.reshape(32, 4, 64, NACC)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, lane ^ o, :]
        red = v[:, :, 0, :]
        partial[c0] = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    s = np.zeros((32, NACC), np.float32)
    last = (ch_n // 8) * 8 if mutate == "reduce_no_tail" else ch_n
    for c0 in range(last):
        s = s + partial[c0]
    return s[:, :27].copy(), s[:, 27].copy(), partial


def backward64(bits, code, g, ld, n, scale):
    """dw, db in float64 from the same float32 terms, and asum = the sum of their magnitudes
    (float64 [32, 28]: what an order-free rounding bound is stated in)."""
    if n == 0:
        z = np.zeros((32, NACC))
        return z[:, :27], z[:, 27], z
    gc, sel = _terms(bits, code, g, ld, n, scale)
    kbit = np.arange(NACC, dtype=np.uint32)
    s, asum = np.zeros((32, NACC)), np.zeros((32, NACC))
    for r0 in range(0, n, CHUNK):
        t = gc[r0:r0 + CHUNK].astype(np.float64).reshape(-1, 32, NPOOL)
        on = ((sel[r0:r0 + CHUNK].reshape(-1, 32, NPOOL)[..., None] >> kbit) & 1).astype(np.float64)
        s += np.einsum("ncq,ncqk->ck", t, on)
        asum += np.einsum("ncq,ncqk->ck", np.abs(t), on)
    return s[:, :27], s[:, 27], asum
