"""The learner's head + loss kernels (csrc/mz_trainer.hip: k_head_loss, k_loss_sum,
k_head_loss_bwd with mz_colsum_f32; k_q_loss_fwd / k_q_loss_bwd) through the C ABI against the
float64 models of tests/learner_model.py, at the shapes where the kernels' loops change path.

Every bound is a count of f32 roundings (u = 2^-24, each rounding relative error <= u); none is
taken from the kernels' output.

  Q values   one f32 chain per value: the activation (LeakyReLU's product), one FMA per 64 columns
             (a lane's columns j, j + 64, ...), six butterfly adds, the bias: <= ceil(H/64) + 8
             roundings, each on a partial sum bounded by mag_k = sum_j |h_j||w_kj| + |b_k|:
             |q - q64| <= (ceil(H/64) + 10) u mag_k.
  diff       q(s,a) - (v * gamma + r): the two Q errors (gamma times the second) and three
             roundings on |gamma v|, |gamma v| + |r| and |q| + |gamma v| + |r|:
             |d diff| <= tol_q(s,a) + gamma tol_q(v) + 3 u (|q| + |gamma v| + |r|).
             Holds where kernel and model pick the same s' column. A row whose float64 top-two q_n
             gap is <= 2 max_k tol_q might be left out; the recipe has no such row, and the tests
             assert that from the model before they look at the kernel's output (cap: zero rows).
  loss       as a reduction of the kernel's own diff: d * d, the workgroup's four wave values, a
             thread's ceil(nblk/256) partials, six butterfly adds, four wave sums, the division
             = ceil(b/1024) + 16 roundings of non-negative sums: <= (ceil(b/1024) + 18) u loss.
  dz2        from a given diff and an upstream gradient != 1: (diff * norm) * g * W3[a][j], three
             products: 3 u |dz2|; LeakyReLU's z <= 0 branch multiplies by the f32 slope once more
             (head_act_grad<0>: g * 0.01f), a fourth rounding: 4 u |dz2| on those entries only.
             (With 3 u everywhere one such entry of H = 512, b = 67 came out at 1.007 x 3 u on
             an MI355X: the rounding a three-product count leaves out.) Exactly 0 where the model
             gives 0.
  dW3, db3   t_i = g_i * act(z_ij): four roundings; <= 15 adds inside a 16-row block; the column
             sum's tree over the blocks' partials (<= 8 adds that are not + 0). For every listed b
             that is <= b + 8 roundings: (b + 8) u sum_i |t_i| per element. Exactly +0 for an
             action no row takes.
  mz_q_loss  the same 3-rounding diff bound (its Q rows are inputs: no tol_q, and the argmax sees
             the same f32 values as the model: no near-tie exclusion); the loss as a reduction of
             its own diff within (ceil(b/1024) + 12) u loss. (The one workgroup's chain is d * d,
             a thread's ceil(b/1024) adds, six butterfly adds, 15 adds of the 16 wave sums and the
             division: up to ceil(b/1024) + 23 roundings in the worst case; the tighter + 12 is
             what the kernel is held to.)

Memory contract (QNet.forward_rows: "rows >= n_grad are left unwritten"): every output buffer is
filled with a NaN sentinel, padded to its row pitch and wrapped in guard rows; after a launch the
sentinel must still stand in rows >= b of dz2, in pitch columns >= H and in every guard. Input pad
columns hold NaN too: a kernel that read them would poison its result."""
import math

import numpy as np
import pytest
import torch

import learner_model as M
import learner_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = M.U32
SENT = 0x7FC0BEEF  # a quiet NaN with a payload no arithmetic produces
HS = [4, 8, 60, 252, 256, 260, 512, 1024]
BS = [1, 3, 4, 5, 15, 16, 17, 67]


def _lib():
    from mazerl import _native as N
    return N, N.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Buf:
    """[rows, width] at row pitch ld inside guard rows, all NaN sentinel; `data` in the top left."""

    def __init__(self, rows, width=1, ld=None, data=None, guard=2):
        self.rows, self.width, self.ld, self.g = rows, width, ld or width, guard
        self.full = torch.full((rows + 2 * guard, self.ld), SENT, dtype=torch.int32,
                               device=DEV).view(torch.float32)
        if data is not None:
            d = np.asarray(data, np.float32).reshape(-1, width)
            self.body[:d.shape[0], :width] = _dev(d)

    @property
    def body(self):
        return self.full[self.g:self.g + self.rows]

    @property
    def ptr(self):
        return self.body.data_ptr()

    def host(self, rows=None):
        return self.body[:rows, :self.width].cpu().numpy().astype(np.float64)

    def intact_outside(self, rows, cols=None):
        """True when everything but body[:rows, :cols] still holds the sentinel."""
        x = self.full.view(torch.int32).clone()
        x[self.g:self.g + rows, :self.width if cols is None else cols] = SENT
        return bool((x == SENT).all())


def _forward(c, b, dbl, pad):
    """mz_head_loss on case c: (rc, diff Buf, loss Buf, part Buf, nblk)."""
    N, L = _lib()
    H = c["H"]
    ld = H + pad
    ns = 2 * b if dbl else b
    zs = Buf(ns, H, ld, c["z2s"][:ns])
    zt = Buf(b, H, ld, c["z2t"][:b])
    w = [_dev(c[k]) for k in ("w3s", "b3s", "w3t", "b3t")]
    a, r = _dev(c["action"][:b]), _dev(c["reward"][:b])
    nblk = L.mz_head_loss_workspace_floats(b)
    diff, loss, part = Buf(b), Buf(1), Buf(nblk)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = L.mz_head_loss(zs.ptr, ld, w[0].data_ptr(), w[1].data_ptr(), zt.ptr, ld, w[2].data_ptr(),
                        w[3].data_ptr(), H, c["act"], dbl, a.data_ptr(), r.data_ptr(), c["gamma"],
                        b, part.ptr, ticket.data_ptr(), loss.ptr, diff.ptr, _stream())
    torch.cuda.synchronize()
    return rc, diff, loss, part, nblk


def _backward(c, b, diff_in, gradient, pad, rows=None):
    """mz_head_loss_backward + mz_colsum_f32: (rc, dz2 Buf, row Buf [1, 4H + 4], part Buf)."""
    N, L = _lib()
    H = c["H"]
    ld = H + pad
    rows = 2 * b if rows is None else rows
    zs = Buf(rows, H, ld, c["z2s"][:rows])
    w3 = _dev(c["w3s"])
    a = _dev(c["action"][:b])
    d = _dev(np.asarray(diff_in, np.float32))
    g = torch.tensor(gradient, dtype=torch.float32, device=DEV)
    nblk = L.mz_head_loss_backward_workspace_floats(b, H) // (4 * H + 4)
    dz2, part, row = Buf(rows, H, ld), Buf(nblk, 4 * H + 4), Buf(1, 4 * H + 4)
    rc = L.mz_head_loss_backward(g.data_ptr(), d.data_ptr(), a.data_ptr(), b, zs.ptr, ld,
                                 w3.data_ptr(), H, c["act"], dz2.ptr, ld, part.ptr, _stream())
    if rc == 0:
        N.check(L.mz_colsum_f32(part.ptr, nblk, 4 * H + 4, 4 * H + 4, row.ptr, _stream()))
    torch.cuda.synchronize()
    return rc, dz2, row, part


def _model_fw(c, b, dbl):
    return M.head_forward(c["z2s"], c["w3s"], c["b3s"], c["z2t"], c["w3t"], c["b3t"], c["action"],
                          c["reward"], c["gamma"], b, c["act"], dbl)


def _check_loss(loss_gpu, diff_gpu, b, extra):
    own = float(np.sum(diff_gpu * diff_gpu) / b)
    bound = (math.ceil(b / 1024) + extra) * U32 * own
    print(f"  loss {loss_gpu!r} own {own!r} err/bound {abs(loss_gpu - own) / bound:.3f}")
    assert abs(loss_gpu - own) <= bound


def _check_forward(c, b, dbl, pad):
    H = c["H"]
    fw = _model_fw(c, b, dbl)
    tol, near = M.head_tolerances(fw, c["action"], c["reward"], c["gamma"], H, dbl)
    assert int(near.sum()) == 0  # the cap on left-out rows, from the model alone
    rc, diff, loss, part, nblk = _forward(c, b, dbl, pad)
    assert rc == 0
    d = diff.host()[:, 0]
    err = np.abs(d - fw["diff"])
    print(f"H {H} b {b} act {c['act']} dbl {dbl} pad {pad}: diff err/tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol), (H, b, dbl, pad, float(np.max(err / tol)))
    _check_loss(float(loss.host()[0, 0]), d, b, 18)
    assert diff.intact_outside(b) and loss.intact_outside(1) and part.intact_outside(nblk)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("H", HS)
def test_head_forward_matches_float64_model(H, act):
    for b in BS + ([1029] if H == 8 else []):  # 1029: 258 workgroup partials into k_loss_sum
        c = U.head_case(H, b, act)
        for dbl in (0, 1):
            for pad in (0, 12):
                _check_forward(c, b, dbl, pad)


def _check_grad_sums(row, aW, ab, dW, db, b, H):
    got = row.host()[0]
    gW, gb = got[:4 * H].reshape(4, H), got[4 * H:]
    for name, x, ref, mag in (("dW3", gW, dW, aW), ("db3", gb, db, ab)):
        fin = np.isfinite(ref) & np.isfinite(mag)
        assert np.array_equal(np.isnan(x), np.isnan(ref)), name
        assert np.array_equal(x[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), name  # +-inf
        with np.errstate(invalid="ignore"):
            assert np.all(np.abs(x - ref)[fin] <= ((b + 8) * U32 * mag)[fin]), name
    return gW, gb


def _check_backward(c, b, pad, missing=None):
    H, act = c["H"], c["act"]
    rng = np.random.default_rng(7 * H + b)
    diff_in = rng.standard_normal(b).astype(np.float32)  # any diff: the chain is products only
    gradient = float(np.float32(0.7))
    dz2_m, dW, db, aW, ab = M.head_backward(gradient, diff_in, c["action"], b, c["z2s"], c["w3s"],
                                            act, mags=True)
    rc, dz2, row, part = _backward(c, b, diff_in, gradient, pad)
    assert rc == 0
    x = dz2.host(b)
    z = c["z2s"][:b]
    slope = (z <= 0) & (act == 0)  # LeakyReLU's z <= 0 branch: the slope is a fourth product
    tol = np.where(slope, 4.0, 3.0) * U32 * np.abs(dz2_m)
    ratio = np.abs(x - dz2_m) / np.maximum(tol, 1e-300)
    print(f"H {H} b {b} act {act} pad {pad}: dz2 err/tol {ratio.max():.3f}"
          f" (slope branch {ratio[slope].max() if slope.any() else 0.0:.3f})")
    assert np.all(np.abs(x - dz2_m) <= tol), (H, b, pad, float(ratio.max()))
    assert np.all(x[dz2_m == 0] == 0)
    assert dz2.intact_outside(b, H)  # rows >= b, pitch columns, guards
    assert part.intact_outside(part.rows) and row.intact_outside(1)
    gW, gb = _check_grad_sums(row, aW, ab, dW, db, b, H)
    if missing is not None:
        bits = row.body[0].view(torch.int32).cpu().numpy()
        assert not bits[missing * H:(missing + 1) * H].any() and bits[4 * H + missing] == 0  # +0


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("H", HS)
def test_head_backward_matches_float64_model(H, act):
    for b in BS + ([1029] if H == 8 else []):  # 1029: 65 backward blocks
        c = U.head_case(H, b, act)
        for pad in (0, 12):
            _check_backward(c, b, pad)
    c = U.head_case(H, 17, act, missing_action=3)
    assert 3 not in c["action"]
    _check_backward(c, 17, 0, missing=3)


def _same_values(x, ref, what):
    """NaN where the model has NaN; every other entry equal to the model's value rounded to f32
    (the special rows leave one inexact f32 operation per chain at most)."""
    assert np.array_equal(np.isnan(x), np.isnan(ref)), (what, x, ref)
    ok = ~np.isnan(ref)
    with np.errstate(over="ignore"):
        r32 = ref.astype(np.float32).astype(np.float64)
    assert np.array_equal(x[ok], r32[ok]), (what, x, r32)


@pytest.mark.parametrize("c", U.special_head_cases(), ids=lambda c: c["name"])
def test_head_special_rows_are_exact(c):
    """Ties (first maximum: DDQN takes column 1 of 1 == 2, column 0 of a three-way tie), +0.0 and
    -0.0 under both activations, a NaN row (its diff and the loss are NaN, the other rows keep
    their values), +-inf entries (inf * 0 = NaN in the other Q columns: the first NaN wins the
    argmax), NaN in fc3's bias, and the Q rows of test_fused_q_loss_propagates_nan_like_torch under
    an identity W3 — forward and backward, value for value against the float64 model."""
    b, H, dbl = c["b"], c["H"], c["dbl"]
    fw = _model_fw(c, b, dbl)
    if "choice" in c:
        assert list(fw["choice"]) == list(c["choice"])
    rc, diff, loss, part, nblk = _forward(c, b, dbl, 0)
    assert rc == 0
    d = diff.host()[:, 0]
    _same_values(d, fw["diff"], "diff")
    lg = float(loss.host()[0, 0])
    if np.isfinite(fw["loss"]):
        _check_loss(lg, d, b, 18)
    else:
        assert np.isnan(lg) == np.isnan(fw["loss"]) and (np.isnan(lg) or lg == fw["loss"])
    assert diff.intact_outside(b) and loss.intact_outside(1) and part.intact_outside(nblk)
    own = diff.body[:, 0].cpu().numpy()  # the kernel's diff, NaN / inf included
    for diff_in in (np.array([1.5, -2.0, 0.75, -0.5], np.float32), own):
        dz2_m, dW, db, aW, ab = M.head_backward(0.5, diff_in, c["action"], b, c["z2s"], c["w3s"],
                                                c["act"], mags=True)
        rc, dz2, row, _ = _backward(c, b, diff_in, 0.5, 0)
        assert rc == 0
        _same_values(dz2.host(b), dz2_m, "dz2")
        assert dz2.intact_outside(b, H)
        _check_grad_sums(row, aW, ab, dW, db, b, H)


def test_head_rejects_bad_arguments_without_writing():
    good = U.head_case(8, 5, 0)
    for what, kw in (("H % 4", dict(H=6)), ("b = 0", dict(b=0)), ("lds < H", dict(pad=-4)),
                     ("act = 2", dict(act=2))):
        c = dict(good, **{k: v for k, v in kw.items() if k in ("H", "act")})
        if "H" in kw:
            for k in ("z2s", "z2t", "w3s", "w3t"):
                c[k] = np.ascontiguousarray(good[k][:, :6])
        b, pad = kw.get("b", 5), kw.get("pad", 0)
        N, L = _lib()
        H, ld = c["H"], c["H"] + pad
        zs, zt = Buf(10, 8, 8, good["z2s"]), Buf(5, 8, 8, good["z2t"])
        w = [_dev(c[k]) for k in ("w3s", "b3s", "w3t", "b3t")]
        a, r = _dev(good["action"]), _dev(good["reward"])
        diff, loss, part = Buf(5), Buf(1), Buf(4)
        ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
        rc = L.mz_head_loss(zs.ptr, ld, w[0].data_ptr(), w[1].data_ptr(), zt.ptr, ld,
                            w[2].data_ptr(), w[3].data_ptr(), H, c["act"], 1, a.data_ptr(),
                            r.data_ptr(), 0.7, b, part.ptr, ticket.data_ptr(), loss.ptr, diff.ptr,
                            _stream())
        torch.cuda.synchronize()
        assert rc != 0, what
        assert diff.intact_outside(0) and loss.intact_outside(0) and part.intact_outside(0), what
        g = torch.tensor(0.5, device=DEV)
        d = _dev(np.ones(5, np.float32))
        dz2, bp = Buf(10, 8, 8), Buf(1, 36)
        rc = L.mz_head_loss_backward(g.data_ptr(), d.data_ptr(), a.data_ptr(), b, zs.ptr, ld,
                                     w[0].data_ptr(), H, c["act"], dz2.ptr, ld, bp.ptr, _stream())
        torch.cuda.synchronize()
        assert rc != 0, what
        assert dz2.intact_outside(0) and bp.intact_outside(0), what


@pytest.mark.parametrize("ld", [4, 7])
@pytest.mark.parametrize("dbl", [0, 1])
def test_q_loss_matches_float64_model(dbl, ld):
    """mz_q_loss (one workgroup of 1,024 threads striding over the rows: one trip up to b = 1,024,
    two and three beyond) and mz_q_loss_backward (rows = 2b + 3 >= b: the rows past b are exactly
    zero) at row pitches 4 and 7, with ties and NaN rows among the random ones."""
    N, L = _lib()
    for b in (1, 63, 64, 65, 1023, 1024, 1025, 2049):
        rng = np.random.default_rng(100 * b + 10 * ld + dbl)
        rows = 2 * b + 3
        q, qn, qt = (rng.standard_normal((n, 4)).astype(np.float32) for n in (rows, b, b))
        if b >= 63:
            qn[5:9, 3] = qn[5:9, 1] = 4.0  # ties: the first maximum
            qt[10:13, 2] = qt[10:13, 0] = 4.0
        a = rng.integers(0, 4, b).astype(np.int64)
        r = rng.choice(U.REWARDS, b).astype(np.float32)
        for poison in ((False, True) if b == 65 else (False,)):
            if poison:
                qn[3, 1] = qn[3, 2] = qt[4, 3] = q[6, a[6]] = np.nan
            m = M.q_loss_forward(q, qn if dbl else None, qt, a, r, 0.7, b)
            bq, bn, bt = Buf(rows, 4, ld, q), Buf(b, 4, ld, qn), Buf(b, 4, ld, qt)
            ad, rd = _dev(a), _dev(r)
            diff, loss = Buf(b), Buf(1)
            N.check(L.mz_q_loss(bq.ptr, ld, bn.ptr if dbl else None, ld if dbl else 0, bt.ptr, ld,
                                ad.data_ptr(), rd.data_ptr(), 0.7, b, loss.ptr, diff.ptr, _stream()))
            torch.cuda.synchronize()
            d = diff.host()[:, 0]
            fin = ~np.isnan(m["diff"])
            assert np.array_equal(np.isnan(d), ~fin)
            g32 = float(np.float32(0.7))
            with np.errstate(invalid="ignore"):
                tol = 3 * U32 * (np.abs(q[np.arange(b), a].astype(np.float64)) +
                                 np.abs(g32 * m["v"]) + np.abs(r.astype(np.float64)))
            assert np.all(np.abs(d - m["diff"])[fin] <= tol[fin]), (b, ld, dbl)
            lg = float(loss.host()[0, 0])
            if poison:
                assert np.isnan(lg) and np.isnan(m["loss"])
            else:
                _check_loss(lg, d, b, 12)
            assert diff.intact_outside(b) and loss.intact_outside(1)
            # backward from the kernel's own diff and an upstream gradient != 1
            gradient = float(np.float32(0.7))
            own = diff.body[:, 0].contiguous()
            g = torch.tensor(gradient, dtype=torch.float32, device=DEV)
            dq = Buf(rows, 4)
            N.check(L.mz_q_loss_backward(g.data_ptr(), own.data_ptr(), ad.data_ptr(), b, rows,
                                         dq.ptr, _stream()))
            torch.cuda.synchronize()
            x = dq.host()
            ref = M.q_loss_backward(gradient, own.cpu().numpy(), a, b, rows)
            assert np.array_equal(np.isnan(x), np.isnan(ref))
            ok = ~np.isnan(ref)
            assert np.all(np.abs(x - ref)[ok] <= 2 * U32 * np.abs(ref)[ok])  # two products
            assert not x[b:].any() and np.all(x[ref == 0] == 0)
            assert dq.intact_outside(rows)
