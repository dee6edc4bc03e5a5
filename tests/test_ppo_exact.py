"""The PPO device path (csrc/mz_ppo.hip: k_ppo_act, k_ppo_scan, k_ppo_finish, k_ppo_head1/2;
k_pair_surrogate of csrc/mz_optim.hip) through the C ABI against tests/ppo_model.py, at the sizes
where the kernels change path: the scan's 1,024-instance chunks, finish's 256-thread / 2,048-reward
chunks and its 2,048-workgroup grid stride, the head's 256-row blocks and 1,024-thread stride loop.

Bounds, none taken from a kernel's output:
  scan      everything exact.
  finish    record columns bit-equal; returns / advantages within 1 float32 ulp of the model on
            episodes the model calls clear (every statistic away from a float32 rounding midpoint,
            where the kernel's order of float64 additions cannot matter), rtol 1e-6 on the others
            (at most 2 per list, asserted for the model alone in tests/test_ppo_model.py).
  act       the action equals the model's on rows whose uniform is 2^-20 away from every
            cumulative boundary; one of the actions across the boundary otherwise (at most 2 rows).
  libm-bound tensors (act's log-prob; the head's loss, dlogits, dvalue): with e_ref the largest
            error of torch's float32 CPU evaluation against the model and e_k the kernel's,
                e_k <= 4 e_ref + 8 u max|tensor|,  u = 2^-24
            (4: another expf / logf and another summation order over a chain of the same length;
            the floor: values torch happens to get exactly) — the rule of tests/test_drqn_gpu.py.

Memory: every output buffer is filled with a sentinel, padded to its pitch and wrapped in guard
elements; whatever the contract does not write must still hold the sentinel afterwards. Input pad
columns hold a NaN sentinel too. Every index handed to a kernel is inside its buffers."""
import numpy as np
import pytest
import torch

import ppo_cases as K
import ppo_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = 2.0 ** -24
SENT32, SENT64 = 0x7FC0BEEF, 0x7FF8BEEF7FC0BEEF  # quiet NaNs with a payload no arithmetic produces
GUARD = 64  # guard elements (of the buffer's type) before and after it


def _lib():
    from mazerl import _native as N
    return N, N.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Buf:
    """rows x width elements of `dtype` at row pitch ld between guards, all sentinel; `data`
    (rows x width) in the body. Compared as raw bits, so NaN sentinels and values alike."""

    def __init__(self, dtype, rows, width=1, ld=None, data=None):
        self.dt = np.dtype(dtype)
        self.it = {4: np.int32, 8: np.int64, 1: np.uint8}[self.dt.itemsize]
        self.sent = {4: np.int32(SENT32), 8: np.int64(SENT64), 1: np.uint8(0xA5)}[self.dt.itemsize]
        self.rows, self.width, self.ld = rows, width, ld or width
        self.init = np.full(GUARD + rows * self.ld + GUARD, self.sent, self.it)
        if data is not None:
            self._body(self.init)[:, :width] = np.asarray(data, self.dt).reshape(rows, width).view(self.it)
        self.t = _dev(self.init)

    def _body(self, flat):
        return flat[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.dt.itemsize

    def bits(self):
        return self.t.cpu().numpy()

    def host(self):
        """the body's rows x width as `dtype`"""
        return np.ascontiguousarray(self._body(self.bits())[:, :self.width]).view(self.dt)

    def expect(self, written=None, mask=None):
        """The initial content with `written` (rows x width, dtype) stored where mask (rows x
        width bool; default everywhere) is set: what the whole buffer, guards included, must be."""
        e = self.init.copy()
        if written is not None:
            w = np.ascontiguousarray(np.asarray(written, self.dt).reshape(self.rows, self.width)).view(self.it)
            body = self._body(e)[:, :self.width]
            if mask is None:
                body[...] = w
            else:
                m = np.asarray(mask, bool).reshape(self.rows, self.width)
                body[m] = w[m]
        return e

    def same(self, written=None, mask=None):
        return np.array_equal(self.bits(), self.expect(written, mask))

    def untouched_outside(self, mask):
        """True when every element outside mask (rows x width) still holds its initial content."""
        got, e = self.bits().copy(), self.init.copy()
        m = np.asarray(mask, bool).reshape(self.rows, self.width)
        self._body(got)[:, :self.width][m] = 0
        self._body(e)[:, :self.width][m] = 0
        return np.array_equal(got, e)


def _bound(name, got, model, ref):
    got, model, ref = (np.asarray(a, np.float64) for a in (got, model, ref))
    mx = np.abs(model).max() if model.size else 0.0
    e_k = np.abs(got - model).max() if model.size else 0.0
    e_ref = np.abs(ref - model).max() if model.size else 0.0
    print(f"  {name}: e_k {e_k:.3e} e_ref {e_ref:.3e} ratio {e_k / (e_ref + 2 * U32 * mx + 1e-300):.2f}")
    return e_k <= 4 * e_ref + 8 * U32 * mx, (name, e_k, e_ref, mx)


# ---- scan ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", K.SCAN_PATTERNS)
@pytest.mark.parametrize("B", K.SCAN_BS)
def test_scan_is_the_integer_model(B, pattern):
    """Two consecutive mz_ppo_scan calls on the same state, from a nonzero pool fill and nonzero
    counters; everything the call writes equals the model, everything else keeps its sentinel
    (rec_r outside [i][t], the finished list past fin_count, guards)."""
    N, L = _lib()
    Ls = K.SCAN_L
    st = dict(K.SCAN_STATE0)
    t = Buf(np.int32, B, data=K.scan_t0(B, pattern))
    rec = Buf(np.float64, B, Ls)
    fill, total = Buf(np.int64, 1, data=[st["fill"]]), Buf(np.int64, 1, data=[st["total"]])
    stats = Buf(np.int64, 4, data=st["stats"])
    t_m = K.scan_t0(B, pattern)
    rec_m, rec_mask = np.zeros((B, Ls)), np.zeros((B, Ls), bool)
    for call in (0, 1):
        term, trunc, rew = K.scan_step(B, pattern, call)
        m = M.scan(t_m, term, trunc, rew, Ls, st["fill"], st["total"], st["stats"])
        fid, foff, flen = Buf(np.int32, B), Buf(np.int64, B), Buf(np.int32, B)
        fcount = Buf(np.int32, 1)
        d = [_dev(x) for x in (rew, term, trunc)]
        N.check(L.mz_ppo_scan(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), B, Ls, t.ptr,
                              rec.ptr, fid.ptr, foff.ptr, flen.ptr, fcount.ptr, fill.ptr,
                              total.ptr, stats.ptr, _stream()))
        torch.cuda.synchronize()
        for i, ti, r in m["rec"]:
            rec_m[i, ti], rec_mask[i, ti] = r, True
        n = m["fin_count"]
        listed = np.arange(B) < n
        pad = [0] * (B - n)
        print(f"B {B} {pattern} call {call}: listed {n} (fin_count {int(fcount.host()[0, 0])}) rows"
              f" {m['fill'] - st['fill']} stats {m['stats']} got {stats.host()[:, 0].tolist()}"
              f" fill {int(fill.host()[0, 0])}")
        assert fcount.same([n])
        assert fid.same(m["fin_id"] + pad, listed), "fin_id"
        assert foff.same(m["fin_off"] + pad, listed), "fin_off"
        assert flen.same(m["fin_len"] + pad, listed), "fin_len"
        assert t.same(m["t"]) and rec.same(rec_m, rec_mask)
        assert fill.same([m["fill"]]) and total.same([m["total"]]) and stats.same(m["stats"])
        t_m, st = m["t"], dict(fill=m["fill"], total=m["total"], stats=m["stats"])


# ---- finish -------------------------------------------------------------------------------------
def _records(c):
    B, L = c["B"], c["L"]
    rng = np.random.default_rng(5 + B)
    return dict(s6=rng.random((B, L * 6)).astype(np.float32),
                w=rng.integers(0, 2 ** 32, (B, L * 22), dtype=np.uint64).astype(np.uint32),
                a=rng.integers(0, 4, (B, L)).astype(np.int64),
                lp=(-rng.random((B, L))).astype(np.float32))


def _finish(c, count=None, capacity=None):
    """mz_ppo_finish on a hand-built list -> the six pool Bufs and the records."""
    N, L = _lib()
    B, Lr, rows = c["B"], c["L"], c["alloc"]
    r = _records(c)
    d = [_dev(x) for x in (c["rec_r"], r["s6"], r["w"], r["a"], r["lp"], c["rec_v"])]
    n = len(c["ids"])
    ids, offs, lens = np.zeros(B, np.int32), np.zeros(B, np.int64), np.full(B, 2, np.int32)
    ids[:n], offs[:n], lens[:n] = c["ids"], c["offs"], c["lens"]  # entries past the count: valid, unused
    f = [_dev(x) for x in (ids, offs, lens, np.array([n if count is None else count], np.int32))]
    pool = dict(s6=Buf(np.float32, rows, 6), w=Buf(np.uint32, rows, 22), a=Buf(np.int64, rows),
                lp=Buf(np.float32, rows), adv=Buf(np.float32, rows), ret=Buf(np.float32, rows))
    N.check(L.mz_ppo_finish(*[x.data_ptr() for x in d], B, Lr, *[x.data_ptr() for x in f],
                            c["gamma"], c["cap"] if capacity is None else capacity,
                            pool["s6"].ptr, pool["w"].ptr, pool["a"].ptr, pool["lp"].ptr,
                            pool["adv"].ptr, pool["ret"].ptr, _stream()))
    torch.cuda.synchronize()
    return pool, r


def _ulps(got, model):
    """|got - model| in units of the model's float32 spacing; NaN where the model is NaN must be
    NaN (distance 0), anything else there counts as infinitely far."""
    g, m = got.astype(np.float64), model.astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(g - m) / np.spacing(np.abs(model)).astype(np.float64)
    both = np.isnan(g) & np.isnan(m)
    return np.where(both, 0.0, np.where(np.isnan(d), np.inf, d))


def _check_finish(c, pool, r, written):
    """`written`: indices into the list of the episodes the call must have stored."""
    model = K.finish_model(c["name"], c["gamma"])
    rows = c["alloc"]
    mask = np.zeros(rows, bool)
    exp = {k: np.zeros((rows, w), dt) for k, w, dt in (("s6", 6, np.float32), ("w", 22, np.uint32),
                                                       ("a", 1, np.int64), ("lp", 1, np.float32))}
    ret_m, adv_m = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
    clear_row = np.zeros(rows, bool)
    unclear = 0
    for k in written:
        i, o, n = c["ids"][k], c["offs"][k], c["lens"][k]
        mask[o:o + n] = True
        exp["s6"][o:o + n] = r["s6"][i, :n * 6].reshape(n, 6)
        exp["w"][o:o + n] = r["w"][i, :n * 22].reshape(n, 22)
        exp["a"][o:o + n, 0] = r["a"][i, :n]
        exp["lp"][o:o + n, 0] = r["lp"][i, :n]
        ret_m[o:o + n], adv_m[o:o + n], clear = model[k]
        clear_row[o:o + n] = clear
        unclear += not clear
    for k, w in (("s6", 6), ("w", 22), ("a", 1), ("lp", 1)):
        assert pool[k].same(exp[k], np.repeat(mask[:, None], w, axis=1)), k  # bit-equal, rest sentinel
    for k, m in (("ret", ret_m), ("adv", adv_m)):
        assert pool[k].untouched_outside(mask), k
        got = pool[k].host()[:, 0]
        u = _ulps(got[mask], m[mask])
        cl = clear_row[mask]
        g, w = np.ascontiguousarray(got[mask]), np.ascontiguousarray(m[mask])
        differ = int(((g.view(np.int32) != w.view(np.int32)) & ~(np.isnan(g) & np.isnan(w))).sum())
        print(f"  {c['name']} gamma {c['gamma']} {k}: {int(mask.sum())} rows, not bit-equal {differ},"
              f" max ulp {u.max() if u.size else 0.0:.2f}, episodes not clear {unclear}")
        assert np.all(u[cl] <= 1.0), (k, float(u[cl].max()))
        if (~cl).any():
            np.testing.assert_allclose(got[mask][~cl], m[mask][~cl], rtol=1e-6, atol=0, equal_nan=True)
    assert unclear <= 2


@pytest.mark.parametrize("gamma", [0.9, 0.99])
def test_finish_chunk_edges_match_the_model(gamma):
    """Episodes of 2 ... 4,097 steps on both sides of finish's 64 / 256 / 2,048 / 4,096 edges;
    fin_id a permutation, gaps between the episodes' pool rows, 13 listed of B = 16."""
    c = K.finish_list("main", gamma)
    pool, r = _finish(c)
    _check_finish(c, pool, r, range(len(c["ids"])))


def test_finish_with_an_empty_list_writes_nothing():
    c = K.finish_list("main", 0.99)
    pool, r = _finish(c, count=0)
    _check_finish(c, pool, r, [])


def test_finish_strides_over_more_episodes_than_workgroups():
    """2,100 listed episodes of 2 to 4 steps: the last 52 are reached only by the grid stride of
    the 2,048 workgroups."""
    c = K.finish_list("stride", 0.99)
    assert len(c["ids"]) == 2100 > 2048
    pool, r = _finish(c)
    _check_finish(c, pool, r, range(2100))


def test_finish_zero_variance_and_the_capacity_edge():
    """All-zero rewards: std 0, so returns and advantages are NaN at every row while the record
    columns are still copied. An episode with off + n == capacity is written; one with off + n ==
    capacity + 1 leaves every pool column alone (its rows overlap the former's: those keep the
    former's values)."""
    c = K.finish_list("edge", 0.99)
    assert c["offs"][1] + c["lens"][1] == c["cap"] and c["offs"][2] + c["lens"][2] == c["cap"] + 1
    pool, r = _finish(c)
    _check_finish(c, pool, r, [0, 1])
    o, n = c["offs"][0], c["lens"][0]
    assert np.isnan(pool["ret"].host()[o:o + n]).all() and np.isnan(pool["adv"].host()[o:o + n]).all()


# ---- act ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldl,ldv", [(4, 1), (8, 3)])
@pytest.mark.parametrize("B", K.ACT_BS)
def test_act_draw_log_prob_and_records(B, ldl, ldv):
    """The draw is a pure function of (seed, counter, instance): predicted exactly. An instance
    whose step index is outside [0, L) records nothing and leaves act_out[i] as it was."""
    N, L = _lib()
    c = K.act_case(B)
    Lr, m, t = c["L"], c["model"], c["t"]
    live = (t >= 0) & (t < Lr)
    logits, value = Buf(np.float32, B, 4, ldl, c["logits"]), Buf(np.float32, B, 1, ldv, c["value"])
    obs6, bits, td = _dev(c["obs6"]), _dev(c["bits"]), _dev(t)
    rs6, rw = Buf(np.float32, B * Lr, 6), Buf(np.uint32, B * Lr, 22)
    ra, rlp, rv = Buf(np.int64, B, Lr), Buf(np.float32, B, Lr), Buf(np.float32, B, Lr)
    out = Buf(np.int32, B)
    N.check(L.mz_ppo_act(logits.ptr, ldl, value.ptr, ldv, obs6.data_ptr(), bits.data_ptr(), B, Lr,
                         K.ACT_SEED, K.ACT_COUNTER, td.data_ptr(), rs6.ptr, rw.ptr, ra.ptr, rlp.ptr,
                         rv.ptr, out.ptr, _stream()))
    torch.cuda.synchronize()
    at = np.zeros((B, Lr), bool)
    at[np.arange(B)[live], t[live]] = True
    row = at.reshape(-1)
    got_a = out.host()[:, 0].astype(np.int64)
    clear = m["clear"] & live
    odd = live & ~m["clear"]
    print(f"B {B} ldl {ldl} ldv {ldv}: live {int(live.sum())} rows not clear {int(odd.sum())}"
          f" actions differing from the model {int((got_a != m['action'])[live].sum())}")
    assert odd.sum() <= 2
    assert np.array_equal(got_a[clear], m["action"][clear])
    assert np.all(m["allowed"][np.arange(B)[odd], np.clip(got_a[odd], 0, 3)]) and np.all((got_a[odd] >= 0) & (got_a[odd] <= 3))
    a = np.where(live, np.where(clear, m["action"], np.clip(got_a, 0, 3)), 0)
    assert out.same(a.astype(np.int32), live)  # act_out: the action where live, the sentinel elsewhere
    assert ra.same(np.where(at, a[:, None], 0), at)  # the recorded action is act_out's
    assert rs6.same(np.repeat(c["obs6"], Lr, axis=0), np.repeat(row[:, None], 6, axis=1))
    assert rw.same(np.repeat(c["bits"], Lr, axis=0), np.repeat(row[:, None], 22, axis=1))
    assert rv.same(np.repeat(c["value"][:, None], Lr, axis=1), at)
    assert rlp.untouched_outside(at)
    assert logits.same() and value.same()  # inputs, pads and guards as they were
    ar = np.arange(B)[live]
    lp_m = m["logp"][ar, a[live]]
    z = torch.from_numpy(c["logits"][live])
    lp_ref = torch.log(torch.softmax(z, dim=-1).gather(1, torch.from_numpy(a[live])[:, None]).squeeze(1))
    ok, info = _bound("log-prob", rlp.host()[at], lp_m, lp_ref.numpy())
    assert ok, info


# ---- head loss and pair surrogate ---------------------------------------------------------------
_REF32 = {}


def _ref32(b, mode):
    if (b, mode) not in _REF32:
        _REF32[(b, mode)] = K.torch_head(K.head_case(b, mode), torch.float32)
    return _REF32[(b, mode)]


@pytest.mark.parametrize("strides", [(4, 1, 4, 1), (8, 3, 6, 2)], ids=["dense", "padded"])
@pytest.mark.parametrize("mode", K.HEAD_MODES)
@pytest.mark.parametrize("b", K.HEAD_BS)
def test_head_loss_matches_float64_model(b, mode, strides):
    """mz_ppo_head_loss against the float64 model; e_ref from the package's float32 torch
    expressions on the CPU. Rows whose surrogate column has a ratio within 2^-18 of a clip
    boundary are left out of dlogits (a float32 expf may land across it, which moves dsum by a
    whole term), and those columns' model terms are taken off every side of the loss."""
    N, L = _lib()
    ldl, ldv, ldg, ldvg = strides
    c = K.head_case(b, mode)
    m = c["model"]
    logits, value = Buf(np.float32, b, 4, ldl, c["logits"]), Buf(np.float32, b, 1, ldv, c["value"])
    d = [_dev(c[k]) for k in ("action", "lp_old", "adv", "ret")]
    coef = _dev(np.array([c["coef"]], np.float32))
    scratch, loss = Buf(np.float32, 12 * b), Buf(np.float32, 1)
    dlogits, dvalue = Buf(np.float32, b, 4, ldg), Buf(np.float32, b, 1, ldvg)
    N.check(L.mz_ppo_head_loss(logits.ptr, ldl, value.ptr, ldv, *[x.data_ptr() for x in d],
                               coef.data_ptr(), b, c["clip"], scratch.ptr, loss.ptr, dlogits.ptr,
                               ldg, dvalue.ptr, ldvg, _stream()))
    torch.cuda.synchronize()
    every4, every1 = np.ones((b, 4), bool), np.ones((b, 1), bool)
    assert dlogits.untouched_outside(every4) and dvalue.untouched_outside(every1)
    assert loss.untouched_outside(np.ones((1, 1), bool)) and scratch.untouched_outside(np.ones((12 * b, 1), bool))
    assert logits.same() and value.same()
    total32, dl32, dv32 = _ref32(b, mode)
    ok = m["clear"]
    left = K.pair_terms_left_out(c)
    print(f"b {b} {mode} strides {strides}: columns not clear {int((~ok).sum())}")
    assert (~ok).sum() <= b // 100
    res = [_bound("loss", [float(loss.host()[0, 0]) + left], [m["total"] + left], [total32 + left]),
           _bound("dlogits", dlogits.host()[ok], m["dlogits"][ok], dl32[ok]),
           _bound("dvalue", dvalue.host()[:, 0], m["dvalue"], dv32)]
    for good, info in res:
        assert good, info


@pytest.mark.parametrize("b", K.HEAD_BS)
def test_pair_surrogate_ties_and_inclusive_boundaries_are_exact(b):
    """lp_new[i] == lp_old[j] for all pairs, so r = expf(0) = 1 exactly. clip = 0: every pair is a
    tie on an inclusive boundary (w = 1): part[i] == b adv[i], dsum[i] == b. clip = 0.3 with zero
    advantages: s1 == s2 == 0 with r inside: dsum[i] == b, part[i] == 0. Advantages are multiples
    of 1/64 below 4, so every float32 partial sum of b of them is exact."""
    N, L = _lib()
    rng = np.random.default_rng(b)
    lp = _dev(np.full(b, np.float32(-0.8125)))
    adv = (rng.integers(-256, 257, b) / 64.0).astype(np.float32)
    for clip, a in ((0.0, adv), (0.3, np.zeros(b, np.float32)), (0.3, adv)):
        pm, dm, clear = M.pair(np.full(b, -0.8125), np.full(b, -0.8125), a, clip)
        assert clear.all() and np.array_equal(dm, np.full(b, float(b)))
        ad = _dev(a)
        part, dsum = Buf(np.float32, b), Buf(np.float32, b)
        N.check(L.mz_pair_surrogate(lp.data_ptr(), lp.data_ptr(), ad.data_ptr(), b, clip, part.ptr,
                                    dsum.ptr, _stream()))
        torch.cuda.synchronize()
        gp, gd = part.host()[:, 0], dsum.host()[:, 0]
        print(f"b {b} clip {clip}: part differs in {int((gp != pm).sum())}, dsum in {int((gd != dm).sum())};"
              f" dsum[0] {gd[0]} part[0] {gp[0]} (model {dm[0]}, {pm[0]})")
        assert part.same(pm.astype(np.float32)) and dsum.same(dm.astype(np.float32))
        assert np.array_equal(gp.astype(np.float64), b * a.astype(np.float64))
