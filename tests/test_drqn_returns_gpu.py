"""The returns kernel and the forwards' second form (csrc/mz_drqn.hip: k_drqn_seq_ret, k_drqn_win_ret,
k_drqn_seq_fwd_q, k_drqn_win_fwd_q) through the C ABI on the hand-built memory of
tests/drqn_nstep_mem.py (L = 8, 12 episodes of 1 .. 8 steps, both term values).

1. The returns kernel on hand-written qa, q4, sel and rewards equals tests/drqn_nstep_model.py's
   returns_exact bit for bit (a NaN compares as a NaN: its payload is nobody's contract).
2. With n_step = 1 and no sel the new chain (both forwards, returns, backward) gives the old chain's
   bits, and max over q4 is the old qmax."""
import numpy as np
import pytest
import torch

import drqn_nstep_mem as MM
import drqn_nstep_model as NM
import drqn_window_model as W

pytestmark = pytest.mark.gpu
L = MM.L
LENS = [1, 2, 3, 4, 5, 6, 7, 8, 3, 6, 8, 7]
NEG0 = np.array(0x80000000, np.uint32).view(np.float32)[()]


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def js_of(lens, T):
    """test_drqn_window_gpu's choice: first, inner and last windows all occur."""
    return [(e + e // 6 + 1) % W.windows_in(n, T) for e, n in enumerate(lens)]


def directory(kind, seed, K=0, stored=True):
    """kind: "seq" (whole episodes) or the window T."""
    if kind == "seq":
        return MM.Mem(LENS, seed, L).episodes()
    return MM.Mem(LENS, seed, kind).windows(js_of(LENS, kind), K, stored)


def same_bits(a, b):
    """Equal bit for bit where neither is a NaN; NaN exactly where the other is."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))


def hand_rows(mem, seed):
    """Hand-written rows for one learner: qa [R], q4 [R][4], sel [R] over the whole buffer, with
    +-0, a NaN row, a partly NaN row, ties and sel mostly off the maximum; rewards +-0 in the
    memory. Rows outside the directory are NaN (sel: a sentinel)."""
    rng = np.random.default_rng(seed)
    R = mem.rows_cap
    qa, q4 = np.full(R, np.nan, np.float32), np.full((R, 4), np.nan, np.float32)
    sel = np.full(R, -7, np.int32)
    rows, steps = mem.all_rows(), mem.step_rows()
    qa[steps] = (rng.random(len(steps)) - 0.5).astype(np.float32)
    q4[rows] = (rng.random((len(rows), 4)) * 2 - 1).astype(np.float32)
    sel[rows] = rng.integers(0, 4, len(rows))
    qa[steps[0]], qa[steps[-1]] = 0.0, NEG0
    # the step after the first training step of spans 1, 2, 3, 4 and 5 (m >= 1: the row exists)
    r1 = mem.row0 + 1
    q4[r1[1]] = [NEG0, 0.0, -1.0, -2.0]          # the maximum is a zero beside its twin
    q4[r1[2]] = [0.25, 0.75, 0.75, 0.75]         # a tie at the maximum
    q4[r1[3]] = [np.nan, 1.0, np.nan, 0.5]       # fmaxf passes a NaN by
    sel[r1[3]] = 3
    q4[r1[4]] = [np.nan] * 4                     # a NaN row: y, d and the span's loss are NaN
    q4[r1[5]] = [NEG0, NEG0, NEG0, NEG0]
    sel[r1[2]] = 0                               # not the maximum
    for e, ep in enumerate(mem.eps):             # rewards +0 and -0
        if len(ep["r"]) >= 2:
            ep["r"][e % len(ep["r"])] = NEG0 if e % 2 else 0.0
    mem.write()
    return qa, q4, sel


@pytest.mark.parametrize("kind", ["seq", 3, 8], ids=lambda k: f"{k}")
@pytest.mark.parametrize("N", [1, 2, 3, 5, 9])
def test_returns_equal_the_exact_model(lib, kind, N):
    """Two learners in one launch: learner 0 with n_step N, learner 1 with another; each is run
    double (reads sel) and not (its flag is 0, or no sel is given at all)."""
    N1 = {1: 3, 2: 9, 3: 1, 5: 2, 9: 5}[N]
    mems = [directory(kind, 40 + p, K=0) for p in range(2)]
    hand = [hand_rows(m, 50 + p) for p, m in enumerate(mems)]
    pop = MM.Pop(lib, mems)
    if kind == 3:  # the shapes the case is there for
        ends = {(w["s"] + w["m"] == n, w["term"]) for w, n in zip(mems[0].ws, mems[0].lens)}
        assert ends == {(True, True), (True, False), (False, False)}
        assert any(w["m"] == 1 and w["s"] > 0 for w in mems[0].ws)
    assert any(m_ == 1 for m_ in mems[0].m) and max(mems[0].m) < 9  # N = 9 > every m
    for double, with_sel in [((1, 1), True), ((1, 0), True), (None, True), (None, False)]:
        o = pop.buffers()
        for k, j in (("qa", 0), ("q4", 1), ("sel", 2)):
            o[k].copy_(torch.from_numpy(np.stack([h[j] for h in hand])))
        pop.returns(o, [N, N1], double, with_sel)
        torch.cuda.synchronize()
        for p, (mem, (qa, q4, sel)) in enumerate(zip(mems, hand)):
            reads_sel = with_sel and (double is None or bool(double[p]))
            y = np.full(mem.rows_cap, np.nan, np.float32)
            d = y.copy()
            loss = np.zeros(mem.E)
            for e, (w, r0) in enumerate(zip(mem.ws, mem.row0)):
                m = len(w["a"])
                rows = r0 + np.arange(m + 1)
                r = mem.eps[e]["r"][w["s"]:w["s"] + m]
                y[rows[:m]], d[rows[:m]], loss[e] = NM.returns_exact(
                    r, qa[rows[:m]], q4[rows], sel[rows] if reads_sel else None, (N, N1)[p],
                    MM.GAMMA, w["term"], mem.steps)
            tag = (kind, N, double, with_sel, p)
            assert same_bits(o["y"][p].cpu().numpy(), y), tag      # NaN outside the directory
            assert same_bits(o["d"][p].cpu().numpy(), d), tag
            assert same_bits(o["ep_loss"][p].cpu().numpy(), loss), tag
            if (N, N1)[p] == 1 and not reads_sel:  # every step bootstraps from the row after it
                assert np.isnan(loss).sum() == 1 and np.isnan(y[mem.step_rows()]).sum() == 1
            # the inputs are inputs
            assert same_bits(o["qa"][p].cpu().numpy(), qa) and same_bits(o["q4"][p].cpu().numpy(), q4)
            assert np.array_equal(o["sel"][p].cpu().numpy(), sel)


@pytest.mark.parametrize("kind", ["seq", 3, 8], ids=lambda k: f"{k}")
@pytest.mark.parametrize("P", [1, 3])
def test_n_step_one_without_sel_is_the_old_chain(lib, kind, P):
    """The same directory through both chains; P = 3: learner 1 is not due and keeps its
    sentinels in both. Windows: K = 3 (T = 3) with stored state, zero state for learner 2."""
    K = 3 if kind == 3 else 0
    mems = [directory(kind, 60 + p, K=K, stored=p != 2) for p in range(P)]
    pop = MM.Pop(lib, mems)
    due = None if P == 1 else [1, 0, 1]
    old, new = pop.buffers(), pop.buffers()
    pop.forward_old(old, due)
    pop.backward(old, due)
    pop.forward_q(new, due)
    pop.returns(new, [1] * P, None, False, due)
    pop.backward(new, due)
    torch.cuda.synchronize()
    for k in ("y", "d", "ep_loss", "qa", "stash", "gpart", "grads", "loss"):
        a, b = old[k].cpu().numpy(), new[k].cpu().numpy()
        assert np.array_equal(a, b, equal_nan=True), k
    for p, mem in enumerate(mems):
        rows = mem.all_rows()
        rest = np.setdiff1d(np.arange(mem.rows_cap), rows)
        q4, qmax = new["q4"][p].cpu().numpy(), old["qmax"][p].cpu().numpy()
        sel = new["sel"][p].cpu().numpy()
        if due is not None and not due[p]:
            assert np.isnan(q4).all() and np.isnan(qmax).all() and (sel == -7).all()
            assert np.isnan(new["y"][p].cpu().numpy()).all()
            continue
        assert np.array_equal(q4[rows].max(axis=1), qmax[rows]) and not np.isnan(qmax[rows]).any()
        assert np.isnan(q4[rest]).all() and np.isnan(qmax[rest]).all() and (sel[rest] == -7).all()
        assert set(sel[rows].tolist()) <= {0, 1, 2, 3}
        y = new["y"][p].cpu().numpy()
        assert not np.isnan(y[mem.step_rows()]).any()
        assert np.isnan(y[np.setdiff1d(np.arange(mem.rows_cap), mem.step_rows())]).all()
        assert not np.isnan(new["grads"][p].cpu().numpy()).any()


def test_the_new_entry_points_refuse_bad_arguments(lib):
    from mazerl import _native as N
    z = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    p, st = z.data_ptr(), torch.cuda.current_stream().cuda_stream

    def fq(params=p, hid=32, target=1, P=2, E=2, T=3, K=3, cap=5, q4=p, stash=p, sel=p, burn=p):
        return lib.mz_drqn_pop_window_forward_q(params, hid, target, P, E, L, T, K, cap, burn, p,
                                                None, p, None, p, p, p, q4, stash, p, sel, st)

    def sq(params=p, hid=32, target=1, P=2, E=2, cap=5, q4=p, sel=p, slot=p):
        return lib.mz_drqn_pop_seq_forward_q(params, hid, target, P, E, L, cap, None, p, slot, p, p,
                                             p, q4, p, p, sel, st)

    def wr(ns=p, nmax=3, gamma=p, P=2, E=2, T=3, K=3, cap=5, q4=p, y=p, burn=p):
        return lib.mz_drqn_pop_window_returns(ns, nmax, None, gamma, burn, None, P, E, L, T, K, cap,
                                              p, p, p, p, p, p, q4, None, y, p, p, st)

    def sr(ns=p, nmax=3, gamma=p, P=2, E=2, cap=5, q4=p, y=p, term=p):
        return lib.mz_drqn_pop_seq_returns(ns, nmax, None, gamma, None, P, E, L, cap, p, term, p, p,
                                           p, p, p, q4, None, y, p, p, st)

    bad = [lambda: fq(params=None), lambda: fq(q4=None), lambda: fq(target=0, sel=None),
           lambda: fq(target=0, stash=None), lambda: fq(hid=16), lambda: fq(P=0), lambda: fq(E=0),
           lambda: fq(E=6), lambda: fq(T=0), lambda: fq(K=-3), lambda: fq(K=4),
           lambda: fq(burn=None),
           lambda: sq(params=None), lambda: sq(q4=None), lambda: sq(target=0, sel=None),
           lambda: sq(hid=16), lambda: sq(P=0), lambda: sq(E=0), lambda: sq(E=6),
           lambda: sq(slot=None),
           lambda: wr(ns=None), lambda: wr(nmax=0), lambda: wr(nmax=-2), lambda: wr(gamma=None),
           lambda: wr(P=0), lambda: wr(E=0), lambda: wr(E=6), lambda: wr(T=0), lambda: wr(K=4),
           lambda: wr(q4=None), lambda: wr(y=None), lambda: wr(burn=None),
           lambda: sr(ns=None), lambda: sr(nmax=0), lambda: sr(gamma=None), lambda: sr(P=0),
           lambda: sr(E=0), lambda: sr(E=6), lambda: sr(q4=None), lambda: sr(y=None),
           lambda: sr(term=None)]
    for k, f in enumerate(bad):
        assert f() == -1, k  # MZ_EINVAL
        with pytest.raises(ValueError):
            N.check(f())
    torch.cuda.synchronize()
    assert bool((z == 0).all())
