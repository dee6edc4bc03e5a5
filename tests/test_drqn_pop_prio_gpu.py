"""The prioritized replay-window kernels with per-learner parameters (csrc/mz_drqn.hip:
k_drqn_prio_store, k_drqn_prio_sample, k_drqn_prio_update under mz_drqn_pop_prio_*) through the C
ABI, L = 8, P = 3 learners with different seeds, update counts, burn-ins (0 and T), alpha (0, 0.5,
0.9), beta (0, 0.4, 1), eta and eps. A population launch over [P]... buffers is defined as the
single entry point on each learner's block with that learner's values, and the two run the same
device code, so every comparison with the single entry point is `==` on the bits;
tests/test_drqn_prio_gpu.py holds the single entry points to tests/drqn_prio_model.py, and one case
here is compared with the model directly, under that test's conditions (directory and sums exact,
isw within one float32 ulp, masses within one unit)."""
import numpy as np
import pytest
import torch

import drqn_prio_model as PM
import drqn_window_model as W
import test_drqn_window_gpu as WG

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, L = WG.H, WG.L
ONE, CEIL = PM.ONE, PM.CEIL
SENT = 0x7FFFFFF1  # no mass: above 2^30
P = 3
SEEDS, COUNTERS = (5, 6, 77), (0, 3, 9)
ALPHA, BETA = (0.0, 0.5, 0.9), (0.0, 0.4, 1.0)
ETA, EPS = (0.9, 0.5, 1.0), (1e-3, 1e-2, 0.25)
_d, _stream = WG._d, WG._stream


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def _i32(a):
    return _d(np.asarray(a, np.int32))


def _i64(a):
    return _d(np.asarray(a, np.int64))


def _f64(a):
    return _d(np.asarray(a, np.float64))


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _burn(T):
    return [0, T, 0]


# ---- entry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [5, 7])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_store_is_the_single_store_on_every_learners_block(lib, cap, T):
    """b = 9 instances per learner; learner 0 finishes two episodes, learner 1 nine (more than
    there are slots), learner 2 none. Every learner has its own head and its own prio_max."""
    from mazerl import _native as N
    b, Wn = 9, W.windows_in(L, T)
    t1 = T + 1 if T + 1 <= L else L - 1
    fin = [(2, 2), (7, T)] + [(b + i, [2, T, t1, L, 5, 1, 3, L, 2][i]) for i in range(b)]
    B = P * b
    fin_id = _i32([i for i, _ in fin] + [0] * (B - len(fin)))
    fin_len = _i32([n for _, n in fin] + [0] * (B - len(fin)))
    fin_count = _i32([len(fin)])
    ring = _i64([[cap - 1, cap], [2, 3], [1, 1]])
    pmax = _i32([ONE, 3 * ONE + 17, CEIL, SENT])
    kw = dict(device=DEV)
    prio = torch.full((P + 1, cap, Wn), SENT, dtype=torch.int32, **kw)
    psum = torch.full((P + 1, cap), -1, dtype=torch.int64, **kw)
    N.check(lib.mz_drqn_pop_prio_store(H, P, b, L, T, fin_id.data_ptr(), fin_len.data_ptr(),
                                       fin_count.data_ptr(), cap, prio.data_ptr(), psum.data_ptr(),
                                       pmax.data_ptr(), ring.data_ptr(), _stream()))
    runs = [fin[:2], fin[2:], []]
    for p in range(P):
        one_prio = torch.full((cap, Wn), SENT, dtype=torch.int32, **kw)
        one_psum = torch.full((cap,), -1, dtype=torch.int64, **kw)
        run = runs[p]
        ids = _i32([i - p * b for i, _ in run] + [0] * (b - len(run)))
        lens = _i32([n for _, n in run] + [0] * (b - len(run)))
        count, one_ring = _i32([len(run)]), ring[p].clone()
        N.check(lib.mz_drqn_prio_store(H, b, L, T, ids.data_ptr(), lens.data_ptr(),
                                       count.data_ptr(), cap, one_prio.data_ptr(),
                                       one_psum.data_ptr(), pmax[p:].data_ptr(),
                                       one_ring.data_ptr(), _stream()))
        assert _eq(prio[p], one_prio) and _eq(psum[p], one_psum), p
        # and the model of that learner's run
        mp, ms = np.full((cap, Wn), SENT, np.int64), np.full(cap, -1, np.int64)
        PM.store(mp, ms, int(pmax[p]), int(ring[p, 0]), [(i - p * b, n) for i, n in run], b, L, T)
        assert np.array_equal(prio[p].cpu().numpy(), mp) and np.array_equal(psum[p].cpu().numpy(), ms)
    assert (prio[1] != SENT).all()                              # nine episodes over <= 7 slots
    assert (prio[2] == SENT).all() and (psum[2] == -1).all()    # no episode: nothing written
    assert (prio[P] == SENT).all() and (psum[P] == -1).all()    # the row past the population
    assert pmax.cpu().tolist() == [ONE, 3 * ONE + 17, CEIL, SENT]  # read, never written


# ---- sampling -----------------------------------------------------------------------------------
def _masses(rng, cap, T, empty=()):
    """test_drqn_prio_gpu's memory: lengths 1 .. L (the first four 1, T, T + 1 or L - 1, L), masses
    from 1 to 2^30 on every window an episode has, the slots in `empty` without an episode."""
    Wn = W.windows_in(L, T)
    lens = rng.integers(1, L + 1, cap).astype(np.int32)
    lens[:4] = [1, T, T + 1 if T + 1 <= L else L - 1, L]
    lens[list(empty)] = 0
    prio = np.zeros((cap, Wn), np.int64)
    for s, n in enumerate(lens):
        if n:
            nw = W.windows_in(n, T)
            prio[s, :nw] = np.minimum(CEIL, 1 + (rng.random(nw) ** 4 * CEIL).astype(np.int64))
    return lens, prio


class _Sampled:
    """One population launch over P learners' memories (a sentinel row past them) and the single
    entry point on each learner's block, into buffers of its own."""

    def __init__(self, lib, cap, E, T, seed, empty=(), due=(1, 1, 1)):
        from mazerl import _native as N
        rng = np.random.default_rng(seed)
        self.E, self.T, self.cap, self.K = E, T, cap, _burn(T)
        mem = [_masses(rng, cap, T, empty) for _ in range(P)]
        self.lens, self.prio = np.stack([m[0] for m in mem]), np.stack([m[1] for m in mem])
        lens_d, prio_d = _i32(self.lens), _i32(self.prio)
        psum_d = _i64(self.prio.sum(axis=2))
        kw = dict(device=DEV)
        self.out = out = {
            "wdir": torch.full((P + 1, 5, E), -9, dtype=torch.int32, **kw),
            "off": torch.full((P + 1, E), -9, dtype=torch.int64, **kw),
            "tot": torch.full((P + 1, 2), -9, dtype=torch.int64, **kw),
            "isw": torch.full((P + 1, E), float("nan"), **kw)}
        per = (_i64(SEEDS), _i64(COUNTERS), _i32(self.K), _f64(BETA), _i32(due))
        N.check(lib.mz_drqn_pop_prio_sample(
            *(t.data_ptr() for t in per), H, P, E, L, T, T, cap, lens_d.data_ptr(),
            prio_d.data_ptr(), psum_d.data_ptr(), out["wdir"].data_ptr(), out["off"].data_ptr(),
            out["tot"].data_ptr(), out["isw"].data_ptr(), _stream()))
        self.one = []
        for p in range(P):
            o = {"wdir": torch.full((5, E), -9, dtype=torch.int32, **kw),
                 "off": torch.full((E,), -9, dtype=torch.int64, **kw),
                 "tot": torch.full((2,), -9, dtype=torch.int64, **kw),
                 "isw": torch.full((E,), float("nan"), **kw)}
            N.check(lib.mz_drqn_prio_sample(
                SEEDS[p], COUNTERS[p], H, E, L, T, self.K[p], cap, lens_d[p].data_ptr(),
                prio_d[p].data_ptr(), psum_d[p].data_ptr(), o["wdir"].data_ptr(),
                o["off"].data_ptr(), o["tot"].data_ptr(), o["isw"].data_ptr(), BETA[p], _stream()))
            self.one.append(o)

    def check(self, due=(1, 1, 1)):
        for k, t in self.out.items():
            for p in range(P):
                if due[p]:
                    assert _eq(t[p], self.one[p][k]), (k, p)
                else:  # a learner that sits the update out keeps its sentinels
                    assert _eq(t[p], t[P]), (k, p)
            assert bool((t[P] == -9).all()) if k != "isw" else bool(torch.isnan(t[P]).all()), k


@pytest.mark.parametrize("cap", [5, 7])
@pytest.mark.parametrize("E", [1, 3, 65])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_sampler_is_the_single_sampler_on_every_learners_block(lib, cap, E, T):
    s = _Sampled(lib, cap, E, T, 1800 + 10 * cap + E + T, empty=(4,) if cap == 7 else ())
    s.check()
    wd = s.out["wdir"].cpu().numpy()
    assert (wd[:P, 4] >= 1).all()  # every position of every learner has a window
    # learner 1 alone burns in (K = T); with T = 8 = L no window has a step before it
    if T < L and E == 65:
        assert (wd[1, 3] > 0).any() and (wd[0, 3] == 0).all() and (wd[2, 3] == 0).all()
    isw = s.out["isw"].cpu().numpy()
    assert (isw[0] == 1.0).all()  # beta_0 = 0


def test_sampler_matches_the_integer_model(lib):
    """One case against tests/drqn_prio_model.py directly: the directory and the totals exact, isw
    within one float32 ulp of the model's float64 value rounded to float32."""
    cap, E, T = 7, 65, 3
    s = _Sampled(lib, cap, E, T, 1900, empty=(4,))
    s.check()
    for p in range(P):
        m = PM.sample(s.prio[p], s.lens[p], SEEDS[p], COUNTERS[p], E, T, s.K[p], BETA[p])
        wd = s.out["wdir"][p].cpu().numpy()
        for row, key in enumerate(("slot", "n", "b", "k", "m")):
            assert np.array_equal(wd[row], np.array(m[key])), (p, key)
        assert np.array_equal(s.out["off"][p].cpu().numpy(), m["off"])
        assert tuple(s.out["tot"][p].tolist()) == m["tot"]
        isw = s.out["isw"][p].cpu().numpy()
        want = m["isw"].astype(np.float32)
        worst = np.abs(isw.astype(np.float64) - want) / np.spacing(want)
        print(f"learner {p} (beta {BETA[p]}): isw off by at most {worst.max():.2f} ulp")
        assert (worst <= 1.0).all(), (p, isw, want)
        if BETA[p] == 0.0:
            assert (isw == 1.0).all()
        else:
            assert isw.max() == 1.0 and (isw > 0).all() and isw.min() < 1.0


def test_sampler_leaves_a_learner_that_is_not_due_alone(lib):
    due = (1, 0, 1)
    s = _Sampled(lib, 7, 3, 3, 1901, due=due)
    s.check(due)
    assert bool((s.out["wdir"][1] == -9).all()) and bool(torch.isnan(s.out["isw"][1]).all())


def test_sampler_over_more_than_one_group_of_slots(lib):
    """200 slots are 4 groups of 64 (a last one of 8): the group path under a nonzero offset of
    the learner's rows."""
    s = _Sampled(lib, 200, 3, 8, 1902, empty=range(40, 120))
    s.check()
    slots = s.out["wdir"][:P, 0].cpu().numpy()
    assert (slots >= 64).any(axis=1).all()  # every learner's last stratum: beyond the first group


# ---- the write-back -----------------------------------------------------------------------------
class _Updated:
    """Hand-made directories (a window twice and two windows of one episode among them), random
    rows qa / y / d, loss terms, weights and masses per learner; one population launch and the
    single entry point on copies of each learner's block."""

    def __init__(self, lib, cap, E, T, seed, due=(1, 1, 1)):
        from mazerl import _native as N
        rng = np.random.default_rng(seed)
        self.E, self.T, self.cap = E, T, cap
        Wn, R = W.windows_in(L, T), E * (min(T, L) + 2)
        K = _burn(T)
        wdir = np.zeros((P, 5, E), np.int32)
        off = np.zeros((P, E), np.int64)
        tot = np.zeros((P, 2), np.int64)
        prio = np.full((P + 1, cap, Wn), SENT, np.int64)
        prio[:P] = 0
        for p in range(P):
            lens, prio[p] = _masses(rng, cap, T)
            for e in range(E):
                slot = int(rng.integers(0, cap)) if e else 3  # slot 3: n = L, every window
                if e == E - 1 and E >= 3:
                    slot = int(wdir[p, 0, 0])
                n = int(lens[slot])
                j = int(rng.integers(0, W.windows_in(n, T)))
                if e == E - 1 and E >= 3:                     # position 0's window once more
                    j = int(wdir[p, 2, 0] + wdir[p, 3, 0]) // T
                s = j * T
                bb = max(0, s - K[p])
                wdir[p, :, e] = (slot, n, bb, s - bb, min(T, n - s))
            m = wdir[p, 4].astype(np.int64)
            off[p] = np.concatenate([[0], np.cumsum(m + 2)[:-1]])
            tot[p] = ((m + 2).sum(), m.sum())
        self.wdir, self.prio0 = wdir, prio
        psum = np.concatenate([prio[:P].sum(axis=2), np.full((1, cap), -1)]).astype(np.int64)
        pmax = np.array([ONE, int(prio[1].max()), 5, SENT], np.int64)
        self.qa = rng.standard_normal((P + 1, R)).astype(np.float32)
        self.y = rng.standard_normal((P + 1, R)).astype(np.float32)
        for p in range(P):  # a window sampled twice has the same rows twice, as a forward gives it
            first = {}
            for e in range(E):
                key = (int(wdir[p, 0, e]), int(wdir[p, 2, e] + wdir[p, 3, e]))
                e0 = first.setdefault(key, e)
                for a in (self.qa, self.y):
                    a[p, off[p, e]:off[p, e] + wdir[p, 4, e] + 2] = \
                        a[p, off[p, e0]:off[p, e0] + wdir[p, 4, e0] + 2]
        d0 = rng.standard_normal((P + 1, R)).astype(np.float32)
        ep0 = rng.random((P + 1, E))
        isw = (0.05 + 0.95 * rng.random((P + 1, E))).astype(np.float32)
        isw[:, 0] = 1.0
        self.isw = isw
        self.inputs = dict(prio=_i32(prio), psum=_i64(psum), pmax=_i32(pmax), d=_d(d0), ep=_d(ep0))
        self.out = o = {k: v.clone() for k, v in self.inputs.items()}
        wd, of, to = _i32(wdir), _i64(off), _i64(tot)
        qa, y, w = _d(self.qa), _d(self.y), _d(isw)
        per = (_f64(ALPHA), _f64(ETA), _f64(EPS), _i32(due))
        N.check(lib.mz_drqn_pop_prio_update(
            *(t.data_ptr() for t in per), H, P, E, L, T, cap, wd.data_ptr(), of.data_ptr(),
            to.data_ptr(),
            qa.data_ptr(), y.data_ptr(), o["d"].data_ptr(), o["ep"].data_ptr(), w.data_ptr(),
            o["prio"].data_ptr(), o["psum"].data_ptr(), o["pmax"].data_ptr(), _stream()))
        self.one = []
        for p in range(P):
            c = {k: v[p].clone() if k != "pmax" else v[p:p + 1].clone()
                 for k, v in self.inputs.items()}
            N.check(lib.mz_drqn_prio_update(
                H, E, L, T, cap, wd[p].data_ptr(), of[p].data_ptr(), to[p].data_ptr(),
                qa[p].data_ptr(), y[p].data_ptr(), c["d"].data_ptr(), c["ep"].data_ptr(),
                w[p].data_ptr(), ALPHA[p], ETA[p], EPS[p], c["prio"].data_ptr(),
                c["psum"].data_ptr(), c["pmax"].data_ptr(), _stream()))
            self.one.append(c)
        self.off = off

    def check(self, due=(1, 1, 1)):
        for k, t in self.out.items():
            for p in range(P):
                got = t[p] if k != "pmax" else t[p:p + 1]
                if due[p]:
                    assert _eq(got, self.one[p][k]), (k, p)
                else:
                    assert _eq(t[p], self.inputs[k][p]), (k, p)
            assert _eq(t[P], self.inputs[k][P]), k  # the row past the population


@pytest.mark.parametrize("cap", [5, 7])
@pytest.mark.parametrize("E", [1, 3, 65])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_update_is_the_single_update_on_every_learners_block(lib, cap, E, T):
    u = _Updated(lib, cap, E, T, 2800 + 10 * cap + E + T)
    u.check()
    prio, psum = u.out["prio"].cpu().numpy().astype(np.int64), u.out["psum"].cpu().numpy()
    assert np.array_equal(psum[:P], prio[:P].sum(axis=2))
    assert (prio[0][u.wdir[0, 0], (u.wdir[0, 2] + u.wdir[0, 3]) // T] == ONE).all()  # alpha_0 = 0
    if E > 1:  # (position 0 has the weight 1)
        assert not _eq(u.out["d"][1], u.inputs["d"][1])  # the weights scaled the rows


def test_update_matches_the_model(lib):
    """One case against tests/drqn_prio_model.py directly: every written mass within one unit of
    the model's under that learner's (alpha, eta, eps), every slot sum exact, prio_max the
    maximum of its start and the written masses."""
    cap, E, T = 7, 65, 3
    u = _Updated(lib, cap, E, T, 2900)
    u.check()
    prio = u.out["prio"].cpu().numpy().astype(np.int64)
    assert np.array_equal(u.out["psum"].cpu().numpy()[:P], prio[:P].sum(axis=2))
    for p in range(P):
        slot, j, m = u.wdir[p, 0], (u.wdir[p, 2] + u.wdir[p, 3]) // T, u.wdir[p, 4]
        rows = [u.off[p, e] + 1 + np.arange(m[e]) for e in range(E)]
        want = np.array([PM.mass_of(np.abs(u.qa[p][r] - u.y[p][r]), ALPHA[p], ETA[p], EPS[p])
                         for r in rows])
        got = prio[p][slot, j]
        diff = np.abs(got - want)
        print(f"learner {p} (alpha {ALPHA[p]}, eta {ETA[p]}, eps {EPS[p]}): {int((diff != 0).sum())}"
              f" of {E} masses differ from the model's, largest difference {int(diff.max())}")
        assert (diff <= 1).all(), (p, got, want)
        touched = np.zeros_like(prio[p], bool)
        touched[slot, j] = True
        assert np.array_equal(prio[p][~touched], u.prio0[p][~touched])
        assert int(u.out["pmax"][p]) == max(int(u.inputs["pmax"][p]), int(got.max()))


def test_update_leaves_a_learner_that_is_not_due_alone(lib):
    due = (0, 1, 1)
    u = _Updated(lib, 5, 3, 3, 2901, due=due)
    u.check(due)
