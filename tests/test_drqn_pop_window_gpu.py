"""Replay windows in recurrent DQN populations (csrc/mz_drqn.hip k_drqn_snap_store,
k_drqn_win_sample, k_drqn_win_fwd, k_drqn_win_bwd at P > 1, k_drqn_reduce's strided lengths)
through the C ABI.

The single-learner window entry points are pinned to the float64 model by
tests/test_drqn_window_gpu.py, so they are the yardstick: learner p of a population call must give
the bits the single call gives on learner p's rows with (T, K_p, stored or NULL state), `==` and no
tolerance. Every output starts as a NaN (or -9) sentinel, so "equal bits" also says that both
wrote the same places and nothing else. One test holds the population chain to the float64 model
(tests/drqn_window_model.py + learner_model.adamw_step) directly with the project's bound
    e_k <= 4 e_ref + 8 u max|tensor|,  u = 2^-24,
e_ref from torch's float32 window_td_loss + autograd on the CPU. Fixed shape: L = 8, P = 3."""
import ctypes as C

import numpy as np
import pytest
import torch

import drqn_model as M
import drqn_window_model as W
import learner_model as LM

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
H, ROW, STASH, PARAMS, SNAP, L = 32, 8, 192, 5252, 64, 8
SHAPES = [(128, 6), (128, 32), (128,), (128,), (4, 32), (4,)]
OFFS = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in SHAPES])])
ADAM = (0.9, 0.999, 1e-8, 1e-2)
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _net(seed, scale=2.0):
    from mazerl.agents.lstm_dqn_agent import DQN
    torch.manual_seed(seed)
    net = DQN(6, 4, H, torch.device("cpu"))
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(scale)
    return net


def _row(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()


def _ptrs(row):
    """The six device pointers of one flat [5252] row (the single-learner entry points' params)."""
    return (C.c_void_p * 6)(*[row.data_ptr() + 4 * int(o) for o in OFFS[:6]])


def _bits(t):
    """A tensor's bits, so sentinels (NaN) compare equal to themselves."""
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32) if t.is_floating_point() \
        else t


def _eq(a, b):
    return torch.equal(_bits(a), _bits(b))


def _signed(u):
    return u - (1 << 64) if u >> 63 else u


def _nan(*s, dtype=torch.float32):
    return torch.full(s, NAN, dtype=dtype, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _episodes(rng, lens, term):
    """Random words everywhere, valid episodes of the given lengths in every slot."""
    P, cap = lens.shape
    mem = rng.integers(-2 ** 31, 2 ** 31 - 1, (P, cap, L + 1, ROW)).astype(np.int32)
    for p in range(P):
        for s in range(cap):
            n = int(lens[p, s])
            mem[p, s, :n + 1, :6] = rng.random((n + 1, 6)).astype(np.float32).view(np.int32)
            mem[p, s, :n, 6] = rng.integers(0, 4, n)
            mem[p, s, :n, 7] = (rng.random(n) - 0.5).astype(np.float32).view(np.int32)
    return mem


# ---- 1. the snapshot store ----------------------------------------------------------------------
def test_snapshot_store_equals_per_learner_stores_and_agrees_with_the_store(lib):
    """P = 3, b = 4, capacity 4, T = 3: learner 0 has no finished episode, learner 1 two, learner 2
    six (more than its slots; b = 4 instances can list six only with repeats, which carry the same
    length so that mz_drqn_store's copies do not race) with its head at 3, so its ring wraps. The
    call comes before mz_drqn_pop_store, reads the heads and leaves them; afterwards every slot
    the store filled holds that episode's snapshots."""
    from mazerl import _native as N
    P, b, CAP, T = 3, 4, 4, 3
    B, NS = P * b, W.windows_in(L, T)
    rng = np.random.default_rng(17)
    fin_id = np.array([5, 7, 8, 9, 9, 10, 11, 11] + [0] * (B - 8), np.int32)
    fin_len = np.array([3, 8, 5, 8, 8, 2, 7, 7] + [0] * (B - 8), np.int32)
    runs = [(0, 0), (0, 2), (2, 8)]
    snap = (rng.random((B, NS, SNAP)) - 0.5).astype(np.float32)
    ring0 = np.array([[2, 3], [1, 1], [3, 4]], np.int64)
    snap_d, ring = _d(snap), _d(ring0)
    ids_d, lens_d, cnt_d = _d(fin_id), _d(fin_len), _d(np.array([8], np.int32))
    state = _nan(P, CAP, NS, SNAP)
    N.check(lib.mz_drqn_pop_snap_store(
        H, P, b, L, T, ids_d.data_ptr(), lens_d.data_ptr(), cnt_d.data_ptr(), snap_d.data_ptr(),
        CAP, state.data_ptr(), ring.data_ptr(), _stream()))
    assert _eq(ring, _d(ring0))  # the heads are read, not advanced
    want = np.full((P, CAP, NS, SNAP), np.nan, np.float32)
    for p, (lo, hi) in enumerate(runs):
        s1, r1 = _nan(CAP, NS, SNAP), _d(ring0[p])
        ids, lens = np.zeros(B, np.int32), np.zeros(B, np.int32)
        ids[:hi - lo], lens[:hi - lo] = fin_id[lo:hi], fin_len[lo:hi]
        ids_1, lens_1, cnt_1 = _d(ids), _d(lens), _d(np.array([hi - lo], np.int32))
        N.check(lib.mz_drqn_snap_store(
            H, B, L, T, ids_1.data_ptr(), lens_1.data_ptr(), cnt_1.data_ptr(), snap_d.data_ptr(),
            CAP, s1.data_ptr(), r1.data_ptr(), _stream()))
        assert _eq(state[p], s1), p
        nfin = hi - lo
        for k in range(max(0, nfin - CAP), nfin):
            i, n = fin_id[lo + k], fin_len[lo + k]
            nw = W.windows_in(int(n), T)
            want[p, (ring0[p, 0] + k) % CAP, 1:nw] = snap[i, 1:nw]
    got = state.cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[0]).all() and np.isnan(got[:, :, 0]).all()  # no episode; entry 0
    assert not np.isnan(got[1]).all() and not np.isnan(got[2]).all()
    # the store that follows gives the same episodes the same slots
    obs6 = _d(rng.random((B, 6)).astype(np.float32))
    term = _d((rng.random(B) < 0.5).astype(np.uint8))
    rec_x = _d(rng.random((B, L + 1, 6)).astype(np.float32))
    rec_a = _d(rng.integers(0, 4, (B, L)).astype(np.int32))
    rec_r = _d(rng.random((B, L)))
    mem = torch.zeros(P, CAP, L + 1, ROW, dtype=torch.int32, device=DEV)
    mem_len = torch.full((P, CAP), -1, dtype=torch.int32, device=DEV)
    mem_term = torch.zeros(P, CAP, dtype=torch.int32, device=DEV)
    N.check(lib.mz_drqn_pop_store(
        obs6.data_ptr(), term.data_ptr(), P, b, L, ids_d.data_ptr(), lens_d.data_ptr(),
        cnt_d.data_ptr(), rec_x.data_ptr(), rec_a.data_ptr(), rec_r.data_ptr(), CAP,
        mem.data_ptr(), mem_len.data_ptr(), mem_term.data_ptr(), ring.data_ptr(), _stream()))
    assert ring.cpu().tolist() == [[2, 3], [3, 3], [1, 4]]
    ml = mem_len.cpu().numpy()
    for p, (lo, hi) in enumerate(runs):
        nfin = hi - lo
        for k in range(max(0, nfin - CAP), nfin):
            slot = (ring0[p, 0] + k) % CAP
            n = int(fin_len[lo + k])
            assert ml[p, slot] == n
            nw = W.windows_in(n, T)
            assert np.array_equal(got[p, slot, 1:nw], snap[fin_id[lo + k], 1:nw])
            assert np.isnan(got[p, slot, nw:]).all()  # nothing past the episode's windows
    assert (ml[0] == -1).all()


# ---- 2. the sampler -----------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 3])
def test_sampler_equals_the_single_window_sampler_per_learner(lib, E):
    from mazerl import _native as N
    P, cap, T = 3, 6, 3
    Ks, due = (0, 3, 6), (1, 0, 1)
    rng = np.random.default_rng(40 + E)
    lens = rng.integers(1, L + 1, (P, cap)).astype(np.int32)
    lens[:, 0], lens[:, 1], lens[:, 2] = L, T + 1, L - 1
    ring = np.array([[3, 6], [0, 5], [4, 4]], np.int64)
    seeds, counts = [41, 2 ** 63 + 42, 43], [5, 9, 12]
    lens_d, ring_d = _d(lens), _d(ring)
    seed_d = _d(np.array([_signed(s) for s in seeds], np.int64))
    cnt_d, k_d, due_d = _d(np.array(counts, np.int64)), _d(np.array(Ks, np.int32)), \
        _d(np.array(due, np.int32))

    def fresh(n):
        return (torch.full((n, 5, E), -9, dtype=torch.int32, device=DEV),
                torch.full((n, E), -9, dtype=torch.int64, device=DEV),
                torch.full((n, 2), -9, dtype=torch.int64, device=DEV))

    def pop(min_filled):
        wdir, off, tot = fresh(P)
        rc = lib.mz_drqn_pop_window_sample(
            seed_d.data_ptr(), cnt_d.data_ptr(), k_d.data_ptr(), due_d.data_ptr(), H, P, E, L, T,
            max(Ks), cap, min_filled, ring_d.data_ptr(), lens_d.data_ptr(), wdir.data_ptr(),
            off.data_ptr(), tot.data_ptr(), _stream())
        return rc, wdir, off, tot

    rc, wdir, off, tot = pop(4)
    N.check(rc)
    for p in range(P):
        w1, o1, t1 = fresh(1)
        if due[p]:
            l1, r1 = _d(lens[p]), _d(ring[p])
            N.check(lib.mz_drqn_window_sample(
                seeds[p], counts[p], H, E, L, T, Ks[p], cap, int(ring[p, 1]), r1.data_ptr(),
                l1.data_ptr(), w1.data_ptr(), o1.data_ptr(), t1.data_ptr(), _stream()))
            slot, n = w1[0, 0].cpu().numpy(), w1[0, 1].cpu().numpy()
            assert (slot >= 0).all() and (slot < ring[p, 1]).all() and len(set(slot.tolist())) == E
            assert np.array_equal(n, lens[p][slot]) and (w1[0, 4].cpu().numpy() >= 1).all()
            assert (w1[0, 3].cpu().numpy() <= Ks[p]).all()
        # (not due: the sentinels)
        assert _eq(wdir[p], w1[0]) and _eq(off[p], o1[0]) and _eq(tot[p], t1[0]), p
    rc, wdir, off, tot = pop(E - 1)  # E > min_filled
    assert rc == -1
    with pytest.raises(ValueError):
        N.check(rc)
    assert bool((wdir == -9).all()) and bool((off == -9).all()) and bool((tot == -9).all())


# ---- 3. forward, backward, reduce, AdamW --------------------------------------------------------
class _Pop:
    """Hand-built rings of P learners (capacity 4, every slot a valid episode: lengths 1, T, T + 1
    (L - 1 where T + 1 > L) and L, terminated and truncated), random state memories whose entry 0
    is NaN (never read), and the state of one update: distinct nets, moments, step counts, seeds,
    update counts, discount factors and learning rates. E = 4, so a batch is every slot."""

    def __init__(self, P, T, Ks, stored, seed):
        self.P, self.T, self.Ks, self.stored = P, T, list(Ks), list(stored)
        self.E = self.cap = 4
        self.NS = W.windows_in(L, T)
        self.R = self.E * (min(T, L) + 2)
        rng = np.random.default_rng(seed)
        base = [1, T, T + 1 if T + 1 <= L else L - 1, L]
        self.lens = np.array([np.roll(base, p) for p in range(P)], np.int32)
        self.term = np.array([[(s * (s + 1) // 2 + p) % 2 for s in range(4)] for p in range(P)],
                             np.int32)
        self.mem = _episodes(rng, self.lens, self.term)
        self.ring = np.array([[1, 4], [0, 4], [3, 4]][:P], np.int64)
        self.state = (rng.random((P, 4, self.NS, SNAP)) - 0.5).astype(np.float32)
        self.state[:, :, 0] = np.nan
        self.src = np.stack([_row(_net(seed + 10 + p)) for p in range(P)])
        self.tgt = np.stack([_row(_net(seed + 20 + p)) for p in range(P)])
        self.m = ((rng.random((P, PARAMS)) - 0.5) * 2e-2).astype(np.float32)
        self.v = (rng.random((P, PARAMS)) * 1e-3 + 1e-6).astype(np.float32)
        self.step = np.array([5, 9, 12][:P], np.float32)
        self.seeds = [41, 2 ** 63 + 42, 43][:P]
        self.counts = [5, 9, 12][:P]
        self.gamma = np.array([0.9, 0.8, 0.95][:P], np.float32)
        self.lr = np.array([1e-3, 5e-4, 2e-3][:P], np.float32)
        self.slots = np.array([rng.permutation(4) for _ in range(P)])

    def episode(self, p, s):
        n = int(self.lens[p, s])
        return dict(x=self.mem[p, s, :n + 1, :6].view(np.float32).copy(),
                    a=self.mem[p, s, :n, 6].astype(np.int64),
                    r=self.mem[p, s, :n, 7].view(np.float32).copy(), term=bool(self.term[p, s]))

    def windows(self, p):
        """Learner p's hand-built batch under its own K_p: the last window of the episodes of L
        steps (the longest burn-in, a snapshot where K_p < L - T), the first or the last (one-step)
        window of the episode of T + 1 steps by the learner's parity, the only window of the rest."""
        out = []
        for s in self.slots[p]:
            n = int(self.lens[p, s])
            nw = W.windows_in(n, self.T)
            j = nw - 1 if n == L else min((p + 1) % 2, nw - 1)
            out.append(W.window_of(self.episode(p, s), self.T, self.Ks[p], j,
                                   self.state[p, s] if self.stored[p] else None))
        return out

    def directory(self, p):
        ws = self.windows(p)
        m = np.array([w["m"] for w in ws])
        wdir = np.stack([self.slots[p], self.lens[p][self.slots[p]], [w["b"] for w in ws],
                         [w["k"] for w in ws], m]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum(m + 2)[:-1]]).astype(np.int64)
        return wdir, off, np.array([(m + 2).sum(), m.sum()], np.int64)

    def buffers(self, n):
        """Sentinel-filled outputs of an update for n learners."""
        E, R = self.E, self.R
        return dict(wdir=torch.full((n, 5, E), -9, dtype=torch.int32, device=DEV),
                    d_off=torch.full((n, E), -9, dtype=torch.int64, device=DEV),
                    d_tot=torch.full((n, 2), -9, dtype=torch.int64, device=DEV),
                    qmax=_nan(n, R), stash=_nan(n, R, STASH), qa=_nan(n, R), y=_nan(n, R),
                    d=_nan(n, R), ep_loss=_nan(n, E, dtype=torch.float64),
                    gpart=_nan(n, E, PARAMS), grad=_nan(n, PARAMS), loss=_nan(n))

    def _load_dirs(self, o, ps, due):
        for k, p in enumerate(ps):
            if due[p]:
                wdir, off, tot = self.directory(p)
                o["wdir"][k].copy_(_d(wdir)), o["d_off"][k].copy_(_d(off)), o["d_tot"][k].copy_(_d(tot))

    def run_pop(self, lib, due, burn=None, sampled=False, write_grad=1):
        from mazerl import _native as N
        P, E, T, cap, K = self.P, self.E, self.T, self.cap, max(self.Ks)
        o = self.buffers(P)
        o.update(src=_d(self.src), tgt=_d(self.tgt), m=_d(self.m), v=_d(self.v), step=_d(self.step))
        mem, term, lens, ring = _d(self.mem), _d(self.term), _d(self.lens), _d(self.ring)
        state = _d(self.state)
        due_d = _d(np.array(due, np.int32))
        burn_d = _d(np.array(self.Ks if burn is None else burn, np.int32))
        stored_d = _d(np.array(self.stored, np.int32))
        seeds = _d(np.array([_signed(s) for s in self.seeds], np.int64))
        counts = _d(np.array(self.counts, np.int64))
        gam, lr = _d(self.gamma), _d(self.lr)
        dirs = tuple(o[k].data_ptr() for k in ("wdir", "d_off", "d_tot"))
        st = _stream()
        if sampled:
            N.check(lib.mz_drqn_pop_window_sample(
                seeds.data_ptr(), counts.data_ptr(), burn_d.data_ptr(), due_d.data_ptr(), H, P, E,
                L, T, K, cap, cap, ring.data_ptr(), lens.data_ptr(), *dirs, st))
        else:
            self._load_dirs(o, range(P), due)
        N.check(lib.mz_drqn_pop_window_forward(
            o["tgt"].data_ptr(), H, 1, P, E, L, T, K, cap, None, burn_d.data_ptr(),
            stored_d.data_ptr(), due_d.data_ptr(), mem.data_ptr(), term.data_ptr(),
            state.data_ptr(), *dirs, o["qmax"].data_ptr(), None, None, None, None, None, st))
        N.check(lib.mz_drqn_pop_window_forward(
            o["src"].data_ptr(), H, 0, P, E, L, T, K, cap, gam.data_ptr(), burn_d.data_ptr(),
            stored_d.data_ptr(), due_d.data_ptr(), mem.data_ptr(), term.data_ptr(),
            state.data_ptr(), *dirs, o["qmax"].data_ptr(), o["stash"].data_ptr(),
            o["qa"].data_ptr(), o["y"].data_ptr(), o["d"].data_ptr(), o["ep_loss"].data_ptr(), st))
        N.check(lib.mz_drqn_pop_window_backward(
            o["src"].data_ptr(), H, P, E, L, T, K, cap, burn_d.data_ptr(), due_d.data_ptr(),
            mem.data_ptr(), *dirs, o["stash"].data_ptr(), o["d"].data_ptr(),
            o["ep_loss"].data_ptr(), o["gpart"].data_ptr(), o["grad"].data_ptr(),
            o["loss"].data_ptr(), st))
        N.check(lib.mz_adamw_pop(
            o["src"].data_ptr(), o["m"].data_ptr(), o["v"].data_ptr(), o["grad"].data_ptr(), P,
            PARAMS, lr.data_ptr(), o["step"].data_ptr(), due_d.data_ptr(), *ADAM, 1.0, 1.0,
            write_grad, st))
        torch.cuda.synchronize()
        return o

    def run_single(self, lib, p, sampled=False):
        """The single-learner window chain on learner p's ring with (T, K_p) and its state memory,
        or a NULL one where the learner does not store."""
        from mazerl import _native as N
        E, T, cap, K = self.E, self.T, self.cap, self.Ks[p]
        o = self.buffers(1)
        o.update(src=_d(self.src[p:p + 1]), tgt=_d(self.tgt[p:p + 1]), m=_d(self.m[p:p + 1]),
                 v=_d(self.v[p:p + 1]), step=_d(self.step[p:p + 1]))
        mem, term, lens, ring = (_d(a[p]) for a in (self.mem, self.term, self.lens, self.ring))
        state = _d(self.state[p]) if self.stored[p] else None
        lr = _d(self.lr[p:p + 1])
        dirs = tuple(o[k].data_ptr() for k in ("wdir", "d_off", "d_tot"))
        ps, pt, pg = _ptrs(o["src"][0]), _ptrs(o["tgt"][0]), _ptrs(o["grad"][0])
        gamma, st = float(self.gamma[p]), _stream()
        if sampled:
            N.check(lib.mz_drqn_window_sample(self.seeds[p], self.counts[p], H, E, L, T, K, cap, cap,
                                              ring.data_ptr(), lens.data_ptr(), *dirs, st))
        else:
            self._load_dirs(o, [p], {p: 1})
        N.check(lib.mz_drqn_window_forward(
            pt, H, 1, E, L, T, K, cap, gamma, mem.data_ptr(), term.data_ptr(), _ptr(state), *dirs,
            o["qmax"].data_ptr(), None, None, None, None, None, st))
        N.check(lib.mz_drqn_window_forward(
            ps, H, 0, E, L, T, K, cap, gamma, mem.data_ptr(), term.data_ptr(), _ptr(state), *dirs,
            o["qmax"].data_ptr(), o["stash"].data_ptr(), o["qa"].data_ptr(), o["y"].data_ptr(),
            o["d"].data_ptr(), o["ep_loss"].data_ptr(), st))
        N.check(lib.mz_drqn_window_backward(
            ps, H, E, L, T, K, cap, mem.data_ptr(), *dirs, o["stash"].data_ptr(),
            o["d"].data_ptr(), o["ep_loss"].data_ptr(), o["gpart"].data_ptr(), pg,
            o["loss"].data_ptr(), st))
        N.check(lib.mz_adamw_flat(
            o["src"].data_ptr(), o["m"].data_ptr(), o["v"].data_ptr(),
            (C.c_void_p * 1)(o["grad"].data_ptr()), (C.c_int64 * 1)(PARAMS), 1, lr.data_ptr(),
            o["step"].data_ptr(), *ADAM, 1.0, 1.0, 1, st))
        torch.cuda.synchronize()
        return o

    def start(self, p):
        """Learner p's state and sentinels before an update."""
        o = self.buffers(1)
        o.update(src=_d(self.src[p:p + 1]), m=_d(self.m[p:p + 1]), v=_d(self.v[p:p + 1]),
                 step=_d(self.step[p:p + 1]))
        return o


KEYS_OUT = ("wdir", "d_off", "d_tot", "qmax", "stash", "qa", "y", "d", "ep_loss", "gpart", "grad",
            "loss", "src", "m", "v", "step")
ROWS = ("qmax", "stash", "qa", "y", "d")
TK = [(1, 0, (0, 0, 0)), (3, 6, (0, 6, 3)), (8, 0, (0, 0, 0))]


@pytest.mark.parametrize("sampled", [False, True], ids=["hand-built", "sampled"])
@pytest.mark.parametrize("due", [(1, 0, 1), (1, 1, 1)], ids=["due101", "all-due"])
@pytest.mark.parametrize("T,K,Ks", TK, ids=["T1-K0", "T3-K6", "T8-K0"])
def test_update_chain_equals_the_single_window_chain_per_learner(lib, T, K, Ks, due, sampled):
    stored = (1, 0, 1)
    pop = _Pop(3, T, Ks, stored, 700 + 10 * T + K)
    assert max(Ks) == K
    o = pop.run_pop(lib, due, sampled=sampled)
    for p in range(3):
        if not due[p]:  # every bit of its state and of its sentinels is still there
            one = pop.start(p)
            for k in KEYS_OUT:
                assert _eq(o[k][p], one[k][0]), (p, k)
            continue
        one = pop.run_single(lib, p, sampled=sampled)  # (stored[p] == 0: a NULL state memory)
        for k in KEYS_OUT:
            assert _eq(o[k][p], one[k][0]), (p, k)
        assert float(o["step"][p]) == pop.step[p] + 1
        assert not torch.isnan(o["grad"][p]).any() and float(o["grad"][p].abs().max()) <= 1.0
        assert not _eq(o["src"][p], _d(pop.src[p]))
        # the sentinels outside the windows' rows: everything past the batch's rows, and of
        # qa / y / d everything but the training-step rows
        w = o["wdir"][p].cpu().numpy()
        off, m = o["d_off"][p].cpu().numpy(), w[4]
        rows, steps = (int(v) for v in o["d_tot"][p].cpu())
        assert rows == int((m + 2).sum()) <= pop.R and steps == int(m.sum()) >= pop.E
        train = np.concatenate([a + 1 + np.arange(n) for a, n in zip(off, m)])
        rest = np.setdiff1d(np.arange(pop.R), train)
        for k in ("qa", "y", "d"):
            v = o[k][p].cpu().numpy()
            assert np.isnan(v[rest]).all() and not np.isnan(v[train]).any(), (p, k)
        for k in ROWS:
            assert torch.isnan(o[k][p][rows:]).all(), (p, k)
        assert not torch.isnan(o["gpart"][p]).any() and not torch.isnan(o["ep_loss"][p]).any()
    assert _eq(o["tgt"], _d(pop.tgt))
    if not sampled and T == 3:  # what the case is there for: the stored learners read snapshots,
        for p in (0, 2):        # burn-ins of 0, T and 2 T steps occur, first / inner / last windows
            assert any(w["b"] > 0 for w in pop.windows(p)), p
        assert {w["k"] for p in range(3) for w in pop.windows(p)} >= {0, 3, 6}
        assert {(w["term"], w["s"] + w["m"] == len(e["a"]))
                for p in range(3) for w, e in zip(pop.windows(p),
                                                  [pop.episode(p, s) for s in pop.slots[p]])} >= \
            {(True, True), (False, True), (False, False)}


def test_a_learner_that_does_not_store_ignores_the_state_memory(lib):
    """stored_dev[p] = 0 with a state memory at hand is the single call with a NULL one (the chain
    test above), so it differs from the same learner reading its snapshots."""
    a = _Pop(3, 3, (0, 0, 0), (1, 0, 1), 912).run_pop(lib, (1, 1, 1))
    b = _Pop(3, 3, (0, 0, 0), (1, 1, 1), 912).run_pop(lib, (1, 1, 1))
    for k in ("qa", "gpart", "src"):
        assert _eq(a[k][0], b[k][0]) and _eq(a[k][2], b[k][2]) and not _eq(a[k][1], b[k][1]), k


def test_an_out_of_rule_burn_in_on_the_device_trains_on_nothing(lib):
    """burn_in_dev[1] = 2 at T = 3 (Python never uploads it; the host cannot see it): learner 1's
    batch has no window, its partials, gradient row and loss are zero, its row buffers keep their
    sentinels, and learners 0 and 2 give the bits they give beside an in-rule learner 1. The same
    with a hand-built directory of valid windows: the forward and the backward refuse them."""
    pop = _Pop(3, 3, (0, 3, 6), (1, 1, 1), 955)
    good = pop.run_pop(lib, (1, 1, 1), sampled=True)
    for burn in ((0, 2, 6), (0, -3, 6), (0, 9, 6)):
        for sampled in (True, False):
            o = pop.run_pop(lib, (1, 1, 1), burn=burn, sampled=sampled)
            ref = good if sampled else pop.run_pop(lib, (1, 1, 1))
            for p in (0, 2):
                for k in KEYS_OUT:
                    assert _eq(o[k][p], ref[k][p]), (burn, p, k)
            assert bool((o["gpart"][1] == 0).all()) and bool((o["grad"][1] == 0).all()), burn
            for k in ROWS:
                assert torch.isnan(o[k][1]).all(), (burn, k)
            assert torch.isnan(o["ep_loss"][1]).all()
            if sampled:
                w = o["wdir"][1].cpu().numpy()
                assert (w[2:] == 0).all() and (w[1] >= 1).all() and o["d_tot"][1].cpu().tolist() == [0, 0]
                assert float(o["loss"][1]) == 0.0
            assert not bool((good["gpart"][1] == 0).all())


# ---- 4. against the float64 model ---------------------------------------------------------------
def _check(name, got, model, ref):
    got, model, ref = (np.asarray(a, np.float64) for a in (got, model, ref))
    mx = np.abs(model).max()
    e_k, e_ref = np.abs(got - model).max(), np.abs(ref - model).max()
    print(f"{name}: e_k {e_k:.3e} e_ref {e_ref:.3e} ratio {e_k / (e_ref + 2 * U * mx + 1e-300):.2f}")
    assert e_k <= 4 * e_ref + 8 * U * mx, (name, e_k, e_ref, mx)


def test_population_window_gradient_and_step_match_the_float64_model(lib):
    """P = 2, T = 3, K = (3, 6), learner 0 from stored state and learner 1 from zero: each
    learner's loss, gradient (before the clamp) and parameters after the AdamW step against
    tests/drqn_window_model.py + learner_model.adamw_step on its hand-built windows, with torch's
    float32 window_td_loss + autograd on the CPU as the reference error.
    Observed on an MI355X, ratios e_k / (e_ref + 2 u max|tensor|) (the bound is 4): loss
    0.23-0.51, gradients 0.51-1.07, parameters 0.14-0.70."""
    from mazerl.agents.lstm_dqn_agent import DQN, window_td_loss
    pop = _Pop(2, 3, (3, 6), (1, 0), 500)
    o = pop.run_pop(lib, (1, 1), write_grad=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
    for p in range(2):
        ws = pop.windows(p)
        assert max(w["k"] for w in ws) == pop.Ks[p]
        sd = lambda row: {k: torch.from_numpy(row[OFFS[j]:OFFS[j + 1]].reshape(SHAPES[j]).copy())  # noqa: E731
                          for j, k in enumerate(M.KEYS)}
        gamma = float(pop.gamma[p])
        out = W.window_td_loss(M.as_f64({k: v.numpy() for k, v in sd(pop.src[p]).items()}),
                               M.as_f64({k: v.numpy() for k, v in sd(pop.tgt[p]).items()}), ws, gamma)
        ns, nt = DQN(6, 4, H, torch.device("cpu")), DQN(6, 4, H, torch.device("cpu"))
        ns.load_state_dict(sd(pop.src[p])), nt.load_state_dict(sd(pop.tgt[p]))
        loss = window_td_loss(ns, nt, [(t(w["x"]), torch.from_numpy(np.asarray(w["a"])), t(w["r"]),
                                        t(w["h0"]), t(w["c0"]), w["k"], w["term"]) for w in ws],
                              gamma)
        loss.backward()
        _check(f"learner {p} loss", [float(o["loss"][p])], [out["loss"]], [loss.item()])
        grad, got = o["grad"][p].cpu().numpy(), o["src"][p].cpu().numpy()
        args = (float(pop.lr[p]), float(pop.step[p])) + ADAM + (1.0, 1.0)
        for j, (k, q) in enumerate(zip(M.KEYS, ns.parameters())):
            a, b = OFFS[j], OFFS[j + 1]
            _check(f"learner {p} grad {k}", grad[a:b], out["grads"][k].ravel(),
                   q.grad.numpy().ravel())
            pm = LM.adamw_step(pop.src[p, a:b], out["grads"][k].ravel(), pop.m[p, a:b],
                               pop.v[p, a:b], *args)[0]
            pr = LM.adamw_step(pop.src[p, a:b], q.grad.numpy().ravel(), pop.m[p, a:b],
                               pop.v[p, a:b], *args)[0]
            _check(f"learner {p} param {k}", got[a:b], pm, pr)
