"""The prioritized replay-window kernels (csrc/mz_drqn.hip: k_drqn_prio_store, k_drqn_prio_sample,
k_drqn_prio_update) through the C ABI, L = 8. The integer parts (entry, the sampler's windows, the
slot sums, prio_max) are compared bit for bit with tests/drqn_prio_model.py; the two float64 pow
results by the argument of one level up: isw is within one float32 ulp of the model's float64 value
rounded to float32 (a pow off by a few of its own ulps moves the rounded value by at most one), a
written mass within one unit of the model's. The chain forward -> update -> backward is held to
test_drqn_window_gpu.py's bound, e_k <= 4 e_ref + 8 u max|tensor|, against the weighted float64
model fed the device's isw, with torch's float32 window_td_loss(weights=isw) as the reference.
The memory, the launches and the bound check are test_drqn_window_gpu.py's (_Mem, _check)."""
from collections import deque

import numpy as np
import pytest
import torch

import drqn_model as M
import drqn_prio_model as PM
import drqn_window_model as W
import test_drqn_window_gpu as WG

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, L, SHAPES = WG.H, WG.L, WG.SHAPES
ONE, CEIL = PM.ONE, PM.CEIL
SENT = 0x7FFFFFF1  # no mass: above 2^30
_d, _stream = WG._d, WG._stream


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def _i32(a):
    return _d(np.asarray(a, np.int32))


# ---- entry --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [5, 7])
@pytest.mark.parametrize("T", [1, 3, 8])
def test_entry_follows_the_ring_like_a_deque(lib, cap, T):
    """Three vector steps of hand-made finished lists (lengths 2, T, T + 1, L; the last step lists
    more episodes than there are slots), prio_max raised by hand in between, mz_drqn_store after
    each: every slot a deque(maxlen=capacity) holds has its windows at the prio_max of its step,
    zeros past ceil(n / T), its sum, and mz_drqn_store's length; nothing else is written."""
    from mazerl import _native as N
    B = 9
    Wn = W.windows_in(L, T)
    kw = dict(device=DEV)
    mem_prio = torch.full((cap + 1, Wn), SENT, dtype=torch.int32, **kw)
    mem_psum = torch.full((cap + 1,), -1, dtype=torch.int64, **kw)
    prio_max = torch.full((2,), ONE, dtype=torch.int32, **kw)
    prio_max[1] = SENT
    ring = torch.zeros(2, dtype=torch.int64, **kw)
    mem = torch.zeros(cap, L + 1, 8, dtype=torch.int32, **kw)
    mem_len, mem_term = (torch.zeros(cap, dtype=torch.int32, **kw) for _ in range(2))
    rec_x = torch.zeros(B, L + 1, 6, **kw)
    rec_a = torch.zeros(B, L, dtype=torch.int32, **kw)
    rec_r = torch.zeros(B, L, dtype=torch.float64, **kw)
    obs6, term = torch.zeros(B, 6, **kw), torch.zeros(B, dtype=torch.uint8, **kw)
    t1 = T + 1 if T + 1 <= L else L - 1
    plan = [[(0, 2), (4, T)], [(1, t1), (2, L), (8, 2)],
            [(i, [2, T, t1, L, 5, 1, 3, L, 2][i]) for i in range(9)]]
    assert len(plan[2]) > cap
    dq, total, pm = deque(maxlen=cap), 0, ONE
    model_prio = np.full((cap, Wn), SENT, np.int64)
    model_psum = np.full(cap, -1, np.int64)
    for step, fin in enumerate(plan):
        pm = [ONE, 3 * ONE + 17, CEIL][step]
        prio_max[0] = pm
        fin_id = _i32([i for i, _ in fin] + [0] * (B - len(fin)))
        fin_len = _i32([n for _, n in fin] + [0] * (B - len(fin)))
        fin_count = _i32([len(fin)])
        fins = (fin_id.data_ptr(), fin_len.data_ptr(), fin_count.data_ptr())
        N.check(lib.mz_drqn_prio_store(H, B, L, T, *fins, cap, mem_prio.data_ptr(),
                                       mem_psum.data_ptr(), prio_max.data_ptr(), ring.data_ptr(),
                                       _stream()))
        N.check(lib.mz_drqn_store(obs6.data_ptr(), term.data_ptr(), B, L, *fins, rec_x.data_ptr(),
                                  rec_a.data_ptr(), rec_r.data_ptr(), cap, mem.data_ptr(),
                                  mem_len.data_ptr(), mem_term.data_ptr(), ring.data_ptr(),
                                  _stream()))
        PM.store(model_prio, model_psum, pm, total % cap, fin, B, L, T)
        for _, n in fin:
            dq.append((n, pm))
        total += len(fin)
        assert tuple(int(v) for v in ring.cpu()) == (total % cap, len(dq))
        got, gs, ml = mem_prio.cpu().numpy(), mem_psum.cpu().numpy(), mem_len.cpu().numpy()
        for j, (n, v) in enumerate(dq):
            slot = (total - len(dq) + j) % cap
            nw = W.windows_in(n, T)
            assert ml[slot] == n, (slot, n)  # the slot mz_drqn_store gave the episode
            assert (got[slot, :nw] == v).all() and (got[slot, nw:] == 0).all(), (slot, n)
            assert gs[slot] == nw * v
        # the model, sentinels of the slots not yet written included; the row past the ring
        assert np.array_equal(got[:cap], model_prio) and np.array_equal(gs[:cap], model_psum)
        assert (got[cap] == SENT).all() and gs[cap] == -1
        assert prio_max.cpu().tolist() == [pm, SENT]  # read, never written
    assert total == 14 and (model_prio != SENT).all()


# ---- sampling -----------------------------------------------------------------------------------
def _masses(rng, cap, T, empty=()):
    """Episode lengths 1 .. L (the first four: 1, T, T + 1 or L - 1, L), masses from 1 to 2^30 on
    every window an episode has, slots in `empty` without an episode."""
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


def _run_sample(lib, seed, counter, E, T, K, cap, lens_d, prio_d, psum_d, beta):
    from mazerl import _native as N
    kw = dict(device=DEV)
    wdir = torch.full((5, E), -9, dtype=torch.int32, **kw)
    off = torch.full((E + 1,), -9, dtype=torch.int64, **kw)
    tot = torch.full((3,), -9, dtype=torch.int64, **kw)
    isw = torch.full((E + 1,), float("nan"), **kw)
    N.check(lib.mz_drqn_prio_sample(seed, counter, H, E, L, T, K, cap, lens_d.data_ptr(),
                                    prio_d.data_ptr(), psum_d.data_ptr(), wdir.data_ptr(),
                                    off.data_ptr(), tot.data_ptr(), isw.data_ptr(), beta, _stream()))
    return wdir.cpu().numpy(), off.cpu().numpy(), tot.cpu().numpy(), isw.cpu().numpy()


def _sample_against_model(lib, cap, E, T, K, rng, empty=(), keys=((5, 0), (5, 1), (6, 0))):
    lens, prio = _masses(rng, cap, T, empty)
    lens_d, prio_d, psum_d = _i32(lens), _i32(prio), _d(prio.sum(axis=1).astype(np.int64))
    seen = []
    for seed, counter in keys:
        for beta in (0.6, 0.0):
            wdir, off, tot, isw = _run_sample(lib, seed, counter, E, T, K, cap, lens_d, prio_d,
                                              psum_d, beta)
            m = PM.sample(prio, lens, seed, counter, E, T, K, beta)
            for row, key in enumerate(("slot", "n", "b", "k", "m")):
                assert np.array_equal(wdir[row], np.array(m[key])), (key, seed, counter)
            assert np.array_equal(off[:E], m["off"]) and off[E] == -9
            assert tuple(tot) == m["tot"] + (-9,)
            assert np.isnan(isw[E])
            if beta == 0.0:
                assert (isw[:E] == 1.0).all()
            else:
                want = m["isw"].astype(np.float32)
                ulp = np.spacing(want)
                assert (np.abs(isw[:E].astype(np.float64) - want) <= ulp).all(), (isw[:E], want)
                assert isw[:E].max() == 1.0 and (isw[:E] > 0).all()
                seen.append((wdir, isw[:E], m))
    again = _run_sample(lib, *keys[0], E, T, K, cap, lens_d, prio_d, psum_d, 0.6)
    assert np.array_equal(again[0], seen[0][0]) and np.array_equal(again[3][:E], seen[0][1])
    return seen


@pytest.mark.parametrize("cap", [5, 7])
@pytest.mark.parametrize("E", [1, 3, 65])
@pytest.mark.parametrize("T,K", [(1, 0), (1, 2), (3, 3), (8, 0)])
def test_sampler_is_the_integer_model_bit_for_bit(lib, cap, E, T, K):
    rng = np.random.default_rng(800 + 10 * cap + E + T)
    seen = _sample_against_model(lib, cap, E, T, K, rng, empty=(4,) if cap == 7 else ())
    (w0, _, m0), (w1, _, _), (w2, _, _) = seen
    if E == 65:  # 65 positions over at most 7 slots: the same window and the same episode twice
        wins = list(zip(w0[0], w0[2] + w0[3]))
        assert len(set(wins)) < E and len(set(w0[0])) < len(set(wins)) or T == 8
        assert len(set(wins)) < E
        # keyed by seed and counter. (Every directory above equals the model's for its own key;
        # 65 strata over a few windows can land on the same windows under two keys, so the
        # directories are required to differ only at T = 1, where the memory has dozens.)
        if T == 1:
            assert not np.array_equal(w0, w1) and not np.array_equal(w0, w2)
    assert m0["t"] != seen[1][2]["t"] and m0["t"] != seen[2][2]["t"]
    # keyed by the position too: two positions never share their 64-bit word
    words = [PM.draw(5, 0, e) for e in range(E)]
    assert len(set(words)) == E
    assert all(lo <= t and (t < hi or lo == hi) for lo, hi, t in zip(m0["lo"], m0["hi"], m0["t"]))


@pytest.mark.parametrize("cap,E", [(200, 3), (70000, 5)])
def test_sampler_over_more_than_one_group_of_slots(lib, cap, E):
    """The sampler sums the slots in groups of 64 g, g = ceil(capacity / 65536): 200 slots are 4
    groups of 64 (a last one of 8), 70,000 are 547 groups of 128 (more groups than one wave scans,
    two rows per group)."""
    rng = np.random.default_rng(900 + E)
    _sample_against_model(lib, cap, E, 8, 0, rng, empty=range(40, 120), keys=((7, 3), (8, 3)))


def test_sampler_with_no_mass_gives_no_window(lib):
    cap, E = 5, 3
    z = torch.zeros(cap, dtype=torch.int64, device=DEV)
    wdir, off, tot, isw = _run_sample(lib, 1, 2, E, 3, 3, cap, _i32(np.zeros(cap)),
                                      _i32(np.zeros((cap, 3))), z, 0.6)
    assert (wdir == 0).all() and (off[:E] == 0).all() and tuple(tot[:2]) == (0, 0)
    assert (isw[:E] == 1.0).all()


def test_sampler_more_positions_than_mass(lib):
    cap, E, T = 5, 65, 2
    lens = np.array([2, 0, 4, 0, 1], np.int32)
    prio = np.zeros((cap, 4), np.int64)
    prio[0, 0] = prio[2, 0] = prio[2, 1] = prio[4, 0] = 1  # S = 4 < E
    wdir, off, tot, isw = _run_sample(lib, 3, 9, E, T, 2, cap, _i32(lens), _i32(prio),
                                      _d(prio.sum(axis=1)), 1.0)
    m = PM.sample(prio, lens, 3, 9, E, T, 2, 1.0)
    for row, key in enumerate(("slot", "n", "b", "k", "m")):
        assert np.array_equal(wdir[row], np.array(m[key])), key
    assert (wdir[4] >= 1).all() and set(wdir[0]) == {0, 2, 4} and (isw[:E] == 1.0).all()


# ---- the write-back and the chain -----------------------------------------------------------------
class _Prio:
    """test_drqn_window_gpu's hand-built memory with a directory that, as a sampler with
    replacement may, holds a window twice and two windows of one episode; masses for every window
    of every stored episode (a row past the ring keeps its sentinel) and importance weights."""

    def __init__(self, lib, E, T, K, seed):
        self.lib, self.E, self.T = lib, E, T
        lens = WG._lens(E, T)
        s = self.s = WG._Mem(lib, lens, seed, T)
        js = WG._js(lens, T)
        ent = [(e, js[e]) for e in range(E)]
        if E >= 3:
            ent[E - 1] = ent[0]                                 # the same window twice
            long = max(range(E), key=lambda e: lens[e])
            if W.windows_in(lens[long], T) > 1:                 # another window of an episode
                ent[E - 2] = (long, (js[long] + 1) % W.windows_in(lens[long], T))
        self.ent = ent
        s.K = K
        s.ws = [W.window_of(s.eps[e], T, K, j, s.state[s.slots[e]]) for e, j in ent]
        s.m = np.array([w["m"] for w in s.ws])
        self.slot = np.array([s.slots[e] for e, _ in ent])
        self.j = np.array([j for _, j in ent])
        wdir = np.stack([self.slot, [lens[e] for e, _ in ent], [w["b"] for w in s.ws],
                         [w["k"] for w in s.ws], s.m]).astype(np.int32)
        s.off = np.concatenate([[0], np.cumsum(s.m + 2)[:-1]]).astype(np.int64)
        s.rows, s.steps = int((s.m + 2).sum()), int(s.m.sum())
        s.wdir, s.w_off = _d(wdir), _d(s.off)
        s.w_tot = _d(np.array([s.rows, s.steps], np.int64))
        rng = np.random.default_rng(seed + 1)
        self.Wn = W.windows_in(L, T)
        prio = np.full((s.cap + 1, self.Wn), SENT, np.int64)
        prio[:s.cap] = 0
        for slot, n in zip(s.slots, lens):
            nw = W.windows_in(n, T)
            prio[slot, :nw] = 1 + rng.integers(0, 4 * ONE, nw)
        self.prio0 = prio
        self.psum0 = np.concatenate([prio[:s.cap].sum(axis=1), [-1]]).astype(np.int64)
        self.pmax0 = int(prio[:s.cap].max())
        self.isw = (0.05 + 0.95 * rng.random(E)).astype(np.float32)
        self.isw[0] = 1.0

    def update(self, o, isw, alpha, eta=0.9, eps=1e-3, pmax=None):
        from mazerl import _native as N
        s = self.s
        self.prio, self.psum = _i32(self.prio0), _d(self.psum0)
        self.pmax = _i32([self.pmax0 if pmax is None else pmax, SENT])
        self.isw_d = _d(np.concatenate([isw, [np.float32("nan")]]).astype(np.float32))
        N.check(self.lib.mz_drqn_prio_update(
            H, self.E, L, self.T, s.cap, s.wdir.data_ptr(), s.w_off.data_ptr(), s.w_tot.data_ptr(),
            o["qa"].data_ptr(), o["y"].data_ptr(), o["d"].data_ptr(), o["ep_loss"].data_ptr(),
            self.isw_d.data_ptr(), alpha, eta, eps, self.prio.data_ptr(), self.psum.data_ptr(),
            self.pmax.data_ptr(), _stream()))

    def forward(self):
        o = self.s.buffers()
        self.s.forward(o, 1)
        self.s.forward(o, 0)
        torch.cuda.synchronize()
        return o


CASES = [(E, T, K) for E in (1, 3, 65) for T, K in [(1, 0), (3, 3), (8, 0)]]
DIFFER = {}  # case -> how many written masses differ from the model's (by one unit at most)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "E%d-T%d-K%d" % c)
def chain(request, lib):
    E, T, K = request.param
    # test_drqn_window_gpu's memory for the same E and T, so the unweighted part of the chain is
    # the one that test pins. (On a memory of its own, seed 270 + 7 E + T, the E = 1, T = 1 loss
    # measured e_k 1.66e-8 against a bound of 1.45e-8 at weight 1.0, that is on the plain
    # forward's own bits: a one-step window's loss is one squared residual of two values near 1,
    # and 8 u max|loss| is then a bound of about a tenth of an ulp of them.)
    p = _Prio(lib, E, T, K, 170 + 7 * E + T)
    o = p.forward()
    before = {k: o[k].cpu().numpy().copy() for k in ("qa", "y", "d", "ep_loss", "stash", "qmax")}
    p.update(o, p.isw, 0.9)
    p.s.backward(o)
    torch.cuda.synchronize()
    p.after = (p.prio.cpu().numpy().astype(np.int64), p.psum.cpu().numpy(), p.pmax.cpu().tolist())
    return p, o, before


def test_update_writes_the_models_masses_and_the_slot_sums(chain):
    p, o, before = chain
    s = p.s
    rows = [s.off[e] + 1 + np.arange(s.m[e]) for e in range(p.E)]
    resid = [np.abs(before["qa"][r] - before["y"][r]) for r in rows]
    assert all(a.dtype == np.float32 for a in resid)
    want = [PM.mass_of(a, 0.9, 0.9, 1e-3) for a in resid]
    got, gs, pmax = p.after
    mass = got[p.slot, p.j]
    diff = np.abs(mass - np.array(want))
    DIFFER[(p.E, p.T)] = int((diff != 0).sum())
    print(f"E {p.E} T {p.T}: {DIFFER[(p.E, p.T)]} of {p.E} masses differ from the model's, "
          f"largest difference {int(diff.max())}")
    assert (diff <= 1).all(), (mass, want)
    assert (mass >= 1).all() and (mass <= CEIL).all()
    # duplicates wrote the same value; every entry no window of the batch names is unchanged
    touched = np.zeros_like(got, bool)
    touched[p.slot, p.j] = True
    assert np.array_equal(got[~touched], p.prio0[~touched])
    assert (got[s.cap] == SENT).all() and gs[s.cap] == -1
    assert np.array_equal(gs[:s.cap], got[:s.cap].sum(axis=1))  # every slot, touched or not
    assert pmax == [max(p.pmax0, int(mass.max())), SENT]
    # the running max only rises
    o2 = p.forward()
    p.update(o2, p.isw, 0.9, pmax=CEIL)
    assert p.pmax.cpu().tolist() == [CEIL, SENT]
    assert np.array_equal(p.prio.cpu().numpy(), got)  # and the same inputs give the same masses


def test_update_scales_the_residuals_and_the_loss_terms_by_the_weights(chain):
    p, o, before = chain
    s = p.s
    rows = s.step_rows()
    w_row = np.concatenate([np.full(m, w, np.float32) for m, w in zip(s.m, p.isw)])
    d = o["d"].cpu().numpy()
    assert np.array_equal(d[rows], before["d"][rows] * w_row)  # one f32 multiply per row
    rest = np.setdiff1d(np.arange(s.rows_cap), rows)
    assert np.isnan(d[rest]).all()
    ep = o["ep_loss"].cpu().numpy()
    assert np.array_equal(ep[:p.E], before["ep_loss"][:p.E] * p.isw.astype(np.float64))
    assert np.isnan(ep[p.E])
    for k in ("qa", "y", "stash", "qmax"):  # read, or not touched at all
        assert np.array_equal(o[k].cpu().numpy(), before[k], equal_nan=True), k


def test_chain_matches_the_weighted_model(chain):
    p, o, before = chain
    s = p.s
    m = PM.weighted_td_loss(WG._f64(s.src), WG._f64(s.tgt), s.ws, 0.9, p.isw.astype(np.float64))
    ref = _torch_ref(s, p.isw)
    rows = s.step_rows()
    w_row = np.concatenate([np.full(k, w, np.float64) for k, w in zip(s.m, p.isw)])
    WG._check("Q_t[a_t]", o["qa"].cpu().numpy()[rows], np.concatenate(m["qa"]), ref["qa"])
    WG._check("y_t", o["y"].cpu().numpy()[rows], np.concatenate(m["y"]), ref["y"])
    WG._check("loss", [float(o["loss"][0])], [m["loss"]], [ref["loss"]])
    md = 2.0 * w_row * (np.concatenate(m["qa"]) - np.concatenate(m["y"])) / s.steps
    rd = 2.0 * w_row * (ref["qa"].astype(np.float64) - ref["y"]) / s.steps
    WG._check("residual", o["d"].cpu().numpy()[rows].astype(np.float64), md, rd)
    for k, g, shape in zip(M.KEYS, o["grads"], SHAPES):
        n = int(np.prod(shape))
        WG._check("grad " + k, g.cpu().numpy()[:n].reshape(shape), m["grads"][k], ref["grads"][k])


def _torch_ref(s, isw):
    from mazerl.agents.lstm_dqn_agent import window_td_loss
    ref = s.torch_ref()  # (qa and y do not depend on the weights)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
    ws = [(t(w["x"]), torch.from_numpy(np.asarray(w["a"])), t(w["r"]), t(w["h0"]), t(w["c0"]),
           w["k"], w["term"]) for w in s.ws]
    for q in s.src.parameters():
        q.grad = None
    loss = window_td_loss(s.src, s.tgt, ws, 0.9, weights=torch.from_numpy(isw))
    loss.backward()
    ref["loss"] = loss.item()
    ref["grads"] = {k: q.grad.numpy().copy() for k, q in s.src.named_parameters()}
    return ref


def test_unit_weights_and_alpha_zero_are_the_unweighted_paths_bits(chain):
    """alpha = 0 writes 2^20 whatever the residuals; weights of 1.0f (what beta = 0 samples) leave
    d, ep_loss and so the gradients exactly the plain window update's on the same directory."""
    p, _, _ = chain
    plain = p.s.run()
    o = p.forward()
    p.update(o, np.ones(p.E, np.float32), 0.0)
    p.s.backward(o)
    torch.cuda.synchronize()
    for k in ("qa", "y", "d", "ep_loss", "gpart", "loss"):
        assert np.array_equal(o[k].cpu().numpy(), plain[k].cpu().numpy(), equal_nan=True), k
    for a, b in zip(o["grads"], plain["grads"]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    got = p.prio.cpu().numpy()
    assert (got[p.slot, p.j] == ONE).all()
    assert np.array_equal(p.psum.cpu().numpy()[:p.s.cap], got[:p.s.cap].astype(np.int64).sum(axis=1))


def test_update_clamps_and_skips_what_the_directory_does_not_describe(lib):
    """A residual of 1e30 and a NaN give 2^30; alpha = 6 on a zero residual gives 1; an entry whose
    slot or window lies outside the memory is skipped and nothing of it is written."""
    from mazerl import _native as N
    E, T, cap = 4, 3, 5
    Wn = W.windows_in(L, T)
    wdir = _i32([[1, 2, 9, 3], [L, L, L, L], [0, 3, 0, 9], [0, 0, 0, 0], [3, 3, 3, 3]])
    off = _d(np.arange(E, dtype=np.int64) * 5)
    tot = _d(np.array([20, 12], np.int64))
    qa = np.zeros(E * (T + 2), np.float32)
    qa[1], qa[6 + 1] = 1e30, np.nan
    qa_d, y_d = _d(qa), _d(np.zeros_like(qa))
    d = _d(np.ones_like(qa))
    ep = _d(np.ones(E, np.float64))
    isw = _d(np.full(E, 0.5, np.float32))
    for alpha, want in ((0.9, (CEIL, CEIL)), (6.0, (CEIL, CEIL))):
        prio = torch.full((cap, Wn), 7, dtype=torch.int32, device=DEV)
        psum = torch.full((cap,), 7 * Wn, dtype=torch.int64, device=DEV)
        pmax = _i32([ONE])
        N.check(lib.mz_drqn_prio_update(H, E, L, T, cap, wdir.data_ptr(), off.data_ptr(),
                                        tot.data_ptr(), qa_d.data_ptr(), y_d.data_ptr(),
                                        d.data_ptr(), ep.data_ptr(), isw.data_ptr(), alpha, 0.9, 1e-3,
                                        prio.data_ptr(), psum.data_ptr(), pmax.data_ptr(), _stream()))
        g = prio.cpu().numpy()
        assert (g[1, 0], g[2, 1]) == want and int(pmax[0]) == CEIL
        touched = np.zeros_like(g, bool)
        touched[1, 0] = touched[2, 1] = True
        assert (g[~touched] == 7).all()  # entries 2 (slot 9) and 3 (window 3 of 3) were skipped
        assert np.array_equal(psum.cpu().numpy(), g.astype(np.int64).sum(axis=1))
    qa_d.zero_()
    prio = torch.full((cap, Wn), 7, dtype=torch.int32, device=DEV)
    N.check(lib.mz_drqn_prio_update(H, E, L, T, cap, wdir.data_ptr(), off.data_ptr(), tot.data_ptr(),
                                    qa_d.data_ptr(), y_d.data_ptr(), d.data_ptr(), ep.data_ptr(),
                                    isw.data_ptr(), 6.0, 0.9, 1e-3, prio.data_ptr(), psum.data_ptr(),
                                    pmax.data_ptr(), _stream()))
    assert int(prio[1, 0]) == 1 and int(prio[2, 1]) == 1 and int(pmax[0]) == CEIL
    # the skipped entries' rows and loss terms were not scaled
    dd, ee = d.cpu().numpy(), ep.cpu().numpy()
    assert (dd[11:14] == 1.0).all() and (dd[16:19] == 1.0).all() and ee[2] == ee[3] == 1.0
    assert (dd[1:4] == 0.125).all() and ee[0] == 0.125  # three launches, 0.5 each
