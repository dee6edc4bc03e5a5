"""The recurrent DQN's replay-window kernels (csrc/mz_drqn.hip: k_drqn_snapshot, k_drqn_snap_store,
k_drqn_win_sample, k_drqn_win_fwd, k_drqn_win_bwd) through the C ABI, against the float64 model
(tests/drqn_window_model.py) and, bit for bit, against the whole-episode kernels.

The error bound is test_drqn_gpu.py's: with e_ref the largest elementwise error of torch's float32
window_td_loss (+ autograd) on the CPU against the model and e_k the kernel's,
    e_k <= 4 e_ref + 8 u max|tensor|,  u = 2^-24.
Each comparison prints its ratio e_k / (e_ref + 2 u max|tensor|)."""
import ctypes as C
from collections import deque

import numpy as np
import pytest
import torch

import drqn_model as M
import drqn_window_model as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
H, ROW, STASH, PARAMS, SNAP, L = 32, 8, 192, 5252, 64, 8
SHAPES = [(128, 6), (128, 32), (128,), (128,), (4, 32), (4,)]
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _net(seed, scale=1.0):
    from mazerl.agents.lstm_dqn_agent import DQN
    torch.manual_seed(seed)
    net = DQN(6, 4, H, torch.device("cpu"))
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(scale)
    return net


def _dev_params(net):
    ts = [p.detach().to(DEV).contiguous() for p in net.parameters()]
    return ts, (C.c_void_p * 6)(*[t.data_ptr() for t in ts])


def _f64(net):
    return M.as_f64({k: v.detach().numpy() for k, v in net.state_dict().items()})


def _check(name, got, model, ref):
    got, model, ref = (np.asarray(a, np.float64) for a in (got, model, ref))
    mx = np.abs(model).max()
    e_k, e_ref = np.abs(got - model).max(), np.abs(ref - model).max()
    print(f"{name}: e_k {e_k:.3e} e_ref {e_ref:.3e} ratio {e_k / (e_ref + 2 * U * mx + 1e-300):.2f}")
    assert e_k <= 4 * e_ref + 8 * U * mx, (name, e_k, e_ref, mx)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(*s, dtype=torch.float32):
    return torch.full(s, NAN, dtype=dtype, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Mem:
    """A hand-built memory of E episodes (L = 8) in E of E + 2 slots with random snapshots (entry 0
    of every slot is NaN: never read), and the launches over a hand-built window directory."""

    def __init__(self, lib, lens, seed, T):
        self.lib, self.E, self.T = lib, len(lens), T
        E = self.E
        rng = np.random.default_rng(seed)
        self.cap = E + 2
        self.src, self.tgt = _net(seed, 2.0), _net(seed + 1000, 2.0)
        self.eps = [dict(x=rng.random((n + 1, 6)).astype(np.float32), a=rng.integers(0, 4, n),
                         r=(rng.random(n) - 0.5).astype(np.float32), term=bool((e + n + e // 6) % 2))
                    for e, n in enumerate(lens)]
        self.slots = rng.permutation(self.cap)[:E]
        mem = rng.integers(-2 ** 31, 2 ** 31 - 1, (self.cap, L + 1, ROW)).astype(np.int32)
        mem_term, mem_len = np.zeros(self.cap, np.int32), np.zeros(self.cap, np.int32)
        for ep, s in zip(self.eps, self.slots):
            n = len(ep["a"])
            mem[s, :n + 1, :6] = ep["x"].view(np.int32)
            mem[s, :n, 6] = ep["a"]
            mem[s, :n, 7] = ep["r"].view(np.int32)
            mem_term[s], mem_len[s] = ep["term"], n
        self.NS = W.windows_in(L, T)
        self.state = (rng.random((self.cap, self.NS, SNAP)) - 0.5).astype(np.float32)
        self.state[:, 0] = np.nan
        self.mem, self.mem_term, self.mem_len = _d(mem), _d(mem_term), _d(mem_len)
        self.mem_state = _d(self.state)
        self.lens = np.array(lens)
        self.ps, self.pps = _dev_params(self.src)
        self.pt, self.ppt = _dev_params(self.tgt)
        self.rows_cap = E * (min(T, L) + 2)

    def directory(self, js, K):
        """Window js[e] of episode e under burn-in K -> the model's windows (stored state)."""
        self.K = K
        self.ws = [W.window_of(ep, self.T, K, j, self.state[s])
                   for ep, j, s in zip(self.eps, js, self.slots)]
        m = np.array([w["m"] for w in self.ws])
        wdir = np.stack([self.slots, self.lens, [w["b"] for w in self.ws],
                         [w["k"] for w in self.ws], m]).astype(np.int32)
        self.m = m
        self.off = np.concatenate([[0], np.cumsum(m + 2)[:-1]]).astype(np.int64)
        self.rows, self.steps = int((m + 2).sum()), int(m.sum())
        self.wdir, self.w_off = _d(wdir), _d(self.off)
        self.w_tot = _d(np.array([self.rows, self.steps], np.int64))
        return self

    def step_rows(self):
        return np.concatenate([o + 1 + np.arange(m) for o, m in zip(self.off, self.m)])

    def buffers(self):
        E, R = self.E, self.rows_cap
        return dict(qmax=_nan(R), stash=_nan(R, STASH), qa=_nan(R), y=_nan(R), d=_nan(R),
                    ep_loss=_nan(E + 1, dtype=torch.float64), gpart=_nan(E + 1, PARAMS),
                    loss=_nan(2), grads=[_nan(int(np.prod(s)) + 4) for s in SHAPES])

    def forward(self, o, target, state="own", K=None, gamma=0.9):
        from mazerl import _native as N
        K = self.K if K is None else K
        st = self.mem_state if isinstance(state, str) else state
        pp = self.ppt if target else self.pps
        outs = [None] * 5 if target else [o[k] for k in ("stash", "qa", "y", "d", "ep_loss")]
        N.check(self.lib.mz_drqn_window_forward(
            pp, H, int(target), self.E, L, self.T, K, self.cap, gamma, self.mem.data_ptr(),
            self.mem_term.data_ptr(), _ptr(st), self.wdir.data_ptr(), self.w_off.data_ptr(),
            self.w_tot.data_ptr(), o["qmax"].data_ptr(), *[_ptr(t) for t in outs], _stream()))

    def backward(self, o, K=None):
        from mazerl import _native as N
        K = self.K if K is None else K
        pg = (C.c_void_p * 6)(*[g.data_ptr() for g in o["grads"]])
        N.check(self.lib.mz_drqn_window_backward(
            self.pps, H, self.E, L, self.T, K, self.cap, self.mem.data_ptr(),
            self.wdir.data_ptr(), self.w_off.data_ptr(), self.w_tot.data_ptr(),
            o["stash"].data_ptr(), o["d"].data_ptr(), o["ep_loss"].data_ptr(),
            o["gpart"].data_ptr(), pg, o["loss"].data_ptr(), _stream()))

    def run(self, state="own"):
        o = self.buffers()
        self.forward(o, 1, state)
        self.forward(o, 0, state)
        self.backward(o)
        torch.cuda.synchronize()
        return o

    def model(self, gamma=0.9):
        return W.window_td_loss(_f64(self.src), _f64(self.tgt), self.ws, gamma)

    def torch_ref(self, gamma=0.9):
        from mazerl.agents.lstm_dqn_agent import window_td_loss
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))  # noqa: E731
        ws = [(t(w["x"]), torch.from_numpy(np.asarray(w["a"])), t(w["r"]), t(w["h0"]), t(w["c0"]),
               w["k"], w["term"]) for w in self.ws]
        for p in self.src.parameters():
            p.grad = None
        loss = window_td_loss(self.src, self.tgt, ws, gamma)
        loss.backward()
        qa, y = [], []
        with torch.no_grad():
            for x, a, r, h0, c0, k, term in ws:
                m = a.shape[0]
                q = self.src.unroll_from(x[None, :k + m], h0[None], c0[None])[0][0, k:]
                qa.append(q.gather(1, a[:, None]).squeeze(1).numpy())
                yy = r + np.float32(gamma) * self.tgt.unroll_from(
                    x[None], h0[None], c0[None])[0][0, k + 1:].max(dim=1)[0]
                if term:
                    yy[m - 1] = r[m - 1]
                y.append(yy.numpy())
        return dict(qa=np.concatenate(qa), y=np.concatenate(y), loss=loss.item(),
                    grads={k: p.grad.numpy().copy() for k, p in self.src.named_parameters()})

    # the whole-episode kernels on the same memory and episodes
    def whole(self, params, target, qmax=None, gamma=0.9):
        from mazerl import _native as N
        E = self.E
        R = E * (L + 1)
        off = np.concatenate([[0], np.cumsum(self.lens + 1)[:-1]]).astype(np.int64)
        dirs = [_d(self.slots.astype(np.int32)), _d(self.lens.astype(np.int32)), _d(off),
                _d(np.array([(self.lens + 1).sum(), self.lens.sum()], np.int64))]
        o = dict(qmax=_nan(R) if qmax is None else qmax, stash=_nan(R, STASH), qa=_nan(R), y=_nan(R),
                 d=_nan(R), ep_loss=_nan(E, dtype=torch.float64), gpart=_nan(E, PARAMS),
                 loss=_nan(1), grads=[_nan(int(np.prod(s))) for s in SHAPES], off=off, dirs=dirs)
        outs = [None] * 5 if target else [o[k] for k in ("stash", "qa", "y", "d", "ep_loss")]
        N.check(self.lib.mz_drqn_seq_forward(
            params, H, int(target), E, L, self.cap, gamma, self.mem.data_ptr(),
            self.mem_term.data_ptr(), *[t.data_ptr() for t in dirs], o["qmax"].data_ptr(),
            *[_ptr(t) for t in outs], _stream()))
        return o

    def whole_backward(self, o):
        from mazerl import _native as N
        pg = (C.c_void_p * 6)(*[g.data_ptr() for g in o["grads"]])
        N.check(self.lib.mz_drqn_seq_backward(
            self.pps, H, self.E, L, self.cap, self.mem.data_ptr(),
            *[t.data_ptr() for t in o["dirs"]], o["stash"].data_ptr(), o["d"].data_ptr(),
            o["ep_loss"].data_ptr(), o["gpart"].data_ptr(), pg, o["loss"].data_ptr(), _stream()))


def _lens(E, T):
    """n = 1, T, T + 1 (a last window of one step; L - 1 where T + 1 > L), L and two more; E = 1:
    the longest."""
    if E == 1:
        return [L]
    base = [1, T, T + 1 if T + 1 <= L else L - 1, L, 5, 2]
    return [base[e % 6] for e in range(E)]


def _js(lens, T):
    """Window (e + e // 6 + 1) mod ceil(n / T): first, inner and last windows all occur."""
    return [(e + e // 6 + 1) % W.windows_in(n, T) for e, n in enumerate(lens)]


CASES = [(E, T, K) for E in (1, 3, 65) for T, K in
         [(1, 0), (1, 1), (1, 2), (3, 0), (3, 3), (3, 6), (8, 0)]]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "E%d-T%d-K%d" % c)
def win(request, lib):
    E, T, K = request.param
    lens = _lens(E, T)
    s = _Mem(lib, lens, 170 + 7 * E + T, T).directory(_js(lens, T), K)
    return s, s.run(), s.model(), s.torch_ref()


def test_windows_match_the_model(win):
    s, o, m, ref = win
    rows = s.step_rows()
    if s.E == 65:  # the shapes the case is there for
        ks = {w["k"] for w in s.ws}
        assert s.K in ks and 0 in ks
        assert {(w["term"], w["s"] + w["m"] == n) for w, n in zip(s.ws, s.lens)} >= \
            {(True, True), (False, True)} | ({(False, False)} if s.T < L else set())
        assert any(w["m"] == 1 and w["s"] > 0 for w in s.ws) or s.T == 8
    _check("Q_t[a_t]", o["qa"].cpu().numpy()[rows], np.concatenate(m["qa"]), ref["qa"])
    _check("y_t", o["y"].cpu().numpy()[rows], np.concatenate(m["y"]), ref["y"])
    _check("loss", [float(o["loss"][0])], [m["loss"]], [ref["loss"]])
    d = o["d"].cpu().numpy()[rows].astype(np.float64)
    md = 2.0 * (np.concatenate(m["qa"]) - np.concatenate(m["y"])) / s.steps
    rd = 2.0 * (ref["qa"].astype(np.float64) - ref["y"]) / s.steps
    _check("residual", d, md, rd)
    for k, g, shape in zip(M.KEYS, o["grads"], SHAPES):
        n = int(np.prod(shape))
        _check("grad " + k, g.cpu().numpy()[:n].reshape(shape), m["grads"][k], ref["grads"][k])


def test_rows_outside_the_windows_keep_their_sentinels(win):
    s, o, _, _ = win
    rows = s.step_rows()
    entry, guard = s.off, s.off + s.m + 1
    rest = np.setdiff1d(np.arange(s.rows_cap), rows)  # entry rows, guard rows and the pad
    for k in ("qa", "y", "d"):
        v = o[k].cpu().numpy()
        assert np.isnan(v[rest]).all() and not np.isnan(v[rows]).any(), k
    st = o["stash"].cpu().numpy()
    assert not np.isnan(st[rows]).any()
    assert np.isnan(st[entry, :4 * H]).all() and not np.isnan(st[entry, 4 * H:]).any()
    assert np.isnan(st[np.setdiff1d(rest, entry)]).all()
    q = o["qmax"].cpu().numpy()
    assert not np.isnan(q[rows]).any() and not np.isnan(q[guard]).any()
    assert np.isnan(q[np.setdiff1d(rest, guard)]).all()
    assert torch.isnan(o["gpart"][s.E]).all() and not torch.isnan(o["gpart"][:s.E]).any()
    assert torch.isnan(o["ep_loss"][s.E]) and not torch.isnan(o["ep_loss"][:s.E]).any()
    assert torch.isnan(o["loss"][1])
    for g, shape in zip(o["grads"], SHAPES):
        assert torch.isnan(g[int(np.prod(shape)):]).all()  # nothing past the segment


def test_two_runs_are_bit_identical(win):
    s, o, _, _ = win
    o2 = s.run()
    for k in ("qmax", "stash", "qa", "y", "d", "ep_loss", "gpart", "loss"):
        assert np.array_equal(o[k].cpu().numpy(), o2[k].cpu().numpy(), equal_nan=True), k
    for a, b in zip(o["grads"], o2["grads"]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("E", [1, 3, 65])
def test_one_window_per_whole_episode_is_the_sequence_kernels_bits(lib, E):
    """T = L, K = 0: every output the two paths share, on the same episodes."""
    lens = [L] if E == 1 else [[1, 2, 7, 3, 8][e % 5] for e in range(E)]
    s = _Mem(lib, lens, 300 + E, L).directory([0] * E, 0)
    o = s.run()
    t = s.whole(s.ppt, 1)
    w = s.whole(s.pps, 0, qmax=t["qmax"])
    s.whole_backward(w)
    torch.cuda.synchronize()
    rw = np.concatenate([a + np.arange(n) for a, n in zip(w["off"], s.lens)])
    rows = s.step_rows()
    for k in ("qa", "y", "d", "stash"):
        assert np.array_equal(o[k].cpu().numpy()[rows], w[k].cpu().numpy()[rw]), k
    # the target's q of x_0 .. x_n: the window's step rows and its guard row
    rq = np.concatenate([a + np.arange(n + 1) for a, n in zip(w["off"], s.lens)])
    rqw = np.concatenate([a + 1 + np.arange(n + 1) for a, n in zip(s.off, s.lens)])
    assert np.array_equal(o["qmax"].cpu().numpy()[rqw], w["qmax"].cpu().numpy()[rq])
    for k in ("ep_loss", "gpart"):
        assert np.array_equal(o[k].cpu().numpy()[:E], w[k].cpu().numpy()), k
    assert float(o["loss"][0]) == float(w["loss"][0])
    for a, b, shape in zip(o["grads"], w["grads"], SHAPES):
        assert np.array_equal(a.cpu().numpy()[:int(np.prod(shape))], b.cpu().numpy())


@pytest.mark.parametrize("T", [1, 3])
def test_a_window_from_the_whole_episode_state_gives_the_whole_episode_rows(lib, T):
    """Snapshot j = the whole-episode forward's (h, c) after step j T - 1 (the source's for the
    source net, the target's for the target net), K = 0: the window's qa, stash and qmax rows are
    the whole-episode rows j T .. j T + m - 1 (qmax: .. + m). Without any snapshot, K = 2 T L
    (burn-in from the episode's start): the same."""
    lens = [L, L - 1, T + 1, L, 5, 2]
    s = _Mem(lib, lens, 400 + T, T)
    js = [(e + 1) % W.windows_in(n, T) for e, n in enumerate(lens)]
    assert max(js) >= 2 and 0 in js
    tq = s.whole(s.ppt, 1)
    ws = s.whole(s.pps, 0, qmax=tq["qmax"])
    wt = s.whole(s.ppt, 0)  # (the target's parameters in source mode: its stash)
    torch.cuda.synchronize()

    def snaps(stash):
        st = np.full((s.cap, s.NS, SNAP), np.nan, np.float32)
        v = stash.cpu().numpy()
        for e, (n, slot) in enumerate(zip(lens, s.slots)):
            for j in range(1, W.windows_in(n, T)):
                row = v[ws["off"][e] + j * T - 1]
                st[slot, j] = np.concatenate([row[5 * H:], row[4 * H:5 * H]])  # (h, c)
        return _d(st)

    s.directory(js, 0)
    rows = s.step_rows()
    rw = np.concatenate([ws["off"][e] + js[e] * T + np.arange(m) for e, m in enumerate(s.m)])
    rq = np.concatenate([ws["off"][e] + js[e] * T + np.arange(m + 1) for e, m in enumerate(s.m)])
    rqw = np.concatenate([a + 1 + np.arange(m + 1) for a, m in zip(s.off, s.m)])
    runs = [("stored", 0, snaps(ws["stash"]), snaps(wt["stash"]))]
    s2 = _Mem(lib, lens, 400 + T, T)  # the same memory; burn-in from the episode's start
    s2.directory(js, 2 * T * L)
    assert all(w["b"] == 0 for w in s2.ws) and np.array_equal(s2.off, s.off)
    runs.append(("zero", 2 * T * L, None, None))
    for name, K, st_src, st_tgt in runs:
        mm = s if name == "stored" else s2
        o = mm.buffers()
        mm.forward(o, 1, st_tgt, K)
        mm.forward(o, 0, st_src, K)
        torch.cuda.synchronize()
        assert np.array_equal(o["qmax"].cpu().numpy()[rqw], tq["qmax"].cpu().numpy()[rq]), name
        for k in ("qa", "y", "stash"):
            assert np.array_equal(o[k].cpu().numpy()[rows], ws[k].cpu().numpy()[rw]), (name, k)


@pytest.mark.parametrize("T,K", [(1, 2), (3, 3), (3, 6)])
def test_burn_in_carries_no_gradient(lib, T, K):
    """A window with K > 0, and the same window with K = 0 whose snapshot is the state the burn-in
    produced (read back from the source forward's entry row) on the same targets: the same
    gradient bits."""
    lens = [L, L - 1, T + 1, L, 5, 2 * T]
    s = _Mem(lib, lens, 500 + T + K, T)
    js = [W.windows_in(n, T) - 1 - (e % 2) for e, n in enumerate(lens)]
    s.directory(js, K)
    assert max(w["k"] for w in s.ws) == K
    a = s.run()
    entry = a["stash"].cpu().numpy()[s.off]
    st = np.full((s.cap, s.NS, SNAP), np.nan, np.float32)
    for e, slot in enumerate(s.slots):
        st[slot, js[e]] = np.concatenate([entry[e, 5 * H:], entry[e, 4 * H:5 * H]])
    off = s.off.copy()
    s.directory(js, 0)
    assert np.array_equal(off, s.off)
    b = s.buffers()
    b["qmax"] = a["qmax"]
    # (window 0 has no snapshot: its entry state is zero in both runs)
    s.forward(b, 0, _d(st))
    s.backward(b)
    torch.cuda.synchronize()
    for k in ("qa", "y", "d", "stash", "ep_loss", "gpart", "loss"):
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), equal_nan=True), k
    for x, y in zip(a["grads"], b["grads"]):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
    for x, shape in zip(a["grads"], SHAPES):
        assert not torch.isnan(x[:int(np.prod(shape))]).any()


def _sample(lib, seed, counter, E, T, K, cap, ring, mem_len, wdir, off, tot):
    from mazerl import _native as N
    N.check(lib.mz_drqn_window_sample(seed, counter, H, E, L, T, K, cap, cap, ring.data_ptr(),
                                      mem_len.data_ptr(), wdir.data_ptr(), off.data_ptr(),
                                      tot.data_ptr(), _stream()))


@pytest.mark.parametrize("E", [1, 3, 65])
def test_sampler_takes_the_episode_sampler_slots_and_builds_the_directory(lib, E):
    from mazerl import _native as N
    cap, T, K = 70, 3, 3
    rng = np.random.default_rng(600 + E)
    lens = rng.integers(1, L + 1, cap).astype(np.int32)
    lens[:4] = [1, T, T + 1, L]
    mem_len = _d(lens)
    ring = _d(np.array([17, cap], np.int64))
    kw = dict(device=DEV)
    seen = []
    for seed, counter in [(5, 0), (5, 1), (6, 0), (5, 0)]:
        wdir = torch.full((5, E), -9, dtype=torch.int32, **kw)
        off, tot = torch.full((E,), -9, dtype=torch.int64, **kw), torch.zeros(2, dtype=torch.int64, **kw)
        _sample(lib, seed, counter, E, T, K, cap, ring, mem_len, wdir, off, tot)
        ds, dl = torch.zeros(E, dtype=torch.int32, **kw), torch.zeros(E, dtype=torch.int32, **kw)
        do, dt = torch.zeros(E, dtype=torch.int64, **kw), torch.zeros(2, dtype=torch.int64, **kw)
        N.check(lib.mz_drqn_sample(seed, counter, E, L, cap, cap, ring.data_ptr(),
                                   mem_len.data_ptr(), ds.data_ptr(), dl.data_ptr(), do.data_ptr(),
                                   dt.data_ptr(), _stream()))
        w = wdir.cpu().numpy()
        slot, n, b, k, m = w
        assert np.array_equal(slot, ds.cpu().numpy()) and np.array_equal(n, lens[slot])
        s = b + k
        j = s // T
        assert (s % T == 0).all() and (j >= 0).all() and (j < (n - 1) // T + 1).all()
        assert np.array_equal(b, np.maximum(0, s - K)) and np.array_equal(m, np.minimum(T, n - s))
        assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum(m + 2)[:-1]]))
        assert tot.cpu().tolist() == [int((m + 2).sum()), int(m.sum())]
        seen.append(w)
    assert np.array_equal(seen[0], seen[3])  # the same key, the same bits
    if E > 1:  # (one draw over at most 3 windows may well repeat)
        assert not np.array_equal(seen[0][2:], seen[1][2:]) or not np.array_equal(seen[0][0], seen[1][0])
        assert not np.array_equal(seen[0][2:], seen[2][2:]) or not np.array_equal(seen[0][0], seen[2][0])


def test_sampler_windows_are_uniform_within_an_episode(lib):
    """770 launches of E = 65 over 70 episodes of 5 steps, T = 1 (5 windows each): 50,050 draws,
    chi-square against uniform (p > 1e-6, the other draw tests' significance); and the window
    draw is independent of the batch position's slot draw (its own stream): the counts per
    window are uniform at the first batch position too."""
    from scipy.stats import chi2
    cap, E, T, n_launch = 70, 65, 1, 770
    mem_len = _d(np.full(cap, 5, np.int32))
    ring = _d(np.array([0, cap], np.int64))
    kw = dict(device=DEV)
    wdir = torch.full((n_launch, 5, E), -9, dtype=torch.int32, **kw)
    off, tot = torch.zeros(E, dtype=torch.int64, **kw), torch.zeros(2, dtype=torch.int64, **kw)
    for c in range(n_launch):
        _sample(lib, 9, c, E, T, 0, cap, ring, mem_len, wdir[c], off, tot)
    w = wdir.cpu().numpy()
    j = w[:, 2] + w[:, 3]  # b + k = j T
    assert j.min() == 0 and j.max() == 4 and (w[:, 4] == 1).all()
    n = np.bincount(j.ravel(), minlength=5)
    exp = j.size / 5
    assert j.size >= 50000
    assert chi2.sf(((n - exp) ** 2 / exp).sum(), 4) > 1e-6, n.tolist()
    other = torch.full((5, E), -9, dtype=torch.int32, **kw)
    _sample(lib, 10, 3, E, T, 0, cap, ring, mem_len, other, off, tot)
    assert not np.array_equal(other.cpu().numpy()[2], w[3, 2])


@pytest.mark.parametrize("B", [1, 130])
def test_snapshot_lands_only_at_window_starts(lib, B):
    from mazerl import _native as N
    T = 3
    NS = W.windows_in(L, T)
    rng = np.random.default_rng(700 + B)
    t = ((np.arange(B) + 7) % (L + 3) - 1).astype(np.int32)  # -1 .. L + 1; B = 1: t = 6
    h = (rng.random((H, B)) - 0.5).astype(np.float32)
    c = (rng.random((H, B)) - 0.5).astype(np.float32)
    rec = _nan(B, NS, SNAP)
    td, hd, cd = _d(t), _d(h), _d(c)
    N.check(lib.mz_drqn_snapshot(H, B, L, T, td.data_ptr(), hd.data_ptr(), cd.data_ptr(),
                                 rec.data_ptr(), _stream()))
    got = rec.cpu().numpy()
    hit = 0
    for i in range(B):
        want = np.full((NS, SNAP), np.nan, np.float32)
        if 0 < t[i] < L and t[i] % T == 0:
            want[t[i] // T] = np.concatenate([h[:, i], c[:, i]])
            hit += 1
        assert np.array_equal(got[i], want, equal_nan=True), (i, t[i])
    assert hit == int(((t > 0) & (t < L) & (t % T == 0)).sum()) and hit >= 1


def test_snapshot_store_follows_the_ring_like_a_deque(lib):
    """test_drqn_gpu's store plan (capacity 5, four instances, 8 episodes over three steps, the
    ring wraps, one 1-step episode that mz_ppo_scan drops), T = 3: mem_state[slot][1 .. ceil(n / T)
    - 1] holds the stored episode's snapshots for every slot a deque(maxlen=5) holds; entry 0 and
    slots not yet written keep their sentinels."""
    from mazerl import _native as N
    B, CAP, T = 4, 5, 3
    NS = W.windows_in(L, T)
    rng = np.random.default_rng(60)
    kw = dict(device=DEV)
    t = torch.zeros(B, dtype=torch.int32, **kw)
    rec_x = torch.zeros(B, L + 1, 6, **kw)
    rec_a = torch.zeros(B, L, dtype=torch.int32, **kw)
    rec_r = torch.zeros(B, L, dtype=torch.float64, **kw)
    fin_id = torch.zeros(B, dtype=torch.int32, **kw)
    fin_off = torch.zeros(B, dtype=torch.int64, **kw)
    fin_len = torch.zeros(B, dtype=torch.int32, **kw)
    fin_count = torch.zeros(1, dtype=torch.int32, **kw)
    pool = torch.zeros(2, dtype=torch.int64, **kw)
    stats = torch.zeros(4, dtype=torch.int64, **kw)
    mem = torch.zeros(CAP, L + 1, ROW, dtype=torch.int32, **kw)
    mem_len = torch.zeros(CAP, dtype=torch.int32, **kw)
    mem_term = torch.zeros(CAP, dtype=torch.int32, **kw)
    mem_state = _nan(CAP, NS, SNAP)
    ring = torch.zeros(2, dtype=torch.int64, **kw)
    dq, total = deque(maxlen=CAP), 0
    plan = [{0: (2, 1), 2: (8, 0), 3: (5, 1)},
            {0: (1, 1), 1: (7, 0), 2: (3, 1)},
            {0: (4, 0), 1: (2, 1), 3: (6, 1)}]
    for step in plan:
        tv = np.array([step[i][0] - 1 if i in step else 3 for i in range(B)], np.int32)
        term = np.array([step[i][1] if i in step else 0 for i in range(B)], np.uint8)
        trunc = np.array([1 - step[i][1] if i in step else 0 for i in range(B)], np.uint8)
        snap = rng.random((B, NS, SNAP)).astype(np.float32)
        t.copy_(torch.from_numpy(tv))
        r64, tm_d, tr_d = _d(rng.random(B)), _d(term), _d(trunc)
        o6, snap_d = _d(rng.random((B, 6)).astype(np.float32)), _d(snap)
        N.check(lib.mz_ppo_scan(r64.data_ptr(), tm_d.data_ptr(), tr_d.data_ptr(), B, L, t.data_ptr(),
                                rec_r.data_ptr(), fin_id.data_ptr(), fin_off.data_ptr(),
                                fin_len.data_ptr(), fin_count.data_ptr(), pool[0:].data_ptr(),
                                pool[1:].data_ptr(), stats.data_ptr(), _stream()))
        N.check(lib.mz_drqn_snap_store(H, B, L, T, fin_id.data_ptr(), fin_len.data_ptr(),
                                       fin_count.data_ptr(), snap_d.data_ptr(), CAP,
                                       mem_state.data_ptr(), ring.data_ptr(), _stream()))
        N.check(lib.mz_drqn_store(o6.data_ptr(), tm_d.data_ptr(), B, L, fin_id.data_ptr(),
                                  fin_len.data_ptr(), fin_count.data_ptr(), rec_x.data_ptr(),
                                  rec_a.data_ptr(), rec_r.data_ptr(), CAP, mem.data_ptr(),
                                  mem_len.data_ptr(), mem_term.data_ptr(), ring.data_ptr(),
                                  _stream()))
        for i in sorted(step):
            n = step[i][0]
            if n >= 2:  # mz_ppo_scan drops 1-step episodes
                dq.append((n, snap[i]))
                total += 1
        assert tuple(int(v) for v in ring.cpu()) == (total % CAP, len(dq))
        ms = mem_state.cpu().numpy()
        assert np.isnan(ms[:, 0]).all()
        for j, (n, sn) in enumerate(dq):
            slot = (total - len(dq) + j) % CAP
            nw = W.windows_in(n, T)
            assert int(mem_len[slot]) == n
            assert np.array_equal(ms[slot, 1:nw], sn[1:nw]), (slot, n)
        if total == 3:  # no slot written twice yet: nothing but the snapshots above
            assert np.isnan(ms[3:]).all()
            for j, (n, _) in enumerate(dq):
                assert np.isnan(ms[j, W.windows_in(n, T):]).all(), j
    assert total == 8


def test_window_entry_points_refuse_bad_arguments(lib):
    from mazerl import _native as N
    net = _net(7)
    _, ptrs = _keep = _dev_params(net)
    z = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = z.data_ptr()
    st = _stream()
    nul = [None] * 5

    def fwd(pp=ptrs, hid=H, target=1, E=2, T=3, K=3, cap=5, mem=p, outs=nul):
        return lib.mz_drqn_window_forward(pp, hid, target, E, L, T, K, cap, 0.9, mem, p, None, p, p,
                                          p, p, *outs, st)

    def bwd(pp=ptrs, hid=H, E=2, T=3, K=3, cap=5, grads=ptrs, gpart=p):
        return lib.mz_drqn_window_backward(pp, hid, E, L, T, K, cap, p, p, p, p, p, p, p, gpart,
                                           grads, p, st)

    def smp(hid=H, E=2, T=3, K=3, cap=5, filled=5, wdir=p):
        return lib.mz_drqn_window_sample(0, 0, hid, E, L, T, K, cap, filled, p, p, wdir, p, p, st)

    def snap(hid=H, B=4, T=3, rec=p):
        return lib.mz_drqn_snapshot(hid, B, L, T, p, p, p, rec, st)

    def sst(hid=H, B=4, T=3, cap=5, ms=p):
        return lib.mz_drqn_snap_store(hid, B, L, T, p, p, p, p, cap, ms, p, st)

    bad = [
        lambda: fwd(pp=None), lambda: fwd(mem=None), lambda: fwd(target=0),  # null outputs
        lambda: fwd(T=0), lambda: fwd(K=-3), lambda: fwd(K=4), lambda: fwd(hid=16),
        lambda: fwd(E=0), lambda: fwd(E=6),
        lambda: bwd(pp=None), lambda: bwd(grads=None), lambda: bwd(gpart=None),
        lambda: bwd(T=0), lambda: bwd(K=-3), lambda: bwd(K=2), lambda: bwd(hid=8),
        lambda: bwd(E=0), lambda: bwd(E=6),
        lambda: smp(wdir=None), lambda: smp(T=0), lambda: smp(K=-3), lambda: smp(K=5),
        lambda: smp(hid=16), lambda: smp(E=0), lambda: smp(E=6), lambda: smp(filled=1),
        lambda: snap(rec=None), lambda: snap(T=0), lambda: snap(hid=16), lambda: snap(B=0),
        lambda: sst(ms=None), lambda: sst(T=0), lambda: sst(hid=16), lambda: sst(B=0),
        lambda: sst(cap=0),
    ]
    for k, f in enumerate(bad):
        assert f() == -1, k  # MZ_EINVAL
        with pytest.raises(ValueError):
            N.check(f())
    torch.cuda.synchronize()
    assert bool((z == 0).all())
