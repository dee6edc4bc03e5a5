"""The recurrent DQN kernels (csrc/mz_drqn.hip) through the C ABI against the float64 model
(tests/drqn_model.py).

Error bounds, none taken from the kernels' output. The device expf / tanhf / division cannot be
counted in roundings, so every compared tensor is also computed by torch's float32 nn.LSTMCell +
nn.Linear (+ autograd) on the CPU from the same weights and inputs: with e_ref its largest
elementwise error against the model and e_k the kernel's,
    e_k <= 4 e_ref + 8 u max|tensor|,  u = 2^-24
(4: another summation order and another libm over chains of the same length; the floor: tensors
torch happens to get exactly). Each test prints its ratios e_k / (e_ref + 2 u max|tensor|)."""
import ctypes as C
from collections import deque

import numpy as np
import pytest
import torch

import drqn_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
H, ROW, STASH, PARAMS = 32, 8, 192, 5252
SHAPES = [(128, 6), (128, 32), (128,), (128,), (4, 32), (4,)]


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
    assert [tuple(t.shape) for t in ts] == SHAPES
    return ts, (C.c_void_p * 6)(*[t.data_ptr() for t in ts])


def _f64(net):
    return M.as_f64({k: v.detach().numpy() for k, v in net.state_dict().items()})


def _check(name, got, model, ref):
    got, model, ref = (np.asarray(a, np.float64) for a in (got, model, ref))
    mx = np.abs(model).max()
    e_k, e_ref = np.abs(got - model).max(), np.abs(ref - model).max()
    print(f"{name}: e_k {e_k:.3e} e_ref {e_ref:.3e} ratio {e_k / (e_ref + 2 * U * mx + 1e-300):.2f}")
    assert e_k <= 4 * e_ref + 8 * U * mx, (name, e_k, e_ref, mx)


def _act(lib, ptrs, obs6, L, eps, explore, seed, counter, t, h, c, rec_x, rec_a, out, q=None):
    from mazerl import _native as N
    N.check(lib.mz_drqn_act(ptrs, H, obs6.data_ptr(), obs6.shape[0], L, eps, explore, seed, counter,
                            t.data_ptr(), h.data_ptr(), c.data_ptr(),
                            rec_x.data_ptr() if rec_x is not None else None,
                            rec_a.data_ptr() if rec_a is not None else None, out.data_ptr(),
                            q.data_ptr() if q is not None else None, _stream()))


# ---- mz_drqn_act ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 130])
def test_act_matches_the_model_and_records_at_the_step_index_only(lib, B):
    L = 8
    net = _net(5, 2.0)
    rng = np.random.default_rng(50 + B)
    x = rng.random((B, 6)).astype(np.float32)
    h0 = (rng.random((B, H)) - 0.5).astype(np.float32)
    c0 = (rng.random((B, H)) - 0.5).astype(np.float32)
    t = (np.arange(B) % L).astype(np.int32)
    hz, cz = np.where(t[:, None] == 0, 0, h0), np.where(t[:, None] == 0, 0, c0)
    hz, cz = hz.astype(np.float32), cz.astype(np.float32)
    (mh, mc, mq), (rh, rc, rq), q_bound = _one_step(net, x, hz, cz)
    # the greedy action is decided: the model's top-two gap exceeds twice the q bound on every row
    top = np.sort(mq, axis=1)
    assert ((top[:, 3] - top[:, 2]) > 2 * q_bound).all()
    _, ptrs = _keep = _dev_params(net)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    obs6, tt = d(x), d(t)
    h, c = d(h0.T), d(c0.T)  # [32][B]
    rec_x = torch.full((B, L + 1, 6), float("nan"), device=DEV)
    rec_a = torch.full((B, L), -7, dtype=torch.int32, device=DEV)
    out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    q = torch.zeros(B, 4, device=DEV)
    _act(lib, ptrs, obs6, L, 0.0, 4, 9, 0, tt, h, c, rec_x, rec_a, out, q)
    a = out.cpu().numpy()
    assert np.array_equal(a, mq.argmax(axis=1))
    _check("act h'", h.cpu().numpy().T, mh, rh)
    _check("act c'", c.cpu().numpy().T, mc, rc)
    _check("act q", q.cpu().numpy(), mq, rq)
    rx, ra = rec_x.cpu().numpy(), rec_a.cpu().numpy()
    for i in range(B):
        assert np.array_equal(rx[i, t[i]], x[i]) and ra[i, t[i]] == a[i]
        assert np.isnan(np.delete(rx[i], t[i], axis=0)).all()
        assert (np.delete(ra[i], t[i]) == -7).all()


def _one_step(net, x, h, c):
    """Model and torch-f32 (h', c', q) of one step, and the q bound of the module docstring."""
    P = _f64(net)
    mh, mc, _ = M.cell(P, x.astype(np.float64), h.astype(np.float64), c.astype(np.float64))
    mq = M.head(P, mh)
    with torch.no_grad():
        rh, rc = net.lstm_cell(torch.from_numpy(x), (torch.from_numpy(h), torch.from_numpy(c)))
        rq = net.fc(rh)
    bound = 4 * np.abs(rq.numpy() - mq).max() + 8 * U * np.abs(mq).max()
    return (mh, mc, mq), (rh.numpy(), rc.numpy(), rq.numpy()), bound


def test_act_out_of_range_step_index_acts_without_record_or_state_change(lib):
    B, L = 70, 8
    net = _net(6, 2.0)
    _, ptrs = _keep = _dev_params(net)
    rng = np.random.default_rng(61)
    x = rng.random((B, 6)).astype(np.float32)
    h0 = (rng.random((B, H)) - 0.5).astype(np.float32)
    c0 = (rng.random((B, H)) - 0.5).astype(np.float32)
    (mh, mc, mq), (rh, rc, rq), bound = _one_step(net, x, h0, c0)
    top = np.sort(mq, axis=1)
    assert ((top[:, 3] - top[:, 2]) > 2 * bound).all()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    obs6, h, c = d(x), d(h0.T), d(c0.T)
    t = torch.tensor([L, -1, 100, L + 1, -2 ** 31] * (B // 5), dtype=torch.int32, device=DEV)
    rec_x = torch.full((B, L + 1, 6), float("nan"), device=DEV)
    rec_a = torch.full((B, L), -7, dtype=torch.int32, device=DEV)
    out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _act(lib, ptrs, obs6, L, 0.0, 4, 9, 0, t, h, c, rec_x, rec_a, out)
    assert np.array_equal(out.cpu().numpy(), mq.argmax(axis=1))
    assert np.array_equal(h.cpu().numpy().T, h0) and np.array_equal(c.cpu().numpy().T, c0)
    assert torch.isnan(rec_x).all() and bool((rec_a == -7).all())
    # L == 0, the evaluation mode: no record buffers, every state advances
    out.fill_(-1)
    _act(lib, ptrs, obs6, 0, 0.0, 4, 9, 0, torch.ones_like(t), h, c, None, None, out)
    assert np.array_equal(out.cpu().numpy(), mq.argmax(axis=1))
    _check("eval h'", h.cpu().numpy().T, mh, rh)
    _check("eval c'", c.cpu().numpy().T, mc, rc)


@pytest.mark.parametrize("explore", [4, 2])
def test_act_exploration_draws_are_uniform_and_keyed(lib, explore):
    """eps = 1: 4 x 10^4 draws over 10 counters, chi-square against uniform over explore_actions
    (p-value > 1e-6, the other draw tests' significance); same (seed, counter) -> same bits."""
    from scipy.stats import chi2
    B, L = 4000, 8
    net = _net(7)
    _, ptrs = _keep = _dev_params(net)
    obs6 = torch.rand(B, 6, device=DEV)
    t = torch.zeros(B, dtype=torch.int32, device=DEV)
    h, c = torch.zeros(H, B, device=DEV), torch.zeros(H, B, device=DEV)
    rec_x = torch.zeros(B, L + 1, 6, device=DEV)
    rec_a = torch.zeros(B, L, dtype=torch.int32, device=DEV)
    outs = []
    for k in range(10):
        out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        _act(lib, ptrs, obs6, L, 1.0, explore, 77, k, t, h, c, rec_x, rec_a, out)
        outs.append(out)
    again = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _act(lib, ptrs, obs6, L, 1.0, explore, 77, 3, t, h, c, rec_x, rec_a, again)
    assert torch.equal(again, outs[3]) and not torch.equal(outs[3], outs[4])
    other = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _act(lib, ptrs, obs6, L, 1.0, explore, 78, 3, t, h, c, rec_x, rec_a, other)
    assert not torch.equal(other, outs[3])
    a = torch.cat(outs).cpu().numpy()
    n = np.bincount(a, minlength=4)
    assert n[explore:].sum() == 0
    exp = a.size / explore
    stat = ((n[:explore] - exp) ** 2 / exp).sum()
    assert chi2.sf(stat, explore - 1) > 1e-6, n.tolist()


def test_entry_points_refuse_bad_arguments(lib):
    from mazerl import _native as N
    net = _net(7)
    _, ptrs = _keep = _dev_params(net)
    z = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = z.data_ptr()
    st = _stream()
    bad = [
        lambda: lib.mz_drqn_act(ptrs, 16, p, 4, 8, 0.0, 4, 0, 0, p, p, p, p, p, p, None, st),
        lambda: lib.mz_drqn_act(ptrs, H, p, 0, 8, 0.0, 4, 0, 0, p, p, p, p, p, p, None, st),
        lambda: lib.mz_drqn_act(ptrs, H, None, 4, 8, 0.0, 4, 0, 0, p, p, p, p, p, p, None, st),
        lambda: lib.mz_drqn_act(None, H, p, 4, 8, 0.0, 4, 0, 0, p, p, p, p, p, p, None, st),
        lambda: lib.mz_drqn_act(ptrs, H, p, 4, 8, 0.0, 5, 0, 0, p, p, p, p, p, p, None, st),
        lambda: lib.mz_drqn_store(p, p, 0, 8, p, p, p, p, p, p, 5, p, p, p, p, st),
        lambda: lib.mz_drqn_store(p, p, 4, 8, p, p, p, p, p, p, 5, None, p, p, p, st),
        lambda: lib.mz_drqn_sample(0, 0, 0, 8, 5, 5, p, p, p, p, p, p, st),
        lambda: lib.mz_drqn_sample(0, 0, 6, 8, 5, 5, p, p, p, p, p, p, st),   # capacity < E
        lambda: lib.mz_drqn_sample(0, 0, 4, 8, 5, 3, p, p, p, p, p, p, st),   # E > filled
        lambda: lib.mz_drqn_seq_forward(ptrs, 16, 1, 2, 8, 5, 0.9, p, p, p, p, p, p, p, None, None,
                                        None, None, None, st),
        lambda: lib.mz_drqn_seq_forward(ptrs, H, 0, 2, 8, 5, 0.9, p, p, p, p, p, p, p, None, None,
                                        None, None, None, st),
        lambda: lib.mz_drqn_seq_forward(ptrs, H, 1, 0, 8, 5, 0.9, p, p, p, p, p, p, p, None, None,
                                        None, None, None, st),
        lambda: lib.mz_drqn_seq_forward(ptrs, H, 1, 6, 8, 5, 0.9, p, p, p, p, p, p, p, None, None,
                                        None, None, None, st),
        lambda: lib.mz_drqn_seq_backward(ptrs, H, 2, 8, 5, p, p, p, p, p, p, p, p, p, None, p, st),
        lambda: lib.mz_drqn_seq_backward(ptrs, 8, 2, 8, 5, p, p, p, p, p, p, p, p, p, ptrs, p, st),
    ]
    for k, f in enumerate(bad):
        assert f() == -1, k  # MZ_EINVAL
        with pytest.raises(ValueError):
            N.check(f())
    assert bool((z == 0).all())


# ---- mz_drqn_store / mz_drqn_sample ---------------------------------------------------------
def test_store_fills_the_ring_like_a_deque_and_sample_draws_distinct_slots(lib):
    """Capacity 5, four instances, L = 8: 8 episodes finish over three steps (3, 2 and 3 in a
    step; the ring wraps), and one 1-step episode that mz_ppo_scan drops. Slot contents, order,
    head and count equal a Python deque(maxlen=5)."""
    from mazerl import _native as N
    from scipy.stats import chi2
    B, L, CAP = 4, 8, 5
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
    mem = torch.full((CAP, L + 1, ROW), -1, dtype=torch.int32, **kw)
    mem_len = torch.zeros(CAP, dtype=torch.int32, **kw)
    mem_term = torch.full((CAP,), -1, dtype=torch.int32, **kw)
    ring = torch.zeros(2, dtype=torch.int64, **kw)
    dq = deque(maxlen=CAP)
    total = 0
    # per step: instance -> (length of the episode ending now, terminated) or None
    plan = [{0: (2, 1), 2: (8, 0), 3: (5, 1)},
            {0: (1, 1), 1: (7, 0), 2: (3, 1)},
            {0: (4, 0), 1: (2, 1), 3: (6, 1)}]
    for step in plan:
        tv = np.zeros(B, np.int32)
        term, trunc = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
        xs = rng.random((B, L + 1, 6)).astype(np.float32)
        av = rng.integers(0, 4, (B, L)).astype(np.int32)
        rv = rng.random((B, L))  # float64 with bits below float32's
        obs6 = rng.random((B, 6)).astype(np.float32)
        for i in range(B):
            if i in step:
                n, tm = step[i]
                tv[i] = n - 1
                term[i], trunc[i] = tm, 1 - tm
            else:
                tv[i] = 3
        r_now = rv[np.arange(B), tv].copy()
        rv_before = rv.copy()
        rv_before[np.arange(B), tv] = -5.0  # the scan writes the step's reward here
        t.copy_(torch.from_numpy(tv))
        rec_x.copy_(torch.from_numpy(xs))
        rec_a.copy_(torch.from_numpy(av))
        rec_r.copy_(torch.from_numpy(rv_before))
        d = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
        r64, tm_d, tr_d, o6 = d(r_now), d(term), d(trunc), d(obs6)
        N.check(lib.mz_ppo_scan(r64.data_ptr(), tm_d.data_ptr(), tr_d.data_ptr(), B, L, t.data_ptr(),
                                rec_r.data_ptr(), fin_id.data_ptr(), fin_off.data_ptr(),
                                fin_len.data_ptr(), fin_count.data_ptr(), pool[0:].data_ptr(),
                                pool[1:].data_ptr(), stats.data_ptr(), _stream()))
        N.check(lib.mz_drqn_store(o6.data_ptr(), tm_d.data_ptr(), B, L, fin_id.data_ptr(),
                                  fin_len.data_ptr(), fin_count.data_ptr(), rec_x.data_ptr(),
                                  rec_a.data_ptr(), rec_r.data_ptr(), CAP, mem.data_ptr(),
                                  mem_len.data_ptr(), mem_term.data_ptr(), ring.data_ptr(),
                                  _stream()))
        for i in sorted(step):
            n, tm = step[i]
            if n < 2:
                continue  # mz_ppo_scan drops 1-step episodes: never in the memory
            x = xs[i, :n + 1].copy()
            x[n] = obs6[i]
            dq.append(dict(x=x, a=av[i, :n].copy(), r=rv[i, :n].astype(np.float32), term=tm))
            total += 1
            assert np.array_equal(rec_x[i, n].cpu().numpy(), obs6[i])  # x_n into the record too
        head, count = (int(v) for v in ring.cpu())
        assert (head, count) == (total % CAP, len(dq))
        m = mem.cpu().numpy()
        for j, ep in enumerate(dq):  # the deque's j-th element is episode total - len + j
            slot = (total - len(dq) + j) % CAP
            n = len(ep["a"])
            assert int(mem_len[slot]) == n and int(mem_term[slot]) == ep["term"]
            assert np.array_equal(m[slot, :n + 1, :6].view(np.float32), ep["x"])
            assert np.array_equal(m[slot, :n, 6], ep["a"])
            assert np.array_equal(m[slot, :n, 7].view(np.float32), ep["r"])
        if total == 3:  # partly filled: slots 0..2
            ds = torch.full((400, 2), -1, dtype=torch.int32, **kw)
            dl, do = torch.zeros(2, dtype=torch.int32, **kw), torch.zeros(2, dtype=torch.int64, **kw)
            dt = torch.zeros(2, dtype=torch.int64, **kw)
            for k in range(400):
                N.check(lib.mz_drqn_sample(5, k, 2, L, CAP, 3, ring.data_ptr(), mem_len.data_ptr(),
                                           ds[k].data_ptr(), dl.data_ptr(), do.data_ptr(),
                                           dt.data_ptr(), _stream()))
            s = ds.cpu().numpy()
            assert s.min() == 0 and s.max() == 2 and (s[:, 0] != s[:, 1]).all()
            assert lib.mz_drqn_sample(5, 0, 4, L, CAP, 3, ring.data_ptr(), mem_len.data_ptr(),
                                      ds.data_ptr(), dl.data_ptr(), do.data_ptr(), dt.data_ptr(),
                                      _stream()) == -1  # E > filled
    assert total == 8 and int(stats[2]) == 1
    # the directory of one draw, then 2 x 10^4 draws over counters: every slot equally likely
    E, n_launch = 3, 6667
    ds = torch.full((n_launch, E), -1, dtype=torch.int32, **kw)
    dl, do = torch.zeros(E, dtype=torch.int32, **kw), torch.zeros(E, dtype=torch.int64, **kw)
    dt = torch.zeros(2, dtype=torch.int64, **kw)
    for k in range(n_launch):
        N.check(lib.mz_drqn_sample(5, k, E, L, CAP, CAP, ring.data_ptr(), mem_len.data_ptr(),
                                   ds[k].data_ptr(), dl.data_ptr(), do.data_ptr(), dt.data_ptr(),
                                   _stream()))
    s = ds.cpu().numpy()
    lens = mem_len.cpu().numpy()
    assert np.array_equal(dl.cpu().numpy(), lens[s[-1]])
    assert np.array_equal(do.cpu().numpy(), np.concatenate([[0], np.cumsum(lens[s[-1]] + 1)[:-1]]))
    assert dt.cpu().tolist() == [int((lens[s[-1]] + 1).sum()), int(lens[s[-1]].sum())]
    assert s.min() == 0 and s.max() == CAP - 1
    srt = np.sort(s, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    n = np.bincount(s.ravel(), minlength=CAP)
    exp = s.size / CAP
    # (slots of one draw are distinct, which only lowers the variance of the counts)
    assert chi2.sf(((n - exp) ** 2 / exp).sum(), CAP - 1) > 1e-6, n.tolist()
    again = torch.zeros(E, dtype=torch.int32, **kw)
    N.check(lib.mz_drqn_sample(5, 17, E, L, CAP, CAP, ring.data_ptr(), mem_len.data_ptr(),
                               again.data_ptr(), dl.data_ptr(), do.data_ptr(), dt.data_ptr(),
                               _stream()))
    assert torch.equal(again, ds[17])


# ---- sequence forward / backward ------------------------------------------------------------
class _Seq:
    """A hand-built memory and directory of E episodes (L = 8 unless given) and the three
    launches."""

    def __init__(self, lib, E, seed, lens=None, L=8):
        self.lib, self.E, self.L = lib, E, L
        L = self.L
        rng = np.random.default_rng(seed)
        self.cap = E + 2
        lens = lens or [[1, 2, 7, 3, 5][e % 5] if E > 1 else 7 for e in range(E)]
        self.src, self.tgt = _net(seed, 2.0), _net(seed + 1000, 2.0)
        self.eps = [dict(x=rng.random((n + 1, 6)).astype(np.float32),
                         a=rng.integers(0, 4, n), r=(rng.random(n) - 0.5).astype(np.float32),
                         term=bool((e + n) % 2)) for e, n in enumerate(lens)]
        slots = rng.permutation(self.cap)[:E]
        mem = rng.integers(-2 ** 31, 2 ** 31 - 1, (self.cap, L + 1, ROW)).astype(np.int32)
        mem_term = np.zeros(self.cap, np.int32)
        for ep, s in zip(self.eps, slots):
            n = len(ep["a"])
            mem[s, :n + 1, :6] = ep["x"].view(np.int32)
            mem[s, :n, 6] = ep["a"]
            mem[s, :n, 7] = ep["r"].view(np.int32)
            mem_term[s] = ep["term"]
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        self.mem, self.mem_term = d(mem), d(mem_term)
        self.lens = np.array(lens)
        self.off = np.concatenate([[0], np.cumsum(self.lens + 1)[:-1]])
        self.d_slot, self.d_len = d(slots.astype(np.int32)), d(self.lens.astype(np.int32))
        self.d_off = d(self.off.astype(np.int64))
        self.rows, self.steps = int((self.lens + 1).sum()), int(self.lens.sum())
        self.d_tot = d(np.array([self.rows, self.steps], np.int64))
        self.ps, self.pps = _dev_params(self.src)
        self.pt, self.ppt = _dev_params(self.tgt)

    def run(self, gamma=0.9):
        from mazerl import _native as N
        lib, E, L = self.lib, self.E, self.L
        R = E * (L + 1)
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        o = dict(qmax=nan(R), stash=nan(R, STASH), qa=nan(R), y=nan(R), d=nan(R),
                 ep_loss=torch.full((E + 1,), float("nan"), dtype=torch.float64, device=DEV),
                 gpart=nan(E + 1, PARAMS), loss=nan(2),
                 grads=[nan(int(np.prod(s)) + 4) for s in SHAPES])
        dirs = (self.d_slot.data_ptr(), self.d_len.data_ptr(), self.d_off.data_ptr(),
                self.d_tot.data_ptr())
        pg = (C.c_void_p * 6)(*[g.data_ptr() for g in o["grads"]])
        N.check(lib.mz_drqn_seq_forward(self.ppt, H, 1, E, L, self.cap, gamma, self.mem.data_ptr(),
                                        self.mem_term.data_ptr(), *dirs, o["qmax"].data_ptr(), None,
                                        None, None, None, None, _stream()))
        N.check(lib.mz_drqn_seq_forward(self.pps, H, 0, E, L, self.cap, gamma, self.mem.data_ptr(),
                                        self.mem_term.data_ptr(), *dirs, o["qmax"].data_ptr(),
                                        o["stash"].data_ptr(), o["qa"].data_ptr(), o["y"].data_ptr(),
                                        o["d"].data_ptr(), o["ep_loss"].data_ptr(), _stream()))
        N.check(lib.mz_drqn_seq_backward(self.pps, H, E, L, self.cap, self.mem.data_ptr(), *dirs,
                                         o["stash"].data_ptr(), o["d"].data_ptr(),
                                         o["ep_loss"].data_ptr(), o["gpart"].data_ptr(), pg,
                                         o["loss"].data_ptr(), _stream()))
        torch.cuda.synchronize()
        return o

    def single(self, e):
        """The same memory with a directory of episode e alone."""
        import copy
        one = copy.copy(self)
        n = int(self.lens[e])
        one.E, one.lens, one.off = 1, self.lens[e:e + 1], np.zeros(1, np.int64)
        one.d_slot, one.d_len = self.d_slot[e:e + 1].clone(), self.d_len[e:e + 1].clone()
        one.d_off = torch.zeros(1, dtype=torch.int64, device=DEV)
        one.d_tot = torch.tensor([n + 1, n], dtype=torch.int64, device=DEV)
        return one

    def step_rows(self):
        return np.concatenate([o + np.arange(n) for o, n in zip(self.off, self.lens)])

    def model(self, gamma=0.9):
        return M.td_loss(_f64(self.src), _f64(self.tgt), self.eps, gamma)

    def torch_ref(self, gamma=0.9):
        from mazerl.agents.lstm_dqn_agent import td_loss
        eps = [(torch.from_numpy(e["x"]), torch.from_numpy(e["a"]), torch.from_numpy(e["r"]),
                e["term"]) for e in self.eps]
        for p in self.src.parameters():
            p.grad = None
        loss = td_loss(self.src, self.tgt, eps, gamma)
        loss.backward()
        qa, y = [], []
        with torch.no_grad():
            for x, a, r, term in eps:
                n = a.shape[0]
                qa.append(self.src.unroll(x[None, :n])[0].gather(1, a[:, None]).squeeze(1).numpy())
                yy = r + np.float32(gamma) * self.tgt.unroll(x[None])[0, 1:].max(dim=1)[0]
                if term:
                    yy[n - 1] = r[n - 1]
                y.append(yy.numpy())
        return dict(qa=np.concatenate(qa), y=np.concatenate(y), loss=loss.item(),
                    grads={k: p.grad.numpy().copy() for k, p in self.src.named_parameters()})


@pytest.fixture(scope="module", params=[1, 3, 65])
def seq(request, lib):
    s = _Seq(lib, request.param, 70 + request.param)
    return s, s.run(), s.model(), s.torch_ref()


def test_seq_forward_backward_match_the_model(seq):
    s, o, m, ref = seq
    rows = s.step_rows()
    assert any(e["term"] for e in s.eps) or s.E == 1
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
        assert torch.isnan(g[n:]).all()  # nothing past the segment


def test_seq_pad_and_guard_rows_keep_their_sentinels(seq):
    s, o, _, _ = seq
    rows = s.step_rows()
    guard = np.setdiff1d(np.arange(s.E * (s.L + 1)), rows)  # each episode's row n and the pad
    for k in ("stash", "qa", "y", "d"):
        v = o[k].cpu().numpy()
        assert np.isnan(v[guard]).all() and not np.isnan(v[rows]).any(), k
    q = o["qmax"].cpu().numpy()
    assert np.isnan(q[s.rows:]).all() and not np.isnan(q[:s.rows]).any()
    assert torch.isnan(o["gpart"][s.E]).all() and not torch.isnan(o["gpart"][:s.E]).any()
    assert torch.isnan(o["ep_loss"][s.E]) and torch.isnan(o["loss"][1])


def test_seq_backward_writes_only_inside_six_separate_gradient_segments(lib):
    """The reduce after the backward writes through six segment pointers. E = 3, L = 5: six
    separately allocated tensors, each with NaN sentinels before and after its segment; the
    sentinels are still NaN afterwards and the segments hold the bits of the plain run."""
    from mazerl import _native as N
    G = 4
    s = _Seq(lib, 3, 91, lens=[1, 5, 3], L=5)
    o = s.run()
    sizes = [int(np.prod(sh)) for sh in SHAPES]
    bufs = [torch.full((G + n + G,), float("nan"), device=DEV) for n in sizes]
    pg = (C.c_void_p * 6)(*[b.data_ptr() + 4 * G for b in bufs])
    loss = torch.full((1,), float("nan"), device=DEV)
    N.check(s.lib.mz_drqn_seq_backward(
        s.pps, H, s.E, s.L, s.cap, s.mem.data_ptr(), s.d_slot.data_ptr(), s.d_len.data_ptr(),
        s.d_off.data_ptr(), s.d_tot.data_ptr(), o["stash"].data_ptr(), o["d"].data_ptr(),
        o["ep_loss"].data_ptr(), o["gpart"].data_ptr(), pg, loss.data_ptr(), _stream()))
    torch.cuda.synchronize()
    for b, g, n in zip(bufs, o["grads"], sizes):
        assert torch.isnan(b[:G]).all() and torch.isnan(b[G + n:]).all()
        assert not torch.isnan(b[G:G + n]).any() and torch.equal(b[G:G + n], g[:n])
    assert float(loss) == float(o["loss"][0])


def test_seq_two_runs_are_bit_identical(seq):
    s, o, _, _ = seq
    o2 = s.run()
    for k in ("qmax", "stash", "qa", "y", "d", "ep_loss", "gpart", "loss"):
        assert np.array_equal(o[k].cpu().numpy(), o2[k].cpu().numpy(), equal_nan=True), k
    for a, b in zip(o["grads"], o2["grads"]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def test_batch_gradient_is_the_weighted_sum_of_single_episode_gradients(lib):
    """Lengths 1, 2, 4, 1 (sum 8): every folded weight 1 / n_e and 1 / sum n is a power of two, so
    an episode's gradient in the batch is exactly its gradient run alone times n_e / sum n, and the
    batch's gradient (before any clamp) is their sum rounded once: 2 u sum_e |term_e| per element
    (the float64 sum's own rounding is far below u)."""
    s = _Seq(lib, 4, 91, lens=[1, 2, 4, 1])
    whole = s.run()
    acc = [np.zeros(int(np.prod(sh))) for sh in SHAPES]
    mag = [np.zeros(int(np.prod(sh))) for sh in SHAPES]
    for e in range(s.E):
        g = s.single(e).run()["grads"]
        for j, sh in enumerate(SHAPES):
            term = g[j].cpu().numpy()[:int(np.prod(sh))].astype(np.float64) * s.lens[e] / s.steps
            acc[j] += term
            mag[j] += np.abs(term)
    for j, sh in enumerate(SHAPES):
        got = whole["grads"][j].cpu().numpy()[:int(np.prod(sh))].astype(np.float64)
        assert np.abs(got).max() > 0
        assert (np.abs(got - acc[j]) <= 2 * U * mag[j]).all(), M.KEYS[j]
