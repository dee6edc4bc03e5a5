"""The recurrent DQN's kernels at P > 1 learners (csrc/mz_drqn.hip through the mz_drqn_pop_* entry
points, csrc/mz_optim.hip k_adamw_pop) through the C ABI.

The single-learner entry points are pinned to the float64 model by tests/test_drqn_gpu.py, so they
are the yardstick here: learner p of a population call must give the bits the single-learner call
gives on learner p's slice, `==` and no tolerance. One test holds the population chain to the
float64 model (tests/drqn_model.py) directly, with test_drqn_gpu.py's bound
    e_k <= 4 e_ref + 8 u max|tensor|,  u = 2^-24,
e_ref from torch's float32 CPU LSTMCell + Linear + autograd. Shapes: 9x9-sized records, L = 8."""
import ctypes as C

import numpy as np
import pytest
import torch

import drqn_model as M
import learner_model as LM

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
H, ROW, STASH, PARAMS, L = 32, 8, 192, 5252, 8
SHAPES = [(128, 6), (128, 32), (128,), (128,), (4, 32), (4,)]
OFFS = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in SHAPES])])
ADAM = (0.9, 0.999, 1e-8, 1e-2)


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


def _rows(seeds):
    return _d(np.stack([_row(_net(s)) for s in seeds]))


# ---- 1. act -----------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [5, 16, 21])
@pytest.mark.parametrize("Lr", [L, 0])
def test_act_equals_the_single_learner_act_on_each_slice(lib, b, Lr):
    from mazerl import _native as N
    P, B = 3, 3 * b
    rng = np.random.default_rng(100 + b)
    params = _rows([31, 32, 33])
    eps = [0.0, 1.0, 0.5]
    seeds = [11, 2 ** 63 + 5, 7]
    counter = 3
    tv = np.array([0, 3, L, -1, 5, 100, 0, 7, L - 1, -2 ** 31, 1])[np.arange(B) % 11].astype(np.int32)
    x = rng.random((B, 6)).astype(np.float32)
    h0 = (rng.random((H, B)) - 0.5).astype(np.float32)
    c0 = (rng.random((H, B)) - 0.5).astype(np.float32)
    nan = float("nan")

    def fresh(n):
        return (torch.full((n, Lr + 1, 6), nan, device=DEV), torch.full((n, max(Lr, 1)), -7,
                dtype=torch.int32, device=DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV),
                torch.full((n, 4), nan, device=DEV))

    obs6, t, h, c = _d(x), _d(tv), _d(h0), _d(c0)
    rec_x, rec_a, out, q = fresh(B)
    eps_d = _d(np.array(eps, np.float32))
    seed_d = _d(np.array([_signed(s) for s in seeds], np.int64))
    N.check(lib.mz_drqn_pop_act(
        params.data_ptr(), H, P, b, obs6.data_ptr(), Lr, eps_d.data_ptr(),
        4, seed_d.data_ptr(), counter, t.data_ptr(),
        h.data_ptr(), c.data_ptr(), rec_x.data_ptr() if Lr else None,
        rec_a.data_ptr() if Lr else None, out.data_ptr(), q.data_ptr(), _stream()))
    explored = 0
    for p in range(P):
        s = slice(p * b, (p + 1) * b)
        hs, cs = _d(h0[:, s]), _d(c0[:, s])
        rx, ra, o1, q1 = fresh(b)
        xs, ts = _d(x[s]), _d(tv[s])
        N.check(lib.mz_drqn_act(
            _ptrs(params[p]), H, xs.data_ptr(), b, Lr, eps[p], 4, seeds[p], counter,
            ts.data_ptr(), hs.data_ptr(), cs.data_ptr(), rx.data_ptr() if Lr else None,
            ra.data_ptr() if Lr else None, o1.data_ptr(), q1.data_ptr(), _stream()))
        assert _eq(h[:, s], hs) and _eq(c[:, s], cs), p
        assert _eq(rec_x[s], rx) and _eq(rec_a[s], ra), p
        assert _eq(out[s], o1) and _eq(q[s], q1), p
        assert int(o1.min()) >= 0
        explored += int((o1 != q1.argmax(dim=1)).sum())
    assert explored > 0 or b < 16  # eps = 1 explores: the draws are the single learner's
    if Lr:  # some instance recorded, some did not
        assert not torch.isnan(rec_x).all() and torch.isnan(rec_x).any()


# ---- 2. store ---------------------------------------------------------------------------------
def test_store_equals_per_learner_stores_on_the_sublists(lib):
    """P = 3, capacity 4, b = 6: learner 0 has no finished episode, learner 1 two, learner 2 six
    (more than its slots) with its head at 3, so its ring wraps."""
    from mazerl import _native as N
    P, b, CAP = 3, 6, 4
    B = P * b
    rng = np.random.default_rng(7)
    fin_id = np.array([7, 10, 12, 13, 14, 15, 16, 17] + [0] * (B - 8), np.int32)
    fin_len = np.array([3, 8, 2, 5, 8, 1 + 1, 7, 4] + [0] * (B - 8), np.int32)
    runs = [(0, 0), (0, 2), (2, 8)]
    obs6 = _d(rng.random((B, 6)).astype(np.float32))
    term = _d((rng.random(B) < 0.5).astype(np.uint8))
    rec_x0 = rng.random((B, L + 1, 6)).astype(np.float32)
    rec_a = _d(rng.integers(0, 4, (B, L)).astype(np.int32))
    rec_r = _d(rng.random((B, L)))
    mem0 = rng.integers(-2 ** 31, 2 ** 31 - 1, (P, CAP, L + 1, ROW)).astype(np.int32)
    len0 = rng.integers(1, L + 1, (P, CAP)).astype(np.int32)
    term0 = rng.integers(0, 2, (P, CAP)).astype(np.int32)
    ring0 = np.array([[2, 3], [1, 1], [3, 4]], np.int64)
    rec_x, mem, mem_len, mem_term, ring = (_d(a) for a in (rec_x0, mem0, len0, term0, ring0))
    ids_d, lens_d, cnt_d = _d(fin_id), _d(fin_len), _d(np.array([8], np.int32))
    N.check(lib.mz_drqn_pop_store(
        obs6.data_ptr(), term.data_ptr(), P, b, L, ids_d.data_ptr(), lens_d.data_ptr(),
        cnt_d.data_ptr(), rec_x.data_ptr(), rec_a.data_ptr(),
        rec_r.data_ptr(), CAP, mem.data_ptr(), mem_len.data_ptr(), mem_term.data_ptr(),
        ring.data_ptr(), _stream()))
    rx1 = _d(rec_x0)
    for p, (lo, hi) in enumerate(runs):
        m1, l1, t1, r1 = (_d(a[p]) for a in (mem0, len0, term0, ring0))
        ids, lens = np.zeros(B, np.int32), np.zeros(B, np.int32)
        ids[:hi - lo], lens[:hi - lo] = fin_id[lo:hi], fin_len[lo:hi]
        ids_1, lens_1, cnt_1 = _d(ids), _d(lens), _d(np.array([hi - lo], np.int32))
        N.check(lib.mz_drqn_store(
            obs6.data_ptr(), term.data_ptr(), B, L, ids_1.data_ptr(), lens_1.data_ptr(),
            cnt_1.data_ptr(), rx1.data_ptr(), rec_a.data_ptr(),
            rec_r.data_ptr(), CAP, m1.data_ptr(), l1.data_ptr(), t1.data_ptr(), r1.data_ptr(),
            _stream()))
        assert _eq(mem[p], m1) and _eq(mem_len[p], l1) and _eq(mem_term[p], t1), p
        assert _eq(ring[p], r1), p
    assert _eq(rec_x, rx1)
    # the learner without a finished episode: ring and memory keep their bits
    assert _eq(mem[0], _d(mem0[0])) and _eq(ring[0], _d(ring0[0]))
    assert _eq(mem_len[0], _d(len0[0])) and _eq(mem_term[0], _d(term0[0]))
    assert ring.cpu().tolist() == [[2, 3], [3, 3], [1, 4]]
    # learner 2 kept its last four episodes: slot (3 + k) mod 4 holds episode k = 2 .. 5
    assert mem_len[2].cpu().tolist() == [int(fin_len[2 + k]) for k in (5, 2, 3, 4)]


# ---- 3. / 4. the update chain --------------------------------------------------------------
class _Pop:
    """Hand-built rings of P learners (capacity 6, every slot a valid episode) and the state of
    one update: distinct nets, moments, step counts, seeds and update counts."""

    def __init__(self, P, E, seed):
        self.P, self.E, self.cap = P, E, 6
        rng = np.random.default_rng(seed)
        cap = self.cap
        mem = rng.integers(-2 ** 31, 2 ** 31 - 1, (P, cap, L + 1, ROW)).astype(np.int32)
        self.lens = rng.integers(1, L + 1, (P, cap)).astype(np.int32)
        self.lens[:, 0], self.lens[:, 1] = 1, L
        self.term = rng.integers(0, 2, (P, cap)).astype(np.int32)
        for p in range(P):
            for s in range(cap):
                n = int(self.lens[p, s])
                mem[p, s, :n + 1, :6] = rng.random((n + 1, 6)).astype(np.float32).view(np.int32)
                mem[p, s, :n, 6] = rng.integers(0, 4, n)
                mem[p, s, :n, 7] = (rng.random(n) - 0.5).astype(np.float32).view(np.int32)
        self.mem = mem
        self.ring = np.array([[3, 6], [0, 5], [4, 4]][:P], np.int64)
        self.src = np.stack([_row(_net(seed + 10 + p)) for p in range(P)])
        self.tgt = np.stack([_row(_net(seed + 20 + p)) for p in range(P)])
        self.m = ((rng.random((P, PARAMS)) - 0.5) * 2e-2).astype(np.float32)
        self.v = (rng.random((P, PARAMS)) * 1e-3 + 1e-6).astype(np.float32)
        self.step = np.array([5, 9, 12][:P], np.float32)
        self.seeds = [41, 2 ** 63 + 42, 43][:P]
        self.counts = [5, 9, 12][:P]
        self.gamma = np.array([0.9, 0.8, 0.95][:P], np.float32)
        self.lr = np.array([1e-3, 5e-4, 2e-3][:P], np.float32)

    def buffers(self, n):
        """Sentinel-filled outputs of an update for n learners."""
        E, R = self.E, self.E * (L + 1)
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        i32 = lambda *s: torch.full(s, -9, dtype=torch.int32, device=DEV)  # noqa: E731
        return dict(d_slot=i32(n, E), d_len=i32(n, E),
                    d_off=torch.full((n, E), -9, dtype=torch.int64, device=DEV),
                    d_tot=torch.full((n, 2), -9, dtype=torch.int64, device=DEV),
                    qmax=nan(n, R), stash=nan(n, R, STASH), qa=nan(n, R), y=nan(n, R), d=nan(n, R),
                    ep_loss=torch.full((n, E), float("nan"), dtype=torch.float64, device=DEV),
                    gpart=nan(n, E, PARAMS), grad=nan(n, PARAMS), loss=nan(n))

    def run_pop(self, lib, due, write_grad=1):
        from mazerl import _native as N
        P, E, cap = self.P, self.E, self.cap
        o = self.buffers(P)
        o.update(src=_d(self.src), tgt=_d(self.tgt), m=_d(self.m), v=_d(self.v), step=_d(self.step))
        mem, term, lens, ring = _d(self.mem), _d(self.term), _d(self.lens), _d(self.ring)
        due_d = _d(np.array(due, np.int32))
        seeds = _d(np.array([_signed(s) for s in self.seeds], np.int64))
        counts = _d(np.array(self.counts, np.int64))
        gam, lr = _d(self.gamma), _d(self.lr)
        dirs = tuple(o[k].data_ptr() for k in ("d_slot", "d_len", "d_off", "d_tot"))
        st = _stream()
        filled = min(int(self.ring[p, 1]) for p in range(P) if due[p])
        N.check(lib.mz_drqn_pop_sample(seeds.data_ptr(), counts.data_ptr(), due_d.data_ptr(), P, E,
                                       L, cap, filled, ring.data_ptr(), lens.data_ptr(), *dirs, st))
        N.check(lib.mz_drqn_pop_seq_forward(
            o["tgt"].data_ptr(), H, 1, P, E, L, cap, None, due_d.data_ptr(), mem.data_ptr(),
            term.data_ptr(), *dirs, o["qmax"].data_ptr(), None, None, None, None, None, st))
        N.check(lib.mz_drqn_pop_seq_forward(
            o["src"].data_ptr(), H, 0, P, E, L, cap, gam.data_ptr(), due_d.data_ptr(),
            mem.data_ptr(), term.data_ptr(), *dirs, o["qmax"].data_ptr(), o["stash"].data_ptr(),
            o["qa"].data_ptr(), o["y"].data_ptr(), o["d"].data_ptr(), o["ep_loss"].data_ptr(), st))
        N.check(lib.mz_drqn_pop_seq_backward(
            o["src"].data_ptr(), H, P, E, L, cap, due_d.data_ptr(), mem.data_ptr(), *dirs,
            o["stash"].data_ptr(), o["d"].data_ptr(), o["ep_loss"].data_ptr(),
            o["gpart"].data_ptr(), o["grad"].data_ptr(), o["loss"].data_ptr(), st))
        N.check(lib.mz_adamw_pop(
            o["src"].data_ptr(), o["m"].data_ptr(), o["v"].data_ptr(), o["grad"].data_ptr(), P,
            PARAMS, lr.data_ptr(), o["step"].data_ptr(), due_d.data_ptr(), *ADAM, 1.0, 1.0,
            write_grad, st))
        torch.cuda.synchronize()
        return o

    def run_single(self, lib, p):
        """The single-learner chain on learner p's ring."""
        from mazerl import _native as N
        E, cap = self.E, self.cap
        o = self.buffers(1)
        o.update(src=_d(self.src[p:p + 1]), tgt=_d(self.tgt[p:p + 1]), m=_d(self.m[p:p + 1]),
                 v=_d(self.v[p:p + 1]), step=_d(self.step[p:p + 1]))
        mem, term, lens, ring = (_d(a[p]) for a in (self.mem, self.term, self.lens, self.ring))
        lr = _d(self.lr[p:p + 1])
        dirs = tuple(o[k].data_ptr() for k in ("d_slot", "d_len", "d_off", "d_tot"))
        ps, pt, pg = _ptrs(o["src"][0]), _ptrs(o["tgt"][0]), _ptrs(o["grad"][0])
        gamma, st = float(self.gamma[p]), _stream()
        N.check(lib.mz_drqn_sample(self.seeds[p], self.counts[p], E, L, cap, int(self.ring[p, 1]),
                                   ring.data_ptr(), lens.data_ptr(), *dirs, st))
        N.check(lib.mz_drqn_seq_forward(pt, H, 1, E, L, cap, gamma, mem.data_ptr(), term.data_ptr(),
                                        *dirs, o["qmax"].data_ptr(), None, None, None, None, None,
                                        st))
        N.check(lib.mz_drqn_seq_forward(ps, H, 0, E, L, cap, gamma, mem.data_ptr(), term.data_ptr(),
                                        *dirs, o["qmax"].data_ptr(), o["stash"].data_ptr(),
                                        o["qa"].data_ptr(), o["y"].data_ptr(), o["d"].data_ptr(),
                                        o["ep_loss"].data_ptr(), st))
        N.check(lib.mz_drqn_seq_backward(ps, H, E, L, cap, mem.data_ptr(), *dirs,
                                         o["stash"].data_ptr(), o["d"].data_ptr(),
                                         o["ep_loss"].data_ptr(), o["gpart"].data_ptr(), pg,
                                         o["loss"].data_ptr(), st))
        N.check(lib.mz_adamw_flat(
            o["src"].data_ptr(), o["m"].data_ptr(), o["v"].data_ptr(),
            (C.c_void_p * 1)(o["grad"].data_ptr()), (C.c_int64 * 1)(PARAMS), 1, lr.data_ptr(),
            o["step"].data_ptr(), *ADAM, 1.0, 1.0, 1, st))
        torch.cuda.synchronize()
        return o


KEYS_OUT = ("d_slot", "d_len", "d_off", "d_tot", "qmax", "stash", "qa", "y", "d", "ep_loss",
            "gpart", "grad", "loss", "src", "m", "v", "step")


@pytest.mark.parametrize("E", [1, 3])
def test_update_chain_equals_the_single_learner_chain_and_skips_learners_not_due(lib, E):
    pop = _Pop(3, E, 300 + E)
    due = (1, 0, 1)
    o = pop.run_pop(lib, due)
    for p in (0, 2):
        one = pop.run_single(lib, p)
        for k in KEYS_OUT:
            assert _eq(o[k][p], one[k][0]), (p, k)
        assert float(o["step"][p]) == pop.step[p] + 1
        assert not torch.isnan(o["grad"][p]).any() and float(o["grad"][p].abs().max()) <= 1.0
        assert not _eq(o["src"][p], _d(pop.src[p]))
    # the learner that is not due: every bit of its state and of its sentinels is still there
    start = pop.buffers(1)
    start.update(src=_d(pop.src[1:2]), m=_d(pop.m[1:2]), v=_d(pop.v[1:2]), step=_d(pop.step[1:2]))
    for k in KEYS_OUT:
        assert _eq(o[k][1], start[k][0]), k
    assert _eq(o["tgt"], _d(pop.tgt))


def test_target_sync_copies_the_flagged_rows_only(lib):
    from mazerl import _native as N
    pop = _Pop(3, 1, 77)
    src, tgt = _d(pop.src), _d(pop.tgt)
    mask = _d(np.array([0, 1, 1], np.int32))
    N.check(lib.mz_drqn_pop_sync(src.data_ptr(), tgt.data_ptr(), mask.data_ptr(), 3, _stream()))
    assert _eq(tgt[0], _d(pop.tgt[0])) and _eq(tgt[1], src[1]) and _eq(tgt[2], src[2])
    assert _eq(src, _d(pop.src)) and not _eq(tgt[0], src[0])


def _check(name, got, model, ref):
    got, model, ref = (np.asarray(a, np.float64) for a in (got, model, ref))
    mx = np.abs(model).max()
    e_k, e_ref = np.abs(got - model).max(), np.abs(ref - model).max()
    print(f"{name}: e_k {e_k:.3e} e_ref {e_ref:.3e} ratio {e_k / (e_ref + 2 * U * mx + 1e-300):.2f}")
    assert e_k <= 4 * e_ref + 8 * U * mx, (name, e_k, e_ref, mx)


def test_population_gradient_and_step_match_the_float64_model(lib):
    """P = 2, E = 3: each learner's gradient (before the clamp) and its parameters after the AdamW
    step against tests/drqn_model.py + learner_model.adamw_step on the episodes its directory
    names, with torch's float32 CPU autograd as the reference error."""
    from mazerl.agents.lstm_dqn_agent import DQN, td_loss
    pop = _Pop(2, 3, 500)
    o = pop.run_pop(lib, (1, 1), write_grad=0)
    for p in range(2):
        slots, lens = o["d_slot"][p].cpu().numpy(), o["d_len"][p].cpu().numpy()
        assert len(set(slots.tolist())) == 3 and (lens == pop.lens[p][slots]).all()
        eps = [dict(x=pop.mem[p, s, :n + 1, :6].view(np.float32).copy(),
                    a=pop.mem[p, s, :n, 6].astype(np.int64),
                    r=pop.mem[p, s, :n, 7].view(np.float32).copy(), term=bool(pop.term[p, s]))
               for s, n in zip(slots, lens)]
        sd = lambda row: {k: torch.from_numpy(row[OFFS[j]:OFFS[j + 1]].reshape(SHAPES[j]).copy())  # noqa: E731
                          for j, k in enumerate(M.KEYS)}
        gamma = float(pop.gamma[p])
        out = M.td_loss(M.as_f64({k: v.numpy() for k, v in sd(pop.src[p]).items()}),
                        M.as_f64({k: v.numpy() for k, v in sd(pop.tgt[p]).items()}), eps, gamma)
        ns, nt = DQN(6, 4, H, torch.device("cpu")), DQN(6, 4, H, torch.device("cpu"))
        ns.load_state_dict(sd(pop.src[p])), nt.load_state_dict(sd(pop.tgt[p]))
        loss = td_loss(ns, nt, [(torch.from_numpy(e["x"]), torch.from_numpy(e["a"]),
                                 torch.from_numpy(e["r"]), e["term"]) for e in eps], gamma)
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
