"""The hand-built replay memory of tests/test_drqn_window_gpu.py (L = 8, E episodes in E of E + 2
slots, nets scaled by 2.0, random snapshots) as numpy arrays, with a directory of windows or of
whole episodes over it, and P such memories as one population's device buffers with the launches of
the update's two chains through the C ABI (mz_drqn_pop_*): the old one (forwards, backward) and the
one for double-Q targets and n-step returns (forwards in their second form, returns, backward).
Building a Mem and its directory needs no GPU."""
import numpy as np

import drqn_model as M
import drqn_nstep_model as NM
import drqn_window_model as W

H, ROW, STASH, PARAMS, SNAP, L = 32, 8, 192, 5252, 64, 8
NAN = float("nan")
GAMMA = 0.9


def net(seed, scale=2.0):
    import torch
    from mazerl.agents.lstm_dqn_agent import DQN
    torch.manual_seed(seed)
    n = DQN(6, 4, H, torch.device("cpu"))
    with torch.no_grad():
        for p in n.parameters():
            p.mul_(scale)
    return n


def f64(n):
    return M.as_f64({k: v.detach().numpy() for k, v in n.state_dict().items()})


def flat(n):
    return np.concatenate([p.detach().numpy().ravel() for p in n.parameters()]).astype(np.float32)


class Mem:
    def __init__(self, lens, seed, T):
        self.E, self.T = len(lens), T
        E = self.E
        rng = np.random.default_rng(seed)
        self.cap = E + 2
        self.src, self.tgt = net(seed), net(seed + 1000)
        self.eps = [dict(x=rng.random((n + 1, 6)).astype(np.float32), a=rng.integers(0, 4, n),
                         r=(rng.random(n) - 0.5).astype(np.float32), term=bool((e + n + e // 6) % 2))
                    for e, n in enumerate(lens)]
        self.slots = rng.permutation(self.cap)[:E]
        self.mem = rng.integers(-2 ** 31, 2 ** 31 - 1, (self.cap, L + 1, ROW)).astype(np.int32)
        self.mem_term, self.mem_len = np.zeros(self.cap, np.int32), np.zeros(self.cap, np.int32)
        self.NS = W.windows_in(L, T)
        self.state = (rng.random((self.cap, self.NS, SNAP)) - 0.5).astype(np.float32)
        self.state[:, 0] = np.nan
        self.lens = np.array(lens)
        self.write()

    def write(self):
        """The episodes into their slots (again, after a test changed a reward)."""
        for ep, s in zip(self.eps, self.slots):
            n = len(ep["a"])
            self.mem[s, :n + 1, :6] = ep["x"].view(np.int32)
            self.mem[s, :n, 6] = ep["a"]
            self.mem[s, :n, 7] = ep["r"].view(np.int32)
            self.mem_term[s], self.mem_len[s] = ep["term"], n

    def windows(self, js, K, stored=True):
        """Window js[e] of episode e under burn-in K: the model's spans and the window directory
        (a window owns m + 2 rows: entry, m steps, guard)."""
        self.kind, self.K, self.stored = "win", K, stored
        self.ws = [W.window_of(ep, self.T, K, j, self.state[s] if stored else None)
                   for ep, j, s in zip(self.eps, js, self.slots)]
        self.m = np.array([w["m"] for w in self.ws])
        self.dir = np.stack([self.slots, self.lens, [w["b"] for w in self.ws],
                             [w["k"] for w in self.ws], self.m]).astype(np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.m + 2)[:-1]]).astype(np.int64)
        self.row0 = self.off + 1
        self.tot = np.array([(self.m + 2).sum(), self.m.sum()], np.int64)
        self.rows_cap = self.E * (min(self.T, L) + 2)
        return self

    def episodes(self):
        """Whole episodes from zero state: the spans and the episode directory (n + 1 rows each)."""
        self.kind, self.K, self.stored = "seq", 0, False
        self.ws = [NM.episode_span(ep) for ep in self.eps]
        self.m = self.lens.copy()
        self.dir = np.stack([self.slots, self.lens]).astype(np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.m + 1)[:-1]]).astype(np.int64)
        self.row0 = self.off.copy()
        self.tot = np.array([(self.m + 1).sum(), self.m.sum()], np.int64)
        self.rows_cap = self.E * (L + 1)
        return self

    @property
    def steps(self):
        return int(self.m.sum())

    def step_rows(self):
        return np.concatenate([o + np.arange(m) for o, m in zip(self.row0, self.m)])

    def all_rows(self):
        """Rows row .. row + m of every span: the training steps and the step after."""
        return np.concatenate([o + np.arange(m + 1) for o, m in zip(self.row0, self.m)])


class Pop:
    """P memories with the same E, T and kind of directory as one population on the device."""

    def __init__(self, lib, mems, dev="cuda"):
        import torch
        self.lib, self.mems, self.P, self.dev = lib, mems, len(mems), dev
        m0 = mems[0]
        self.E, self.T, self.cap, self.kind, self.R = m0.E, m0.T, m0.cap, m0.kind, m0.rows_cap
        assert all((m.E, m.T, m.kind) == (m0.E, m0.T, m0.kind) for m in mems)
        self.Kmax = max(m.K for m in mems)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        st = lambda k: d(np.stack([getattr(m, k) for m in mems]))  # noqa: E731
        self.src = d(np.stack([flat(m.src) for m in mems]))
        self.tgt = d(np.stack([flat(m.tgt) for m in mems]))
        self.mem, self.mem_term, self.state = st("mem"), st("mem_term"), st("state")
        self.dir, self.off, self.tot = st("dir"), st("off"), st("tot")
        self.gamma = d(np.full(self.P, GAMMA, np.float32))
        self.burn = d(np.array([m.K for m in mems], np.int32))
        self.stored = d(np.array([int(m.stored) for m in mems], np.int32))
        self.d = d

    def buffers(self):
        import torch
        P, E, R = self.P, self.E, self.R
        nan = lambda *s, dtype=torch.float32: torch.full(s, NAN, dtype=dtype, device=self.dev)  # noqa: E731
        return dict(qmax=nan(P, R), q4=nan(P, R, 4), stash=nan(P, R, STASH), qa=nan(P, R), y=nan(P, R),
                    d=nan(P, R), sel=torch.full((P, R), -7, dtype=torch.int32, device=self.dev),
                    ep_loss=nan(P, E, dtype=torch.float64),
                    gpart=nan(P, E, PARAMS), grads=nan(P, PARAMS), loss=nan(P))

    def _st(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def _dirs(self):
        """The window directory as the entry points take it: wdir [P][5][E], win_off, win_tot."""
        return (self.dir.data_ptr(), self.off.data_ptr(), self.tot.data_ptr())

    def _due(self, due):
        return None if due is None else self.d(np.array(due, np.int32))

    def forward_old(self, o, due=None):
        from mazerl import _native as N
        dv = self._due(due)
        rows = [o[k].data_ptr() for k in ("stash", "qa", "y", "d", "ep_loss")]
        for net_, target, out in ((self.tgt, 1, [None] * 5), (self.src, 0, rows)):
            if self.kind == "win":
                N.check(self.lib.mz_drqn_pop_window_forward(
                    net_.data_ptr(), H, target, self.P, self.E, L, self.T, self.Kmax, self.cap,
                    self.gamma.data_ptr(), self.burn.data_ptr(), self.stored.data_ptr(),
                    None if dv is None else dv.data_ptr(), self.mem.data_ptr(),
                    self.mem_term.data_ptr(), self.state.data_ptr(), *self._dirs(),
                    o["qmax"].data_ptr(), *out, self._st()))
            else:
                N.check(self.lib.mz_drqn_pop_seq_forward(
                    net_.data_ptr(), H, target, self.P, self.E, L, self.cap, self.gamma.data_ptr(),
                    None if dv is None else dv.data_ptr(), self.mem.data_ptr(),
                    self.mem_term.data_ptr(), *self._seq_dirs(), o["qmax"].data_ptr(), *out,
                    self._st()))

    def _seq_dirs(self):
        """The episode directory as the entry points take it: d_slot [P][E], d_len [P][E] (their
        own contiguous arrays), d_off, d_tot."""
        if not hasattr(self, "_sd"):
            self._sd = (self.dir[:, 0].contiguous(), self.dir[:, 1].contiguous())
        return (self._sd[0].data_ptr(), self._sd[1].data_ptr(), self.off.data_ptr(),
                self.tot.data_ptr())

    def forward_q(self, o, due=None):
        from mazerl import _native as N
        dv = self._due(due)
        dp = None if dv is None else dv.data_ptr()
        out = (o["q4"].data_ptr(), o["stash"].data_ptr(), o["qa"].data_ptr(), o["sel"].data_ptr(),
               self._st())
        for net_, target in ((self.tgt, 1), (self.src, 0)):
            if self.kind == "win":
                N.check(self.lib.mz_drqn_pop_window_forward_q(
                    net_.data_ptr(), H, target, self.P, self.E, L, self.T, self.Kmax, self.cap,
                    self.burn.data_ptr(), self.stored.data_ptr(), dp, self.mem.data_ptr(),
                    self.state.data_ptr(), *self._dirs(), *out))
            else:
                N.check(self.lib.mz_drqn_pop_seq_forward_q(
                    net_.data_ptr(), H, target, self.P, self.E, L, self.cap, dp,
                    self.mem.data_ptr(), *self._seq_dirs(), *out))

    def returns(self, o, n_step, double=None, sel=True, due=None):
        """n_step: P ints; double: P flags or None (no array); sel False: no argmax rows."""
        from mazerl import _native as N
        dv = self._due(due)
        dp = None if dv is None else dv.data_ptr()
        ns = self.d(np.array(n_step, np.int32))
        db = None if double is None else self.d(np.array(double, np.int32))
        head = (ns.data_ptr(), int(max(n_step)), None if db is None else db.data_ptr(),
                self.gamma.data_ptr())
        tail = (o["qa"].data_ptr(), o["q4"].data_ptr(), o["sel"].data_ptr() if sel else None,
                o["y"].data_ptr(), o["d"].data_ptr(), o["ep_loss"].data_ptr(), self._st())
        if self.kind == "win":
            N.check(self.lib.mz_drqn_pop_window_returns(
                *head, self.burn.data_ptr(), dp, self.P, self.E, L, self.T, self.Kmax, self.cap,
                self.mem.data_ptr(), self.mem_term.data_ptr(), *self._dirs(), *tail))
        else:
            N.check(self.lib.mz_drqn_pop_seq_returns(
                *head, dp, self.P, self.E, L, self.cap, self.mem.data_ptr(),
                self.mem_term.data_ptr(), *self._seq_dirs(), *tail))

    def backward(self, o, due=None):
        from mazerl import _native as N
        dv = self._due(due)
        dp = None if dv is None else dv.data_ptr()
        back = (o["stash"].data_ptr(), o["d"].data_ptr(), o["ep_loss"].data_ptr(),
                o["gpart"].data_ptr(), o["grads"].data_ptr(), o["loss"].data_ptr(), self._st())
        if self.kind == "win":
            N.check(self.lib.mz_drqn_pop_window_backward(
                self.src.data_ptr(), H, self.P, self.E, L, self.T, self.Kmax, self.cap,
                self.burn.data_ptr(), dp, self.mem.data_ptr(), *self._dirs(), *back))
        else:
            N.check(self.lib.mz_drqn_pop_seq_backward(
                self.src.data_ptr(), H, self.P, self.E, L, self.cap, dp, self.mem.data_ptr(),
                *self._seq_dirs(), *back))
