"""Vectorised recurrent DQN — the reference's LSTM agent (agents/lstm_dqn_agent.py: an
nn.LSTMCell(6, 32) + nn.Linear(32, 4) Q-network over obs6, whole episodes in
SequentialExperienceReplayMemory, lib/replay_memory.py:26-43) over B instances at once, on plain
(enrich=False) or Enrich envs, euclidean or toroidal. Only obs6 is read.

Per vector step, with no device-to-host read once the memory holds a batch (csrc/mz_drqn.hip; every
launch but the snapshot is a population entry point, mz_drqn_pop_*, with P = 1; the host sends
eps per step and a block of scalars per update, two small host-to-device copies):
  act      mz_drqn_pop_act: the cell and the head from each instance's (h, c) ([32][B] in HBM), the
           eps-greedy draw, the record of (x_t, a_t) at t[i];
  step     the env step;
  scan     mz_ppo_scan, unchanged (the f32 reward widened to its float64 record; t[i] += 1; the
           finished episodes' list in instance order). It drops 1-step episodes, so none reaches
           the memory;
  store    mz_drqn_pop_store: x_n and each finished episode into ring slot (head + k) mod capacity;
  reset    winners get new mazes, truncated instances restart theirs (schedule.py as REINFORCE);
  update   when due: mz_drqn_pop_sample (E distinct slots + the batch directory), the target net's
           sequence forward (max_a Q'_t), the source net's (Q_t[a_t], y_t, residuals, the stash),
           mz_drqn_pop_seq_backward (BPTT, gradients reduced in a fixed order into the flat gradient
           segments), then FlatAdamW (the reference's clamp_(-1, 1) + AdamW in one launch).
With window=T the update trains on one window of T steps per sampled episode (departures 7-9):
mz_drqn_snapshot runs before act, mz_drqn_pop_snap_store before store, and the update is
mz_drqn_pop_window_sample / _forward / _backward; its row buffers hold E (T + 2) rows whatever the
maze size and the burn-in are. With window=None (the default) none of these is launched.

The reference defines the net, the gate order, eps = final + (start - final) exp(-steps / decay),
episodes as the unit of replay sampled without replacement, the MSE loss, the clamp, AdamW at
torch's defaults, CosineAnnealingLR(T_max=30, eta_min=1e-6), the target sync by load_state_dict
and update_steps_done; all kept. It leaves the agent unfinished (no trainer drives it,
optimize_model zips episodes as transitions, get_action explores over randrange(2), the hidden
state is resized to the batch and never restored). Six departures fix the semantics:
  1. acting state: each instance carries (h, c), zero at the first step of every episode,
     advanced once per env step with the parameters of that moment;
  2. exploration: with probability eps a uniform action over `explore_actions` (default 4, the
     env's action_space.n; 2 reproduces the reference's leftover);
  3. eps clock: one step count per population, +1 per vector step (every instance has made that
     many get_action calls); update_steps_done() halves it;
  4. episode record: x_0 .. x_n (x_n: the observation after the last step), a_0 .. a_{n-1},
     r_0 .. r_{n-1} (float32 of the env's reward), terminated; records are L + 1 rows,
     L = episode_bound;
  5. loss: over E sampled episodes, source unrolled from zero state over x_0 .. x_{n-1}, target
     over x_0 .. x_n; y_t = r_t + gamma max_a Q'_{t+1}[a], y_{n-1} = r_{n-1} when terminated (a
     truncated last step bootstraps from x_n); loss = mean over all sum n steps of
     (Q_t[a_t] - y_t)^2; no gradient through y;
  6. cadence: one update per `train_every` vector steps once the memory holds >= batch_size
     episodes; target sync every `target_update_frequency` updates; the cosine schedule advances
     once per update.
Replay windows, stored recurrent state and burn-in (R2D2's way to train from replay) are the
option window=T, burn_in=K, initial_state="stored" | "zero"; window=None is the trainer above:
  7. state snapshots: the (h, c) an instance holds before it acts at episode step t = j T, j >= 1,
     is kept with the episode as snapshot j (64 f32); snapshot 0 is zero by definition. An episode
     of n steps has windows j = 0 .. ceil(n / T) - 1. The snapshots are the acting kernel's own
     values, computed with the parameters of that moment: they go stale as the net trains, which
     is what the burn-in is for. With initial_state="zero" none is recorded or stored;
  8. the unit of a batch: the memory stays the ring of whole episodes. A batch is E distinct
     episodes chosen with exactly mz_drqn_pop_sample's draws for the same (seed, update count), then
     one window j per chosen episode, uniform over its ceil(n / T) windows, from a Philox stream of
     its own keyed by (seed, update count, position in the batch). Windows are therefore uniform
     within an episode, not over the memory: a step of a short episode is trained on more often;
  9. the loss of a window: s = j T, m = min(T, n - s) training steps, b = max(0, s - K), k = s - b
     burn-in steps. Both nets start at step b from the same state (snapshot b / T when "stored",
     zero when "zero" or b = 0); the source unrolls x_b .. x_{s+m-1}, the target x_b .. x_{s+m},
     each with its own parameters. The burn-in steps carry no loss term and no gradient flows into
     them or through the state that enters step s. y_t = r_t + gamma max_a Q'_{t+1}[a] for the
     training steps, r_t alone only at t = n - 1 of a terminated episode (a window that ends
     before the episode does bootstraps from x_{s+m}); loss = sum (Q_t[a_t] - y_t)^2 / sum m.
K must be a multiple of T. Overlapping windows (a stride other than T) are out of scope.
Prioritized windows (the other half of R2D2's replay) are the option priority_alpha=a with
window=T (priority_beta, priority_eta, priority_eps beside it; R2D2's values are 0.9, 0.6, 0.9);
priority_alpha=None is the trainer above, and then nothing below is allocated or launched. Every
window (slot, j) of the ring carries a mass: an unsigned 32-bit fixed-point priority with 20
fractional bits, 0 = no such window. Masses are integers on purpose: every sum over them is exact
in 64 bits, so the sampler does not depend on a reduction's order and equals a host model bit for
bit (tests/drqn_prio_model.py). With W = ceil(L / T):
 10. entry: a stored episode of n steps gives its ceil(n / T) windows the mass prio_max, the
     largest mass any update has written so far (2^20, priority 1, at the start); the slot's other
     entries are 0 and its sum psum[slot] = ceil(n / T) prio_max. mz_drqn_pop_prio_store follows
     mz_drqn_pop_store's slot rule and validity tests and runs before it, as
     mz_drqn_pop_snap_store does;
 11. sampling, in departure 8's place: with replacement and stratified, in integers. S = the sum
     of psum over the slots; batch position e draws t = lo + mulhi64(r, hi - lo), lo =
     floor(e S / E), hi = floor((e + 1) S / E), r a 64-bit word of a Philox stream of its own keyed
     by (seed, update count, e), and takes the window (slot, j) with prefix <= t < prefix + mass,
     the prefix running slot-major, j-minor. Two positions may hold the same window. b, k, m and
     the directory follow from j as in 8-9. A window's share deviates from mass / S by at most
     E / S. Its importance weight is w_e = (float) (M_min / M_e)^beta, M_e its mass when sampled
     and M_min the batch's smallest: (N P)^-beta / max, in which N and S cancel. With alpha = 0
     every window has mass 2^20: sampling is uniform over the memory's windows, without departure
     8's bias towards short episodes;
 12. after the source forward, before the backward: with a_i = |Q_i[a_i] - y_i| (float32) over the
     window's m training steps, pr = eta max a_i + (1 - eta) mean a_i (float64, the mean summed in
     time order), mass = clamp(llrint((pr + eps)^alpha 2^20), 1, 2^30) goes to (slot, j), prio_max
     becomes the maximum of itself and the batch's masses, and every touched slot's psum is
     recomputed from its W entries. Then the residuals d and the window's loss term are scaled by
     w_e, so the unchanged backward gives the gradient and value of loss = sum_e w_e sum_t
     (Q_t[a_t] - y_t)^2 / sum m.
Double-Q targets and n-step returns (R2D2's remaining pieces; the feed-forward DDQN's estimator)
are the options double_q=True and n_step=N, with whole episodes or windows, uniform or prioritized.
double_q=False, n_step=1 is the trainer above: nothing below is allocated or launched. A span is
what one wave unrolls: training steps s .. s + m - 1 of an n-step episode (a whole episode: s = 0,
m = n; a window: s = j T, m = min(T, n - s), after its burn-in). Off the defaults the target net
writes all four Q'_u of the span's steps s .. s + m, the source net its stash and Q_t[a_t] as
before, and mz_drqn_pop_seq_returns / mz_drqn_pop_window_returns forms y, d and the loss terms
between the source forward and the priority update (which then reads the new y) or the backward:
 13. double_q: the bootstrap value at step u is Q'_u[a*_u], a*_u = argmax_a Q_u[a] with the source
     net's Q at the update's own parameters; the first maximum in action order, 0 for a NaN row (the
     acting kernel's rule). For that the source net unrolls one step further than above, x_{s+m},
     continuing from its own state; the extra step has no stash row, no loss term and no gradient,
     and the selection is a constant of the loss. Both nets still start at step b from the same
     state (9);
 14. n_step = N: for training step t of a span, k = min(N, s + m - t) and u = t + k: the return is
     cut at the span's end, no reward past a window's end is read and only the guard row's Q' is
     used there. boot = Q'_u[a*_u] when double, else max_a Q'_u[a]; no bootstrap where u = n and
     the episode terminated (a truncated one bootstraps from x_n as above). In float32, in this
     order: acc = r_{u-1} without bootstrap, else fmaf(gamma, boot, r_{u-1}); acc = fmaf(gamma, acc,
     r_i) for i = u - 2 down to t; y_t = acc. N = 1 is departure 5's and 9's expression, op for op,
     so a default learner beside others in a population keeps the default trainer's bits. The
     residuals, the loss and a prioritized window's mass follow from y_t as above.
R2D2's value rescaling h(x) is out of scope.
The vector step and the update above are written once, for P learners over the mz_drqn_pop_* entry
points: RecurrentDQNBase below. VectorRecurrentDQNPopulation (drqn_population.py) is that driver
with P learners, each with its own values of the per-learner arguments (T shared; K, the initial
state and the four priority arguments per learner, an alpha of None keeping that learner on
departure 8's sampler); this trainer is the same driver with P = 1. Its ring, directory and row
buffers without a leading dimension are the [1, ...] layout, its nets' flat parameter and gradient
buffers begin with a population row, and eps, seed, gamma, the counters and the window and priority
settings go up as one-element arrays. A class adds its optimizer step and target sync (FlatAdamW and
copy_flat here, mz_adamw_pop and mz_drqn_pop_sync there), its public surface (scalars here, lists of
P there) and its checkpoint format. The single-learner mz_drqn_* entry points stay exported
(include/mazerl.h); of them only mz_drqn_act (the evaluator) and mz_drqn_snapshot are called here.
"""
import copy
import ctypes as C
import math

import numpy as np
import torch

from .. import _native as N
from ..agents.flat import FlatAdamW, copy_flat, flatten_grads, flatten_params, grad_segment
from ..agents.lstm_dqn_agent import DQN, ETA_MIN, HIDDEN, T_MAX, epsilon_at
from ..agents.rf_agent import cosine_lr
from .episodic import EpisodicTrainer, episode_bound

FORMAT = "mazerl.VectorRecurrentDQNTrainer/1"
EVAL_KEY = 0x4556414C
ROW, STASH, PARAMS = 8, 192, 5252
SHAPES = ((128, 6), (128, 32), (128,), (128,), (4, 32), (4,))  # a net, in state_dict order
PRIO_ONE = 1 << 20  # the mass of priority 1 (MZ_DRQN_PRIO_FRAC)
U64 = 0xFFFFFFFFFFFFFFFF


def param_ptrs(net):
    """The host array of six device pointers the mz_drqn_* entry points take (state_dict order)."""
    ps = list(net.parameters())
    assert tuple(tuple(p.shape) for p in ps) == SHAPES
    return (C.c_void_p * 6)(*[p.data_ptr() for p in ps])


def check_window(window, burn_in, initial_state):
    """The replay-window arguments' rules (departures 7-9); ValueError otherwise."""
    ints = all(isinstance(v, int) and not isinstance(v, bool) for v in (burn_in,) +
               (() if window is None else (window,)))
    if not ints or initial_state not in ("stored", "zero") or burn_in < 0 or \
            (window is None and burn_in != 0) or \
            (window is not None and (window < 1 or burn_in % window != 0)):
        raise ValueError("window: None or an int >= 1; burn_in: an int >= 0, a multiple of the "
                         "window, 0 without one; initial_state: 'stored' or 'zero' "
                         f"(got {window!r}, {burn_in!r}, {initial_state!r})")


def check_priority(window, alpha, beta, eta, eps):
    """The prioritized-replay arguments' rules (departures 10-12); ValueError otherwise. alpha None
    is off; beta is a number or (beta0, beta1, updates)."""
    if alpha is None:
        return

    def num(v, lo=0.0, hi=float("inf")):
        return isinstance(v, (int, float)) and not isinstance(v, bool) and \
            math.isfinite(v) and lo <= v <= hi

    sched = isinstance(beta, (tuple, list)) and len(beta) == 3 and num(beta[0]) and \
        num(beta[1]) and isinstance(beta[2], int) and not isinstance(beta[2], bool) and beta[2] >= 1
    if window is None or not num(alpha) or not (num(beta) or sched) or not num(eta, 0.0, 1.0) or \
            not num(eps) or eps <= 0:
        raise ValueError("priority_alpha needs window=T; priority_alpha >= 0, priority_beta >= 0 "
                         "or (beta0, beta1, updates >= 1), priority_eta in [0, 1], priority_eps > "
                         f"0, all finite (got window {window!r}, {alpha!r}, {beta!r}, {eta!r}, "
                         f"{eps!r})")


def check_returns(double_q, n_step):
    """The target's arguments' rules (departures 13-14); ValueError otherwise."""
    if not isinstance(double_q, bool) or not isinstance(n_step, int) or isinstance(n_step, bool) \
            or n_step < 1:
        raise ValueError("double_q: a bool; n_step: an int >= 1 "
                         f"(got {double_q!r}, {n_step!r})")


def per_learner(value, P, name, kind=float):
    """A scalar for all learners or one value per learner -> a list of P."""
    if isinstance(value, (list, tuple, np.ndarray)):
        vals = [kind(v) for v in value]
        if len(vals) == 1:
            vals = vals * P
        if len(vals) != P:
            raise ValueError(f"{name}: {len(vals)} values for {P} learners")
        return vals
    return [kind(value)] * P


def _signed(u):
    """A 64-bit key as the int64 torch stores."""
    u &= U64
    return u - (1 << 64) if u >> 63 else u


class _PerLearner:
    """A per-learner host value of the driver. The list of P lives at `_<name>`, which is what
    RecurrentDQNBase reads and writes; the public attribute is that list for a population and its
    one entry for the single trainer (_ONE). Assigning gamma, seed, burn_in, priority_eta or
    priority_eps (the whole value, not an entry of the list) also renews the copy the kernels read
    (_mirror); so does n_step, within a trainer that was built with a learner off the target's
    defaults (the new values are checked first). initial_state, stored, priority_alpha and double_q
    fix the buffers and are not to be assigned after construction."""
    MIRRORED = ("gamma", "seed", "burn_in", "priority_eta", "priority_eps", "n_step")

    def __init__(self, name):
        self.key, self.mirrored = "_" + name, name in self.MIRRORED

    def __get__(self, obj, cls=None):
        if obj is None:
            return self
        v = getattr(obj, self.key)
        return v[0] if obj._ONE else v

    def __set__(self, obj, value):
        if self.key == "_n_step":
            obj._check_n_step([value] if obj._ONE else value)
        setattr(obj, self.key, [value] if obj._ONE else value)
        if self.mirrored and hasattr(obj, "upd"):  # (the device arrays exist)
            obj._mirror()


class RecurrentDQNBase(EpisodicTrainer):
    """The host driver of P recurrent DQN learners over B = P b instances, learner p on the block
    [p b, (p + 1) b): the arguments' checks, the buffers, the vector step (act, scan and store, the
    cadence), an update (the per-update scalars, the three samplers, the whole-episode and the
    window chains with the priority update between the source forward and the backward), the
    greedy rollout and the replay half of a checkpoint. Every launch is an mz_drqn_pop_* entry
    point. A subclass sets src, tgt and grad (flat [P][5252] rows), _learn() (sample, update, its
    optimizer step and target sync) and its public surface and checkpoint format; with _ONE it is
    the single trainer, P = 1, whose buffers carry no leading dimension."""
    _REC = ("rec_x", "rec_a", "rec_r")
    _ONE = False
    _PER = ("lr", "gamma", "starting_epsilon", "final_epsilon", "epsilon_decay", "seed", "tuf",
            "burn_in", "initial_state", "stored", "priority_beta", "priority_eta", "priority_eps",
            "double_q", "n_step", "steps_done", "updates", "filled", "last_lr")

    def _configure(self, P, B, lr, starting_epsilon, final_epsilon, epsilon_decay, discount_factor,
                   batch_size, memory_size, target_update_frequency, explore_actions, train_every,
                   seed, window, burn_in, initial_state, priority_alpha, priority_beta,
                   priority_eta, priority_eps, double_q=False, n_step=1):
        """The arguments' checks and the per-learner host values (each argument from lr to seed
        and from burn_in on: a scalar or a length-P sequence). Touches no GPU."""
        same = lambda v: v  # noqa: E731 (the checks want the values as they were given)
        self._double_q = per_learner(double_q, P, "double_q", same)
        self._n_step = per_learner(n_step, P, "n_step", same)
        for dq, ns in zip(self._double_q, self._n_step):
            check_returns(dq, ns)
        # whether the update forms its targets in a launch of its own (a learner is off the
        # defaults): fixed here, as it decides which buffers exist
        self._returns = any(self._double_q) or any(ns != 1 for ns in self._n_step)
        self._burn_in = per_learner(burn_in, P, "burn_in", same)
        self._initial_state = per_learner(initial_state, P, "initial_state", same)
        for K, S in zip(self._burn_in, self._initial_state):
            check_window(window, K, S)
        self.window = None if window is None else int(window)
        self._stored = [self.window is not None and S == "stored" for S in self._initial_state]
        alpha = per_learner(priority_alpha, P, "priority_alpha", same)
        beta = [priority_beta] * P if isinstance(priority_beta, tuple) else \
            per_learner(priority_beta, P, "priority_beta", same)
        eta = per_learner(priority_eta, P, "priority_eta", same)
        eps = per_learner(priority_eps, P, "priority_eps", same)
        for a, b, h, x in zip(alpha, beta, eta, eps):
            check_priority(window, a, b, h, x)
        # prio[p]: whether learner p is prioritized; its four settings (None for a uniform learner)
        self.prio = [a is not None for a in alpha]
        on = lambda vs, f: [f(v) if q else None for v, q in zip(vs, self.prio)]  # noqa: E731
        self._priority_alpha = on(alpha, float)
        self._priority_beta = on(beta, lambda b: float(b) if isinstance(b, (int, float)) else
                                 (float(b[0]), float(b[1]), int(b[2])))
        self._priority_eta, self._priority_eps = on(eta, float), on(eps, float)
        self._tuf = per_learner(target_update_frequency, P, "target_update_frequency", int)
        if batch_size < 1 or memory_size < batch_size or train_every < 1 or min(self._tuf) < 1 or \
                explore_actions not in (1, 2, 3, 4):
            raise ValueError("batch_size >= 1, memory_size >= batch_size, train_every >= 1, "
                             "target_update_frequency >= 1, explore_actions in 1..4")
        self.P, self.b = P, B // P
        self._lr = per_learner(lr, P, "lr")
        self._gamma = per_learner(discount_factor, P, "discount_factor")
        self._starting_epsilon = per_learner(starting_epsilon, P, "starting_epsilon")
        self._final_epsilon = per_learner(final_epsilon, P, "final_epsilon")
        self._epsilon_decay = per_learner(epsilon_decay, P, "epsilon_decay")
        self._seed = per_learner(seed, P, "seed", int)
        self.batch_size, self.capacity = int(batch_size), int(memory_size)
        self.explore_actions, self.train_every = int(explore_actions), int(train_every)
        self._steps_done = [0] * P  # the eps clocks
        self.counter = 0            # vector steps (the exploration draws' counter)
        self.launches = 0           # update launches (the overflow look's clock)
        self._updates = [0] * P
        self._filled = [0] * P      # the host's lower bounds of the rings' counts
        self._last_lr = [None] * P
        self.last_due = [False] * P  # the learners the last vector step updated

    def _check_n_step(self, values):
        """ValueError unless `values` may replace the learners' n_step."""
        values = per_learner(values, self.P, "n_step", lambda v: v)
        for ns in values:
            check_returns(False, ns)
        if not self._returns and any(ns != 1 for ns in values):
            raise ValueError("n_step above 1 needs a trainer built with double_q or n_step off "
                             "their defaults: the default update has no launch that reads it")

    @property
    def priority_alpha(self):
        """None when no learner is prioritized, else the learners' alphas (None: uniform)."""
        if not any(self.prio):
            return None
        return self._priority_alpha[0] if self._ONE else self._priority_alpha

    def _alloc_scalars(self):
        """The per-learner scalars on the device, uploaded once, and the per-update block."""
        P, kw = self.P, dict(device=self.device)
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.gamma_dev = torch.tensor(self._gamma, dtype=f32, **kw)
        self.seed_dev = torch.tensor([_signed(s) for s in self._seed], dtype=i64, **kw)
        self.eps_dev = torch.zeros(P, dtype=f32, **kw)
        # the per-update scalars, one upload: sample counters (int64), due, sync, lr (f32 bits);
        # prioritized: then the two samplers' masks and every learner's beta (float64)
        self.upd = torch.zeros((9 * P + P % 2) if any(self.prio) else 5 * P, dtype=i32, **kw)
        self.cnt_dev = self.upd[:2 * P].view(i64)
        self.due_dev, self.sync_dev = self.upd[2 * P:3 * P], self.upd[3 * P:4 * P]
        self.lr_dev = self.upd[4 * P:5 * P].view(f32)
        if any(self.prio):
            self.due_prio_dev, self.due_uni_dev = self.upd[5 * P:6 * P], self.upd[6 * P:7 * P]
            self.beta_dev = self.upd[7 * P + P % 2:].view(torch.float64)  # (8-byte aligned)
            f64 = lambda vs, ph: torch.tensor(  # noqa: E731 (a uniform learner: a valid placeholder)
                [ph if v is None else v for v in vs], dtype=torch.float64, **kw)
            self.prio_alpha_dev = f64(self._priority_alpha, 0.0)
            self.prio_eta_dev = f64(self._priority_eta, 0.0)
            self.prio_eps_dev = f64(self._priority_eps, 1.0)
        if self._returns:
            self.n_step_dev = torch.tensor(self._n_step, dtype=i32, **kw)
            self.double_dev = torch.tensor([int(v) for v in self._double_q], dtype=i32, **kw)
        self._prio_due = False  # whether the update under way has a due prioritized learner
        self._stage = {}  # (_send's pinned rows)
        if self.window is not None:
            self.burn_in_dev = torch.tensor(self._burn_in, dtype=i32, **kw)
            self.stored_dev = torch.tensor([int(s) for s in self._stored], dtype=i32, **kw)

    def _send(self, dev, values):
        """values (a numpy array of dev's shape and width) -> dev on the launch stream, without
        draining it: through a ring of pinned host rows, each reused only after the event of its
        last copy (a wait that only a host more than SLOTS copies ahead of the device meets)."""
        SLOTS = 8
        st = self._stage.get(dev.data_ptr())
        if st is None:
            rows = torch.zeros(SLOTS, dev.numel(), dtype=dev.dtype).pin_memory()
            st = self._stage[dev.data_ptr()] = [rows, rows.numpy(), [None] * SLOTS, 0]
        rows, host, events, k = st
        if events[k] is not None:
            events[k].synchronize()
        host[k] = values
        dev.copy_(rows[k], non_blocking=True)
        events[k] = torch.cuda.Event()
        events[k].record(torch.cuda.current_stream(self.device))
        st[3] = (k + 1) % SLOTS

    def _mirror(self):
        """The once-uploaded values that may be assigned later (_PerLearner.MIRRORED, a loaded
        checkpoint's seeds among them) go up again, in place."""
        pairs = [(self.gamma_dev, self._gamma), (self.seed_dev, [_signed(s) for s in self._seed])]
        if self.window is not None:
            pairs.append((self.burn_in_dev, self._burn_in))
        if self._returns:
            pairs.append((self.n_step_dev, self._n_step))
        if any(self.prio):
            pairs += [(self.prio_eta_dev, [v or 0.0 for v in self._priority_eta]),
                      (self.prio_eps_dev, [1.0 if v is None else v for v in self._priority_eps])]
        for dev, host in pairs:
            dev.copy_(torch.tensor(host, dtype=dev.dtype))

    def _alloc(self):
        """The per-instance buffers, the replay ring, an update's directory and row buffers
        (population: a leading P dimension) and, when a learner stores state, the snapshots' two
        buffers; then _alloc_scalars."""
        B, E, L = self.env.num_envs, self.batch_size, self.L
        lead = () if self._ONE else (self.P,)
        kw = dict(device=self.device)
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.h = torch.zeros(HIDDEN, B, dtype=f32, **kw)
        self.c = torch.zeros(HIDDEN, B, dtype=f32, **kw)
        self.rec_x = torch.zeros(B, L + 1, 6, dtype=f32, **kw)
        self.rec_a = torch.zeros(B, L, dtype=i32, **kw)
        self.rec_r = torch.zeros(B, L, dtype=torch.float64, **kw)
        self.r64 = torch.zeros(B, dtype=torch.float64, **kw)
        self.pool = torch.zeros(2, dtype=i64, **kw)  # mz_ppo_scan's row counters (unused here)
        # the replay memory: fixed-stride slots of L + 1 rows of 32 B
        self.mem = torch.zeros(*lead, self.capacity, L + 1, ROW, dtype=i32, **kw)
        self.mem_len = torch.zeros(*lead, self.capacity, dtype=i32, **kw)
        self.mem_term = torch.zeros(*lead, self.capacity, dtype=i32, **kw)
        self.ring = torch.zeros(*lead, 2, dtype=i64, **kw)  # head, count
        # an update's directory and row buffers: whole episodes, or windows of m <= T steps
        # (+ the entry-state row and the guard row), which the burn-in does not lengthen
        rows = E * (L + 1) if self.window is None else E * (min(self.window, L) + 2)
        if self.window is not None:
            self.wdir = torch.zeros(*lead, 5, E, dtype=i32, **kw)  # slot, n, b, k, m
            self.snaps = (L - 1) // self.window + 1
        self._state = any(self._stored)
        if self._state:
            self.snap_rec = torch.zeros(B, self.snaps, 2 * HIDDEN, dtype=f32, **kw)
            self.mem_state = torch.zeros(*lead, self.capacity, self.snaps, 2 * HIDDEN, dtype=f32,
                                         **kw)
        if any(self.prio):
            # a window's mass: u32 fixed point, 20 fractional bits (<= 2^30, so int32 holds it);
            # a slot's sum (< 2^63, so int64 holds it); the largest mass written, from priority 1
            self.mem_prio = torch.zeros(*lead, self.capacity, self.snaps, dtype=i32, **kw)
            self.mem_psum = torch.zeros(*lead, self.capacity, dtype=i64, **kw)
            self.prio_max = torch.full(lead or (1,), PRIO_ONE, dtype=i32, **kw)
            self.isw = torch.ones(*lead, E, dtype=f32, **kw)
        self.d_slot = torch.zeros(*lead, E, dtype=i32, **kw)
        self.d_len = torch.zeros(*lead, E, dtype=i32, **kw)
        self.d_off = torch.zeros(*lead, E, dtype=i64, **kw)
        self.d_tot = torch.zeros(*lead, 2, dtype=i64, **kw)
        if self._returns:  # the target's four Q' of a row and the source's argmax, in qmax's place
            self.q4 = torch.zeros(*lead, rows, 4, dtype=f32, **kw)
            self.sel = torch.zeros(*lead, rows, dtype=i32, **kw)
        self.qmax = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.stash = torch.zeros(*lead, rows, STASH, dtype=f32, **kw)
        self.qa = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.y = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.d = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.ep_loss = torch.zeros(*lead, E, dtype=torch.float64, **kw)
        self.gpart = torch.zeros(*lead, E, PARAMS, dtype=f32, **kw)
        self.loss = torch.zeros(*(lead or (1,)), dtype=f32, **kw)
        self._alloc_scalars()

    def epsilon(self, p=0):
        return epsilon_at(self._steps_done[p], self._starting_epsilon[p], self._final_epsilon[p],
                          self._epsilon_decay[p])

    def update_steps_done(self, p=None):
        for k in range(self.P) if p is None else (int(p),):
            self._steps_done[k] = self._steps_done[k] // 2

    def beta(self, p=0):
        """Learner p's importance exponent at its coming update: its priority_beta, or its linear
        schedule over its own update count (computed here, on the host)."""
        b = self._priority_beta[p]
        if isinstance(b, float):
            return b
        return b[0] + (b[1] - b[0]) * min(self._updates[p] / b[2], 1.0)

    # ---- a vector step --------------------------------------------------------------------------
    def _act(self):
        env = self.env
        eps = [min(max(self.epsilon(p), 0.0), 1.0) for p in range(self.P)]
        for p in range(self.P):
            self._steps_done[p] += 1
        self._send(self.eps_dev, np.asarray(eps, np.float32))
        if self._state:  # (all P b instances: a zero-state learner's snapshots are never read)
            N.check(self.lib.mz_drqn_snapshot(
                HIDDEN, env.num_envs, self.L, self.window, self.t.data_ptr(), self.h.data_ptr(),
                self.c.data_ptr(), self.snap_rec.data_ptr(), self._stream()))
        N.check(self.lib.mz_drqn_pop_act(
            self.src.data_ptr(), HIDDEN, self.P, self.b, env.obs6.data_ptr(), self.L,
            self.eps_dev.data_ptr(), self.explore_actions, self.seed_dev.data_ptr(),
            self.counter & U64, self.t.data_ptr(), self.h.data_ptr(), self.c.data_ptr(),
            self.rec_x.data_ptr(), self.rec_a.data_ptr(), self.act_out.data_ptr(), None,
            self._stream()))
        self.counter += 1

    def _scan_store(self):
        env, L, P, b, st = self.env, self.L, self.P, self.b, self._stream()
        self.r64.copy_(env.reward)
        self._scan(self.r64, env.terminated, env.truncated, self.rec_r,
                   self.pool[0:].data_ptr(), self.pool[1:].data_ptr())
        fin = (self.fin_id.data_ptr(), self.fin_len.data_ptr(), self.fin_count.data_ptr())
        if self._state:  # (reads the ring's head, which the store advances)
            N.check(self.lib.mz_drqn_pop_snap_store(
                HIDDEN, P, b, L, self.window, *fin, self.snap_rec.data_ptr(), self.capacity,
                self.mem_state.data_ptr(), self.ring.data_ptr(), st))
        if any(self.prio):  # (reads the head too: new windows enter at prio_max)
            N.check(self.lib.mz_drqn_pop_prio_store(
                HIDDEN, P, b, L, self.window, *fin, self.capacity, self.mem_prio.data_ptr(),
                self.mem_psum.data_ptr(), self.prio_max.data_ptr(), self.ring.data_ptr(), st))
        N.check(self.lib.mz_drqn_pop_store(
            env.obs6.data_ptr(), env.terminated.data_ptr(), P, b, L, *fin, self.rec_x.data_ptr(),
            self.rec_a.data_ptr(), self.rec_r.data_ptr(), self.capacity, self.mem.data_ptr(),
            self.mem_len.data_ptr(), self.mem_term.data_ptr(), self.ring.data_ptr(), st))

    def vector_step(self):
        self._act()
        self.env.step(self.act_out)
        self._scan_store()
        self._reset_winners()
        E = self.batch_size
        if min(self._filled) < E:  # (only until every learner has its first batch: one sync a step)
            counts = self.ring.view(-1, 2)[:, 1].tolist()
            self._filled = [f if f >= E else int(n) for f, n in zip(self._filled, counts)]
        due = [False] * self.P
        if self.counter % self.train_every == 0:
            due = [f >= E for f in self._filled]
        self.last_due = due
        if any(due):
            self._update(due)

    # ---- an update ------------------------------------------------------------------------------
    def _update(self, due):
        if self.launches % 256 == 0 and int(self.stats[3]):  # (one look every 256 updates)
            raise RuntimeError(f"recurrent DQN episode records overflowed L = {self.L} steps "
                               "(mz_ppo_scan stats[3])")
        self.launches += 1
        lr, sync = [0.0] * self.P, [0] * self.P
        for p in range(self.P):
            if due[p]:
                lr[p] = self._last_lr[p] = cosine_lr(self._updates[p], self._lr[p], T_MAX, ETA_MIN)
                sync[p] = int((self._updates[p] + 1) % self._tuf[p] == 0)
        self._learn(due, sync, lr)
        for p in range(self.P):
            self._updates[p] += int(due[p])

    def _upload(self, due, sync, lr):
        """The per-update scalars of the coming update, one host-to-device copy (_send)."""
        P = self.P
        buf = np.zeros(self.upd.numel(), np.int32)
        buf[:2 * P].view(np.int64)[:] = self._updates
        buf[2 * P:3 * P] = due
        buf[3 * P:4 * P] = sync
        buf[4 * P:5 * P].view(np.float32)[:] = lr
        if any(self.prio):  # the two samplers' masks; beta_p at learner p's own update count
            buf[5 * P:6 * P] = [d and q for d, q in zip(due, self.prio)]
            buf[6 * P:7 * P] = [d and not q for d, q in zip(due, self.prio)]
            buf[7 * P + P % 2:].view(np.float64)[:] = [self.beta(p) if q else 0.0
                                                       for p, q in enumerate(self.prio)]
            self._prio_due = bool(buf[5 * P:6 * P].any())
        self._send(self.upd, buf)

    def _draw(self, due):
        """E distinct slots and the directory (d_slot, d_len, d_off, d_tot) of every due learner,
        keyed by its update count; windowed: the same slots, one window each and the window
        directory (wdir, d_off, d_tot); a prioritized learner: E windows in proportion to their
        mass, the same directory, and its importance weights (isw)."""
        mask = self.due_dev
        if any(self.prio):
            if self._prio_due:
                N.check(self.lib.mz_drqn_pop_prio_sample(
                    self.seed_dev.data_ptr(), self.cnt_dev.data_ptr(), self.burn_in_dev.data_ptr(),
                    self.beta_dev.data_ptr(), self.due_prio_dev.data_ptr(), HIDDEN, self.P,
                    self.batch_size, self.L, self.window, max(self._burn_in), self.capacity,
                    self.mem_len.data_ptr(), self.mem_prio.data_ptr(), self.mem_psum.data_ptr(),
                    self.wdir.data_ptr(), self.d_off.data_ptr(), self.d_tot.data_ptr(),
                    self.isw.data_ptr(), self._stream()))
            due = [d and not q for d, q in zip(due, self.prio)]
            if not any(due):
                return
            mask = self.due_uni_dev
        filled = min(f for f, d in zip(self._filled, due) if d)
        if self.window is not None:
            N.check(self.lib.mz_drqn_pop_window_sample(
                self.seed_dev.data_ptr(), self.cnt_dev.data_ptr(), self.burn_in_dev.data_ptr(),
                mask.data_ptr(), HIDDEN, self.P, self.batch_size, self.L, self.window,
                max(self._burn_in), self.capacity, filled, self.ring.data_ptr(),
                self.mem_len.data_ptr(), self.wdir.data_ptr(), self.d_off.data_ptr(),
                self.d_tot.data_ptr(), self._stream()))
            return
        N.check(self.lib.mz_drqn_pop_sample(
            self.seed_dev.data_ptr(), self.cnt_dev.data_ptr(), self.due_dev.data_ptr(), self.P,
            self.batch_size, self.L, self.capacity, filled, self.ring.data_ptr(),
            self.mem_len.data_ptr(), self.d_slot.data_ptr(), self.d_len.data_ptr(),
            self.d_off.data_ptr(), self.d_tot.data_ptr(), self._stream()))

    def _gradients(self):
        """Every due learner's loss (self.loss, on the device) and gradient (self.grad) on its
        directory's episodes or windows: the target net's forward, the source net's, a prioritized
        learner's new masses and weighted residuals, the backward and its reduction."""
        if self._returns:
            return self._gradients_returns()
        P, E, L, cap, st = self.P, self.batch_size, self.L, self.capacity, self._stream()
        due, gam = self.due_dev.data_ptr(), self.gamma_dev.data_ptr()
        rows = (self.stash.data_ptr(), self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(),
                self.ep_loss.data_ptr())
        back = (self.stash.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(),
                self.gpart.data_ptr(), self.grad.data_ptr(), self.loss.data_ptr(), st)
        if self.window is None:
            dirs = (self.d_slot.data_ptr(), self.d_len.data_ptr(), self.d_off.data_ptr(),
                    self.d_tot.data_ptr())
            for net, target, out in ((self.tgt, 1, (None,) * 5), (self.src, 0, rows)):
                N.check(self.lib.mz_drqn_pop_seq_forward(
                    net.data_ptr(), HIDDEN, target, P, E, L, cap, gam, due, self.mem.data_ptr(),
                    self.mem_term.data_ptr(), *dirs, self.qmax.data_ptr(), *out, st))
            N.check(self.lib.mz_drqn_pop_seq_backward(
                self.src.data_ptr(), HIDDEN, P, E, L, cap, due, self.mem.data_ptr(), *dirs, *back))
            return
        T, K = self.window, max(self._burn_in)
        state = self.mem_state.data_ptr() if self._state else None
        burn, stored = self.burn_in_dev.data_ptr(), self.stored_dev.data_ptr()
        dirs = (self.wdir.data_ptr(), self.d_off.data_ptr(), self.d_tot.data_ptr())
        for net, target, out in ((self.tgt, 1, (None,) * 5), (self.src, 0, rows)):
            N.check(self.lib.mz_drqn_pop_window_forward(
                net.data_ptr(), HIDDEN, target, P, E, L, T, K, cap, gam, burn, stored, due,
                self.mem.data_ptr(), self.mem_term.data_ptr(), state, *dirs, self.qmax.data_ptr(),
                *out, st))
        if self._prio_due:  # the new masses; d and ep_loss times the weights
            N.check(self.lib.mz_drqn_pop_prio_update(
                self.prio_alpha_dev.data_ptr(), self.prio_eta_dev.data_ptr(),
                self.prio_eps_dev.data_ptr(), self.due_prio_dev.data_ptr(), HIDDEN, P, E, L, T,
                cap, *dirs, self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(),
                self.ep_loss.data_ptr(), self.isw.data_ptr(), self.mem_prio.data_ptr(),
                self.mem_psum.data_ptr(), self.prio_max.data_ptr(), st))
        N.check(self.lib.mz_drqn_pop_window_backward(
            self.src.data_ptr(), HIDDEN, P, E, L, T, K, cap, burn, due, self.mem.data_ptr(), *dirs,
            *back))

    def _gradients_returns(self):
        """_gradients when a learner is off the target's defaults (departures 13-14), for all due
        learners: the target net's four Q' per row, the source net's forward with its argmax and
        one step more, the returns launch that forms y, d and ep_loss (sel only when a learner is
        double: without it N = 1 is the default chain's arithmetic), then the priority update and
        the backward as they are."""
        P, E, L, cap, st = self.P, self.batch_size, self.L, self.capacity, self._stream()
        due = self.due_dev.data_ptr()
        fwd = (self.q4.data_ptr(), self.stash.data_ptr(), self.qa.data_ptr(), self.sel.data_ptr(),
               st)
        ret = (self.qa.data_ptr(), self.q4.data_ptr(),
               self.sel.data_ptr() if any(self._double_q) else None, self.y.data_ptr(),
               self.d.data_ptr(), self.ep_loss.data_ptr(), st)
        per = (self.n_step_dev.data_ptr(), max(self._n_step), self.double_dev.data_ptr(),
               self.gamma_dev.data_ptr())
        back = (self.stash.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(),
                self.gpart.data_ptr(), self.grad.data_ptr(), self.loss.data_ptr(), st)
        if self.window is None:
            dirs = (self.d_slot.data_ptr(), self.d_len.data_ptr(), self.d_off.data_ptr(),
                    self.d_tot.data_ptr())
            for net, target in ((self.tgt, 1), (self.src, 0)):
                N.check(self.lib.mz_drqn_pop_seq_forward_q(
                    net.data_ptr(), HIDDEN, target, P, E, L, cap, due, self.mem.data_ptr(), *dirs,
                    *fwd))
            N.check(self.lib.mz_drqn_pop_seq_returns(
                *per, due, P, E, L, cap, self.mem.data_ptr(), self.mem_term.data_ptr(), *dirs,
                *ret))
            N.check(self.lib.mz_drqn_pop_seq_backward(
                self.src.data_ptr(), HIDDEN, P, E, L, cap, due, self.mem.data_ptr(), *dirs, *back))
            return
        T, K = self.window, max(self._burn_in)
        state = self.mem_state.data_ptr() if self._state else None
        burn, stored = self.burn_in_dev.data_ptr(), self.stored_dev.data_ptr()
        dirs = (self.wdir.data_ptr(), self.d_off.data_ptr(), self.d_tot.data_ptr())
        for net, target in ((self.tgt, 1), (self.src, 0)):
            N.check(self.lib.mz_drqn_pop_window_forward_q(
                net.data_ptr(), HIDDEN, target, P, E, L, T, K, cap, burn, stored, due,
                self.mem.data_ptr(), state, *dirs, *fwd))
        N.check(self.lib.mz_drqn_pop_window_returns(
            *per, burn, due, P, E, L, T, K, cap, self.mem.data_ptr(), self.mem_term.data_ptr(),
            *dirs, *ret))
        if self._prio_due:  # on the new y: the new masses; d and ep_loss times the weights
            N.check(self.lib.mz_drqn_pop_prio_update(
                self.prio_alpha_dev.data_ptr(), self.prio_eta_dev.data_ptr(),
                self.prio_eps_dev.data_ptr(), self.due_prio_dev.data_ptr(), HIDDEN, P, E, L, T,
                cap, *dirs, self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(),
                self.ep_loss.data_ptr(), self.isw.data_ptr(), self.mem_prio.data_ptr(),
                self.mem_psum.data_ptr(), self.prio_max.data_ptr(), st))
        N.check(self.lib.mz_drqn_pop_window_backward(
            self.src.data_ptr(), HIDDEN, P, E, L, T, K, cap, burn, due, self.mem.data_ptr(), *dirs,
            *back))

    # ---- the settings and the replay half of a checkpoint ---------------------------------------
    def _window_settings(self):
        """T with the burn-in and the initial state (a population's: the per-learner lists); None
        without windows."""
        if self.window is None:
            return None
        return {"window": self.window, "burn_in": copy.copy(self.burn_in),
                "initial_state": copy.copy(self.initial_state)}

    def _priority_settings(self):
        if not any(self.prio):
            return None
        s = {"alpha": list(self._priority_alpha),
             "beta": [list(b) if isinstance(b, tuple) else b for b in self._priority_beta],
             "eta": list(self._priority_eta), "eps": list(self._priority_eps)}
        return {k: v[0] for k, v in s.items()} if self._ONE else s

    def _returns_settings(self):
        """double_q and n_step (a population's: the per-learner lists); None where every learner
        has the defaults."""
        if not any(self._double_q) and all(ns == 1 for ns in self._n_step):
            return None
        return {"double_q": copy.copy(self.double_q), "n_step": copy.copy(self.n_step)}

    def _check_settings(self, sd):
        """ValueError unless the checkpoint's window, priority and target settings are this
        object's. (A checkpoint from before an option has no such key: window=None,
        priority_alpha=None, double_q=False and n_step=1.)"""
        kind = "trainer" if self._ONE else "population"
        if sd.get("window") != self._window_settings():
            raise ValueError(f"the checkpoint's replay windows {sd.get('window')} differ from this "
                             f"{kind}'s {self._window_settings()}")
        if sd.get("priority") != self._priority_settings():
            raise ValueError(f"the checkpoint's prioritized replay {sd.get('priority')} differs "
                             f"from this {kind}'s {self._priority_settings()}")
        if sd.get("returns") != self._returns_settings():
            raise ValueError(f"the checkpoint's targets {sd.get('returns')} differ from this "
                             f"{kind}'s {self._returns_settings()}")

    def _slots(self, k):
        """Buffer k as [P][capacity][...] (the single trainer's has no leading dimension)."""
        t = getattr(self, k)
        return t[None] if self._ONE else t

    def _save_slots(self, sd, keys):
        """Each ring's filled slots of the buffers `keys` (a population: a list of P per key)."""
        counts = [int(n) for n in self.ring.view(-1, 2)[:, 1].tolist()]
        for k in keys:
            parts = [self._slots(k)[p, :n].clone() for p, n in enumerate(counts)]
            sd[k] = parts[0] if self._ONE else parts

    def _load_slots(self, sd, keys):
        for k in keys:
            for p, part in enumerate([sd[k]] if self._ONE else sd[k]):
                self._slots(k)[p, :part.shape[0]].copy_(part)

    def _save_own(self, sd):
        """_OWN whole and the ring's filled slots."""
        sd.update({k: getattr(self, k).clone() for k in self._OWN})
        self._save_slots(sd, ("mem", "mem_len", "mem_term"))

    def _save_options(self, sd):
        """What the options add: double_q and n_step where a learner leaves their defaults; the
        window and priority settings, the in-flight and the filled slots' snapshots when a learner
        stores state, the filled slots' masses and sums and prio_max when one is prioritized."""
        if self._returns_settings() is not None:
            sd["returns"] = self._returns_settings()
        if self.window is not None:
            sd["window"] = self._window_settings()
        if self._state:
            sd["snap_rec"] = self.snap_rec.clone()
            self._save_slots(sd, ("mem_state",))
        if any(self.prio):
            sd["priority"] = self._priority_settings()
            self._save_slots(sd, ("mem_prio", "mem_psum"))
            sd["prio_max"] = self.prio_max.clone()

    def _load_replay(self, sd):
        """_OWN, the rings' slots and the options' buffers. (The seeds a checkpoint carries went
        up when they were assigned.)"""
        for k in self._OWN:
            getattr(self, k).copy_(sd[k])
        self._load_slots(sd, ("mem", "mem_len", "mem_term"))
        if self._state:
            self.snap_rec.copy_(sd["snap_rec"])
            self._load_slots(sd, ("mem_state",))
        if any(self.prio):
            self._load_slots(sd, ("mem_prio", "mem_psum"))
            self.prio_max.copy_(sd["prio_max"])

    @staticmethod
    def greedy_rollout(env, act, limit):
        """One greedy episode per row of `env`, at most `limit` vector steps: act(k) gives step
        k's int32 actions. Returns (the rows that won, the vector steps made)."""
        finished = torch.zeros(env.num_envs, dtype=torch.bool, device=env.device)
        won = torch.zeros(env.num_envs, dtype=torch.bool, device=env.device)
        k = 0
        while k < limit:
            acts = act(k)
            env.step(torch.where(finished, torch.full_like(acts, -1), acts))
            term = env.terminated.bool()
            won |= term & ~finished
            finished |= term | env.truncated.bool()
            k += 1
            if k % 32 == 0 and bool(finished.all()):
                break
        return won, k


for _name in RecurrentDQNBase._PER:
    setattr(RecurrentDQNBase, _name, _PerLearner(_name))
RecurrentDQNBase.target_update_frequency = _PerLearner("tuf")  # (the argument's name)


class VectorRecurrentDQNTrainer(RecurrentDQNBase):
    _FORMAT = FORMAT
    _SHAPE = ("L", "capacity")
    _COUNTERS = ("seed", "steps_done", "counter", "updates", "filled")
    _ONE = True
    _DUE = (True,)

    def __init__(self, env, device, lr=1e-3, starting_epsilon=0.9, final_epsilon=0.05,
                 epsilon_decay=1000.0, discount_factor=0.99, batch_size=32, memory_size=20000,
                 target_update_frequency=10, explore_actions=4, train_every=1, seed=0, bank=True,
                 curriculum=False, growth=None, algorithm="r-prim", bank_candidates=1, window=None,
                 burn_in=0, initial_state="stored", archive=None, priority_alpha=None,
                 priority_beta=0.6, priority_eta=0.9, priority_eps=1e-3, double_q=False, n_step=1):
        """archive: EpisodicTrainer's explored-maze pool (None: off). priority_alpha: prioritized
        replay windows (departures 10-12; None: off, nothing of it is allocated or launched);
        priority_beta: a number, or (beta0, beta1, updates) for a linear schedule over the update
        count. double_q, n_step: double-Q targets and n-step returns (departures 13-14; False and
        1: off, the update's launches and bits are those without the arguments)."""
        one = lambda *vs: ([v] for v in vs)  # noqa: E731 (each value is the one learner's)
        self._configure(
            1, getattr(env, "num_envs", 1),
            *one(lr, starting_epsilon, final_epsilon, epsilon_decay, discount_factor), batch_size,
            memory_size, [target_update_frequency], explore_actions, train_every, [seed], window,
            *one(burn_in, initial_state, priority_alpha, priority_beta, priority_eta, priority_eps,
                 double_q, n_step))
        super().__init__(env, device, bank=bank, curriculum=curriculum, growth=growth,
                         algorithm=algorithm, bank_candidates=bank_candidates, archive=archive)
        torch.manual_seed(seed)
        self.source_net = DQN(6, 4, HIDDEN, self.device)
        self.target_net = DQN(6, 4, HIDDEN, self.device)
        self.tgt = flatten_params(self.target_net)
        self.grad = flatten_grads(self.source_net)
        self.src = self.source_net._flat_params
        # the flat buffers begin with a population row: no segment is padded
        assert self.source_net._flat_sizes == [math.prod(s) for s in SHAPES] and \
            sum(self.source_net._flat_sizes) == PARAMS
        copy_flat(self.target_net, self.source_net)
        for p in self.source_net.parameters():
            p.grad = grad_segment(p)
        self.opt = FlatAdamW(self.source_net, lr=lr, clamp=1.0)
        self._ps = param_ptrs(self.source_net)  # (_Evaluator's)
        self._alloc()

    def sample(self):
        """The coming update's scalars go up and its batch is drawn (_draw). Of the block this
        trainer's kernels read the sample counter, the due mask and beta; its lr is FlatAdamW's
        and its sync copy_flat's, so both go up as zeros."""
        self._upload(self._DUE, (0,), (0.0,))
        self._draw(self._DUE)

    def update(self, lr):
        """One optimizer step on the directory's episodes at learning rate `lr`; the loss stays on
        the device (self.loss)."""
        self.opt.param_groups[0]["lr"].fill_(float(lr))
        self._gradients()
        self.opt.step()

    def _learn(self, due, sync, lr):
        # (one learner, always due: of the three lists only lr[0] and sync[0] are consumed)
        self.sample()
        self.update(lr[0])
        if sync[0]:
            copy_flat(self.target_net, self.source_net)

    def _log_fields(self):
        if self.priority_alpha is None:
            return {"loss": float(self.loss)}
        return {"loss": float(self.loss), "prio_max": int(self.prio_max) / PRIO_ONE,
                "mean_weight": float(self.isw.mean())}

    # ---- evaluation (vector_trainer.evaluate) ---------------------------------------------------
    def evaluator(self):
        """A learner for vector_trainer.evaluate: greedy actions from a per-row (h, c) that starts
        at zero (evaluate plays one episode per row) and advances once per greedy() call."""
        return _Evaluator(self)

    def greedy(self, obs6, window=None, bits=None):
        """The greedy action of every row, carrying (h, c) per row between calls; the state is
        zeroed by reset_greedy() or when the number of rows changes. For an evaluation of its own
        state use evaluator()."""
        ev = getattr(self, "_eval", None)
        if ev is None:
            ev = self._eval = _Evaluator(self)
        return ev.greedy(obs6, window, bits)

    def reset_greedy(self):
        if getattr(self, "_eval", None) is not None:
            self._eval.reset()

    # ---- checkpoint / resume (mazerl/checkpoint.py) -------------------------------------------
    _OWN = ("h", "c", "ring", "pool", "loss")

    def state_dict(self):
        """The run between two vector steps: both nets, the optimizer, (h, c), the in-flight
        records, the filled replay slots with head and count, the counters and the env
        (_save_common); a windowed trainer adds its settings and, when it stores state, the
        in-flight and the filled slots' snapshots; a prioritized one its settings, masses and
        sums."""
        sd, o = self._save_common(), self.opt
        self._save_options(sd)
        self._save_own(sd)
        sd["source"] = {k: v.clone() for k, v in self.source_net.state_dict().items()}
        sd["target"] = {k: v.clone() for k, v in self.target_net.state_dict().items()}
        sd["opt"] = {"exp_avg": o.exp_avg.clone(), "exp_avg_sq": o.exp_avg_sq.clone(),
                     "step": o._step_buf.clone(), "lr": o.param_groups[0]["lr"].clone()}
        return sd

    def load_state_dict(self, sd):
        self._check_settings(sd)
        self._load_common(sd)
        self.launches = self.updates  # (the overflow look's clock is not in this format)
        with torch.no_grad():
            self.source_net.load_state_dict(sd["source"])
            self.target_net.load_state_dict(sd["target"])
        o = self.opt
        o.exp_avg.copy_(sd["opt"]["exp_avg"])
        o.exp_avg_sq.copy_(sd["opt"]["exp_avg_sq"])
        o._step_buf.copy_(sd["opt"]["step"])
        o.param_groups[0]["lr"].copy_(sd["opt"]["lr"])
        self._load_replay(sd)


def evaluate_plain(learner, num_mazes, dim, algorithm="r-prim", seed=0x7E57, toroidal=False,
                   device=None):
    """vector_trainer.evaluate on plain (enrich=False) mazes, which exist from 9x9 up (an Enrich
    env needs room for the 15x15 window): the fraction of `num_mazes` fresh mazes solved greedily
    in one episode. `learner`: a trainer's evaluator(). Returns (rate, vector steps)."""
    from ..vector_env import VectorMazeEnv
    env = VectorMazeEnv(num_mazes, dim, toroidal=toroidal, enrich=False, device=device,
                        algorithm=algorithm, seed=seed, pos=False, done_list=False)
    won, k = RecurrentDQNBase.greedy_rollout(
        env, lambda k: learner.greedy(env.obs6, None, None).to(torch.int32),
        episode_bound(dim, toroidal) + 1)
    rate = float(won.float().mean())
    env.close()
    return rate, k


class _Evaluator:
    supports_bits = True

    def __init__(self, trainer):
        self.trainer = trainer
        self.n = 0
        self.h = self.c = self.t = None
        self.calls = 0

    def reset(self):
        if self.h is not None:
            self.h.zero_()
            self.c.zero_()
            self.t.zero_()

    def greedy(self, obs6, window=None, bits=None):
        tr = self.trainer
        n = obs6.shape[0]
        if n != self.n:
            kw = dict(device=obs6.device)
            self.h = torch.zeros(HIDDEN, n, dtype=torch.float32, **kw)
            self.c = torch.zeros(HIDDEN, n, dtype=torch.float32, **kw)
            self.t = torch.zeros(n, dtype=torch.int32, **kw)
            self.n = n
        obs6 = obs6.contiguous()
        out = torch.empty(n, dtype=torch.int32, device=obs6.device)
        N.check(tr.lib.mz_drqn_act(
            tr._ps, HIDDEN, obs6.data_ptr(), n, 0, 0.0, tr.explore_actions,
            (tr.seed ^ EVAL_KEY) & U64, self.calls & U64, self.t.data_ptr(), self.h.data_ptr(),
            self.c.data_ptr(), None, None, out.data_ptr(), None,
            torch.cuda.current_stream(obs6.device).cuda_stream))
        self.calls += 1
        self.t.fill_(1)  # zero state was the first call's; from now on the carried one
        return out.long()
