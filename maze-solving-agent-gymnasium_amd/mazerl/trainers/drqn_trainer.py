"""Vectorised recurrent DQN — the reference's LSTM agent (agents/lstm_dqn_agent.py: an
nn.LSTMCell(6, 32) + nn.Linear(32, 4) Q-network over obs6, whole episodes in
SequentialExperienceReplayMemory, lib/replay_memory.py:26-43) over B instances at once, on plain
(enrich=False) or Enrich envs, euclidean or toroidal. Only obs6 is read.

Per vector step, with no host round trip once the memory holds a batch (csrc/mz_drqn.hip):
  act      mz_drqn_act: the cell and the head from each instance's (h, c) ([32][B] in HBM), the
           eps-greedy draw, the record of (x_t, a_t) at t[i];
  step     the env step;
  scan     mz_ppo_scan, unchanged (the f32 reward widened to its float64 record; t[i] += 1; the
           finished episodes' list in instance order). It drops 1-step episodes, so none reaches
           the memory;
  store    mz_drqn_store: x_n and each finished episode into ring slot (head + k) mod capacity;
  reset    winners get new mazes, truncated instances restart theirs (schedule.py as REINFORCE);
  update   when due: mz_drqn_sample (E distinct slots + the batch directory), the target net's
           sequence forward (max_a Q'_t), the source net's (Q_t[a_t], y_t, residuals, the stash),
           mz_drqn_seq_backward (BPTT, gradients reduced in a fixed order into the flat gradient
           segments), then FlatAdamW (the reference's clamp_(-1, 1) + AdamW in one launch).
With window=T the update trains on one window of T steps per sampled episode (departures 7-9):
mz_drqn_snapshot runs before act, mz_drqn_snap_store before store, and the update is
mz_drqn_window_sample / _forward / _backward; its row buffers hold E (T + 2) rows whatever the maze
size and the burn-in are. With window=None (the default) none of these is launched.

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
     episodes chosen with exactly mz_drqn_sample's draws for the same (seed, update count), then
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
     entries are 0 and its sum psum[slot] = ceil(n / T) prio_max. mz_drqn_prio_store follows
     mz_drqn_store's slot rule and validity tests and runs before it, as mz_drqn_snap_store does;
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
VectorRecurrentDQNPopulation takes the four priority arguments per learner (an alpha of None keeps
that learner on departure 8's sampler); its learner p is this trainer with learner p's values,
departures 10-12 included, and the three kernels serve all prioritized learners in one launch each.
VectorRecurrentDQNPopulation takes the same three arguments (T shared, K and the initial state per
learner); its learner p is this trainer with (T, K_p, S_p), departures 7-9 included. On the device
the two are one: every mz_drqn_* entry point here launches the population's kernel with P = 1.
RecurrentDQNBase holds what the two classes share on the host.
"""
import copy
import ctypes as C
import math

import torch

from .. import _native as N
from ..agents.flat import FlatAdamW, copy_flat, flatten_grads, flatten_params, grad_segment
from ..agents.lstm_dqn_agent import DQN, ETA_MIN, HIDDEN, T_MAX, epsilon_at
from ..agents.rf_agent import cosine_lr
from .episodic import EpisodicTrainer, episode_bound

FORMAT = "mazerl.VectorRecurrentDQNTrainer/1"
EVAL_KEY = 0x4556414C
ROW, STASH, PARAMS = 8, 192, 5252
PRIO_ONE = 1 << 20  # the mass of priority 1 (MZ_DRQN_PRIO_FRAC)
U64 = 0xFFFFFFFFFFFFFFFF


def param_ptrs(net):
    """The host array of six device pointers the mz_drqn_* entry points take (state_dict order)."""
    ps = list(net.parameters())
    assert [tuple(p.shape) for p in ps] == [(128, 6), (128, 32), (128,), (128,), (4, 32), (4,)]
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


class RecurrentDQNBase(EpisodicTrainer):
    """What the trainer and the population (drqn_population.py) share: the buffers, the scan and
    store of a vector step, the overflow look, the window settings and the greedy rollout. The
    population's ring, directory and row buffers carry a leading P dimension and its store calls
    (_snap_store_call, _prio_store_call, _store_call) take (P, b) where the trainer's take B;
    nothing else differs."""
    _REC = ("rec_x", "rec_a", "rec_r")
    _KIND = "trainer"  # (load_state_dict's error text)
    # prioritized windows: None is off. The trainer holds its alpha; the population None when every
    # learner's is None and the list of its learners' alphas otherwise.
    priority_alpha = None

    def _alloc(self, P=None, state=False):
        """The per-instance buffers, the replay ring, an update's directory and row buffers
        (population: a leading P dimension) and, with `state`, the snapshots' two buffers."""
        B, E, L = self.env.num_envs, self.batch_size, self.L
        lead = () if P is None else (P,)
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
        self._state = bool(state)
        if self._state:
            self.snap_rec = torch.zeros(B, self.snaps, 2 * HIDDEN, dtype=f32, **kw)
            self.mem_state = torch.zeros(*lead, self.capacity, self.snaps, 2 * HIDDEN, dtype=f32,
                                         **kw)
        if self.priority_alpha is not None:
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
        self.qmax = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.stash = torch.zeros(*lead, rows, STASH, dtype=f32, **kw)
        self.qa = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.y = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.d = torch.zeros(*lead, rows, dtype=f32, **kw)
        self.ep_loss = torch.zeros(*lead, E, dtype=torch.float64, **kw)
        self.gpart = torch.zeros(*lead, E, PARAMS, dtype=f32, **kw)
        self.loss = torch.zeros(*(lead or (1,)), dtype=f32, **kw)

    def _scan_store(self):
        env, L, st = self.env, self.L, self._stream()
        self.r64.copy_(env.reward)
        self._scan(self.r64, env.terminated, env.truncated, self.rec_r,
                   self.pool[0:].data_ptr(), self.pool[1:].data_ptr())
        fin = (self.fin_id.data_ptr(), self.fin_len.data_ptr(), self.fin_count.data_ptr())
        if self._state:  # (reads the ring's head, which the store advances)
            self._snap_store_call(L, self.window, *fin, self.snap_rec.data_ptr(), self.capacity,
                                  self.mem_state.data_ptr(), self.ring.data_ptr(), st)
        if self.priority_alpha is not None:  # (reads the head too: new windows enter at prio_max)
            self._prio_store_call(L, self.window, *fin, self.capacity, self.mem_prio.data_ptr(),
                                  self.mem_psum.data_ptr(), self.prio_max.data_ptr(),
                                  self.ring.data_ptr(), st)
        self._store_call(L, *fin, self.rec_x.data_ptr(), self.rec_a.data_ptr(),
                         self.rec_r.data_ptr(), self.capacity, self.mem.data_ptr(),
                         self.mem_len.data_ptr(), self.mem_term.data_ptr(), self.ring.data_ptr(), st)

    def _overflow_look(self, clock):
        if clock % 256 == 0 and int(self.stats[3]):  # (one look every 256 updates)
            raise RuntimeError(f"recurrent DQN episode records overflowed L = {self.L} steps "
                               "(mz_ppo_scan stats[3])")

    def _window_settings(self):
        """T with the burn-in and the initial state (a population's: the per-learner lists); None
        without windows."""
        if self.window is None:
            return None
        return {"window": self.window, "burn_in": copy.copy(self.burn_in),
                "initial_state": copy.copy(self.initial_state)}

    def _check_window_settings(self, sd):
        # (a checkpoint from before the window option has no "window" key: window=None)
        if sd.get("window") != self._window_settings():
            raise ValueError(f"the checkpoint's replay windows {sd.get('window')} differ from this "
                             f"{self._KIND}'s {self._window_settings()}")

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


class VectorRecurrentDQNTrainer(RecurrentDQNBase):
    _FORMAT = FORMAT
    _SHAPE = ("L", "capacity")
    _COUNTERS = ("seed", "steps_done", "counter", "updates", "filled")

    def __init__(self, env, device, lr=1e-3, starting_epsilon=0.9, final_epsilon=0.05,
                 epsilon_decay=1000.0, discount_factor=0.99, batch_size=32, memory_size=20000,
                 target_update_frequency=10, explore_actions=4, train_every=1, seed=0, bank=True,
                 curriculum=False, growth=None, algorithm="r-prim", bank_candidates=1, window=None,
                 burn_in=0, initial_state="stored", archive=None, priority_alpha=None,
                 priority_beta=0.6, priority_eta=0.9, priority_eps=1e-3):
        """archive: EpisodicTrainer's explored-maze pool (None: off). priority_alpha: prioritized
        replay windows (departures 10-12; None: off, nothing of it is allocated or launched);
        priority_beta: a number, or (beta0, beta1, updates) for a linear schedule over the update
        count."""
        check_window(window, burn_in, initial_state)
        check_priority(window, priority_alpha, priority_beta, priority_eta, priority_eps)
        if batch_size < 1 or memory_size < batch_size or train_every < 1 or \
                target_update_frequency < 1 or explore_actions not in (1, 2, 3, 4):
            raise ValueError("batch_size >= 1, memory_size >= batch_size, train_every >= 1, "
                             "target_update_frequency >= 1, explore_actions in 1..4")
        super().__init__(env, device, bank=bank, curriculum=curriculum, growth=growth,
                         algorithm=algorithm, bank_candidates=bank_candidates, archive=archive)
        torch.manual_seed(seed)
        self.source_net = DQN(6, 4, HIDDEN, self.device)
        self.target_net = DQN(6, 4, HIDDEN, self.device)
        flatten_params(self.target_net)
        flatten_grads(self.source_net)
        copy_flat(self.target_net, self.source_net)
        for p in self.source_net.parameters():
            p.grad = grad_segment(p)
        self.opt = FlatAdamW(self.source_net, lr=lr, clamp=1.0)
        self._ps, self._pt = param_ptrs(self.source_net), param_ptrs(self.target_net)
        self._pg = (C.c_void_p * 6)(*[p.grad.data_ptr() for p in self.source_net.parameters()])
        self.lr, self.gamma = float(lr), float(discount_factor)
        self.starting_epsilon, self.final_epsilon = float(starting_epsilon), float(final_epsilon)
        self.epsilon_decay = float(epsilon_decay)
        self.batch_size, self.capacity = int(batch_size), int(memory_size)
        self.target_update_frequency = int(target_update_frequency)
        self.explore_actions, self.train_every = int(explore_actions), int(train_every)
        self.seed = int(seed)
        self.window = None if window is None else int(window)
        self.burn_in, self.initial_state = int(burn_in), initial_state
        if priority_alpha is not None:
            self.priority_alpha = float(priority_alpha)
            self.priority_beta = float(priority_beta) if isinstance(priority_beta, (int, float)) \
                else (float(priority_beta[0]), float(priority_beta[1]), int(priority_beta[2]))
            self.priority_eta, self.priority_eps = float(priority_eta), float(priority_eps)
        self.steps_done = 0   # the eps clock
        self.counter = 0      # vector steps (the exploration draws' counter)
        self.updates = 0
        self.filled = 0       # the host's lower bound of the ring's count
        self.stored = self.window is not None and initial_state == "stored"
        self._alloc(None, self.stored)
        self.last_lr = None

    def epsilon(self):
        return epsilon_at(self.steps_done, self.starting_epsilon, self.final_epsilon,
                          self.epsilon_decay)

    def update_steps_done(self):
        self.steps_done = self.steps_done // 2

    def _act(self):
        env = self.env
        eps = min(max(self.epsilon(), 0.0), 1.0)
        self.steps_done += 1
        if self.stored:
            N.check(self.lib.mz_drqn_snapshot(
                HIDDEN, env.num_envs, self.L, self.window, self.t.data_ptr(), self.h.data_ptr(),
                self.c.data_ptr(), self.snap_rec.data_ptr(), self._stream()))
        N.check(self.lib.mz_drqn_act(
            self._ps, HIDDEN, env.obs6.data_ptr(), env.num_envs, self.L, eps, self.explore_actions,
            self.seed & U64, self.counter & U64, self.t.data_ptr(), self.h.data_ptr(),
            self.c.data_ptr(), self.rec_x.data_ptr(), self.rec_a.data_ptr(),
            self.act_out.data_ptr(), None, self._stream()))
        self.counter += 1

    def _snap_store_call(self, *tail):
        N.check(self.lib.mz_drqn_snap_store(HIDDEN, self.env.num_envs, *tail))

    def _prio_store_call(self, *tail):
        N.check(self.lib.mz_drqn_prio_store(HIDDEN, self.env.num_envs, *tail))

    def _store_call(self, *tail):
        env = self.env
        N.check(self.lib.mz_drqn_store(env.obs6.data_ptr(), env.terminated.data_ptr(),
                                       env.num_envs, *tail))

    def sample(self):
        """E distinct slots and the directory (d_slot, d_len, d_off, d_tot), keyed by the update
        count; windowed: the same slots, one window each and the window directory (wdir, d_off,
        d_tot). Prioritized: E windows in proportion to their mass, the same directory, and the
        importance weights (isw)."""
        if self.priority_alpha is not None:
            N.check(self.lib.mz_drqn_prio_sample(
                self.seed & U64, self.updates & U64, HIDDEN, self.batch_size, self.L, self.window,
                self.burn_in, self.capacity, self.mem_len.data_ptr(), self.mem_prio.data_ptr(),
                self.mem_psum.data_ptr(), self.wdir.data_ptr(), self.d_off.data_ptr(),
                self.d_tot.data_ptr(), self.isw.data_ptr(), self.beta(), self._stream()))
            return
        if self.window is not None:
            N.check(self.lib.mz_drqn_window_sample(
                self.seed & U64, self.updates & U64, HIDDEN, self.batch_size, self.L, self.window,
                self.burn_in, self.capacity, self.filled, self.ring.data_ptr(),
                self.mem_len.data_ptr(), self.wdir.data_ptr(), self.d_off.data_ptr(),
                self.d_tot.data_ptr(), self._stream()))
            return
        N.check(self.lib.mz_drqn_sample(
            self.seed & U64, self.updates & U64, self.batch_size, self.L, self.capacity,
            self.filled, self.ring.data_ptr(), self.mem_len.data_ptr(), self.d_slot.data_ptr(),
            self.d_len.data_ptr(), self.d_off.data_ptr(), self.d_tot.data_ptr(), self._stream()))

    def update(self, lr):
        """One optimizer step on the directory's episodes at learning rate `lr`; the loss stays on
        the device (self.loss)."""
        E, L, st = self.batch_size, self.L, self._stream()
        dirs = (self.d_slot.data_ptr(), self.d_len.data_ptr(), self.d_off.data_ptr(),
                self.d_tot.data_ptr())
        self.opt.param_groups[0]["lr"].fill_(float(lr))
        if self.window is not None:
            self._window_update(st)
            self.opt.step()
            return
        N.check(self.lib.mz_drqn_seq_forward(
            self._pt, HIDDEN, 1, E, L, self.capacity, self.gamma, self.mem.data_ptr(),
            self.mem_term.data_ptr(), *dirs, self.qmax.data_ptr(), None, None, None, None, None,
            st))
        N.check(self.lib.mz_drqn_seq_forward(
            self._ps, HIDDEN, 0, E, L, self.capacity, self.gamma, self.mem.data_ptr(),
            self.mem_term.data_ptr(), *dirs, self.qmax.data_ptr(), self.stash.data_ptr(),
            self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(), st))
        N.check(self.lib.mz_drqn_seq_backward(
            self._ps, HIDDEN, E, L, self.capacity, self.mem.data_ptr(), *dirs,
            self.stash.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(),
            self.gpart.data_ptr(), self._pg, self.loss.data_ptr(), st))
        self.opt.step()

    def _window_update(self, st):
        E, L, T, K = self.batch_size, self.L, self.window, self.burn_in
        state = self.mem_state.data_ptr() if self.stored else None
        dirs = (self.wdir.data_ptr(), self.d_off.data_ptr(), self.d_tot.data_ptr())
        N.check(self.lib.mz_drqn_window_forward(
            self._pt, HIDDEN, 1, E, L, T, K, self.capacity, self.gamma, self.mem.data_ptr(),
            self.mem_term.data_ptr(), state, *dirs, self.qmax.data_ptr(), None, None, None, None,
            None, st))
        N.check(self.lib.mz_drqn_window_forward(
            self._ps, HIDDEN, 0, E, L, T, K, self.capacity, self.gamma, self.mem.data_ptr(),
            self.mem_term.data_ptr(), state, *dirs, self.qmax.data_ptr(), self.stash.data_ptr(),
            self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(), st))
        if self.priority_alpha is not None:  # the new masses; d and ep_loss times the weights
            N.check(self.lib.mz_drqn_prio_update(
                HIDDEN, E, L, T, self.capacity, *dirs, self.qa.data_ptr(), self.y.data_ptr(),
                self.d.data_ptr(), self.ep_loss.data_ptr(), self.isw.data_ptr(),
                self.priority_alpha, self.priority_eta, self.priority_eps,
                self.mem_prio.data_ptr(), self.mem_psum.data_ptr(), self.prio_max.data_ptr(), st))
        N.check(self.lib.mz_drqn_window_backward(
            self._ps, HIDDEN, E, L, T, K, self.capacity, self.mem.data_ptr(), *dirs,
            self.stash.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(),
            self.gpart.data_ptr(), self._pg, self.loss.data_ptr(), st))

    def _update(self):
        self._overflow_look(self.updates)
        self.last_lr = cosine_lr(self.updates, self.lr, T_MAX, ETA_MIN)
        self.sample()
        self.update(self.last_lr)
        self.updates += 1
        if self.updates % self.target_update_frequency == 0:
            copy_flat(self.target_net, self.source_net)

    def vector_step(self):
        self._act()
        self.env.step(self.act_out)
        self._scan_store()
        self._reset_winners()
        if self.filled < self.batch_size:  # (only until the first batch exists: one sync a step)
            self.filled = int(self.ring[1])
        if self.filled >= self.batch_size and self.counter % self.train_every == 0:
            self._update()

    def beta(self):
        """The importance exponent of the coming update: priority_beta, or its linear schedule
        over the update count (computed here, on the host)."""
        b = self.priority_beta
        if isinstance(b, float):
            return b
        return b[0] + (b[1] - b[0]) * min(self.updates / b[2], 1.0)

    def _log_fields(self):
        if self.priority_alpha is None:
            return {"loss": float(self.loss)}
        return {"loss": float(self.loss), "prio_max": int(self.prio_max) / PRIO_ONE,
                "mean_weight": float(self.isw.mean())}

    def _priority_settings(self):
        if self.priority_alpha is None:
            return None
        b = self.priority_beta
        return {"alpha": self.priority_alpha, "beta": b if isinstance(b, float) else list(b),
                "eta": self.priority_eta, "eps": self.priority_eps}

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
        in-flight and the filled slots' snapshots."""
        sd, o = self._save_common(), self.opt
        n = int(self.ring[1])
        if self.window is not None:
            sd["window"] = self._window_settings()
        if self.stored:
            sd["snap_rec"] = self.snap_rec.clone()
            sd["mem_state"] = self.mem_state[:n].clone()
        if self.priority_alpha is not None:
            sd["priority"] = self._priority_settings()
            sd["mem_prio"] = self.mem_prio[:n].clone()
            sd["mem_psum"] = self.mem_psum[:n].clone()
            sd["prio_max"] = self.prio_max.clone()
        sd.update({k: getattr(self, k).clone() for k in self._OWN})
        sd.update({k: getattr(self, k)[:n].clone() for k in ("mem", "mem_len", "mem_term")})
        sd["source"] = {k: v.clone() for k, v in self.source_net.state_dict().items()}
        sd["target"] = {k: v.clone() for k, v in self.target_net.state_dict().items()}
        sd["opt"] = {"exp_avg": o.exp_avg.clone(), "exp_avg_sq": o.exp_avg_sq.clone(),
                     "step": o._step_buf.clone(), "lr": o.param_groups[0]["lr"].clone()}
        return sd

    def load_state_dict(self, sd):
        self._check_window_settings(sd)
        # (a checkpoint of a trainer without priorities has no "priority" key: priority_alpha=None)
        if sd.get("priority") != self._priority_settings():
            raise ValueError(f"the checkpoint's prioritized replay {sd.get('priority')} differs "
                             f"from this trainer's {self._priority_settings()}")
        self._load_common(sd)
        with torch.no_grad():
            self.source_net.load_state_dict(sd["source"])
            self.target_net.load_state_dict(sd["target"])
        o = self.opt
        o.exp_avg.copy_(sd["opt"]["exp_avg"])
        o.exp_avg_sq.copy_(sd["opt"]["exp_avg_sq"])
        o._step_buf.copy_(sd["opt"]["step"])
        o.param_groups[0]["lr"].copy_(sd["opt"]["lr"])
        for k in self._OWN:
            getattr(self, k).copy_(sd[k])
        n = sd["mem"].shape[0]
        for k in ("mem", "mem_len", "mem_term"):
            getattr(self, k)[:n].copy_(sd[k])
        if self.stored:
            self.snap_rec.copy_(sd["snap_rec"])
            self.mem_state[:n].copy_(sd["mem_state"])
        if self.priority_alpha is not None:
            self.mem_prio[:n].copy_(sd["mem_prio"])
            self.mem_psum[:n].copy_(sd["mem_psum"])
            self.prio_max.copy_(sd["prio_max"])


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
