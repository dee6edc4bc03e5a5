"""Populations of recurrent DQN learners: P independent VectorRecurrentDQNTrainers advanced by the
same launches (csrc/mz_drqn.hip's kernels, each of which serves P learners; csrc/mz_optim.hip
k_adamw_pop), so P seeds or P hyper-parameter settings of agents/lstm_dqn_agent.py cost about one
run's launches. The buffers, the scan and store of a vector step and the window settings are
drqn_trainer.RecurrentDQNBase's, shared with that trainer.

A population is P learners over B = P b instances; learner p owns the block [p b, (p + 1) b).
Shared: the env, L = episode_bound, batch_size E, memory_size (capacity, in episodes),
train_every, explore_actions. Per learner (a scalar or a length-P sequence): lr, discount_factor,
starting_epsilon, final_epsilon, epsilon_decay, target_update_frequency, seed.

Learner p is, by definition and bit for bit, what VectorRecurrentDQNTrainer (drqn_trainer.py: its
six departures, its accumulation order, Philox streams and ring semantics) would be on its b
instances with its hyper-parameters and seed: every stage has one kernel, which runs its device
code on learner p's rows, and that trainer's entry points launch it with P = 1. The acting draw of
instance i is keyed by (seed_p, counter, i - p b), the sample by (seed_p, updates_p); P = 1 is
that trainer.

Layout. Parameters, gradients and AdamW moments are flat [P][5252] f32, a row in state_dict order;
h, c stay [32][B]; the replay memory is [P][capacity][L + 1][8] words with mem_len / mem_term
[P][capacity] and an int64 ring [P][2] (head, count); an update's directory is [P][E] and its row
buffers [P][E (L + 1)].

The learners never couple on the device: each has its own ring, nets, moments and step count, its
own eps clock steps_done[p] and its own update count updates[p] (its cosine schedule and target
sync). A learner starts updating at the first vector step at which its own ring holds >= E
episodes. The host reads the P ring counts once per vector step only until every learner has its
first batch; from then on it knows every updates[p], uploads the per-update scalars (lr[p] from
cosine_lr in float64 as the single trainer, the due mask, the sync mask, the sample counters) as
one small array, and a vector step makes no device -> host read (beyond the single trainer's look
at the overflow counter every 256 updates).

Replay windows (window=T, burn_in, initial_state; window=None, the default, is the population
above: no new launch, the same bits, the same checkpoint keys). T is shared by the population: it
fixes the layouts (ceil(L / T) snapshots per episode, row buffers [P][E (min(T, L) + 2)], a window
directory [P][5][E]). burn_in and initial_state are per learner (a scalar or a length-P sequence),
each K_p a multiple of T, checked before anything touches the GPU and uploaded once. Learner p is
VectorRecurrentDQNTrainer(window=T, burn_in=K_p, initial_state=S_p) on its block, bit for bit
(its departures 7-9): its episode draw is keyed by (seed_p, updates_p), its window draw by
(seed_p, updates_p, position in the batch). mz_drqn_snapshot runs over all P b instances and the
state memory [P][capacity][ceil(L / T)][64] exists when at least one learner is "stored"; a "zero"
learner never reads it. A checkpoint then also holds T and the two per-learner lists and, when
stored, snap_rec and each ring's filled slots of mem_state; it loads only into a population with
the same window settings.

Prioritized windows (priority_alpha, priority_beta, priority_eta, priority_eps: each a value or a
list of P; with every alpha None, the default, this is the population above: nothing of it is
allocated or launched, the same bits, the same checkpoint keys). An entry of priority_alpha may be
None: that learner keeps the uniform-per-episode window sampler. priority_beta is a number, a tuple
(beta0, beta1, updates) - one schedule for every learner - or a list of P numbers or such triples;
a learner's schedule runs over its own update count and is evaluated on the host, as the single
trainer's beta(), and goes up with the per-update scalars. Learner p with an alpha is
VectorRecurrentDQNTrainer(window=T, priority_alpha=a_p, priority_beta=b_p, priority_eta=h_p,
priority_eps=x_p) on its block, bit for bit (its departures 10-12). Then mem_prio
[P][capacity][ceil(L / T)], mem_psum [P][capacity], prio_max [P] and isw [P][E] exist for all
learners (a uniform learner's masses are kept by the store launch and never read). Per update:
mz_drqn_pop_prio_sample under the mask due-and-prioritized, mz_drqn_pop_window_sample under
due-and-uniform (each launched only where its mask has an entry; the uniform sampler's smallest
fill is taken over its own mask), and mz_drqn_pop_prio_update under the first mask between the
source forward and the backward. The forward, backward, reduce, AdamW and sync launches run under
the one due mask, unchanged. A checkpoint then also holds the per-learner settings, each ring's
filled slots of mem_prio and mem_psum, and prio_max; it loads only into a population with the same
settings, and a checkpoint without them only into a population without priorities.

curriculum="global" counts wins across all instances and would couple the learners: it is refused.
With bank=False a learner's whole run is independent of the other learners, bit for bit. With the
winner bank the maze a winner receives depends on how many instances of other learners won before
it, so the learners then share the stream of replacement mazes.
"""
import ctypes as C

import numpy as np
import torch

from .. import _native as N
from ..agents.lstm_dqn_agent import DQN, ETA_MIN, HIDDEN, T_MAX, epsilon_at
from ..agents.rf_agent import cosine_lr
from .drqn_trainer import (EVAL_KEY, PARAMS, PRIO_ONE, ROW, STASH, U64, RecurrentDQNBase,
                           _Evaluator, check_priority, check_window)
from .episodic import episode_bound

FORMAT = "mazerl.VectorRecurrentDQNPopulation/1"
KEYS = ("lstm_cell.weight_ih", "lstm_cell.weight_hh", "lstm_cell.bias_ih", "lstm_cell.bias_hh",
        "fc.weight", "fc.bias")
SHAPES = ((128, 6), (128, 32), (128,), (128,), (4, 32), (4,))
PER_LEARNER = ("lr", "discount_factor", "starting_epsilon", "final_epsilon", "epsilon_decay",
               "target_update_frequency", "seed")
BETAS, ADAM_EPS, WEIGHT_DECAY, CLAMP = (0.9, 0.999), 1e-8, 1e-2, 1.0


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


def footprint(P, B, L, E, capacity, window=None, stored=False, prio=False):
    """Bytes of the replay rings, the in-flight records, and an update's stash and row buffers;
    windowed: the row buffers hold E (min(T, L) + 2) rows, and with stored state the state memory
    (P capacity ceil(L / T) snapshots of 256 B) and the in-flight snapshots are added; prioritized:
    the masses (P capacity ceil(L / T) words and a 64-bit sum per slot), prio_max, the importance
    weights and the three float64 settings per learner."""
    rows = E * (L + 1) if window is None else E * (min(window, L) + 2)
    ring = P * capacity * ((L + 1) * ROW * 4 + 8)
    records = B * ((L + 1) * 6 * 4 + L * 4 + L * 8)
    update = P * (rows * (STASH + 4) * 4 + E * (PARAMS * 4 + 8 + 16))
    out = {"replay": ring, "records": records, "update": update,
           "total": ring + records + update}
    if window is not None:
        snaps = ((L - 1) // window + 1) * 2 * HIDDEN * 4 if stored else 0
        out["state"], out["snap_rec"] = P * capacity * snaps, B * snaps
        out["update"] += P * 5 * E * 4
        out["total"] = ring + records + out["update"] + out["state"] + out["snap_rec"]
    if prio:
        out["prio"] = P * (capacity * (((L - 1) // window + 1) * 4 + 8) + 4 + E * 4 + 3 * 8)
        out["total"] += out["prio"]
    return out


class _LearnerView:
    """What drqn_trainer._Evaluator reads of a trainer, for one learner of a population."""

    def __init__(self, pop, p):
        self.lib, self.explore_actions, self.seed = pop.lib, pop.explore_actions, pop.seed[p]
        self._rows = pop.src  # keeps the buffer alive
        base, off = pop.src[p].data_ptr(), 0
        ptrs = []
        for s in SHAPES:
            ptrs.append(base + 4 * off)
            off += int(np.prod(s))
        self._ps = (C.c_void_p * 6)(*ptrs)


class VectorRecurrentDQNPopulation(RecurrentDQNBase):
    _FORMAT = FORMAT
    _SHAPE = ("L", "capacity", "P")
    _COUNTERS = ("counter", "launches")
    _KIND = "population"

    def __init__(self, env, device, learners=1, lr=1e-3, starting_epsilon=0.9, final_epsilon=0.05,
                 epsilon_decay=1000.0, discount_factor=0.99, batch_size=32, memory_size=20000,
                 target_update_frequency=10, explore_actions=4, train_every=1, seed=0, bank=True,
                 curriculum=False, growth=None, algorithm="r-prim", bank_candidates=1, window=None,
                 burn_in=0, initial_state="stored", archive=None, priority_alpha=None,
                 priority_beta=0.6, priority_eta=0.9, priority_eps=1e-3):
        """archive (None: off): an int C or a MazePoolSet of this env with one group per learner
        — every learner's explored mazes in a pool of C entries of its own, all filled by one
        launch per vector step (evaluate_explored_all). priority_alpha .. priority_eps: prioritized
        replay windows per learner (the module's docstring; every alpha None: off)."""
        P = int(learners)
        if P < 1 or env.num_envs % P:
            raise ValueError(f"env.num_envs {env.num_envs} must be a multiple of learners {P} >= 1")
        if curriculum is True or curriculum == "global":
            raise ValueError('curriculum="global" counts wins across all instances and would '
                             'couple the learners; use False or "per-instance"')
        same = lambda v: v  # noqa: E731 (check_window wants the values as they were given)
        self.burn_in = per_learner(burn_in, P, "burn_in", same)
        self.initial_state = per_learner(initial_state, P, "initial_state", same)
        for K, S in zip(self.burn_in, self.initial_state):
            check_window(window, K, S)
        self.window = None if window is None else int(window)
        self.stored = [self.window is not None and S == "stored" for S in self.initial_state]
        self._priority(P, window, priority_alpha, priority_beta, priority_eta, priority_eps)
        self.tuf = per_learner(target_update_frequency, P, "target_update_frequency", int)
        if batch_size < 1 or memory_size < batch_size or train_every < 1 or min(self.tuf) < 1 or \
                explore_actions not in (1, 2, 3, 4):
            raise ValueError("batch_size >= 1, memory_size >= batch_size, train_every >= 1, "
                             "target_update_frequency >= 1, explore_actions in 1..4")
        self.P, self.b = P, env.num_envs // P
        self.lr = per_learner(lr, P, "lr")
        self.gamma = per_learner(discount_factor, P, "discount_factor")
        self.starting_epsilon = per_learner(starting_epsilon, P, "starting_epsilon")
        self.final_epsilon = per_learner(final_epsilon, P, "final_epsilon")
        self.epsilon_decay = per_learner(epsilon_decay, P, "epsilon_decay")
        self.seed = per_learner(seed, P, "seed", int)
        self.batch_size, self.capacity = int(batch_size), int(memory_size)
        self.explore_actions, self.train_every = int(explore_actions), int(train_every)
        B, E = env.num_envs, self.batch_size
        L = episode_bound(env.max_dim, env.toroidal)
        need = footprint(P, B, L, E, self.capacity, self.window, any(self.stored), any(self.prio))
        dev = torch.device(device)
        if dev.type == "cuda":
            free, _ = torch.cuda.mem_get_info(dev)
            if need["total"] > free:
                raise MemoryError(
                    f"{P} learners x {self.capacity} episodes of {L + 1} rows need "
                    f"{need['replay'] / 2 ** 30:.2f} GiB of replay memory and "
                    + (f"{need['state'] / 2 ** 30:.2f} GiB of state memory (mem_state) with "
                       f"{need['snap_rec'] / 2 ** 30:.2f} GiB of in-flight snapshots (snap_rec) and "
                       if any(self.stored) else "") +
                    (f"{need['prio'] / 2 ** 30:.2f} GiB of window priorities (mem_prio, mem_psum) "
                     "and " if any(self.prio) else "") +
                    f"{need['total'] / 2 ** 30:.2f} GiB in all; {free / 2 ** 30:.2f} GiB are free. "
                    "Lower memory_size or learners.")
        super().__init__(env, device, bank=bank, curriculum=curriculum, growth=growth,
                         algorithm=algorithm, bank_candidates=bank_candidates, archive=archive,
                         archive_groups=P)
        kw = dict(device=self.device)
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.src = torch.zeros(P, PARAMS, dtype=f32, **kw)
        for p in range(P):  # learner p's initial net: the single trainer's under its seed
            torch.manual_seed(self.seed[p])
            net = DQN(6, 4, HIDDEN, self.device)
            DQN(6, 4, HIDDEN, self.device)  # (the single trainer's target net: the same draws)
            self.load_learner(p, net.state_dict())
        self.tgt = self.src.clone()
        self.grad = torch.zeros_like(self.src)
        self.exp_avg = torch.zeros_like(self.src)
        self.exp_avg_sq = torch.zeros_like(self.src)
        self.step = torch.zeros(P, dtype=f32, **kw)  # the optimizer's step counts
        self.steps_done = [0] * P  # the eps clocks
        self.counter = 0           # vector steps (the exploration draws' counter)
        self.launches = 0          # update launches (the overflow look's clock)
        self.updates = [0] * P
        self.filled = [0] * P      # the host's lower bounds of the rings' counts
        self.gamma_dev = torch.tensor(self.gamma, dtype=f32, **kw)
        self.seed_dev = torch.tensor([_signed(s) for s in self.seed], dtype=i64, **kw)
        self.eps_dev = torch.zeros(P, dtype=f32, **kw)
        # the per-update scalars, one upload: sample counters (int64), due, sync, lr (f32 bits);
        # prioritized: then the two samplers' masks and every learner's beta (float64)
        self.upd = torch.zeros((9 * P + P % 2) if any(self.prio) else 5 * P, dtype=i32, **kw)
        self.cnt_dev = self.upd[:2 * P].view(i64)
        self.due_dev, self.sync_dev = self.upd[2 * P:3 * P], self.upd[3 * P:4 * P]
        self.lr_dev = self.upd[4 * P:5 * P].view(f32)
        self._alloc(P, any(self.stored))
        if any(self.prio):
            self.due_prio_dev, self.due_uni_dev = self.upd[5 * P:6 * P], self.upd[6 * P:7 * P]
            self.beta_dev = self.upd[7 * P + P % 2:].view(torch.float64)  # (8-byte aligned)
            f64 = lambda vs, ph: torch.tensor(  # noqa: E731 (a uniform learner: a valid placeholder)
                [ph if v is None else v for v in vs], dtype=torch.float64, **kw)
            self.prio_alpha_dev = f64(self.priority_alpha, 0.0)
            self.prio_eta_dev = f64(self.priority_eta, 0.0)
            self.prio_eps_dev = f64(self.priority_eps, 1.0)
        self._prio_due = False  # whether the update under way has a due prioritized learner
        if self.window is not None:
            self.burn_in_dev = torch.tensor(self.burn_in, dtype=i32, **kw)
            self.stored_dev = torch.tensor([int(s) for s in self.stored], dtype=i32, **kw)
        self.last_lr = [None] * P
        self.last_due = [False] * P  # the learners the last vector step updated

    def _priority(self, P, window, alpha, beta, eta, eps):
        """The per-learner priority settings, checked learner by learner before anything touches
        the GPU: prio[p] (whether learner p is prioritized) and, when any is, priority_alpha / _beta
        / _eta / _eps as lists of P (None throughout for a uniform learner)."""
        same = lambda v: v  # noqa: E731 (check_priority wants the values as they were given)
        alpha = per_learner(alpha, P, "priority_alpha", same)
        beta = [beta] * P if isinstance(beta, tuple) else per_learner(beta, P, "priority_beta", same)
        eta = per_learner(eta, P, "priority_eta", same)
        eps = per_learner(eps, P, "priority_eps", same)
        for a, b, h, x in zip(alpha, beta, eta, eps):
            check_priority(window, a, b, h, x)
        self.prio = [a is not None for a in alpha]
        if not any(self.prio):
            return
        on = lambda vs, f: [f(v) if q else None for v, q in zip(vs, self.prio)]  # noqa: E731
        self.priority_alpha = on(alpha, float)
        self.priority_beta = on(beta, lambda b: float(b) if isinstance(b, (int, float)) else
                                (float(b[0]), float(b[1]), int(b[2])))
        self.priority_eta, self.priority_eps = on(eta, float), on(eps, float)

    def beta(self, p):
        """Learner p's importance exponent at its coming update (the single trainer's beta())."""
        b = self.priority_beta[p]
        if isinstance(b, float):
            return b
        return b[0] + (b[1] - b[0]) * min(self.updates[p] / b[2], 1.0)

    def _priority_settings(self):
        if self.priority_alpha is None:
            return None
        return {"alpha": list(self.priority_alpha),
                "beta": [list(b) if isinstance(b, tuple) else b for b in self.priority_beta],
                "eta": list(self.priority_eta), "eps": list(self.priority_eps)}

    # ---- per-learner access -------------------------------------------------------------------
    def memory_bytes(self):
        """The replay, record, stash and row-buffer footprint in bytes (footprint())."""
        return footprint(self.P, self.env.num_envs, self.L, self.batch_size, self.capacity,
                         self.window, any(self.stored), any(self.prio))

    def epsilon(self, p):
        return epsilon_at(self.steps_done[p], self.starting_epsilon[p], self.final_epsilon[p],
                          self.epsilon_decay[p])

    def update_steps_done(self, p=None):
        for k in range(self.P) if p is None else (int(p),):
            self.steps_done[k] = self.steps_done[k] // 2

    def learner_state_dict(self, p):
        """Learner p's source net as the state_dict agents/lstm_dqn_agent.DQN and the reference's
        DQN load."""
        row, off, sd = self.src[int(p)], 0, {}
        for k, s in zip(KEYS, SHAPES):
            n = int(np.prod(s))
            sd[k] = row[off:off + n].view(s).clone()
            off += n
        return sd

    def load_learner(self, p, state_dict):
        """Learner p's source net from a DQN state_dict (its target net follows at its next sync)."""
        row = torch.cat([state_dict[k].detach().to(self.device, torch.float32).reshape(-1)
                         for k in KEYS])
        if row.numel() != PARAMS:
            raise ValueError("not an LSTMCell(6, 32) + Linear(32, 4) state_dict")
        self.src[int(p)].copy_(row)

    def evaluator(self, p):
        """Learner p as a learner for vector_trainer.evaluate / evaluate_plain (greedy actions
        from a per-row (h, c) that starts at zero)."""
        return _Evaluator(_LearnerView(self, int(p)))

    def evaluate_all(self, num_mazes, dim, algorithm="r-prim", seed=0x7E57, toroidal=False):
        """The P greedy win-rates from one rollout of P num_mazes rows on a plain env: every
        learner plays the same num_mazes fresh mazes (those evaluate_plain plays under this seed)
        through the population act in evaluation mode."""
        from ..vector_env import VectorMazeEnv
        P, n = self.P, int(num_mazes)
        env = VectorMazeEnv(P * n, dim, toroidal=toroidal, enrich=False, device=self.device,
                            algorithm=algorithm, seed=seed, pos=False, done_list=False,
                            generate=False)
        for p in range(P):  # an instance's maze is keyed by seed + its index
            ids = torch.arange(p * n, (p + 1) * n, dtype=torch.int32, device=self.device)
            env.generate(env_ids=ids, algorithm=algorithm, seed=(seed - p * n) & U64)
        env.reset()
        won = self._greedy_blocks(env, n, episode_bound(dim, toroidal) + 1)
        rates = won.view(P, n).float().mean(dim=1).tolist()
        env.close()
        return rates

    def _greedy_blocks(self, env, n, limit):
        """One greedy episode per row of `env`, P blocks of n rows, block p played by learner p
        from zero state through the population act in evaluation mode. Returns the rows that won."""
        P = self.P
        kw = dict(device=self.device)
        h = torch.zeros(HIDDEN, P * n, dtype=torch.float32, **kw)
        c = torch.zeros_like(h)
        t = torch.zeros(P * n, dtype=torch.int32, **kw)
        acts = torch.zeros(P * n, dtype=torch.int32, **kw)
        eps = torch.zeros(P, dtype=torch.float32, **kw)
        seeds = torch.tensor([_signed(s ^ EVAL_KEY) for s in self.seed], dtype=torch.int64, **kw)

        def act(k):
            N.check(self.lib.mz_drqn_pop_act(
                self.src.data_ptr(), HIDDEN, P, n, env.obs6.data_ptr(), 0, eps.data_ptr(),
                self.explore_actions, seeds.data_ptr(), k, t.data_ptr(), h.data_ptr(),
                c.data_ptr(), None, None, acts.data_ptr(), None, self._stream()))
            t.fill_(1)
            return acts

        won, _ = self.greedy_rollout(env, act, limit)
        return won

    def evaluate_explored_all(self, n=None):
        """The reference's test(n, new=False) for every learner at once: the P greedy win-rates
        on each learner's own oldest n explored mazes (entries 0 .. n - 1 of its pool; n None: the
        smallest `held` over the learners), from one rollout of P n rows — block p filled from
        pool p by one load launch — through the population act in evaluation mode. Learner p's
        rate is evaluate_explored(self.evaluator(p), self.archive.pool(p), n)'s. An entry the load
        refuses raises a RuntimeError (a corrupt pool: the result is void)."""
        from ..vector_env import VectorMazeEnv
        pools = self.archive
        if pools is None:
            raise ValueError("this population keeps no explored-maze pools (archive=)")
        P, C = self.P, pools.capacity
        low = min(pools.held.tolist())
        n = low if n is None else int(n)
        if n < 1 or n > low:
            raise ValueError(f"n = {n}: the emptiest pool holds {low} entries")
        env = VectorMazeEnv(P * n, pools.pitch, toroidal=pools.toroidal, enrich=False,
                            device=self.device, pos=False, done_list=False)
        k = torch.arange(P * n, dtype=torch.int32, device=self.device)
        pools.load(env, (k // n) * C + k % n)  # row p n + j <- pool p's entry j
        env.reset()
        won = self._greedy_blocks(env, n, episode_bound(pools.pitch, pools.toroidal) + 1)
        wins = won.view(P, n).sum(dim=1)
        *wins, refused = torch.cat([wins, pools.errors.to(wins.dtype)]).tolist()
        env.close()
        if refused:
            raise RuntimeError(f"{refused} pool entries were refused by mz_archive_load "
                               f"(errors): a pool is corrupt, the result is void")
        return [w / n for w in wins]

    # ---- a vector step --------------------------------------------------------------------------
    def _act(self):
        env = self.env
        eps = [min(max(self.epsilon(p), 0.0), 1.0) for p in range(self.P)]
        for p in range(self.P):
            self.steps_done[p] += 1
        self.eps_dev.copy_(torch.tensor(eps, dtype=torch.float32))
        if any(self.stored):  # (all P b instances: a zero-state learner's snapshots are never read)
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

    def _snap_store_call(self, *tail):
        N.check(self.lib.mz_drqn_pop_snap_store(HIDDEN, self.P, self.b, *tail))

    def _prio_store_call(self, *tail):
        N.check(self.lib.mz_drqn_pop_prio_store(HIDDEN, self.P, self.b, *tail))

    def _store_call(self, *tail):
        env = self.env
        N.check(self.lib.mz_drqn_pop_store(env.obs6.data_ptr(), env.terminated.data_ptr(), self.P,
                                           self.b, *tail))

    def _upload(self, due, sync, lr):
        P = self.P
        buf = np.zeros(self.upd.numel(), np.int32)
        buf[:2 * P].view(np.int64)[:] = self.updates
        buf[2 * P:3 * P] = due
        buf[3 * P:4 * P] = sync
        buf[4 * P:5 * P].view(np.float32)[:] = lr
        if any(self.prio):  # the two samplers' masks; beta_p at learner p's own update count
            buf[5 * P:6 * P] = [d and q for d, q in zip(due, self.prio)]
            buf[6 * P:7 * P] = [d and not q for d, q in zip(due, self.prio)]
            buf[7 * P + P % 2:].view(np.float64)[:] = [self.beta(p) if q else 0.0
                                                       for p, q in enumerate(self.prio)]
            self._prio_due = bool(buf[5 * P:6 * P].any())
        self.upd.copy_(torch.from_numpy(buf))

    def sample(self, due):
        """E distinct slots and the directory of every due learner, keyed by its update count;
        windowed: the same slots, one window each and the learner's window directory; a prioritized
        learner: E windows in proportion to their mass and its importance weights."""
        mask = self.due_dev
        if any(self.prio):
            if self._prio_due:
                N.check(self.lib.mz_drqn_pop_prio_sample(
                    self.seed_dev.data_ptr(), self.cnt_dev.data_ptr(), self.burn_in_dev.data_ptr(),
                    self.beta_dev.data_ptr(), self.due_prio_dev.data_ptr(), HIDDEN, self.P,
                    self.batch_size, self.L, self.window, max(self.burn_in), self.capacity,
                    self.mem_len.data_ptr(), self.mem_prio.data_ptr(), self.mem_psum.data_ptr(),
                    self.wdir.data_ptr(), self.d_off.data_ptr(), self.d_tot.data_ptr(),
                    self.isw.data_ptr(), self._stream()))
            due = [d and not q for d, q in zip(due, self.prio)]
            if not any(due):
                return
            mask = self.due_uni_dev
        filled = min(f for f, d in zip(self.filled, due) if d)
        if self.window is not None:
            N.check(self.lib.mz_drqn_pop_window_sample(
                self.seed_dev.data_ptr(), self.cnt_dev.data_ptr(), self.burn_in_dev.data_ptr(),
                mask.data_ptr(), HIDDEN, self.P, self.batch_size, self.L, self.window,
                max(self.burn_in), self.capacity, filled, self.ring.data_ptr(),
                self.mem_len.data_ptr(), self.wdir.data_ptr(), self.d_off.data_ptr(),
                self.d_tot.data_ptr(), self._stream()))
            return
        N.check(self.lib.mz_drqn_pop_sample(
            self.seed_dev.data_ptr(), self.cnt_dev.data_ptr(), self.due_dev.data_ptr(), self.P,
            self.batch_size, self.L, self.capacity, filled, self.ring.data_ptr(),
            self.mem_len.data_ptr(), self.d_slot.data_ptr(), self.d_len.data_ptr(),
            self.d_off.data_ptr(), self.d_tot.data_ptr(), self._stream()))

    def update(self):
        """One optimizer step of every due learner on its directory's episodes at lr_dev[p]; the
        losses stay on the device (self.loss)."""
        P, E, L, st = self.P, self.batch_size, self.L, self._stream()
        dirs = (self.d_slot.data_ptr(), self.d_len.data_ptr(), self.d_off.data_ptr(),
                self.d_tot.data_ptr())
        due, gam = self.due_dev.data_ptr(), self.gamma_dev.data_ptr()
        if self.window is not None:
            self._window_update(due, gam, st)
            self._adamw(due, st)
            return
        N.check(self.lib.mz_drqn_pop_seq_forward(
            self.tgt.data_ptr(), HIDDEN, 1, P, E, L, self.capacity, gam, due, self.mem.data_ptr(),
            self.mem_term.data_ptr(), *dirs, self.qmax.data_ptr(), None, None, None, None, None,
            st))
        N.check(self.lib.mz_drqn_pop_seq_forward(
            self.src.data_ptr(), HIDDEN, 0, P, E, L, self.capacity, gam, due, self.mem.data_ptr(),
            self.mem_term.data_ptr(), *dirs, self.qmax.data_ptr(), self.stash.data_ptr(),
            self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(), st))
        N.check(self.lib.mz_drqn_pop_seq_backward(
            self.src.data_ptr(), HIDDEN, P, E, L, self.capacity, due, self.mem.data_ptr(), *dirs,
            self.stash.data_ptr(), self.d.data_ptr(), self.ep_loss.data_ptr(),
            self.gpart.data_ptr(), self.grad.data_ptr(), self.loss.data_ptr(), st))
        self._adamw(due, st)

    def _adamw(self, due, st):
        N.check(self.lib.mz_adamw_pop(
            self.src.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
            self.grad.data_ptr(), self.P, PARAMS, self.lr_dev.data_ptr(), self.step.data_ptr(),
            due, BETAS[0], BETAS[1], ADAM_EPS, WEIGHT_DECAY, CLAMP, 1.0, 1, st))

    def _window_update(self, due, gam, st):
        P, E, L, T, K = self.P, self.batch_size, self.L, self.window, max(self.burn_in)
        state = self.mem_state.data_ptr() if any(self.stored) else None
        burn, stored = self.burn_in_dev.data_ptr(), self.stored_dev.data_ptr()
        dirs = (self.wdir.data_ptr(), self.d_off.data_ptr(), self.d_tot.data_ptr())
        N.check(self.lib.mz_drqn_pop_window_forward(
            self.tgt.data_ptr(), HIDDEN, 1, P, E, L, T, K, self.capacity, gam, burn, stored, due,
            self.mem.data_ptr(), self.mem_term.data_ptr(), state, *dirs, self.qmax.data_ptr(),
            None, None, None, None, None, st))
        N.check(self.lib.mz_drqn_pop_window_forward(
            self.src.data_ptr(), HIDDEN, 0, P, E, L, T, K, self.capacity, gam, burn, stored, due,
            self.mem.data_ptr(), self.mem_term.data_ptr(), state, *dirs, self.qmax.data_ptr(),
            self.stash.data_ptr(), self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(),
            self.ep_loss.data_ptr(), st))
        if self._prio_due:  # the new masses; d and ep_loss times the weights
            N.check(self.lib.mz_drqn_pop_prio_update(
                self.prio_alpha_dev.data_ptr(), self.prio_eta_dev.data_ptr(),
                self.prio_eps_dev.data_ptr(), self.due_prio_dev.data_ptr(), HIDDEN, P, E, L, T,
                self.capacity, *dirs, self.qa.data_ptr(), self.y.data_ptr(), self.d.data_ptr(),
                self.ep_loss.data_ptr(), self.isw.data_ptr(), self.mem_prio.data_ptr(),
                self.mem_psum.data_ptr(), self.prio_max.data_ptr(), st))
        N.check(self.lib.mz_drqn_pop_window_backward(
            self.src.data_ptr(), HIDDEN, P, E, L, T, K, self.capacity, burn, due,
            self.mem.data_ptr(), *dirs, self.stash.data_ptr(), self.d.data_ptr(),
            self.ep_loss.data_ptr(), self.gpart.data_ptr(), self.grad.data_ptr(),
            self.loss.data_ptr(), st))

    def _update(self, due):
        self._overflow_look(self.launches)
        self.launches += 1
        lr, sync = [0.0] * self.P, [0] * self.P
        for p in range(self.P):
            if due[p]:
                lr[p] = self.last_lr[p] = cosine_lr(self.updates[p], self.lr[p], T_MAX, ETA_MIN)
                sync[p] = int((self.updates[p] + 1) % self.tuf[p] == 0)
        self._upload(due, sync, lr)
        self.sample(due)
        self.update()
        if any(sync):
            N.check(self.lib.mz_drqn_pop_sync(self.src.data_ptr(), self.tgt.data_ptr(),
                                              self.sync_dev.data_ptr(), self.P, self._stream()))
        for p in range(self.P):
            self.updates[p] += int(due[p])

    def vector_step(self):
        self._act()
        self.env.step(self.act_out)
        self._scan_store()
        self._reset_winners()
        E = self.batch_size
        if min(self.filled) < E:  # (only until every learner has its first batch: one sync a step)
            counts = self.ring[:, 1].tolist()
            self.filled = [f if f >= E else int(n) for f, n in zip(self.filled, counts)]
        due = [False] * self.P
        if self.counter % self.train_every == 0:
            due = [f >= E for f in self.filled]
        self.last_due = due
        if any(due):
            self._update(due)

    def _log_fields(self):
        out = {"loss": [round(v, 6) for v in self.loss.tolist()],
               "epsilon": [round(self.epsilon(p), 4) for p in range(self.P)]}
        if any(self.prio):  # (None for a uniform learner)
            on = lambda vs: [v if q else None for v, q in zip(vs, self.prio)]  # noqa: E731
            out["prio_max"] = on([v / PRIO_ONE for v in self.prio_max.tolist()])
            out["mean_weight"] = on(self.isw.mean(dim=1).tolist())
        return out

    # ---- checkpoint / resume (mazerl/checkpoint.py) -------------------------------------------
    _OWN = ("h", "c", "ring", "pool", "loss", "src", "tgt", "exp_avg", "exp_avg_sq", "step")
    _LISTS = ("seed", "steps_done", "updates", "filled")

    def state_dict(self):
        """The run between two vector steps: every learner's nets, moments and step count, (h, c),
        the in-flight records, each ring's filled slots with head and count, the per-learner
        counters and the env (_save_common)."""
        sd = self._save_common()
        sd.update({k: getattr(self, k).clone() for k in self._OWN})
        counts = [int(n) for n in self.ring[:, 1].tolist()]
        for k in ("mem", "mem_len", "mem_term"):
            sd[k] = [getattr(self, k)[p, :n].clone() for p, n in enumerate(counts)]
        sd["learners"] = {k: [int(v) for v in getattr(self, k)] for k in self._LISTS}
        if self.window is not None:
            sd["window"] = self._window_settings()
        if any(self.stored):
            sd["snap_rec"] = self.snap_rec.clone()
            sd["mem_state"] = [self.mem_state[p, :n].clone() for p, n in enumerate(counts)]
        if any(self.prio):
            sd["priority"] = self._priority_settings()
            for k in ("mem_prio", "mem_psum"):
                sd[k] = [getattr(self, k)[p, :n].clone() for p, n in enumerate(counts)]
            sd["prio_max"] = self.prio_max.clone()
        return sd

    def load_state_dict(self, sd):
        self._check_window_settings(sd)
        # (a checkpoint of a population without priorities has no "priority" key)
        if sd.get("priority") != self._priority_settings():
            raise ValueError(f"the checkpoint's prioritized replay {sd.get('priority')} differs "
                             f"from this population's {self._priority_settings()}")
        self._load_common(sd)
        if any(self.prio):
            for k in ("mem_prio", "mem_psum"):
                for p, part in enumerate(sd[k]):
                    getattr(self, k)[p, :part.shape[0]].copy_(part)
            self.prio_max.copy_(sd["prio_max"])
        if any(self.stored):
            self.snap_rec.copy_(sd["snap_rec"])
            for p, part in enumerate(sd["mem_state"]):
                self.mem_state[p, :part.shape[0]].copy_(part)
        for k in self._OWN:
            getattr(self, k).copy_(sd[k])
        for k in ("mem", "mem_len", "mem_term"):
            for p, part in enumerate(sd[k]):
                getattr(self, k)[p, :part.shape[0]].copy_(part)
        for k in self._LISTS:
            setattr(self, k, [int(v) for v in sd["learners"][k]])
        self.seed_dev.copy_(torch.tensor([_signed(s) for s in self.seed], dtype=torch.int64))
