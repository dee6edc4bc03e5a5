"""Populations of recurrent DQN learners: P independent VectorRecurrentDQNTrainers advanced by the
same launches (csrc/mz_drqn.hip's kernels, each of which serves P learners; csrc/mz_optim.hip
k_adamw_pop), so P seeds or P hyper-parameter settings of agents/lstm_dqn_agent.py cost about one
run's launches. The vector step, the update and the replay half of a checkpoint are
drqn_trainer.RecurrentDQNBase's, the one host driver that trainer runs with P = 1; this module adds
the flat nets and moments, AdamW and the target sync for all learners at once, the per-learner
access and evaluation, and the population's checkpoint format.

A population is P learners over B = P b instances; learner p owns the block [p b, (p + 1) b).
Shared: the env, L = episode_bound, batch_size E, memory_size (capacity, in episodes),
train_every, explore_actions. Per learner (a scalar or a length-P sequence): lr, discount_factor,
starting_epsilon, final_epsilon, epsilon_decay, target_update_frequency, seed.

Learner p is what VectorRecurrentDQNTrainer (drqn_trainer.py: its fourteen departures, its
accumulation order, Philox streams and ring semantics) is on its b instances with learner p's
hyper-parameters and seed, bit for bit: both are the same driver over the same kernels, which run
their device code on learner p's rows. The acting draw of instance i is keyed by (seed_p, counter,
i - p b), the sample by (seed_p, updates_p).

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
each K_p a multiple of T, checked before anything touches the GPU and uploaded once (departures
7-9 with (T, K_p, S_p)): learner p's episode draw is keyed by (seed_p, updates_p), its window draw
by (seed_p, updates_p, position in the batch). mz_drqn_snapshot runs over all P b instances and the
state memory [P][capacity][ceil(L / T)][64] exists when at least one learner is "stored"; a "zero"
learner never reads it. A checkpoint then also holds T and the two per-learner lists and, when
stored, snap_rec and each ring's filled slots of mem_state; it loads only into a population with
the same window settings.

Prioritized windows (priority_alpha, priority_beta, priority_eta, priority_eps: each a value or a
list of P; with every alpha None, the default, this is the population above: nothing of it is
allocated or launched, the same bits, the same checkpoint keys). An entry of priority_alpha may be
None: that learner keeps the uniform-per-episode window sampler. priority_beta is a number, a tuple
(beta0, beta1, updates) - one schedule for every learner - or a list of P numbers or such triples;
a learner's schedule runs over its own update count, is evaluated on the host (beta(p)) and goes
up with the per-update scalars (departures 10-12 with learner p's four values). Then mem_prio
[P][capacity][ceil(L / T)], mem_psum [P][capacity], prio_max [P] and isw [P][E] exist for all
learners (a uniform learner's masses are kept by the store launch and never read). Per update:
mz_drqn_pop_prio_sample under the mask due-and-prioritized, mz_drqn_pop_window_sample under
due-and-uniform (each launched only where its mask has an entry; the uniform sampler's smallest
fill is taken over its own mask), and mz_drqn_pop_prio_update under the first mask between the
source forward and the backward. The forward, backward, reduce, AdamW and sync launches run under
the one due mask, unchanged. A checkpoint then also holds the per-learner settings, each ring's
filled slots of mem_prio and mem_psum, and prio_max; it loads only into a population with the same
settings, and a checkpoint without them only into a population without priorities.

Double-Q targets and n-step returns (double_q, n_step: each a value or a list of P; with every
learner at False and 1, the default, this is the population above: nothing of it is allocated or
launched, the same bits, the same checkpoint keys). Otherwise all due learners go through the
target net's forward in its four-Q' form, the source net's in its argmax form and one returns
launch (departures 13-14 with learner p's two values; n_step and the double flag live on the
device as int32 [P], and the argmax rows are read only when a learner is double and only by such a
learner), then the priority update where one is due and the unchanged backward. A default learner
in such a population keeps the default trainer's bits: n_step = 1 without the argmax is its
arithmetic. q4 [P][rows][4] and sel [P][rows] exist for all learners. A checkpoint then also holds
the two per-learner lists and loads only into a population with the same ones.

curriculum="global" counts wins across all instances and would couple the learners: it is refused.
With bank=False a learner's whole run is independent of the other learners, bit for bit. With the
winner bank the maze a winner receives depends on how many instances of other learners won before
it, so the learners then share the stream of replacement mazes.
"""
import ctypes as C

import numpy as np
import torch

from .. import _native as N
from ..agents.lstm_dqn_agent import DQN, HIDDEN
from .drqn_trainer import (EVAL_KEY, PARAMS, PRIO_ONE, ROW, SHAPES, STASH, U64, RecurrentDQNBase,
                           _Evaluator, _signed)
from .episodic import episode_bound

FORMAT = "mazerl.VectorRecurrentDQNPopulation/1"
KEYS = ("lstm_cell.weight_ih", "lstm_cell.weight_hh", "lstm_cell.bias_ih", "lstm_cell.bias_hh",
        "fc.weight", "fc.bias")
PER_LEARNER = ("lr", "discount_factor", "starting_epsilon", "final_epsilon", "epsilon_decay",
               "target_update_frequency", "seed")
BETAS, ADAM_EPS, WEIGHT_DECAY, CLAMP = (0.9, 0.999), 1e-8, 1e-2, 1.0


def footprint(P, B, L, E, capacity, window=None, stored=False, prio=False, returns=False):
    """Bytes of the replay rings, the in-flight records, and an update's stash and row buffers;
    windowed: the row buffers hold E (min(T, L) + 2) rows, and with stored state the state memory
    (P capacity ceil(L / T) snapshots of 256 B) and the in-flight snapshots are added; prioritized:
    the masses (P capacity ceil(L / T) words and a 64-bit sum per slot), prio_max, the importance
    weights and the three float64 settings per learner; with double-Q targets or n-step returns:
    four Q' and an argmax per row."""
    rows = E * (L + 1) if window is None else E * (min(window, L) + 2)
    ring = P * capacity * ((L + 1) * ROW * 4 + 8)
    records = B * ((L + 1) * 6 * 4 + L * 4 + L * 8)
    update = P * (rows * (STASH + 4 + (5 if returns else 0)) * 4 + E * (PARAMS * 4 + 8 + 16))
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

    def __init__(self, env, device, learners=1, lr=1e-3, starting_epsilon=0.9, final_epsilon=0.05,
                 epsilon_decay=1000.0, discount_factor=0.99, batch_size=32, memory_size=20000,
                 target_update_frequency=10, explore_actions=4, train_every=1, seed=0, bank=True,
                 curriculum=False, growth=None, algorithm="r-prim", bank_candidates=1, window=None,
                 burn_in=0, initial_state="stored", archive=None, priority_alpha=None,
                 priority_beta=0.6, priority_eta=0.9, priority_eps=1e-3, double_q=False, n_step=1):
        """archive (None: off): an int C or a MazePoolSet of this env with one group per learner
        — every learner's explored mazes in a pool of C entries of its own, all filled by one
        launch per vector step (evaluate_explored_all). priority_alpha .. priority_eps: prioritized
        replay windows per learner (the module's docstring; every alpha None: off). double_q,
        n_step: double-Q targets and n-step returns per learner (every learner False and 1: off)."""
        P = int(learners)
        if P < 1 or env.num_envs % P:
            raise ValueError(f"env.num_envs {env.num_envs} must be a multiple of learners {P} >= 1")
        if curriculum is True or curriculum == "global":
            raise ValueError('curriculum="global" counts wins across all instances and would '
                             'couple the learners; use False or "per-instance"')
        self._configure(P, env.num_envs, lr, starting_epsilon, final_epsilon, epsilon_decay,
                        discount_factor, batch_size, memory_size, target_update_frequency,
                        explore_actions, train_every, seed, window, burn_in, initial_state,
                        priority_alpha, priority_beta, priority_eta, priority_eps, double_q, n_step)
        B, E = env.num_envs, self.batch_size
        L = episode_bound(env.max_dim, env.toroidal)
        need = footprint(P, B, L, E, self.capacity, self.window, any(self.stored), any(self.prio),
                         self._returns)
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
        self.src = torch.zeros(P, PARAMS, dtype=torch.float32, device=self.device)
        for p in range(P):  # learner p's initial net: the single trainer's under its seed
            torch.manual_seed(self.seed[p])
            net = DQN(6, 4, HIDDEN, self.device)
            DQN(6, 4, HIDDEN, self.device)  # (the single trainer's target net: the same draws)
            self.load_learner(p, net.state_dict())
        self.tgt = self.src.clone()
        self.grad = torch.zeros_like(self.src)
        self.exp_avg = torch.zeros_like(self.src)
        self.exp_avg_sq = torch.zeros_like(self.src)
        self.step = torch.zeros(P, dtype=torch.float32, device=self.device)  # (the optimizer's)
        self._alloc()

    # ---- per-learner access -------------------------------------------------------------------
    def memory_bytes(self):
        """The replay, record, stash and row-buffer footprint in bytes (footprint())."""
        return footprint(self.P, self.env.num_envs, self.L, self.batch_size, self.capacity,
                         self.window, any(self.stored), any(self.prio), self._returns)

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

    # ---- an update: the driver's, with AdamW and the target sync for all learners at once ------
    def sample(self, due):
        """Every due learner's batch (RecurrentDQNBase._draw), after _upload."""
        self._draw(due)

    def update(self):
        """One optimizer step of every due learner on its directory's episodes at lr_dev[p]; the
        losses stay on the device (self.loss)."""
        self._gradients()
        self._adamw(self.due_dev.data_ptr(), self._stream())

    def _adamw(self, due, st):
        N.check(self.lib.mz_adamw_pop(
            self.src.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
            self.grad.data_ptr(), self.P, PARAMS, self.lr_dev.data_ptr(), self.step.data_ptr(),
            due, BETAS[0], BETAS[1], ADAM_EPS, WEIGHT_DECAY, CLAMP, 1.0, 1, st))

    def _learn(self, due, sync, lr):
        self._upload(due, sync, lr)
        self.sample(due)
        self.update()
        if any(sync):
            N.check(self.lib.mz_drqn_pop_sync(self.src.data_ptr(), self.tgt.data_ptr(),
                                              self.sync_dev.data_ptr(), self.P, self._stream()))

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
        counters and the env (_save_common), and what the window and priority options add
        (_save_options)."""
        sd = self._save_common()
        self._save_own(sd)
        sd["learners"] = {k: [int(v) for v in getattr(self, k)] for k in self._LISTS}
        self._save_options(sd)
        return sd

    def load_state_dict(self, sd):
        self._check_settings(sd)
        self._load_common(sd)
        for k in self._LISTS:
            setattr(self, k, [int(v) for v in sd["learners"][k]])
        self._load_replay(sd)
