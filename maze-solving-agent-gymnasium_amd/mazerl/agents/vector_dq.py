"""VectorDoubleQAgent — a population of the reference's double Q-learning agent, DQAgent
(agents/dq_agent.py:5-73), on the vector engine of VectorQAgent: the constructor contract, the
per-table hyper-parameters, the state index, the two storages and the trainer are VectorQAgent's
(vector_q.py); the learner is RuleDQ of csrc/mz_qtab.hip.

A state holds two rows, Q_A and Q_B, side by side ([2, 4] float64, 64 B): self.q is
[T, rows, 2, 4] (dense, 2.1 MB per table at 9x9), self.vals [T, C, 2, 4] (hashed, 68 B per slot,
one key and one probe for both tables); self.qa / self.qb are views of the two tables.

act() is DQAgent.get_action: epsilon-greedy on Q_A alone. update() is DQAgent.update: a coin picks
the table to update, A or B; best = a second get_action on the next observation — epsilon-greedy
on Q_A[s'] whichever table is updated, advancing steps_done again, so steps_done grows by 2 per
training step and by 1 per evaluation step — and td = reward + gamma * Q_other[s'][best] -
Q_chosen[s][a], with no terminated factor, exactly as the reference. One instance per table is
the reference's agent bit for bit in float64; several per table are synchronous-parallel as in
VectorQAgent. The coin and the inner choice draw from their own Philox stream, indexed by
self.ucounter, the count of update() calls.
"""
import torch

from .. import _native as N
from .vector_q import (VectorQAgent, _check_capacity, _ptr, hash_slot,  # noqa: F401
                       state_index, table_rows)

_FORMAT = "mazerl.VectorDoubleQAgent/1"
_FORMAT_HASH = "mazerl.VectorDoubleQAgent/2"


class VectorDoubleQAgent(VectorQAgent):
    _ROW = (2, 4)
    _ABI = "mz_dqtab"
    _FORMATS = (_FORMAT, _FORMAT_HASH)  # dense, hashed
    _COUNTERS = VectorQAgent._COUNTERS + ("ucounter",)

    def __init__(self, env, tables=None, learning_rate=0.1, initial_epsilon=0.95,
                 epsilon_decay=40.0, final_epsilon=0.05, discount_factor=0.7, eta=0.01, seed=0,
                 max_bytes=8 << 30, storage="dense", capacity=None):
        """VectorQAgent's arguments and refusals. The byte checks against max_bytes are
        T * rows * 64 (dense) and T * C * 68 + 12 * T (hashed)."""
        super().__init__(env, tables, learning_rate, initial_epsilon, epsilon_decay,
                         final_epsilon, discount_factor, eta, seed, max_bytes, storage, capacity)
        self.ucounter = 0
        self._took = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        self._which = None if self.table_of is None else torch.zeros_like(self._took)

    @property
    def qa(self):
        """Table A of every state: a view [T, rows, 4] (hashed: [T, C, 4], by slot)."""
        return (self.vals if self.hashed else self.q)[:, :, 0]

    @property
    def qb(self):
        return (self.vals if self.hashed else self.q)[:, :, 1]

    @property
    def update_launches(self):
        """Device launches of one update(): the update (two passes on shared tables) and the
        steps_done advance of its inner get_actions."""
        return 2 if self.table_of is None else 3

    def update(self, actions=None, coins=None, next_actions=None, episode_end=True):
        """DQAgent.update for every instance after env.step(actions), then the episode end as in
        VectorQAgent.update. coins (uint8 / bool [n]: 0 = update A, 1 = update B) and
        next_actions (int32 [n] in 0..3: the inner get_action's result) replace the draws, for
        replaying the reference; with next_actions no epsilon is evaluated, steps_done still
        advances."""
        env, dev = self.env, self.device
        a = self.actions if actions is None else \
            actions.to(device=dev, dtype=torch.int32).contiguous()
        coin = None if coins is None else coins.to(device=dev, dtype=torch.uint8).contiguous()
        nxt = None if next_actions is None else \
            next_actions.to(device=dev, dtype=torch.int32).contiguous()
        for name, t in (("actions", a), ("coins", coin), ("next_actions", nxt)):
            if t is not None and t.numel() != self.n:
                raise ValueError(f"{name}: one per instance ({self.n})")
        head = (env.obs6.data_ptr(), self.n, self.max_dim, _ptr(self.table_of), self.num_tables)
        tail = (self.sidx.data_ptr(), a.data_ptr(), env.reward64.data_ptr(),
                env.terminated.data_ptr(), env.truncated.data_ptr(), self.gamma.data_ptr(),
                self.lr.data_ptr(), self.eta.data_ptr(), self.cum.data_ptr(),
                self.episodes.data_ptr(), self.wins.data_ptr(), _ptr(self._td),
                int(bool(episode_end)), self.steps_done.data_ptr(), self.eps_init.data_ptr(),
                self.eps_final.data_ptr(), self.eps_decay.data_ptr(),
                self.seed & 0xFFFFFFFFFFFFFFFF, self.ucounter & 0xFFFFFFFFFFFFFFFF, _ptr(coin),
                _ptr(nxt), self._took.data_ptr(), _ptr(self._which), self._stream())
        if self.hashed:
            N.check(self.lib.mz_dqtab_hash_update(
                *head, self.keys.data_ptr(), self.vals.data_ptr(), self.capacity,
                self.load.data_ptr(), self.overflow.data_ptr(), *tail))
        else:
            N.check(self.lib.mz_dqtab_update(*head, self.q.data_ptr(), *tail))
        self.ucounter += 1
