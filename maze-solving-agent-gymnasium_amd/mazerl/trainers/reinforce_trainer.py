"""Vectorised REINFORCE — RFAgent under ValueBasedTrainer.train (agents/rf_agent.py:51-129,
lib/trainers/value_based_trainer.py:25-92) over B instances at once, euclidean or toroidal.

Per vector step, with no host round trip (csrc/mz_reinforce.hip, csrc/mz_ppo.hip):
  act      the f32 PolicyNetwork forward (HIP f32 conv stem from the window bits + f32 GEMMs; the
           reference samples from the f32 policy), then mz_rf_act: softmax(logits / 2), one draw
           per instance, and the record of (obs6, window bits, action) at the instance's step
           index t[i] of [B, L] episode buffers (L: episode_bound, as VectorPPOTrainer);
  step     the env step (float64 rewards: the reference's Python floats);
  scan     mz_ppo_scan, unchanged: the reward at t[i], t[i] += 1, the finished episodes' list with
           their pool offsets (instance order), the counters, 1-step episodes dropped (their
           returns are NaN in the reference: torch.std of one element);
  finish   mz_rf_finish: per finished episode get_returns (:88-99) and optimize_model's baseline
           (adv = R - mean(R), :109-110), its rows appended to the update pool with the episode's
           length on every row, and the pooled-episode count;
  reset    winners get new mazes (update_maze), truncated instances restart theirs; with a
           curriculum / growth schedule (schedule.py) the winners' next algorithm
           (change_algorithm, value_based_trainer.py:132-136) and size (+4 growth, the max-shape
           stop, :74-83) first.
The pool's appended-rows total is copied to the host one step late (it only grows); when the pool
held >= update_rows rows at that look, the update runs over EVERY episode in the pool (the pool
only ever holds whole episodes, so it empties): the rows go through the net in chunks of
batch_size, each chunk's loss and its gradient w.r.t. the logits come from mz_rf_head_loss, the
parameter gradients accumulate over the chunks, then one clip_grad_norm_(1.0) + AdamW step
(FlatAdamWGroups, one group, torch's default weight decay) at the cosine schedule's learning rate
(cosine_lr, advanced once per update as scheduler_step).

Two departures from the one-env reference, both forced by the batch:
  * the loss is the MEAN over the pooled episodes of the reference's per-episode loss (the
    reference takes one optimizer step per episode);
  * the forward is recomputed at update time with the parameters of that moment on the recorded
    states. With one instance and an update after every episode (update_rows=1) that is the
    reference's step; with many instances the rows of an episode acted under older parameters
    carry no importance weight.
"""
import torch

from .. import _native as N
from ..agents.flat import FlatAdamWGroups
from ..agents.rf_agent import PolicyNetwork, cosine_lr, head_loss
from .episodic import PooledEpisodicTrainer

FORMAT = "mazerl.VectorReinforceTrainer/1"
SAMPLE_KEY = 0x5A4D504C  # evaluation draws: a key of their own beside the training draws'


class VectorReinforceTrainer(PooledEpisodicTrainer):
    _FORMAT = FORMAT
    _REC = ("b_s6", "b_w", "b_a", "b_r")
    _POOL_COLS = (("p_s6", (6,), torch.float32), ("p_w", (22,), torch.int32),
                  ("p_a", (), torch.int64), ("p_adv", (), torch.float32),
                  ("p_len", (), torch.int32))
    _POOL = tuple(c[0] for c in _POOL_COLS)
    _COUNTERS = ("seed", "counter", "sample_counter", "consumed", "updates", "rows_trained")

    def __init__(self, env, device, lr=1e-3, gamma=0.99, update_rows=16384, batch_size=2048,
                 temperature=2.0, entropy_coef=0.01, hidden_dim=1024, h_channels=32, seed=0,
                 bank=True, curriculum=False, growth=None, algorithm="r-prim", bank_candidates=1,
                 pool_capacity=None, archive=None):
        """update_rows: pool rows that make an update due (1: after every finished episode);
        curriculum / growth / algorithm / bank_candidates: EpisodicTrainer's (schedule.py);
        archive: its explored-maze pool (None: off)."""
        super().__init__(env, device, update_rows, pool_capacity, bank=bank, curriculum=curriculum,
                         growth=growth, algorithm=algorithm, bank_candidates=bank_candidates,
                         archive=archive)
        torch.manual_seed(seed)
        self.net = PolicyNetwork(3, 6, 4, h_channels, hidden_dim).to(self.device)
        self.opt = FlatAdamWGroups(self.net, [(self.net.parameters(), lr)], max_norm=1.0)
        self.lr, self.gamma = float(lr), float(gamma)
        self.batch_size, self.update_rows = int(batch_size), int(update_rows)
        self.temperature, self.entropy_coef = float(temperature), float(entropy_coef)
        if self.batch_size < 1 or self.update_rows < 1:
            raise ValueError("batch_size and update_rows are at least 1")
        self.seed = int(seed)
        self.counter = 0
        self.sample_counter = 0
        B, L = env.num_envs, self.L
        kw = dict(device=self.device)
        # per-instance episode records [B, L]
        self.b_s6 = torch.zeros(B, L, 6, dtype=torch.float32, **kw)
        self.b_w = torch.zeros(B, L, 22, dtype=torch.int32, **kw)
        self.b_a = torch.zeros(B, L, dtype=torch.int64, **kw)
        self.b_r = torch.zeros(B, L, dtype=torch.float64, **kw)
        self.pool_episodes = torch.zeros(1, dtype=torch.int32, **kw)
        self._none = torch.zeros(32, dtype=torch.int64, **kw)  # sample(): records nothing
        self.consumed = 0
        self.updates = 0
        self.rows_trained = 0
        self.last_update = None  # the last update's pool columns, episode count, lr and loss

    @torch.no_grad()
    def _act(self):
        """select_action in f32 for every instance + the record at t[i] (mz_rf_act)."""
        env = self.env
        logits = self.net((env.obs6, env.window_bits)).contiguous()
        N.check(self.lib.mz_rf_act(
            logits.data_ptr(), logits.stride(0), self.temperature, env.obs6.data_ptr(),
            env.window_bits.data_ptr(), env.num_envs, self.L, self.seed & 0xFFFFFFFFFFFFFFFF,
            self.counter & 0xFFFFFFFFFFFFFFFF, self.t.data_ptr(), self.b_s6.data_ptr(),
            self.b_w.data_ptr(), self.b_a.data_ptr(), self.act_out.data_ptr(), self._stream()))
        self.counter += 1
        return logits

    def _finish(self):
        """mz_rf_finish: the finished episodes' returns and baseline, their rows into the pool."""
        N.check(self.lib.mz_rf_finish(
            self.b_r.data_ptr(), self.b_s6.data_ptr(), self.b_w.data_ptr(), self.b_a.data_ptr(),
            self.env.num_envs, self.L, self.fin_id.data_ptr(), self.fin_off.data_ptr(),
            self.fin_len.data_ptr(), self.fin_count.data_ptr(), self.gamma, self.cap,
            self.p_s6.data_ptr(), self.p_w.data_ptr(), self.p_a.data_ptr(), self.p_adv.data_ptr(),
            self.p_len.data_ptr(), self.pool_episodes.data_ptr(), self._stream()))

    def update(self, cols, episodes, lr):
        """One optimizer step on pool rows `cols` = (obs6, window bits, action, adv, length) of
        `episodes` (int32 device scalar) whole episodes at learning rate `lr`: the rows through
        the net in chunks of batch_size, gradients accumulated, clip_grad_norm_(1.0) + AdamW.
        Returns the loss (device scalar)."""
        rows = cols[0].shape[0]
        self.opt.lr_dev.fill_(float(lr))
        self.opt.zero_grad(set_to_none=True)
        total = torch.zeros((), dtype=torch.float32, device=self.device)
        for lo in range(0, rows, self.batch_size):
            s6, w, a, adv, ln = (c[lo:lo + self.batch_size] for c in cols)
            loss = head_loss(self.net((s6, w)), a, adv, ln, episodes, self.temperature,
                             self.entropy_coef)
            loss.backward()
            total += loss.detach()
        self.opt.step()
        return total

    def _update(self):
        # one synchronisation per update: the fill, the episode count, overflows
        fill, n_ep, over = (int(x) for x in torch.cat(
            [self.pool_fill, self.pool_episodes.long(), self.stats[3:4]]).cpu())
        if over:
            raise RuntimeError(f"REINFORCE episode records overflowed: {over} episodes reached "
                               f"L = {self.L} steps (mz_ppo_scan stats[3])")
        if fill > self.cap:
            raise RuntimeError(f"REINFORCE pool overflow: {fill} rows, capacity {self.cap} "
                               "(raise pool_capacity)")
        if fill == 0:
            return
        lr = cosine_lr(self.updates, self.lr)
        cols = tuple(c.clone() for c in self._cols(0, fill))
        episodes = self.pool_episodes.clone()
        loss = self.update(cols, episodes, lr)
        self.last_update = {"cols": cols, "episodes": n_ep, "lr": lr, "loss": loss}
        self.pool_fill.zero_()
        self.pool_episodes.zero_()
        self.consumed += fill
        self.rows_trained += fill
        self.updates += 1

    def vector_step(self):
        self._act()
        self.env.step(self.act_out)
        self._scan_finish()
        # change_algorithm, update_maze's sizes (value_based_trainer.py:72-83)
        self._reset_winners()
        if self._due(self.update_rows):
            self._update()

    # ---- evaluation (vector_trainer.evaluate) ---------------------------------------------------
    @torch.no_grad()
    def greedy(self, obs6, window, bits=None):
        """argmax of the logits (the reference has no greedy mode: sample() is its test())."""
        return torch.argmax(self.net((obs6, bits if bits is not None else window)), dim=-1)

    @torch.no_grad()
    def sample(self, obs6, window, bits=None):
        """The reference's own evaluation (ValueBasedTrainer.test acts through select_action):
        one draw per row from softmax(logits / temperature), by mz_rf_act with no record."""
        if bits is None:
            raise ValueError("sample() reads the packed windows (an env with window_bits=True)")
        n = obs6.shape[0]
        logits = self.net((obs6, bits)).contiguous()
        out = torch.empty(n, dtype=torch.int32, device=logits.device)
        t = torch.zeros(n, dtype=torch.int32, device=logits.device)
        z = self._none.data_ptr()
        N.check(self.lib.mz_rf_act(
            logits.data_ptr(), logits.stride(0), self.temperature, obs6.data_ptr(),
            bits.data_ptr(), n, 0, (self.seed ^ SAMPLE_KEY) & 0xFFFFFFFFFFFFFFFF,
            self.sample_counter & 0xFFFFFFFFFFFFFFFF, t.data_ptr(), z, z, z, out.data_ptr(),
            self._stream()))
        self.sample_counter += 1
        return out.long()

    def sampler(self):
        """A learner for vector_trainer.evaluate whose actions are sample()'s."""
        return _Sampler(self)

    # ---- checkpoint / resume (mazerl/checkpoint.py) -------------------------------------------
    def state_dict(self):
        """The run between two vector steps: the net, the optimizer (moments, step, learning
        rate), the in-flight episodes' records, the update pool's filled rows, the counters and
        the env (_save_common)."""
        sd, o = self._save_common(), self.opt
        sd["net"] = {k: v.clone() for k, v in self.net.state_dict().items()}
        sd["opt"] = {k: getattr(o, k).clone() for k in ("exp_avg", "exp_avg_sq", "step_t", "lr_dev")}
        sd["pool_episodes"] = self.pool_episodes.clone()
        return sd

    def load_state_dict(self, sd):
        self._load_common(sd)
        with torch.no_grad():
            self.net.load_state_dict(sd["net"])
        for k, v in sd["opt"].items():
            getattr(self.opt, k).copy_(v)
        self.pool_episodes.copy_(sd["pool_episodes"])


class _Sampler:
    supports_bits = True

    def __init__(self, trainer):
        self.trainer = trainer

    def greedy(self, obs6, window, bits=None):
        return self.trainer.sample(obs6, window, bits)
