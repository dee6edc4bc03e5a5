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
import time

import torch

from .. import _native as N
from ..agents.flat import FlatAdamWGroups
from ..agents.rf_agent import PolicyNetwork, cosine_lr, head_loss
from .ppo_trainer import episode_bound
from .schedule import WinSchedule, curriculum_rule

FORMAT = "mazerl.VectorReinforceTrainer/1"
SAMPLE_KEY = 0x5A4D504C  # evaluation draws: a key of their own beside the training draws'


class VectorReinforceTrainer:
    def __init__(self, env, device, lr=1e-3, gamma=0.99, update_rows=16384, batch_size=2048,
                 temperature=2.0, entropy_coef=0.01, hidden_dim=1024, h_channels=32, seed=0,
                 bank=True, curriculum=False, growth=None, algorithm="r-prim", bank_candidates=1,
                 pool_capacity=None):
        """update_rows: pool rows that make an update due (1: after every finished episode);
        curriculum / growth / algorithm / bank_candidates: VectorPPOTrainer's (schedule.py)."""
        self.env = env
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("VectorReinforceTrainer runs on the GPU (libmazerl HIP kernels)")
        if env.window_bits is None or env.reward64 is None:
            raise ValueError("VectorReinforceTrainer needs an env with window_bits=True, reward64=True")
        from ..gemm_tuning import enable as _tuned_gemms
        _tuned_gemms(self.device)  # the tuned f32 GEMM choices (gemm_tuning.py)
        rule = curriculum_rule(curriculum)
        self.curriculum = rule
        self.schedule = (WinSchedule(env, rule, growth, None, algorithm)
                         if (rule is not None or growth is not None) else None)
        self.stopped_at = None
        if bank:
            dims = getattr(env, "dims_in_use", None)
            if self.schedule is not None and self.schedule.growth is not None:
                dims = self.schedule.sizes()
            env.enable_bank(algorithms=[0, 1, 2] if rule else None, dims=dims,
                            candidates=bank_candidates)
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
        B = env.num_envs
        self.L = L = episode_bound(env.max_dim, env.toroidal)
        kw = dict(device=self.device)
        # per-instance episode records [B, L]
        self.b_s6 = torch.zeros(B, L, 6, dtype=torch.float32, **kw)
        self.b_w = torch.zeros(B, L, 22, dtype=torch.int32, **kw)
        self.b_a = torch.zeros(B, L, dtype=torch.int64, **kw)
        self.b_r = torch.zeros(B, L, dtype=torch.float64, **kw)
        self.t = torch.zeros(B, dtype=torch.int32, **kw)
        self.act_out = torch.zeros(B, dtype=torch.int32, **kw)
        # the update pool; the fill bound at an update is VectorPPOTrainer's (update_rows + what
        # the vector steps between a check's issue and its use can append)
        self.cap = int(pool_capacity or self.update_rows + 2 * B * L)
        C = self.cap
        self.p_s6 = torch.zeros(C, 6, dtype=torch.float32, **kw)
        self.p_w = torch.zeros(C, 22, dtype=torch.int32, **kw)
        self.p_a = torch.zeros(C, dtype=torch.int64, **kw)
        self.p_adv = torch.zeros(C, dtype=torch.float32, **kw)
        self.p_len = torch.zeros(C, dtype=torch.int32, **kw)
        self.fin_id = torch.zeros(B, dtype=torch.int32, **kw)
        self.fin_off = torch.zeros(B, dtype=torch.int64, **kw)
        self.fin_len = torch.zeros(B, dtype=torch.int32, **kw)
        self.fin_count = torch.zeros(1, dtype=torch.int32, **kw)
        self.pool_fill = torch.zeros(1, dtype=torch.int64, **kw)
        self.pool_total = torch.zeros(1, dtype=torch.int64, **kw)
        self.pool_episodes = torch.zeros(1, dtype=torch.int32, **kw)
        # episodes, wins, dropped 1-step episodes, record-buffer overflows (an error, _update)
        self.stats = torch.zeros(4, dtype=torch.int64, **kw)
        self._total_host = torch.zeros(1, dtype=torch.int64, pin_memory=True)
        self._total_ev = None
        self._none = torch.zeros(32, dtype=torch.int64, **kw)  # sample(): records nothing
        self.consumed = 0
        self.updates = 0
        self.rows_trained = 0
        self.last_update = None  # the last update's pool columns, episode count, lr and loss
        self.lib = N.load()

    @property
    def supports_bits(self):
        return True

    @property
    def episodes(self):
        return int(self.stats[0])

    @property
    def wins(self):
        return int(self.stats[1])

    @property
    def algo(self):
        return None if self.schedule is None else self.schedule.maze_algo

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    _REC = ("b_s6", "b_w", "b_a", "b_r")
    _POOL = ("p_s6", "p_w", "p_a", "p_adv", "p_len")

    def _cols(self, lo, hi):
        return tuple(getattr(self, k)[lo:hi] for k in self._POOL)

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

    def _scan_finish(self, reward64=None, terminated=None, truncated=None):
        """The step's outcome (default: the env's output tensors) -> records, finished episodes
        -> pool."""
        env, B, L, st = self.env, self.env.num_envs, self.L, self._stream()
        r64 = env.reward64 if reward64 is None else reward64
        term = env.terminated if terminated is None else terminated
        trunc = env.truncated if truncated is None else truncated
        N.check(self.lib.mz_ppo_scan(
            r64.data_ptr(), term.data_ptr(), trunc.data_ptr(), B, L,
            self.t.data_ptr(), self.b_r.data_ptr(), self.fin_id.data_ptr(), self.fin_off.data_ptr(),
            self.fin_len.data_ptr(), self.fin_count.data_ptr(), self.pool_fill.data_ptr(),
            self.pool_total.data_ptr(), self.stats.data_ptr(), st))
        N.check(self.lib.mz_rf_finish(
            self.b_r.data_ptr(), self.b_s6.data_ptr(), self.b_w.data_ptr(), self.b_a.data_ptr(),
            B, L, self.fin_id.data_ptr(), self.fin_off.data_ptr(), self.fin_len.data_ptr(),
            self.fin_count.data_ptr(), self.gamma, self.cap, self.p_s6.data_ptr(),
            self.p_w.data_ptr(), self.p_a.data_ptr(), self.p_adv.data_ptr(), self.p_len.data_ptr(),
            self.pool_episodes.data_ptr(), st))

    def _due(self):
        """True when the pool held >= update_rows rows when the last check was issued (the host
        copy of the appended total lands while the next vector step runs; it only grows, so a
        late look never overshoots)."""
        due = False
        if self._total_ev is not None:
            self._total_ev.synchronize()
            due = int(self._total_host[0]) - self.consumed >= self.update_rows
            self._total_ev = None
        self._total_host.copy_(self.pool_total, non_blocking=True)
        self._total_ev = torch.cuda.Event()
        self._total_ev.record()
        return due

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
        env = self.env
        self._act()
        env.step(self.act_out)
        self._scan_finish()
        sch = self.schedule
        if sch is not None:  # change_algorithm for the winners (value_based_trainer.py:72)
            won = env.terminated.bool()
            sch.before_reset(won)
        env.reset_done(regen_won=True)
        if sch is not None:  # update_maze's sizes, the max-shape stop (:74-83)
            sch.after_reset(won)
        if self._due():
            self._update()

    def train(self, vector_steps, log_every=0, log=print):
        t0 = time.perf_counter()
        sch = self.schedule
        for k in range(vector_steps):
            self.vector_step()
            # the max-shape stop (value_based_trainer.py:81-83) once every instance reached it
            if sch is not None and sch.growth is not None and (k + 1) % 32 == 0 and sch.all_retired():
                self.stopped_at = k + 1
                break
            if log_every and (k + 1) % log_every == 0 and log:
                log(dict(step=k + 1, episodes=self.episodes, wins=self.wins, updates=self.updates,
                         seconds=round(time.perf_counter() - t0, 2)))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

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
        rate), the in-flight episodes' records (each instance's first t[i] rows), the update
        pool's filled rows, the counters and the env."""
        torch.cuda.synchronize(self.device)
        t = self.t.clone()
        live = torch.arange(self.L, device=self.device)[None, :] < t[:, None].long()
        fill = int(self.pool_fill.item())
        o = self.opt
        return {"format": FORMAT, "L": self.L, "cap": self.cap,
                "schedule": None if self.schedule is None else self.schedule.state_dict(),
                "net": {k: v.clone() for k, v in self.net.state_dict().items()},
                "opt": {k: getattr(o, k).clone() for k in ("exp_avg", "exp_avg_sq", "step_t", "lr_dev")},
                "t": t, "records": {k: getattr(self, k)[live] for k in self._REC},
                "pool_fill": fill, "pool": {k: getattr(self, k)[:fill].clone() for k in self._POOL},
                "pool_total": self.pool_total.clone(), "pool_episodes": self.pool_episodes.clone(),
                "stats": self.stats.clone(),
                # the appended total the next _due() reads (copied one vector step late)
                "total_host": int(self._total_host[0]) if self._total_ev is not None else None,
                "counters": {k: getattr(self, k) for k in ("seed", "counter", "sample_counter",
                                                           "consumed", "updates", "rows_trained")},
                "env": self.env.state_dict()}

    def load_state_dict(self, sd):
        if sd.get("format") != FORMAT or sd["L"] != self.L or sd["cap"] != self.cap:
            raise ValueError("not a VectorReinforceTrainer state_dict of this shape")
        if (sd["schedule"] is None) != (self.schedule is None):
            raise ValueError("curriculum / growth differ from the saved trainer's")
        self.env.load_state_dict(sd["env"])
        if self.schedule is not None:
            self.schedule.load_state_dict(sd["schedule"])
        with torch.no_grad():
            self.net.load_state_dict(sd["net"])
        for k, v in sd["opt"].items():
            getattr(self.opt, k).copy_(v)
        self.t.copy_(sd["t"])
        live = torch.arange(self.L, device=self.device)[None, :] < self.t[:, None].long()
        for k in self._REC:
            getattr(self, k)[live] = sd["records"][k].to(self.device)
        fill = int(sd["pool_fill"])
        for k in self._POOL:
            getattr(self, k)[:fill].copy_(sd["pool"][k])
        self.pool_fill.fill_(fill)
        self.pool_total.copy_(sd["pool_total"])
        self.pool_episodes.copy_(sd["pool_episodes"])
        self.stats.copy_(sd["stats"])
        for k, v in sd["counters"].items():
            setattr(self, k, int(v))
        self._total_ev = None
        if sd["total_host"] is not None:  # what the saved trainer's next _due() would have read
            self._total_host[0] = int(sd["total_host"])
            self._total_ev = torch.cuda.Event()
            self._total_ev.record()


class _Sampler:
    supports_bits = True

    def __init__(self, trainer):
        self.trainer = trainer

    def greedy(self, obs6, window, bits=None):
        return self.trainer.sample(obs6, window, bits)
