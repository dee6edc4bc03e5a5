"""Vectorised PPO (config 5: variable-size toroidal mazes) — PPOTrainer.train/PPOAgent.do_episode
(lib/trainers/ppo_trainer.py:62-99, agents/ppo_agent.py:143-169) over B instances at once.

Per vector step, with no host round trip (csrc/mz_ppo.hip):
  act      the f32 ActorCriticNet forward (HIP f32 conv stem from the window bits + f32 GEMMs —
           the reference acts in f32, ppo_agent.py:55-68), then mz_ppo_act: softmax, one draw per
           instance, the draw's log-prob, and the record of (obs6, window bits, action, log-prob,
           value) at the instance's step index t[i] of [B, L] episode buffers in HBM (L = more
           than the longest possible episode, episode_bound);
  step     the env step (float64 rewards: the reference's Python floats);
  scan     mz_ppo_scan: the reward at t[i], t[i] += 1; for finished episodes the counters, t[i] = 0
           and the list of finished episodes with their pool offsets (instance order);
  finish   mz_ppo_finish: per finished episode calculate_returns / calculate_advantages
           (:171-186; returns in float64, normalised with the unbiased std) and its rows appended
           to the update pool (fixed-capacity SoA columns in HBM);
  reset    winners get new mazes (update_maze), truncated instances restart theirs; with a
           curriculum / growth schedule (schedule.py) the winners' next algorithm
           (change_algorithm, ppo_trainer.py:137-141) and size (+4 growth, the max-shape stop,
           :96-105) first.
The pool's appended-rows total is copied to the host one step late (it only grows), so the
"pool holds `pool_size` rows" test costs no synchronisation; when it passes, the update runs:
optimize_model over the first pool_size rows (ppo_steps passes of unshuffled minibatches: clipped
surrogate incl. the reference's [b, b] ratio broadcast, entropy bonus with the linear 1e-2 -> 5e-4
schedule, 0.5 * value MSE, clip_grad_norm 0.5), and the rest moves to the front of the pool.
1-step episodes (NaN returns: torch.std of one element) never reach the pool; any other row with a
non-finite advantage or return is dropped at update time (the reference would train on NaN).
"""
import torch
import torch.nn.functional as F

from .. import _native as N
from ..agents.ppo import ActorCriticNet, PPOMinibatchGraph, make_optimizer, optimize_model
from .episodic import PooledEpisodicTrainer, episode_bound  # noqa: F401  (episode_bound: importers)


def pool_update(net, opt, cols, coef, batch_size, ppo_steps, allreduce=None, graph=None):
    """optimize_model on one pool's rows `cols` = (obs6, window bits or f32 window, action,
    log-prob, advantage, return). Rows with a non-finite advantage / return are dropped; with a
    gradient all-reduce every rank keeps the smallest kept count over the ranks, so all ranks run
    the same minibatch schedule (the same collective count and graph-replay / eager split).
    Returns the number of rows trained on."""
    s6, w, a, lp, adv, ret = cols
    P = s6.shape[0]
    keep = torch.isfinite(adv) & torch.isfinite(ret)
    n_keep = keep.sum().reshape(1)
    if allreduce is not None:
        import torch.distributed as dist
        dist.all_reduce(n_keep, op=dist.ReduceOp.MIN)
    n_keep = int(n_keep.item())
    if n_keep < P or not bool(keep[:n_keep].all()):
        rows = torch.nonzero(keep).flatten()[:n_keep]
        s6, w, a, lp, adv, ret = (x.index_select(0, rows) for x in (s6, w, a, lp, adv, ret))
    optimize_model(net, opt, (s6, w), a[:, None], lp[:, None], adv, ret, coef, batch_size,
                   ppo_steps, allreduce=allreduce, graph=graph)
    return n_keep


class VectorPPOTrainer(PooledEpisodicTrainer):
    _FORMAT = "mazerl.VectorPPOTrainer/2"
    _REC = ("b_s6", "b_w", "b_a", "b_lp", "b_v", "b_r")
    _POOL_COLS = (("p_s6", (6,), torch.float32), ("p_w", (22,), torch.int32),
                  ("p_a", (), torch.int64), ("p_lp", (), torch.float32),
                  ("p_adv", (), torch.float32), ("p_ret", (), torch.float32))
    _POOL = tuple(c[0] for c in _POOL_COLS)
    _COUNTERS = ("seed", "counter", "consumed", "updates", "rows_trained", "calls")

    def __init__(self, env, device, actor_lr=3e-4, critic_lr=1e-4, gamma=0.9, batch_size=2048,
                 ppo_steps=4, pool_size=65536, hidden_dim=1024, h_channels=32, seed=0,
                 allreduce=None, use_graph=True, bank=True, pool_capacity=None, curriculum=False,
                 growth=None, algorithm="r-prim", bank_candidates=1, archive=None):
        """curriculum / growth / algorithm / bank_candidates: EpisodicTrainer's (schedule.py);
        archive: its explored-maze pool (None: off). A data-parallel run keeps one per rank."""
        super().__init__(env, device, pool_size, pool_capacity, allreduce, bank=bank,
                         curriculum=curriculum, growth=growth, algorithm=algorithm,
                         bank_candidates=bank_candidates, archive=archive)
        torch.manual_seed(seed)
        self.net = ActorCriticNet(3, 6, 4, h_channels, hidden_dim).to(self.device)
        # the update reads the pool's packed windows through the HIP stem and replays a captured
        # minibatch step (PPOMinibatchGraph)
        self.opt = make_optimizer(self.net, actor_lr, critic_lr, capturable=use_graph)
        self.graph = PPOMinibatchGraph(self.net, self.opt, batch_size, allreduce) if use_graph else None
        self.gamma, self.batch_size, self.ppo_steps = gamma, batch_size, ppo_steps
        self.pool_size = int(pool_size)
        self.seed = int(seed)
        self.counter = 0
        B, L = env.num_envs, self.L
        kw = dict(device=self.device)
        # per-instance episode records [B, L]
        self.b_s6 = torch.zeros(B, L, 6, dtype=torch.float32, **kw)
        self.b_w = torch.zeros(B, L, 22, dtype=torch.int32, **kw)
        self.b_a = torch.zeros(B, L, dtype=torch.int64, **kw)
        self.b_lp = torch.zeros(B, L, dtype=torch.float32, **kw)
        self.b_v = torch.zeros(B, L, dtype=torch.float32, **kw)
        self.b_r = torch.zeros(B, L, dtype=torch.float64, **kw)
        self.consumed = 0
        self.updates = 0
        self.rows_trained = 0

    @torch.no_grad()
    def _act(self):
        """ActorCriticNet.act in f32 for every instance + the record at t[i] (mz_ppo_act)."""
        env = self.env
        logits, value = self.net((env.obs6, env.window_bits))
        logits, value = logits.contiguous(), value.contiguous()
        B = env.num_envs
        N.check(self.lib.mz_ppo_act(
            logits.data_ptr(), logits.stride(0), value.data_ptr(), value.stride(0),
            env.obs6.data_ptr(), env.window_bits.data_ptr(), B, self.L,
            self.seed & 0xFFFFFFFFFFFFFFFF, self.counter & 0xFFFFFFFFFFFFFFFF, self.t.data_ptr(),
            self.b_s6.data_ptr(), self.b_w.data_ptr(), self.b_a.data_ptr(), self.b_lp.data_ptr(),
            self.b_v.data_ptr(), self.act_out.data_ptr(), self._stream()))
        self.counter += 1
        return logits, value

    def _finish(self):
        """mz_ppo_finish: the finished episodes' returns / advantages, their rows into the pool."""
        B, L = self.env.num_envs, self.L
        N.check(self.lib.mz_ppo_finish(
            self.b_r.data_ptr(), self.b_s6.data_ptr(), self.b_w.data_ptr(), self.b_a.data_ptr(),
            self.b_lp.data_ptr(), self.b_v.data_ptr(), B, L, self.fin_id.data_ptr(),
            self.fin_off.data_ptr(), self.fin_len.data_ptr(), self.fin_count.data_ptr(),
            float(self.gamma), self.cap, self.p_s6.data_ptr(), self.p_w.data_ptr(),
            self.p_a.data_ptr(), self.p_lp.data_ptr(), self.p_adv.data_ptr(),
            self.p_ret.data_ptr(), self._stream()))

    def _update(self, frac):
        P = self.pool_size
        k = torch.div(self.pool_fill, P, rounding_mode="floor")
        # [update count, -record overflows, -pool over capacity]: one MIN all-reduce gives the
        # ranks' common update count and the MAX of both error flags, so every rank raises
        # together (a rank raising alone would leave the others blocked in pool_update's
        # collectives)
        chk = torch.cat([k, -self.stats[3:4], -(self.pool_fill > self.cap).to(torch.int64)])
        if self.allreduce is not None:
            import torch.distributed as dist
            dist.all_reduce(chk, op=dist.ReduceOp.MIN)
        # one synchronisation per update: the fill, the update count over the ranks, overflows
        fill, k, over, overcap = (int(x) for x in torch.cat([self.pool_fill, chk]).cpu())
        over, overcap = -over, -overcap
        if over:
            raise RuntimeError(f"PPO episode records overflowed: {over} episodes reached "
                               f"L = {self.L} steps (mz_ppo_scan stats[3], max over the ranks)")
        if overcap:
            raise RuntimeError(f"PPO pool overflow: more rows than the capacity {self.cap} on a "
                               f"rank (this rank: {fill}; raise pool_capacity)")
        coef = 1e-2 - (1e-2 - 5e-4) * frac  # ppo_trainer.py:73
        for j in range(k):
            self.rows_trained += pool_update(self.net, self.opt, self._cols(j * P, (j + 1) * P),
                                             coef, self.batch_size, self.ppo_steps,
                                             allreduce=self.allreduce, graph=self.graph)
            self.updates += 1
        rest = fill - k * P
        if k and rest:
            for col in self._cols(0, self.cap):
                col[:rest].copy_(col[k * P:fill].clone() if rest > k * P else col[k * P:fill])
        self.pool_fill.fill_(rest)
        self.consumed += k * P

    def vector_step(self, frac=0.0):
        self._act()
        self.env.step(self.act_out)
        self._scan_finish()
        self._reset_winners()  # change_algorithm, update_maze's sizes (ppo_trainer.py:95-105)
        if self._due(self.pool_size):
            self._update(frac)

    def _train_step(self, k, n):
        self.vector_step(frac=k / max(1, n))

    # ---- checkpoint / resume (mazerl/checkpoint.py) -------------------------------------------
    def state_dict(self):
        """The run between two vector steps: the net, the optimizer (moments, step, per-group
        learning rates), the in-flight episodes' records, the update pool's filled rows, the
        counters and the env (_save_common)."""
        sd, o = self._save_common(), self.opt
        sd["net"] = {k: v.clone() for k, v in self.net.state_dict().items()}
        if hasattr(o, "exp_avg"):
            sd["opt"] = {k: getattr(o, k).clone() for k in ("exp_avg", "exp_avg_sq", "step_t", "lr_dev")}
        else:
            sd["opt"] = {"torch": o.state_dict()}
        return sd

    def load_state_dict(self, sd):
        if sd.get("format") == "mazerl.VectorPPOTrainer/1":
            raise ValueError("a format-1 VectorPPOTrainer checkpoint (3 stats counters, a different "
                             "record length rule): not loadable by this version")
        self._load_common(sd)
        with torch.no_grad():
            self.net.load_state_dict(sd["net"])
        o, so = self.opt, sd["opt"]
        if "torch" in so:
            o.load_state_dict(so["torch"])
        else:
            for k, v in so.items():
                getattr(o, k).copy_(v)

    @torch.no_grad()
    def greedy(self, obs6, window, bits=None):
        """PPOAgent.evaluate's action (ppo_agent.py:239-252): argmax of softmax(logits), f32."""
        logits, _ = self.net((obs6, bits if bits is not None else window))
        return torch.argmax(F.softmax(logits, dim=-1), dim=-1)
