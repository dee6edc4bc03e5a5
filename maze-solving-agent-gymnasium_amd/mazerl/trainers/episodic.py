"""What the episode-recording trainers share (VectorPPOTrainer, VectorReinforceTrainer,
VectorRecurrentDQNTrainer): every instance records its running episode at its own step index
t[i] of [B, L] buffers in HBM, mz_ppo_scan closes the step (the reward at t[i], t[i] += 1, the
finished episodes' list in instance order, the counters), a trainer-specific launch consumes the
finished episodes, and the winners get their next mazes (schedule.py).

EpisodicTrainer holds that state, the one mz_ppo_scan call, the reset, the train() loop and the
common half of the checkpoint. PooledEpisodicTrainer adds the on-policy update pool of PPO and
REINFORCE: fixed-capacity SoA columns the finish launch appends to, and the one-step-late look at
the appended total that makes an update due without a synchronisation.

Each trainer keeps its own vector_step: the order of the launches is what its file documents.
"""
import time

import torch

from .. import _native as N
from ..archive import MazePool, MazePoolSet
from .schedule import enable_winner_bank, make_schedule, max_shape_stop, reset_winners


def episode_bound(max_dim, toroidal):
    """Record-buffer length L: more than the longest possible episode of any maze up to max_dim.
    An episode ends at the latest on step max_steps + 1 (base_maze_env.py:205-208), max_steps =
    ceil(((N-1)^2 - 1) * len / CE) with CE = (N-1) * ((N-1) // 2) - 1 and len = the solution's
    squares (simple_maze_env.py:52-58), at most the maze's open squares: 2 c - 1 for c cells,
    c = ((N-1)/2)^2 euclidean and ((N+1)/2)^2 on the torus (generated on the (N+2)^2 bordered grid,
    so len / CE can exceed 1 there and (N-1)^2 + 2 is not a bound). +2: the float rounding of
    len / CE and the step that reports truncation."""
    best = 0
    for n in range(5, int(max_dim) + 1, 2):
        c = ((n + 1) // 2) ** 2 if toroidal else ((n - 1) // 2) ** 2
        ce = (n - 1) * ((n - 1) // 2) - 1
        a = (n - 1) ** 2 - 1
        best = max(best, -(-a * (2 * c - 1) // ce) + 2)
    return best


def attach_pool(env, archive, groups=None):
    """A trainer's archive= argument -> its explored-maze pool: an int capacity C makes a
    MazePool(env, C), or with `groups` (a population of learners) a MazePoolSet(env, groups, C), C
    per learner; a pool or pool set of this env is taken as it is. ValueError for another env's,
    for a pool where a set is needed (or the reverse) and for a set of another group count."""
    if isinstance(archive, (MazePool, MazePoolSet)):
        if archive.env is not env:
            raise ValueError("the pool was built for another env")
        if groups is None and type(archive) is not MazePool:
            raise ValueError("this trainer keeps one MazePool (a population of learners keeps a "
                             "MazePoolSet)")
        if groups is not None and not (isinstance(archive, MazePoolSet) and
                                       archive.groups == groups):
            raise ValueError(f"a population of {groups} learners keeps a MazePoolSet of {groups} "
                             "groups")
        return archive
    if isinstance(archive, bool) or not isinstance(archive, int):
        raise ValueError("archive: None, an int capacity, or a MazePool / MazePoolSet of this env")
    return MazePool(env, archive) if groups is None else MazePoolSet(env, groups, archive)


class EpisodicTrainer:
    """A subclass sets _FORMAT (the checkpoint's format string), _SHAPE (the attributes a
    checkpoint must match), _REC (its record buffers, [B, >= L, ...]) and _COUNTERS (its host
    counters), allocates the record buffers and writes vector_step()."""
    _SHAPE = ("L",)

    def __init__(self, env, device, bank=True, curriculum=False, growth=None, algorithm="r-prim",
                 bank_candidates=1, archive=None, archive_groups=None):
        """curriculum (False | True / "global" | "per-instance"), growth ((start, max_dim): the
        variable-size envs' +4 per win and the max-shape stop), algorithm (the initial mazes'),
        bank_candidates (best-of-C replacement mazes): schedule.py, VectorOffPolicyTrainer.
        archive (None: off — no launch, no tensor, no checkpoint key more than before): an int C
        or a pool of this env (attach_pool) — the explored mazes, `env.mazes`, for
        evaluate_explored: every instance's first maze now, then each winner's new one
        (_reset_winners; one more launch and one flag copy per vector step). archive_groups: the
        learners of a population, each with a pool of its own."""
        self.env = env
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the GPU (libmazerl HIP kernels)")
        self.curriculum, self.schedule = make_schedule(env, curriculum, growth, None, algorithm)
        self.stopped_at = None
        if bank:
            enable_winner_bank(env, self.curriculum, self.schedule, bank_candidates)
        B = env.num_envs
        self.L = episode_bound(env.max_dim, env.toroidal)
        kw = dict(device=self.device)
        self.t = torch.zeros(B, dtype=torch.int32, **kw)
        self.act_out = torch.zeros(B, dtype=torch.int32, **kw)
        self.fin_id = torch.zeros(B, dtype=torch.int32, **kw)
        self.fin_off = torch.zeros(B, dtype=torch.int64, **kw)
        self.fin_len = torch.zeros(B, dtype=torch.int32, **kw)
        self.fin_count = torch.zeros(1, dtype=torch.int32, **kw)
        # episodes, wins, dropped 1-step episodes, record-buffer overflows (an error at update)
        self.stats = torch.zeros(4, dtype=torch.int64, **kw)
        self.lib = N.load()
        self.archive = None
        if archive is not None:
            self.archive = attach_pool(env, archive, archive_groups)
            self.archive.record(stamp=0)  # the first mazes (simple_maze_env.py:34)

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

    def _live(self, L=None):
        """[B, L] mask of the rows the running episodes have recorded: row j of instance i is
        live while j < t[i]."""
        L = self.L if L is None else L
        return torch.arange(L, device=self.device)[None, :] < self.t[:, None].long()

    def _scan(self, r64, terminated, truncated, rec_r, fill_ptr, total_ptr):
        """mz_ppo_scan on the step's outcome: the float64 reward into rec_r at t[i], t[i] += 1,
        the finished episodes' list with their offsets from the row counter at fill_ptr (the
        appended total at total_ptr), the counters."""
        N.check(self.lib.mz_ppo_scan(
            r64.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), self.env.num_envs, self.L,
            self.t.data_ptr(), rec_r.data_ptr(), self.fin_id.data_ptr(), self.fin_off.data_ptr(),
            self.fin_len.data_ptr(), self.fin_count.data_ptr(), fill_ptr, total_ptr,
            self.stats.data_ptr(), self._stream()))

    def _reset_winners(self):
        """change_algorithm for the winners, the reset (winners get new mazes, truncated
        instances restart theirs), update_maze's sizes and the max-shape retirements; with a
        pool, env.mazes.append(maze) for the winners' new mazes (simple_maze_env.py:91), stamped
        with the act counter after this step's act."""
        arch, env = self.archive, self.env
        if arch is None:
            return reset_winners(env, self.schedule)
        # the winners that will receive a new maze (the reset clears the flags): all of them, or
        # under per-instance sizes those whose next size is not 0 (update_maze past max_shape
        # appends nothing)
        rd = env._regen_dims
        new_maze = env.terminated.clone() if rd is None else \
            (env.terminated.bool() & (rd > 0)).to(torch.uint8)
        won = reset_winners(env, self.schedule)
        arch.record(new_maze, stamp=self.counter)
        return won

    def summary(self):
        """Host-side counts (synchronises): the vector steps, the max-shape stop, the win
        schedule's summary and the pool's fill — capacity, recorded, held, dropped; a population's
        set reports the last three per learner."""
        out = {"vector_steps": self.counter, "stopped_at": self.stopped_at,
               "schedule": None if self.schedule is None else self.schedule.summary(),
               "archive": None}
        a = self.archive
        if a is not None:
            count, held, dropped = torch.stack([a.count, a.held, a.dropped]).tolist()
            out["archive"] = {"capacity": a.capacity, "recorded": count, "held": held,
                              "dropped": dropped}
            if isinstance(a, MazePoolSet):
                out["archive"]["learners"] = a.groups
        return out

    def _train_step(self, k, n):
        self.vector_step()

    def _log_fields(self):
        return {}

    def train(self, vector_steps, log_every=0, log=print):
        t0 = time.perf_counter()
        sch = self.schedule
        for k in range(vector_steps):
            self._train_step(k, vector_steps)
            # the reference trainers' max-shape stop, once every instance reached it
            if max_shape_stop(sch, k):
                self.stopped_at = k + 1
                break
            if log_every and (k + 1) % log_every == 0 and log:
                log(dict(step=k + 1, episodes=self.episodes, wins=self.wins, updates=self.updates,
                         **self._log_fields(), seconds=round(time.perf_counter() - t0, 2)))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # ---- checkpoint / resume (mazerl/checkpoint.py) -------------------------------------------
    def _save_common(self):
        """The run between two vector steps, the part every trainer saves alike: the shape, the
        schedule, the in-flight episodes' records (only each instance's first t[i] rows of the
        [B, L] buffers), the counters and the env."""
        torch.cuda.synchronize(self.device)
        live = self._live()
        sd = {"format": self._FORMAT, **{k: getattr(self, k) for k in self._SHAPE},
              "schedule": None if self.schedule is None else self.schedule.state_dict(),
              "t": self.t.clone(),
              "records": {k: getattr(self, k)[:, :self.L][live] for k in self._REC},
              "stats": self.stats.clone(),
              "counters": {k: getattr(self, k) for k in self._COUNTERS},
              "env": self.env.state_dict()}
        if self.archive is not None:  # (a trainer without a pool writes the keys it always wrote)
            sd["archive"] = self.archive.state_dict()
        return sd

    def _check_archive(self, sd):
        """ValueError unless `sd` and this trainer agree in having a pool, and in its kind,
        geometry, capacity and group count (nothing is changed)."""
        if ("archive" in sd) != (self.archive is not None):
            raise ValueError("the saved trainer and this one differ in having an explored-maze "
                             "pool (archive=)")
        if self.archive is not None:
            self.archive.check_state_dict(sd["archive"])

    def _load_common(self, sd):
        name = type(self).__name__
        if sd.get("format") != self._FORMAT or any(sd[k] != getattr(self, k) for k in self._SHAPE):
            raise ValueError(f"not a {name} state_dict of this shape")
        if (sd["schedule"] is None) != (self.schedule is None):
            raise ValueError("curriculum / growth differ from the saved trainer's")
        self._check_archive(sd)  # (before anything changes)
        self.env.load_state_dict(sd["env"])
        if self.schedule is not None:
            self.schedule.load_state_dict(sd["schedule"])
        self.t.copy_(sd["t"])
        live = self._live()
        for k in self._REC:
            getattr(self, k)[:, :self.L][live] = sd["records"][k].to(self.device)
        self.stats.copy_(sd["stats"])
        for k, v in sd["counters"].items():
            setattr(self, k, int(v))
        if self.archive is not None:
            self.archive.load_state_dict(sd["archive"])


class PooledEpisodicTrainer(EpisodicTrainer):
    """The update pool of the on-policy trainers. A subclass sets _POOL_COLS, the pool's columns
    as (name, trailing shape, dtype), and _POOL, their names; its record of the rewards is b_r
    and its finish launch _finish()."""
    _SHAPE = ("L", "cap")

    def __init__(self, env, device, rows, pool_capacity=None, allreduce=None, **schedule_kw):
        """rows: the pool rows that make an update due; allreduce: the gradient all-reduce of a
        data-parallel run (the ranks then decide together, _due)."""
        if env.window_bits is None or env.reward64 is None:
            raise ValueError(f"{type(self).__name__} needs an env with window_bits=True, "
                             "reward64=True")
        super().__init__(env, device, **schedule_kw)
        from ..gemm_tuning import enable as _tuned_gemms
        _tuned_gemms(self.device)  # the tuned f32 GEMM choices (gemm_tuning.py)
        kw = dict(device=self.device)
        # Fill bound at an update: < rows + what the w <= 5 vector steps between a check's issue
        # and its use can append (an instance appends <= L + w rows over w steps: one episode of
        # <= L steps ending in the window plus episodes inside it); 2 B L also leaves room for
        # ranks that fill at different rates
        self.cap = int(pool_capacity or int(rows) + 2 * env.num_envs * self.L)
        for name, shape, dtype in self._POOL_COLS:
            setattr(self, name, torch.zeros(self.cap, *shape, dtype=dtype, **kw))
        self.pool_fill = torch.zeros(1, dtype=torch.int64, **kw)
        self.pool_total = torch.zeros(1, dtype=torch.int64, **kw)
        self._total_host = torch.zeros(1, dtype=torch.int64, pin_memory=True)
        self._total_ev = None
        self.allreduce = allreduce
        self.calls = 0  # _due() calls; a pool check is issued every check_every of them
        self.check_every = 1 if allreduce is None else 4

    def _cols(self, lo, hi):
        return tuple(getattr(self, k)[lo:hi] for k in self._POOL)

    def _scan_finish(self, reward64=None, terminated=None, truncated=None):
        """The step's outcome (default: the env's output tensors) -> records, finished episodes
        -> pool."""
        env = self.env
        self._scan(env.reward64 if reward64 is None else reward64,
                   env.terminated if terminated is None else terminated,
                   env.truncated if truncated is None else truncated,
                   self.b_r, self.pool_fill.data_ptr(), self.pool_total.data_ptr())
        self._finish()

    def _mark_total(self):
        self._total_ev = torch.cuda.Event()
        self._total_ev.record()

    def _due(self, threshold):
        """True when the pool held >= threshold rows when the last check was issued (the host
        copy of the appended total lands while the next vector step runs; it only grows, so a
        late look never overshoots). A check is issued every `check_every` vector steps (1 on
        one rank; with a gradient all-reduce every 4th step, and the copy is the MIN over the
        ranks, so all ranks decide alike with one small collective per 4 vector steps: the pool's
        capacity covers the 2 L rows per instance that the delay can add)."""
        due = False
        if self._total_ev is not None:
            self._total_ev.synchronize()
            due = int(self._total_host[0]) - self.consumed >= threshold
            self._total_ev = None
        if self.calls % self.check_every == 0:
            src = self.pool_total
            if self.allreduce is not None:
                import torch.distributed as dist
                src = self.pool_total.clone()
                dist.all_reduce(src, op=dist.ReduceOp.MIN)
            self._total_host.copy_(src, non_blocking=True)
            self._mark_total()
        self.calls += 1
        return due

    def _save_common(self):
        """... and the update pool's filled rows."""
        sd = super()._save_common()
        fill = int(self.pool_fill.item())
        sd.update({"pool_fill": fill,
                   "pool": {k: getattr(self, k)[:fill].clone() for k in self._POOL},
                   "pool_total": self.pool_total.clone(),
                   # the appended total the next _due() reads (copied one vector step late)
                   "total_host": int(self._total_host[0]) if self._total_ev is not None else None})
        return sd

    def _load_common(self, sd):
        super()._load_common(sd)
        fill = int(sd["pool_fill"])
        for k in self._POOL:
            getattr(self, k)[:fill].copy_(sd["pool"][k])
        self.pool_fill.fill_(fill)
        self.pool_total.copy_(sd["pool_total"])
        self._total_ev = None
        if sd["total_host"] is not None:  # what the saved trainer's next _due() would have read
            self._total_host[0] = int(sd["total_host"])
            self._mark_total()
