"""Config 1 vectorised: the reference's tabular loop, OffPolicyTrainer (lib/trainers/
off_policy_trainer.py:11-133), for a population of Q-learners (mazerl.agents.vector_q.VectorQAgent)
over the instances of one VectorMazeEnv. No host synchronisation inside the training loop.

vector_step() is one step of every instance's episode loop (:38-51): act, env.step, update
(which also ends episodes: gamma +- eta, counters), then the reset of the instances whose episode
ended — a win gives that instance a new maze (update_maze, :71), a loss replays the same maze
(the protocol of VectorOffPolicyTrainer). evaluate() is test() (:84-119), one episode per
instance.

archive= keeps what the reference env keeps in `env.mazes` — each instance's first maze and every
update_maze() replacement (simple_maze_env.py:34,91) — in a device-resident MazeArchive, and
evaluate_explored() is test(n, new=False) over them (:84-119, the README's "W/R labirinti
esplorati"). growth= is the variable-size envs' update_maze (simple_variable_maze_env.py:93-112,
toroidal_variable_maze_env.py:113-131) with the trainer's max-shape stop (:60-75), per instance,
through the WinSchedule the neural trainers use. The tabular trainer's change_algorithm is
commented out in the reference (:70) and is not offered here.
"""
import time

import torch

from ..archive import MazeArchive, instance_algorithms
from .schedule import WinSchedule

_FORMAT = "mazerl.VectorTabularTrainer/1"


class VectorTabularTrainer:
    def __init__(self, env, agent, regen_won=True, keep_flags=False, grow_every=0, archive=None,
                 growth=None):
        """keep_flags: keep each step's terminated / truncated flags in self.terminated /
        self.truncated (the reset that follows clears the env's own; two copies per step).
        grow_every (hashed agents; 0: never): every grow_every vector steps read the largest
        load (one synchronisation) and double the capacity C while it is above C / 2. After a
        check every load is <= C / 2 and a table gains at most one key per instance per step, so
        with m instances on the most-shared table a load stays <= C / 2 + grow_every * m until
        the next check: grow_every * m <= C / 2 is required (m = 1 on independent tables), and
        then no table ever fills and no update is dropped. A dense agent ignores grow_every.
        archive (None: off): an int K — a MazeArchive(env, K) — or a MazeArchive of this env.
        Every instance's current maze is recorded now, and after each reset the winners that
        received a new maze record it, so an instance's newest entry is always its current maze
        (with regen_won=False only the first maze is ever recorded; evaluate(new=True) replaces
        the env's mazes without recording them, as update_new_maze does: call it last).
        growth (None: off) = (start, max_dim), every instance holding a maze of size `start`: a
        winner's next maze is 4 larger while that is <= max_dim; a win at max_dim keeps the maze
        and retires the instance; train() returns once every instance is retired."""
        if agent.env is not env:
            raise ValueError("the agent was built for another env")
        self.grow_every = int(grow_every)
        if self.grow_every < 0:
            raise ValueError("grow_every must be >= 0")
        if self.grow_every and getattr(agent, "hashed", False):
            m = 1 if agent.table_of is None else \
                int(torch.bincount(agent.table_of.to(torch.int64)).max())
            if self.grow_every * m > agent.capacity // 2:
                raise ValueError(f"grow_every {self.grow_every} x {m} instances per table "
                                 f"exceeds capacity / 2 = {agent.capacity // 2}: a table could "
                                 f"fill between two checks")
        else:
            self.grow_every = 0
        self.env, self.agent = env, agent
        self.regen_won = bool(regen_won)
        self.vector_steps = 0
        self.evals = 0
        self.stopped_at = None  # vector step of the max-shape stop (growth), if it came
        self.terminated = self.truncated = None
        if keep_flags:
            self.terminated = torch.zeros_like(env.terminated)
            self.truncated = torch.zeros_like(env.truncated)
        if growth is not None:
            if not self.regen_won:
                raise ValueError("growth needs regen_won=True: the growth is the winner's new maze")
            sizes = env.meta()[:, 0]
            if bool((sizes != int(growth[0])).any()):
                raise ValueError(f"growth {tuple(growth)}: every instance must hold a maze of "
                                 f"size {int(growth[0])}")
        self.archive = None
        if archive is not None:
            if isinstance(archive, MazeArchive):
                if archive.env is not env:
                    raise ValueError("the archive was built for another env")
                self.archive = archive
            else:
                self.archive = MazeArchive(env, archive)
            self.archive.record()  # the first maze (simple_maze_env.py:34)
        self.schedule = None
        if growth is not None:
            # the schedule carries each instance's algorithm id (its summary counts mazes by
            # it, and loading a checkpoint sets the env's from it): the handle's own ids, as a
            # push records them — generate(algorithm=...) / set_algorithm() decided them
            self.schedule = WinSchedule(env, None, growth, algorithm=instance_algorithms(env))

    @property
    def launches_per_step(self):
        """Device launches one vector_step() issues: act + steps_done advance, the env step (and
        the memset of its done count, for an env with a done list), the update (two passes on
        shared tables; an agent with update_launches: that many), the flag copies of keep_flags,
        the reset; with an archive the copy of the winners' flags (taken from keep_flags' copy
        when there is one) and the push. A growth schedule's torch bookkeeping is not counted."""
        env = self.env
        extra = 0
        if self.archive is not None and self.regen_won:
            extra = 1 + int(self.terminated is None and self.schedule is None)
        return 2 + 1 + int(env._out.done_count is not None) + \
            getattr(self.agent, "update_launches", 1 if self.agent.table_of is None else 2) + \
            (2 if self.terminated is not None else 0) + 1 + extra

    def vector_step(self):
        env, agent = self.env, self.agent
        env.step(agent.act())
        agent.update()
        if self.terminated is not None:
            self.terminated.copy_(env.terminated)
            self.truncated.copy_(env.truncated)
        sch, arch = self.schedule, self.archive if self.regen_won else None
        won = None
        if sch is not None:
            won = env.terminated.bool()
            sch.before_reset(won)
        elif arch is not None:
            won = self.terminated if self.terminated is not None else env.terminated.clone()
        env.reset_done(regen_won=self.regen_won)
        if arch is not None:
            # the winners that received a new maze: all of them, or under per-instance sizes
            # those whose next size was not 0 (update_maze past max_shape appends nothing)
            rd = env._regen_dims
            arch.record(won if rd is None else won.bool() & (rd > 0))
        if sch is not None:
            sch.after_reset(won)
        self.vector_steps += 1
        if self.grow_every and self.vector_steps % self.grow_every == 0:
            agent.grow()

    def train(self, vector_steps):
        """vector_steps steps of every instance; returns the seconds they took (one
        synchronisation, after the loop). With growth the loop ends at the first check (every
        32nd vector step of this trainer, one host read) that finds every instance retired —
        the reference's max-shape stop; self.stopped_at is that vector step."""
        t0 = time.perf_counter()
        sch = self.schedule
        for _ in range(int(vector_steps)):
            if self.stopped_at is not None:
                break
            self.vector_step()
            if sch is not None and self.vector_steps % 32 == 0 and sch.all_retired():
                self.stopped_at = self.vector_steps
        torch.cuda.synchronize(self.env.device)
        return time.perf_counter() - t0

    def evaluate(self, new, algorithm="r-prim"):
        """One episode per instance with act() and no updates (steps_done keeps advancing, as in
        the reference's test()): new=True on freshly generated mazes (they replace the env's, as
        update_new_maze does; under growth each at the size its instance has reached, with one
        host read of the sizes — the variable-size env's update_new_maze draws a random odd size
        in [START_SHAPE, max_shape) instead, simple_variable_maze_env.py:135-147, sizes the growth
        never trains on), new=False on the mazes currently loaded, each from its start.
        An instance idles once its episode is over. Returns (win flags: bool [n] device tensor,
        win rate)."""
        env, agent = self.env, self.agent
        if new:
            self.evals += 1
            seed = (env.seed + 0xE7A10000 + self.evals * env.num_envs) & ((1 << 63) - 1)
            if self.schedule is None:
                env.generate(algorithm=algorithm, seed=seed)
            else:
                dim = self.schedule.dim
                for n in self.schedule.sizes():
                    ids = torch.nonzero(dim == n).reshape(-1).to(torch.int32)
                    if ids.numel():
                        env.generate(env_ids=ids, algorithm=algorithm, dim=n, seed=seed)
        env.reset()
        horizon = int(env.meta()[:, 5].max()) + 1  # truncation comes at max_steps + 1 steps
        won = torch.zeros(env.num_envs, dtype=torch.bool, device=env.device)
        active = torch.ones(env.num_envs, dtype=torch.uint8, device=env.device)
        for _ in range(horizon):
            env.step(agent.act(active=active))
            won |= env.terminated.bool()
            active.masked_fill_((env.terminated | env.truncated).bool(), 0)
        env.reset()
        agent.cum.zero_()  # the reset cut every running episode
        return won, float(won.double().mean())

    def evaluate_explored(self):
        """The reference's test(n, new=False) (off_policy_trainer.py:84-119) over every maze the
        archive holds: in round k = 0, 1, ... every instance with more than k held entries gets
        its k-th oldest one back (update_visited_maze), is reset and plays one episode with act()
        and no updates (steps_done keeps advancing, as in evaluate()); the others idle. A
        round's horizon is the largest max_steps + 1 among its playing instances. Afterwards
        every instance's newest entry — its training maze — is loaded back and reset, and
        agent.cum is zeroed. One host read per round (the horizon) and one of held.max(). An
        entry the load kernel refused (a corrupt checkpoint) would leave another maze in place of
        the archived one: the archive's error count is read with held.max() and with the result,
        and a RuntimeError is raised if it grew.
        Returns (won bool [n, K], played bool [n, K] — device tensors, K = held.max() — and the
        win rate over the played episodes)."""
        arch = self.archive
        if arch is None:
            raise ValueError("evaluate_explored() replays the archive: build the trainer with "
                             "archive=")
        env, agent = self.env, self.agent
        n = env.num_envs
        K, errors = torch.stack([arch.held.max(), arch.errors[0]]).tolist()
        won = torch.zeros(n, K, dtype=torch.bool, device=env.device)
        played = torch.zeros(n, K, dtype=torch.bool, device=env.device)
        for k in range(K):
            slot = arch.entry_slot(k)
            arch.load(env, slot)
            env.reset()
            plays = slot >= 0
            played[:, k] = plays
            horizon = int(torch.where(plays, env.meta()[:, 5], 0).max()) + 1
            active = plays.to(torch.uint8)
            for _ in range(horizon):
                env.step(agent.act(active=active))
                won[:, k] |= env.terminated.bool() & active.bool()
                active.masked_fill_((env.terminated | env.truncated).bool(), 0)
        arch.load(env, arch.newest_slot())
        env.reset()
        agent.cum.zero_()  # the resets cut every running episode
        games, wins, refused = torch.stack([played.sum(), won.sum(), arch.errors[0] - errors]).tolist()
        if refused:
            raise RuntimeError(f"{refused} archive entries were refused by mz_archive_load "
                               f"(archive.errors): the archive is corrupt, the result is void")
        return won, played, (wins / games if games else 0.0)

    def summary(self):
        """Host-side counts (synchronises): the vector steps, the max-shape stop, the growth
        schedule's summary and the archive's fill."""
        out = {"vector_steps": self.vector_steps, "stopped_at": self.stopped_at,
               "schedule": None if self.schedule is None else self.schedule.summary(),
               "archive": None}
        if self.archive is not None:
            a = self.archive
            out["archive"] = {"slots": a.slots, "recorded": int(a.count.sum()),
                              "held": int(a.held.sum()), "dropped": int(a.dropped.sum())}
        return out

    # -------------------------------------------------------------------------------------------
    def state_dict(self):
        """Checkpoint of the whole run (mazerl/checkpoint.py): the agent, the env, the archive,
        the growth schedule and this trainer's counters. train() calls after a load_state_dict
        continue exactly as further train() calls on the saved trainer would have."""
        return {"format": _FORMAT, "vector_steps": self.vector_steps, "evals": self.evals,
                "stopped_at": self.stopped_at, "regen_won": self.regen_won,
                "grow_every": self.grow_every,
                "agent": self.agent.state_dict(), "env": self.env.state_dict(),
                "archive": None if self.archive is None else self.archive.state_dict(),
                "schedule": None if self.schedule is None else self.schedule.state_dict()}

    def load_state_dict(self, sd):
        if sd.get("format") != _FORMAT:
            raise ValueError("not a VectorTabularTrainer state_dict")
        if bool(sd["regen_won"]) != self.regen_won or \
                (sd["archive"] is None) != (self.archive is None) or \
                (sd["schedule"] is None) != (self.schedule is None):
            raise ValueError("regen_won / archive / growth differ from the saved trainer's")
        if self.archive is not None:  # (before anything changes)
            self.archive.check_state_dict(sd["archive"])
        self.env.load_state_dict(sd["env"])
        self.agent.load_state_dict(sd["agent"])
        if self.archive is not None:
            self.archive.load_state_dict(sd["archive"])
        if self.schedule is not None:
            self.schedule.load_state_dict(sd["schedule"])
        self.vector_steps, self.evals = int(sd["vector_steps"]), int(sd["evals"])
        self.stopped_at = None if sd["stopped_at"] is None else int(sd["stopped_at"])
