"""Config 1 vectorised: the reference's tabular loop, OffPolicyTrainer (lib/trainers/
off_policy_trainer.py:11-133), for a population of Q-learners (mazerl.agents.vector_q.VectorQAgent)
over the instances of one VectorMazeEnv. No host synchronisation inside the training loop.

vector_step() is one step of every instance's episode loop (:38-51): act, env.step, update
(which also ends episodes: gamma +- eta, counters), then the reset of the instances whose episode
ended — a win gives that instance a new maze (update_maze, :71), a loss replays the same maze
(the protocol of VectorOffPolicyTrainer). evaluate() is test() (:84-119), one episode per
instance.
"""
import time

import torch


class VectorTabularTrainer:
    def __init__(self, env, agent, regen_won=True, keep_flags=False, grow_every=0):
        """keep_flags: keep each step's terminated / truncated flags in self.terminated /
        self.truncated (the reset that follows clears the env's own; two copies per step).
        grow_every (hashed agents; 0: never): every grow_every vector steps read the largest
        load (one synchronisation) and double the capacity C while it is above C / 2. After a
        check every load is <= C / 2 and a table gains at most one key per instance per step, so
        with m instances on the most-shared table a load stays <= C / 2 + grow_every * m until
        the next check: grow_every * m <= C / 2 is required (m = 1 on independent tables), and
        then no table ever fills and no update is dropped. A dense agent ignores grow_every."""
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
        self.terminated = self.truncated = None
        if keep_flags:
            self.terminated = torch.zeros_like(env.terminated)
            self.truncated = torch.zeros_like(env.truncated)

    @property
    def launches_per_step(self):
        """Device launches one vector_step() issues: act + steps_done advance, the env step (and
        the memset of its done count, for an env with a done list), the update (two passes on
        shared tables; an agent with update_launches: that many), the flag copies of keep_flags,
        the reset."""
        env = self.env
        return 2 + 1 + int(env._out.done_count is not None) + \
            getattr(self.agent, "update_launches", 1 if self.agent.table_of is None else 2) + \
            (2 if self.terminated is not None else 0) + 1

    def vector_step(self):
        env, agent = self.env, self.agent
        env.step(agent.act())
        agent.update()
        if self.terminated is not None:
            self.terminated.copy_(env.terminated)
            self.truncated.copy_(env.truncated)
        env.reset_done(regen_won=self.regen_won)
        self.vector_steps += 1
        if self.grow_every and self.vector_steps % self.grow_every == 0:
            agent.grow()

    def train(self, vector_steps):
        """vector_steps steps of every instance; returns the seconds they took (one
        synchronisation, after the loop)."""
        t0 = time.perf_counter()
        for _ in range(int(vector_steps)):
            self.vector_step()
        torch.cuda.synchronize(self.env.device)
        return time.perf_counter() - t0

    def evaluate(self, new, algorithm="r-prim"):
        """One episode per instance with act() and no updates (steps_done keeps advancing, as in
        the reference's test()): new=True on freshly generated mazes (they replace the env's, as
        update_new_maze does), new=False on the mazes currently loaded, each from its start.
        An instance idles once its episode is over. Returns (win flags: bool [n] device tensor,
        win rate)."""
        env, agent = self.env, self.agent
        if new:
            self.evals += 1
            env.generate(algorithm=algorithm,
                         seed=(env.seed + 0xE7A10000 + self.evals * env.num_envs) & ((1 << 63) - 1))
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
