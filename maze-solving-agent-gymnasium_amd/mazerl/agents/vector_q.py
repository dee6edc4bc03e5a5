"""VectorQAgent — a population of the reference's tabular QAgent (agents/q_agent.py:8-79) on one
GPU: the Q-tables live in HBM and act / update are HIP kernels (csrc/mz_qtab.hip) over the plain
observations of a VectorMazeEnv, one lane per env instance, with no host round trip.

Instance i learns on table table_of[i]. One instance per table is the reference's agent bit for
bit in float64 (epsilon from steps_done, action_space.sample() exploration, np.argmax, the TD(0)
update, the per-episode gamma drift by +-eta); several instances per table is synchronous-parallel
Q-learning on a shared table: every td of a vector step is taken from the table as it stood
before the step and colliding updates add (float64 atomic adds, so the sum's last bits depend on
the arrival order unless the addends commute exactly).

A table is a dense array of 5 * max_dim^4 rows of 4 float64 (state_index gives the row of an
observation; 1.05 MB at 9x9); every hyper-parameter is a per-table device array, so a population
can sweep learning rate, gamma, eta and the epsilon schedule.
"""
import torch

from .. import _native as N

_FORMAT = "mazerl.VectorQAgent/1"


def _ptr(t):
    return None if t is None else t.data_ptr()


def table_rows(max_dim):
    """Rows of one table for the index pitch max_dim (mz_qtab_states; needs no GPU)."""
    rows = N.C.c_int64()
    N.check(N.load().mz_qtab_states(int(max_dim), N.C.byref(rows)))
    return rows.value


def _dir_class(best_dir):
    br, bc = int(best_dir[0]), int(best_dir[1])
    if br == -1 or br > 1:
        return 1
    if br == 1 or br < -1:
        return 2
    if bc == -1 or bc > 1:
        return 3
    if bc == 1 or bc < -1:
        return 4
    return 0


def state_index(max_dim, agent, target, best_dir):
    """Row of the observation (agent, target, best dir) in a table of pitch max_dim — the
    pure-Python mirror of the kernels' index: (((r P + c) P + gr) P + gc) 5 + class, where the
    class of "best dir" = agent - best_next_cell is 0 for (0, 0), 1 down (br == -1, or br > 1: the
    torus' wrapped neighbour), 2 up (br == 1 or br < -1), 3 right, 4 left (columns alike). Two
    observations of one env share a row iff the reference's str(obs) keys are equal."""
    P = int(max_dim)
    r, c, gr, gc = int(agent[0]), int(agent[1]), int(target[0]), int(target[1])
    for v in (r, c, gr, gc):
        if not 0 <= v < P:
            raise ValueError(f"coordinate {v} outside [0, {P})")
    return (((r * P + c) * P + gr) * P + gc) * 5 + _dir_class(best_dir)


class VectorQAgent:
    def __init__(self, env, tables=None, learning_rate=0.1, initial_epsilon=0.95,
                 epsilon_decay=40.0, final_epsilon=0.05, discount_factor=0.7, eta=0.01, seed=0,
                 max_bytes=8 << 30):
        """env: a VectorMazeEnv(enrich=False, reward64=True). tables: None — one table per
        instance; an int T — instance i uses table i % T; a tensor / sequence — the explicit map
        (tables = its maximum + 1). Each hyper-parameter: a scalar or one value per table."""
        if getattr(env, "enrich", True):
            raise ValueError("VectorQAgent needs plain observations: VectorMazeEnv(enrich=False)")
        if getattr(env, "reward64", None) is None:
            raise ValueError("VectorQAgent needs the float64 reward: VectorMazeEnv(reward64=True)")
        if getattr(env, "_host", None) is not None:
            raise ValueError("VectorQAgent needs device outputs (host_scalars=False)")
        self.env = env
        self.device = env.device
        self.lib = env.lib
        n = self.n = env.num_envs
        self.max_dim = env.max_dim
        self.rows = table_rows(self.max_dim)
        if tables is None:
            T, table_of = n, None
        elif isinstance(tables, int) and not isinstance(tables, bool):
            T = int(tables)
            if T < 1:
                raise ValueError("tables must be >= 1")
            table_of = torch.arange(n, dtype=torch.int64) % T
        else:
            table_of = torch.as_tensor(tables).to("cpu", torch.int64).reshape(-1)
            if table_of.numel() != n:
                raise ValueError("one table id per instance")
            if int(table_of.min()) < 0:
                raise ValueError("negative table id")
            T = int(table_of.max()) + 1
        nbytes = T * self.rows * 32
        if nbytes > int(max_bytes):
            raise MemoryError(f"{T} tables x {self.rows} rows x 32 B = {nbytes} B exceeds "
                              f"max_bytes = {int(max_bytes)}")
        self.num_tables = T
        dev = self.device
        self.table_of = None if table_of is None else table_of.to(dev, torch.int32).contiguous()
        self.q = torch.zeros(T, self.rows, 4, dtype=torch.float64, device=dev)

        def per_table(v, name):
            t = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
            if t.numel() == 1:
                t = t.expand(T)
            if t.numel() != T:
                raise ValueError(f"{name}: a scalar or one value per table ({T})")
            return t.to(dev).contiguous()

        self.lr = per_table(learning_rate, "learning_rate")
        self.eps_init = per_table(initial_epsilon, "initial_epsilon")
        self.eps_decay = per_table(epsilon_decay, "epsilon_decay")
        self.eps_final = per_table(final_epsilon, "final_epsilon")
        self.gamma = per_table(discount_factor, "discount_factor")
        self.eta = per_table(eta, "eta")
        self.steps_done = torch.zeros(T, dtype=torch.int64, device=dev)
        self.episodes = torch.zeros(T, dtype=torch.int64, device=dev)
        self.wins = torch.zeros(T, dtype=torch.int64, device=dev)
        self.cum = torch.zeros(n, dtype=torch.float64, device=dev)
        self.actions = torch.zeros(n, dtype=torch.int32, device=dev)
        self.sidx = torch.full((n,), -1, dtype=torch.int64, device=dev)
        self._td = None if table_of is None else torch.zeros(n, dtype=torch.float64, device=dev)
        self.seed = int(seed)
        self.counter = 0

    # -------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def act(self, active=None):
        """get_action for every instance on the env's current observation: the actions (int32
        [n], also kept in self.actions; self.sidx holds the rows acted from). steps_done of each
        table advances by its acting instances. active (uint8 / bool [n]): instances with 0 idle
        (action -1: the env observes only) and are not counted."""
        a = None
        if active is not None:
            a = active.to(device=self.device, dtype=torch.uint8).contiguous()
        N.check(self.lib.mz_qtab_act(
            self.env.obs6.data_ptr(), self.n, self.max_dim, _ptr(self.table_of), self.num_tables,
            _ptr(a), self.q.data_ptr(), self.steps_done.data_ptr(), self.eps_init.data_ptr(),
            self.eps_final.data_ptr(), self.eps_decay.data_ptr(),
            self.seed & 0xFFFFFFFFFFFFFFFF, self.counter & 0xFFFFFFFFFFFFFFFF,
            self.actions.data_ptr(), self.sidx.data_ptr(), self._stream()))
        self.counter += 1
        return self.actions

    def update(self, actions=None, episode_end=True):
        """QAgent.update for every instance after env.step(actions): the env's outputs are the
        reward, the flags and the next observation; the rows acted from are self.sidx (the last
        act()'s). actions: the actions stepped if they were not act()'s own. episode_end=False:
        QAgent.update alone — an ended episode neither drifts gamma nor counts."""
        env = self.env
        a = self.actions if actions is None else \
            actions.to(device=self.device, dtype=torch.int32).contiguous()
        N.check(self.lib.mz_qtab_update(
            env.obs6.data_ptr(), self.n, self.max_dim, _ptr(self.table_of), self.num_tables,
            self.q.data_ptr(), self.sidx.data_ptr(), a.data_ptr(), env.reward64.data_ptr(),
            env.terminated.data_ptr(), env.truncated.data_ptr(), self.gamma.data_ptr(),
            self.lr.data_ptr(), self.eta.data_ptr(), self.cum.data_ptr(),
            self.episodes.data_ptr(), self.wins.data_ptr(), _ptr(self._td), int(bool(episode_end)),
            self._stream()))

    # -------------------------------------------------------------------------------------------
    def state_index(self, agent, target, best_dir):
        return state_index(self.max_dim, agent, target, best_dir)

    def q_row(self, table, agent, target, best_dir):
        """The 4 Q-values of one state of one table (float64 device tensor, a view)."""
        return self.q[int(table), self.state_index(agent, target, best_dir)]

    def epsilon(self):
        """The next act()'s epsilon per table (float64 device tensor; torch's exp)."""
        return self.eps_final + (self.eps_init - self.eps_final) * \
            torch.exp(-1.0 * self.steps_done.to(torch.float64) / self.eps_decay)

    _TENSORS = ("q", "gamma", "steps_done", "cum", "wins", "episodes", "lr", "eta", "eps_init",
                "eps_final", "eps_decay", "sidx", "actions")

    def state_dict(self):
        sd = {k: getattr(self, k).clone() for k in self._TENSORS}
        sd.update(format=_FORMAT, seed=self.seed, counter=self.counter, max_dim=self.max_dim,
                  num_tables=self.num_tables,
                  table_of=None if self.table_of is None else self.table_of.clone())
        return sd

    def load_state_dict(self, sd):
        if sd.get("format") != _FORMAT:
            raise ValueError("not a VectorQAgent state_dict")
        if sd["max_dim"] != self.max_dim or sd["num_tables"] != self.num_tables or \
                tuple(sd["q"].shape) != tuple(self.q.shape) or \
                (sd["table_of"] is None) != (self.table_of is None):
            raise ValueError("the saved agent's tables do not match this agent's")
        if self.table_of is not None:
            if sd["table_of"].numel() != self.n:
                raise ValueError("the saved agent's table map does not match this agent's")
            self.table_of.copy_(sd["table_of"])
        for k in self._TENSORS:
            getattr(self, k).copy_(sd[k])
        self.seed, self.counter = int(sd["seed"]), int(sd["counter"])
