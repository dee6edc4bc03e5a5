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

storage="hash" keeps each table as the reference's own sparse structure instead (its defaultdict
holds only the states met): an open-addressing hash table of `capacity` slots in HBM, keyed by
the same state index (csrc/mz_qtab.hip; hash_slot is the mirror of its hash). A dense table is
452 MB at 41x41 and 6.9 GB at 81x81; a hashed one is 36 B per slot, so thousands of learners fit
at the reference's maze sizes. Acting never inserts; an update inserts its state's key. A full
table drops the value update and counts it in `overflow` — size `capacity` for the states a
learner meets, or let VectorTabularTrainer(grow_every=...) double it when it is half full.
"""
import math

import torch

from .. import _native as N

_FORMAT = "mazerl.VectorQAgent/1"
_FORMAT_HASH = "mazerl.VectorQAgent/2"
MIN_CAPACITY, MAX_CAPACITY = 16, 1 << 30


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


def _check_capacity(capacity):
    c = int(capacity)
    if not MIN_CAPACITY <= c <= MAX_CAPACITY or c & (c - 1):
        raise ValueError(f"capacity {capacity} is not a power of two in "
                         f"[{MIN_CAPACITY}, {MAX_CAPACITY}]")
    return c


def hash_slot(key, capacity):
    """The slot a hashed table of `capacity` slots probes first for `key` (a state_index) — the
    pure-Python mirror of the kernels' hash: (uint32(key) * 0x9E3779B1) >> (32 - log2 capacity).
    The probe goes on at (slot + 1) % capacity."""
    c = _check_capacity(capacity)
    return ((int(key) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - (c.bit_length() - 1))


class VectorQAgent:
    # what VectorDoubleQAgent (vector_dq.py) changes: a state's values ([4]; there [2, 4]), the
    # entry points' prefix and the checkpoint formats
    _ROW = (4,)
    _ABI = "mz_qtab"
    _FORMATS = (_FORMAT, _FORMAT_HASH)  # dense, hashed

    def __init__(self, env, tables=None, learning_rate=0.1, initial_epsilon=0.95,
                 epsilon_decay=40.0, final_epsilon=0.05, discount_factor=0.7, eta=0.01, seed=0,
                 max_bytes=8 << 30, storage="dense", capacity=None):
        """env: a VectorMazeEnv(enrich=False, reward64=True). tables: None — one table per
        instance; an int T — instance i uses table i % T; a tensor / sequence — the explicit map
        (tables = its maximum + 1). Each hyper-parameter: a scalar or one value per table.
        storage: "dense" (self.q [T, rows, 4]) or "hash" with capacity, a power of two in
        [16, 2^30]: self.keys int32 [T, C] (-1 = empty), self.vals float64 [T, C, 4], self.load
        int32 [T] (occupied slots), self.overflow int64 [T] (updates a full table dropped)."""
        if storage not in ("dense", "hash"):
            raise ValueError(f"storage {storage!r}: 'dense' or 'hash'")
        self.storage = storage
        if storage == "hash":
            if capacity is None:
                raise ValueError("storage='hash' needs a capacity")
            capacity = _check_capacity(capacity)
        elif capacity is not None:
            raise ValueError("capacity belongs to storage='hash'")
        name = type(self).__name__
        if getattr(env, "enrich", True):
            raise ValueError(f"{name} needs plain observations: VectorMazeEnv(enrich=False)")
        if getattr(env, "reward64", None) is None:
            raise ValueError(f"{name} needs the float64 reward: VectorMazeEnv(reward64=True)")
        if getattr(env, "_host", None) is not None:
            raise ValueError(f"{name} needs device outputs (host_scalars=False)")
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
        self.max_bytes = int(max_bytes)
        self.num_tables = T
        if storage == "hash":
            self._check_bytes(capacity)
        else:
            nbytes = T * self.rows * self._row_bytes
            if nbytes > self.max_bytes:
                raise MemoryError(f"{T} tables x {self.rows} rows x {self._row_bytes} B = "
                                  f"{nbytes} B exceeds "
                                  f"max_bytes = {self.max_bytes}")
        dev = self.device
        self.table_of = None if table_of is None else table_of.to(dev, torch.int32).contiguous()
        if storage == "hash":
            self.capacity = capacity
            self.keys, self.vals = self._fresh(capacity)
            self.load = torch.zeros(T, dtype=torch.int32, device=dev)
            self.overflow = torch.zeros(T, dtype=torch.int64, device=dev)
        else:
            self.q = torch.zeros(T, self.rows, *self._ROW, dtype=torch.float64, device=dev)

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
    @property
    def hashed(self):
        return self.storage == "hash"

    @property
    def _row_bytes(self):
        return 8 * math.prod(self._ROW)

    def _fn(self, name):
        return getattr(self.lib, self._ABI + name)

    def _check_bytes(self, capacity):
        T = self.num_tables
        slot = 4 + self._row_bytes
        nbytes = T * capacity * slot + T * 12
        if nbytes > self.max_bytes:
            raise MemoryError(f"{T} tables x {capacity} slots x {slot} B + counters = {nbytes} B "
                              f"exceeds max_bytes = {self.max_bytes}")

    def _fresh(self, capacity):
        T, dev = self.num_tables, self.device
        return (torch.full((T, capacity), -1, dtype=torch.int32, device=dev),
                torch.zeros(T, capacity, *self._ROW, dtype=torch.float64, device=dev))

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
        head = (self.env.obs6.data_ptr(), self.n, self.max_dim, _ptr(self.table_of),
                self.num_tables, _ptr(a))
        tail = (self.steps_done.data_ptr(), self.eps_init.data_ptr(), self.eps_final.data_ptr(),
                self.eps_decay.data_ptr(), self.seed & 0xFFFFFFFFFFFFFFFF,
                self.counter & 0xFFFFFFFFFFFFFFFF, self.actions.data_ptr(), self.sidx.data_ptr(),
                self._stream())
        if self.hashed:
            N.check(self._fn("_hash_act")(*head, self.keys.data_ptr(), self.vals.data_ptr(),
                                          self.capacity, *tail))
        else:
            N.check(self._fn("_act")(*head, self.q.data_ptr(), *tail))
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
        head = (env.obs6.data_ptr(), self.n, self.max_dim, _ptr(self.table_of), self.num_tables)
        tail = (self.sidx.data_ptr(), a.data_ptr(), env.reward64.data_ptr(),
                env.terminated.data_ptr(), env.truncated.data_ptr(), self.gamma.data_ptr(),
                self.lr.data_ptr(), self.eta.data_ptr(), self.cum.data_ptr(),
                self.episodes.data_ptr(), self.wins.data_ptr(), _ptr(self._td),
                int(bool(episode_end)), self._stream())
        if self.hashed:
            N.check(self.lib.mz_qtab_hash_update(
                *head, self.keys.data_ptr(), self.vals.data_ptr(), self.capacity,
                self.load.data_ptr(), self.overflow.data_ptr(), *tail))
        else:
            N.check(self.lib.mz_qtab_update(*head, self.q.data_ptr(), *tail))

    # -------------------------------------------------------------------------------------------
    def state_index(self, agent, target, best_dir):
        return state_index(self.max_dim, agent, target, best_dir)

    def q_row(self, table, agent, target, best_dir):
        """The 4 Q-values of one state of one table (float64 device tensor; dense: a view,
        hashed: a copy — zeros for a state the table does not hold)."""
        s = self.state_index(agent, target, best_dir)
        if self.hashed:
            return self.lookup([int(table)], [s])[0][0]
        return self.q[int(table), s]

    def lookup(self, tables, keys):
        """Hashed tables: for m (table, state index) pairs, (rows float64 [m, 4] — zeros where
        the key is absent, slots int32 [m] — -1 where absent), device tensors."""
        if not self.hashed:
            raise ValueError("lookup() reads hashed tables (storage='hash')")
        dev = self.device
        t = torch.as_tensor(tables).to(dev, torch.int32).reshape(-1).contiguous()
        k = torch.as_tensor(keys).to(dev, torch.int64).reshape(-1).contiguous()
        if t.numel() != k.numel():
            raise ValueError("one table per key")
        m = int(k.numel())
        rows = torch.zeros(m, *self._ROW, dtype=torch.float64, device=dev)
        slots = torch.full((m,), -1, dtype=torch.int32, device=dev)
        N.check(self._fn("_hash_lookup")(
            self.keys.data_ptr(), self.vals.data_ptr(), self.capacity, self.num_tables,
            t.data_ptr(), k.data_ptr(), m, rows.data_ptr(), slots.data_ptr(), self._stream()))
        return rows, slots

    def items(self, table):
        """What one table holds: (state indices int64 [k], rows float64 [k, 4]), sorted by
        index. Dense: the rows that are not all zero; hashed: the occupied slots (a written row
        whose values are all zero included)."""
        t = int(table)
        if self.hashed:
            idx = torch.nonzero(self.keys[t] >= 0).reshape(-1)
            keys = self.keys[t][idx].to(torch.int64)
            rows = self.vals[t][idx]
        else:
            keys = torch.nonzero(self.q[t].ne(0).flatten(1).any(1)).reshape(-1)
            rows = self.q[t][keys]
        order = torch.argsort(keys)
        return keys[order], rows[order]

    def to_dense(self, table):
        """One table as a dense [rows, 4] float64 tensor (a copy; for small pitches)."""
        if not self.hashed:
            return self.q[int(table)].clone()
        keys, rows = self.items(table)
        out = torch.zeros(self.rows, *self._ROW, dtype=torch.float64, device=self.device)
        out[keys] = rows
        return out

    def rehash(self, capacity):
        """Move every hashed table to `capacity` slots: a power of two in [16, 2^30] above the
        largest load (one host read). Contents, load and overflow carry over."""
        if not self.hashed:
            raise ValueError("rehash() belongs to storage='hash'")
        capacity = _check_capacity(capacity)
        top = int(self.load.max())
        if capacity <= top:
            raise ValueError(f"capacity {capacity} must exceed the largest load, {top}")
        self._check_bytes(capacity)
        keys, vals = self._fresh(capacity)
        N.check(self._fn("_hash_rehash")(
            self.keys.data_ptr(), self.vals.data_ptr(), self.capacity, keys.data_ptr(),
            vals.data_ptr(), capacity, self.num_tables, self.overflow.data_ptr(), self._stream()))
        self.keys, self.vals, self.capacity = keys, vals, capacity

    def grow(self):
        """Double the capacity while the fullest hashed table is more than half full (one host
        read). Returns the capacity."""
        top = int(self.load.max())
        c = self.capacity
        while top > c // 2:
            c *= 2
        if c != self.capacity:
            self.rehash(c)
        return self.capacity

    def epsilon(self):
        """The next act()'s epsilon per table (float64 device tensor; torch's exp)."""
        return self.eps_final + (self.eps_init - self.eps_final) * \
            torch.exp(-1.0 * self.steps_done.to(torch.float64) / self.eps_decay)

    _COMMON = ("gamma", "steps_done", "cum", "wins", "episodes", "lr", "eta", "eps_init",
               "eps_final", "eps_decay", "sidx", "actions")
    _TENSORS = ("q",) + _COMMON                                  # format /1, dense
    _TENSORS_HASH = ("keys", "vals", "load", "overflow") + _COMMON  # format /2, hashed
    _COUNTERS = ("seed", "counter")  # host integers

    def state_dict(self):
        names = self._TENSORS_HASH if self.hashed else self._TENSORS
        sd = {k: getattr(self, k).clone() for k in names}
        sd.update(format=self._FORMATS[self.hashed], max_dim=self.max_dim,
                  num_tables=self.num_tables,
                  table_of=None if self.table_of is None else self.table_of.clone())
        sd.update({k: getattr(self, k) for k in self._COUNTERS})
        if self.hashed:
            sd["capacity"] = self.capacity
        return sd

    def load_state_dict(self, sd):
        """Dense agents load format /1, hashed agents format /2 (the saved capacity replaces
        this agent's)."""
        fmt = sd.get("format")
        if fmt not in self._FORMATS:
            raise ValueError(f"not a {type(self).__name__} state_dict")
        if fmt != self._FORMATS[self.hashed]:
            raise ValueError(f"a {fmt} state_dict does not load into a {self.storage} agent")
        if sd["max_dim"] != self.max_dim or sd["num_tables"] != self.num_tables or \
                (sd["table_of"] is None) != (self.table_of is None) or \
                (not self.hashed and tuple(sd["q"].shape) != tuple(self.q.shape)):
            raise ValueError("the saved agent's tables do not match this agent's")
        if self.hashed:
            c = _check_capacity(sd["capacity"])
            if tuple(sd["keys"].shape) != (self.num_tables, c) or \
                    tuple(sd["vals"].shape) != (self.num_tables, c, *self._ROW):
                raise ValueError("the saved agent's tables do not match its capacity")
            if c != self.capacity:
                self._check_bytes(c)
                self.keys, self.vals = self._fresh(c)
                self.capacity = c
        if self.table_of is not None:
            if sd["table_of"].numel() != self.n:
                raise ValueError("the saved agent's table map does not match this agent's")
            self.table_of.copy_(sd["table_of"])
        for k in (self._TENSORS_HASH if self.hashed else self._TENSORS):
            getattr(self, k).copy_(sd[k])
        for k in self._COUNTERS:
            setattr(self, k, int(sd[k]))
