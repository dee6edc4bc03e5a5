"""MazeArchive — the mazes a population trained on, kept on the device (csrc/mz_archive.hip).

The reference env appends every maze it trains on to `env.mazes` — the first one and each
update_maze() replacement (simple_maze_env.py:34,91; simple_variable_maze_env.py:39,106) — and
OffPolicyTrainer.test(n, new=False) replays them one by one through update_visited_maze()
(off_policy_trainer.py:84-119): the "W/R labirinti esplorati" column of its README. Here a win
overwrites the instance's maze, so record() keeps it first: per instance a ring of `slots` entries,
each the maze's open cells as a bit field (pack_grid is the layout), its two meta words and its
algorithm id. load() rebuilds an entry into an instance of any env whose pitch holds it, in one
asynchronous launch with no host copy, exactly as load_mazes would build it.

The ring keeps the newest `slots` entries of an instance where the reference keeps all of them:
size `slots` for the wins expected and report `dropped`.

MazePool is one list for a whole population in exploration order (a learner that trains on B envs
at once), MazePoolSet one such list per learner of a population of learners, filled by one launch.

All archive memory is torch tensors owned by this object (the env handle keeps no pointer to
it), so an archive outlives its env, is saved by state_dict() and loads into another handle.
"""
import numpy as np
import torch

from . import _native as N

_FORMAT = "mazerl.MazeArchive/1"
_POOL_FORMAT = "mazerl.MazePool/1"
_POOLS_FORMAT = "mazerl.MazePoolSet/1"


def archive_words(max_dim):
    """int32 words of one entry's bit field for the pitch max_dim (mz_archive_words; no GPU)."""
    w = N.C.c_int32()
    N.check(N.load().mz_archive_words(int(max_dim), N.C.byref(w)))
    return w.value


def pack_grid(grid, pitch=None):
    """The bit field of one maze (pure numpy mirror of the kernels' layout): grid [N, N] with 0 =
    wall, 1 / 2 = open -> int32 [ceil(pitch^2 / 32)]; bit (r N + c) & 31 of word (r N + c) >> 5 is
    cell (r, c), indexed with the maze's own N; every bit past N N is 0. pitch: default N."""
    g = np.asarray(grid)
    n = g.shape[0]
    if g.ndim != 2 or g.shape[1] != n:
        raise ValueError("a square grid")
    P = n if pitch is None else int(pitch)
    if n > P:
        raise ValueError(f"a {n} x {n} maze does not fit the pitch {P}")
    W = (P * P + 31) // 32
    flat = np.zeros(W * 32, np.uint8)
    flat[:n * n] = (g.reshape(-1) != 0)
    return np.packbits(flat, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def unpack_grid(bits, n, goal=None):
    """pack_grid's inverse for a maze of size n: uint8 [n, n] with 1 = open, and 2 at `goal`
    (row, column) when given — the grid as env.grid() and the fixtures hold it."""
    n = int(n)
    b = np.ascontiguousarray(np.asarray(bits).reshape(-1).astype(np.int32)).view(np.uint32)
    if n * n > b.size * 32:
        raise ValueError(f"{b.size} words hold no {n} x {n} maze")
    flat = np.unpackbits(b.astype("<u4").view(np.uint8), bitorder="little")
    g = flat[:n * n].reshape(n, n).astype(np.uint8)
    if goal is not None:
        g[int(goal[0]), int(goal[1])] = 2
    return g


def unpack_meta(meta):
    """One entry's meta words -> (N, start r, start c, goal r, goal c, max_steps)."""
    m0, m1 = (int(x) & 0xFFFFFFFF for x in meta)
    return (m0 & 0xFF, (m0 >> 16) & 0xFF, m0 >> 24, m1 & 0xFF, (m1 >> 8) & 0xFF, m1 >> 16)


def _load_entries(store, env, slot, env_ids=None):
    """MazeArchive.load / MazePool.load: one mz_archive_load launch from `store`'s bits / meta /
    algo rows (linear entries of `store.words` words) into `env`, refusals counted in
    store.errors."""
    s = torch.as_tensor(slot).to(device=store.device, dtype=torch.int32).reshape(-1).contiguous()
    ids = None
    if env_ids is not None:
        ids = torch.as_tensor(env_ids).to(device=store.device, dtype=torch.int32) \
            .reshape(-1).contiguous()
        if ids.numel() != s.numel():
            raise ValueError("one slot per listed instance")
    elif s.numel() > env.num_envs:
        raise ValueError("more slots than instances")
    if env.device != store.device:
        raise ValueError("the archive and the env live on different devices")
    N.check(store.lib.mz_archive_load(
        env._h, None if ids is None else ids.data_ptr(), int(s.numel()), s.data_ptr(),
        store.words, store.bits.data_ptr(), store.meta.data_ptr(), store.algo.data_ptr(),
        store.errors.data_ptr(), store._stream()))


def _entries_to_mazes(bits, meta):
    """Host rows of bits [m, W] / meta [m, 2] in the snapshot_mazes / best_of_mazes format."""
    info = [unpack_meta(m) for m in meta]
    D = max((x[0] for x in info), default=0)
    grids = np.zeros((len(info), D, D), np.uint8)
    sg = np.zeros((len(info), 4), np.int32)
    sizes = np.zeros(len(info), np.int32)
    for j, (n, sr, sc, gr, gc, _) in enumerate(info):
        grids[j, :n, :n] = unpack_grid(bits[j], n, (gr, gc))
        sg[j] = (sr, sc, gr, gc)
        sizes[j] = n
    return grids, sg, sizes


class MazeArchive:
    def __init__(self, env, slots):
        """A ring of `slots` entries for each instance of `env` (a VectorMazeEnv): bits int32
        [B, slots, W], meta int32 [B, slots, 2], algo uint8 [B, slots], count int32 [B] (pushes
        per instance), errors int32 [1] (entries load() refused; never cleared here)."""
        slots = int(slots)
        if slots < 1:
            raise ValueError("slots must be >= 1")
        self.env, self.lib, self.device = env, env.lib, env.device
        self.num_envs, self.slots, self.pitch = env.num_envs, slots, env.max_dim
        self.words = archive_words(self.pitch)
        B, dev = self.num_envs, self.device
        self.bits = torch.zeros(B, slots, self.words, dtype=torch.int32, device=dev)
        self.meta = torch.zeros(B, slots, 2, dtype=torch.int32, device=dev)
        self.algo = torch.zeros(B, slots, dtype=torch.uint8, device=dev)
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.errors = torch.zeros(1, dtype=torch.int32, device=dev)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # -------------------------------------------------------------------------------------------
    def record(self, flags=None):
        """env.mazes.append(maze) for the instances with flags != 0 (None: all): one launch."""
        f = None
        if flags is not None:
            f = flags.to(device=self.device, dtype=torch.uint8).contiguous()
            if f.numel() != self.num_envs:
                raise ValueError("one flag per instance")
        N.check(self.lib.mz_archive_push(
            self.env._h, None if f is None else f.data_ptr(), self.slots, self.words,
            self.bits.data_ptr(), self.meta.data_ptr(), self.algo.data_ptr(),
            self.count.data_ptr(), self._stream()))

    def load(self, env, slot, env_ids=None):
        """update_visited_maze(): instance env_ids[j] (None: j) of `env` — this archive's env or
        another on the same device whose pitch holds the mazes — becomes linear entry slot[j]
        (entry_slot() gives them; negative: the instance is left alone). One launch, no host
        copy; the instances are reset in the handle — call env.reset() / reset_list() for their
        observations. A refused entry is counted in self.errors."""
        _load_entries(self, env, slot, env_ids)

    # -------------------------------------------------------------------------------------------
    @property
    def held(self):
        """Entries each instance's ring holds: min(count, slots) (int32 device tensor)."""
        return self.count.clamp(max=self.slots)

    @property
    def dropped(self):
        """Entries each instance's ring has overwritten: max(count - slots, 0)."""
        return (self.count - self.slots).clamp(min=0)

    def entry_slot(self, k):
        """Linear slot (for load()) of each instance's k-th oldest held entry, -1 where
        k >= held (int32 [B] device tensor)."""
        k = int(k)
        if k < 0:
            raise ValueError("k must be >= 0")
        i = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
        first = self.count - self.held  # pushes before the oldest held entry
        lin = i * self.slots + (first + k) % self.slots
        return torch.where(self.held > k, lin, torch.full_like(lin, -1))

    def newest_slot(self):
        """Linear slot of each instance's newest entry (-1: none)."""
        i = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
        lin = i * self.slots + (self.count - 1).clamp(min=0) % self.slots
        return torch.where(self.count > 0, lin, torch.full_like(lin, -1))

    def to_mazes(self, ids=None, entry="newest"):
        """Held entries as snapshot_mazes / best_of_mazes return mazes — (grids uint8 [m, D, D],
        start_goal int32 [m, 4], sizes int32 [m]), D = the largest size — for
        evaluate(learner, mazes=...) and load_selected (host copies; synchronises). entry:
        "newest" — the listed instances' (None: all) newest entries, one each; an int k — their
        k-th oldest held entries; "all" — every held entry, instance by instance, oldest first.
        Instances without the entry asked for are left out."""
        idx = range(self.num_envs) if ids is None else [int(i) for i in ids]
        if entry == "newest":
            cols = [self.newest_slot()]
        elif entry == "all":
            cols = [self.entry_slot(k) for k in range(self.slots)]
        else:
            cols = [self.entry_slot(entry)]
        table = torch.stack(cols, 1).cpu().numpy()
        lin = [int(s) for i in idx for s in table[i] if s >= 0]
        sel = torch.as_tensor(lin, dtype=torch.int64, device=self.device)
        bits = self.bits.view(-1, self.words)[sel].cpu().numpy()
        meta = self.meta.view(-1, 2)[sel].cpu().numpy()
        return _entries_to_mazes(bits, meta)

    # -------------------------------------------------------------------------------------------
    _TENSORS = ("bits", "meta", "algo", "count", "errors")

    def state_dict(self):
        sd = {k: getattr(self, k).clone() for k in self._TENSORS}
        sd.update(format=_FORMAT, pitch=self.pitch, slots=self.slots, num_envs=self.num_envs)
        return sd

    def check_state_dict(self, sd):
        """ValueError unless `sd` is a state_dict() of an archive of this pitch, ring and
        population (nothing is changed)."""
        if sd.get("format") != _FORMAT:
            raise ValueError("not a MazeArchive state_dict")
        for k in ("pitch", "slots", "num_envs"):
            if int(sd[k]) != getattr(self, k):
                raise ValueError(f"the saved archive's {k} {sd[k]} differs from this archive's "
                                 f"{getattr(self, k)}")
        for k in self._TENSORS:
            if tuple(sd[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f"the saved archive's {k} has another shape")

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        for k in self._TENSORS:
            getattr(self, k).copy_(sd[k])


def pool_span():
    """Instances one workgroup of the pool push covers (mz_archive_pool_span; no GPU)."""
    s = N.C.c_int32()
    N.check(N.load().mz_archive_pool_span(N.C.byref(s)))
    return s.value


class MazePool:
    """`env.mazes` of a learner that trains on B envs at once: ONE list for the whole population,
    filled in exploration order — record() call by record() call, and within a call by instance
    id — so that entries 0 .. n-1 are the oldest n mazes the run trained on, what the reference's
    test(n, new=False) replays. The pool keeps the first `capacity` entries and counts the rest
    (`dropped`). With one instance it is exactly env.mazes; with B it is deterministic to the bit.
    An entry is a MazeArchive entry plus owner (the instance id) and stamp (record()'s).

    Size it with the entry: at pitch 81, 206 words + 2 meta + algo + owner + stamp = 841 bytes,
    0.84 GB per million entries."""

    def __init__(self, env, capacity):
        """bits int32 [C, W], meta int32 [C, 2], algo uint8 [C], owner int32 [C], stamp int32 [C],
        the count (entries offered so far) and errors int32 [1] (entries load() refused; never
        cleared here)."""
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.env, self.lib, self.device = env, env.lib, env.device
        self.capacity, self.pitch = capacity, env.max_dim
        self.toroidal = bool(getattr(env, "toroidal", False))
        self.enrich = bool(getattr(env, "enrich", False))
        self.words = archive_words(self.pitch)
        C, dev = capacity, self.device
        self.bits = torch.zeros(C, self.words, dtype=torch.int32, device=dev)
        self.meta = torch.zeros(C, 2, dtype=torch.int32, device=dev)
        self.algo = torch.zeros(C, dtype=torch.uint8, device=dev)
        self.owner = torch.zeros(C, dtype=torch.int32, device=dev)
        self.stamp = torch.zeros(C, dtype=torch.int32, device=dev)
        # the push kernel's two-word counter (csrc/mz_archive.hip): a call reads word _cur and
        # writes the other one, so no workgroup reads what another writes
        self._count2 = torch.zeros(2, dtype=torch.int32, device=dev)
        self._cur = 0
        self.errors = torch.zeros(1, dtype=torch.int32, device=dev)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # -------------------------------------------------------------------------------------------
    def record(self, flags=None, stamp=0):
        """env.mazes.append(maze) for the instances with flags != 0 (None: all), in ascending
        id, each stamped `stamp`: one launch on the current stream, no host read."""
        f = None
        if flags is not None:
            f = flags.to(device=self.device, dtype=torch.uint8).contiguous()
            if f.numel() != self.env.num_envs:
                raise ValueError("one flag per instance")
        N.check(self.lib.mz_archive_push_pool(
            self.env._h, None if f is None else f.data_ptr(), self.capacity, self.words,
            self.bits.data_ptr(), self.meta.data_ptr(), self.algo.data_ptr(),
            self.owner.data_ptr(), self.stamp.data_ptr(),
            self._count2.data_ptr() + 4 * self._cur, int(stamp), self._stream()))
        self._cur ^= 1

    def load(self, env, slot, env_ids=None):
        """MazeArchive.load from this pool: instance env_ids[j] (None: j) of `env` becomes entry
        slot[j] (negative: left alone). The caller keeps slot[j] < held."""
        _load_entries(self, env, slot, env_ids)

    # -------------------------------------------------------------------------------------------
    @property
    def count(self):
        """Entries offered so far (int32 0-dim device tensor; saturates at 2^31 - 1)."""
        return self._count2[self._cur]

    @property
    def held(self):
        """Entries the pool holds: min(count, capacity)."""
        return self.count.clamp(max=self.capacity)

    @property
    def dropped(self):
        """Entries offered after the pool was full: max(count - capacity, 0)."""
        return (self.count - self.capacity).clamp(min=0)

    def to_mazes(self, first=0, n=None):
        """Held entries first .. first + n - 1 (n None: up to the last held one), oldest first, as
        snapshot_mazes / best_of_mazes return mazes — (grids uint8 [m, D, D], start_goal int32
        [m, 4], sizes int32 [m]) — for evaluate(learner, mazes=...) (host copies; synchronises)."""
        first, held = int(first), int(self.held)
        n = held - first if n is None else int(n)
        if first < 0 or n < 0 or first + n > held:
            raise ValueError(f"entries {first} .. {first + n - 1} of {held} held")
        return _entries_to_mazes(self.bits[first:first + n].cpu().numpy(),
                                 self.meta[first:first + n].cpu().numpy())

    # -------------------------------------------------------------------------------------------
    _TENSORS = ("bits", "meta", "algo", "owner", "stamp", "errors")
    _GEOMETRY = ("pitch", "capacity", "toroidal", "enrich")

    def state_dict(self):
        sd = {k: getattr(self, k).clone() for k in self._TENSORS}
        sd["count"] = self.count.reshape(1).clone()
        sd.update(format=_POOL_FORMAT, **{k: getattr(self, k) for k in self._GEOMETRY})
        return sd

    def check_state_dict(self, sd):
        """ValueError unless `sd` is a state_dict() of a pool of this pitch, capacity and
        geometry (nothing is changed)."""
        if not isinstance(sd, dict) or sd.get("format") != _POOL_FORMAT:
            raise ValueError("not a MazePool state_dict")
        for k in self._GEOMETRY:
            if k not in sd or int(sd[k]) != int(getattr(self, k)):
                raise ValueError(f"the saved pool's {k} {sd.get(k)} differs from this pool's "
                                 f"{getattr(self, k)}")
        for k in self._TENSORS + ("count",):
            want = (1,) if k == "count" else tuple(getattr(self, k).shape)
            if k not in sd or not torch.is_tensor(sd[k]) or tuple(sd[k].shape) != want or \
                    sd[k].dtype != (torch.int32 if k == "count" else getattr(self, k).dtype):
                raise ValueError(f"the saved pool's {k} has another shape or type")

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        for k in self._TENSORS:
            getattr(self, k).copy_(sd[k])
        self._count2[self._cur:self._cur + 1].copy_(sd["count"])


class MazePoolSet:
    """One MazePool per learner of a population of learners that share an env: the env's B
    instances are `groups` blocks of b = B / groups consecutive instances, and block g has a pool
    of `capacity` entries of its own — rows [g C, (g + 1) C) of the arrays below and a counter of
    its own. record() fills all of them in ONE launch (mz_archive_push_pools). Pool g is, bit for
    bit, the MazePool of an env that holds block g's instances alone: its owners are the ids
    within the block."""

    def __init__(self, env, groups, capacity):
        """bits int32 [G C, W], meta int32 [G C, 2], algo uint8 / owner int32 / stamp int32 [G C],
        the counts int32 [G] (entries offered to each pool so far) and errors int32 [1] (entries
        load() refused, over all pools; never cleared here)."""
        groups, capacity = int(groups), int(capacity)
        if groups < 1 or env.num_envs % groups:
            raise ValueError(f"the env's {env.num_envs} instances must divide into groups "
                             f"{groups} >= 1")
        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.env, self.lib, self.device = env, env.lib, env.device
        self.groups, self.capacity, self.pitch = groups, capacity, env.max_dim
        self.block = env.num_envs // groups
        self.toroidal = bool(getattr(env, "toroidal", False))
        self.enrich = bool(getattr(env, "enrich", False))
        self.words = archive_words(self.pitch)
        R, dev = groups * capacity, self.device
        self.bits = torch.zeros(R, self.words, dtype=torch.int32, device=dev)
        self.meta = torch.zeros(R, 2, dtype=torch.int32, device=dev)
        self.algo = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.owner = torch.zeros(R, dtype=torch.int32, device=dev)
        self.stamp = torch.zeros(R, dtype=torch.int32, device=dev)
        # every pool's two-word counter: a call reads word _cur of each pair and writes the other
        self._count2 = torch.zeros(groups, 2, dtype=torch.int32, device=dev)
        self._cur = 0
        self.errors = torch.zeros(1, dtype=torch.int32, device=dev)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # -------------------------------------------------------------------------------------------
    def record(self, flags=None, stamp=0):
        """env.mazes.append(maze) of every learner: the instances with flags != 0 (None: all) go
        to their block's pool, in ascending id, each stamped `stamp`: one launch on the current
        stream for all pools, no host read."""
        f = None
        if flags is not None:
            f = flags.to(device=self.device, dtype=torch.uint8).contiguous()
            if f.numel() != self.env.num_envs:
                raise ValueError("one flag per instance")
        N.check(self.lib.mz_archive_push_pools(
            self.env._h, None if f is None else f.data_ptr(), self.groups, self.capacity,
            self.words, self.bits.data_ptr(), self.meta.data_ptr(), self.algo.data_ptr(),
            self.owner.data_ptr(), self.stamp.data_ptr(), self._count2.data_ptr(), self._cur,
            int(stamp), self._stream()))
        self._cur ^= 1

    def load(self, env, slot, env_ids=None):
        """MazePool.load over all pools: slot[j] is a linear row, g C + k for pool g's entry k
        (negative: left alone), so one launch fills an env from every pool. The caller keeps
        k < held[g]."""
        _load_entries(self, env, slot, env_ids)

    def pool(self, g):
        """Pool g through MazePool's reading interface (views of this set's arrays: bits, meta,
        algo, owner, stamp, count, held, dropped, errors, load, to_mazes, state_dict), for
        evaluate_explored; record() stays the set's."""
        g = int(g)
        if g < 0 or g >= self.groups:
            raise ValueError(f"pool {g} of {self.groups}")
        return _PoolOfSet(self, g)

    # -------------------------------------------------------------------------------------------
    @property
    def count(self):
        """Entries offered to each pool so far (int32 [G] device tensor; saturates at 2^31 - 1)."""
        return self._count2[:, self._cur]

    @property
    def held(self):
        """Entries each pool holds: min(count, capacity)."""
        return self.count.clamp(max=self.capacity)

    @property
    def dropped(self):
        """Entries offered to each pool after it was full: max(count - capacity, 0)."""
        return (self.count - self.capacity).clamp(min=0)

    # -------------------------------------------------------------------------------------------
    _TENSORS = MazePool._TENSORS
    _GEOMETRY = ("pitch", "capacity", "groups", "toroidal", "enrich")

    def state_dict(self):
        sd = {k: getattr(self, k).clone() for k in self._TENSORS}
        sd["count"] = self.count.clone()
        sd.update(format=_POOLS_FORMAT, **{k: getattr(self, k) for k in self._GEOMETRY})
        return sd

    def check_state_dict(self, sd):
        """ValueError unless `sd` is a state_dict() of a set of this pitch, capacity, group count
        and geometry (nothing is changed)."""
        if not isinstance(sd, dict) or sd.get("format") != _POOLS_FORMAT:
            raise ValueError("not a MazePoolSet state_dict")
        for k in self._GEOMETRY:
            if k not in sd or int(sd[k]) != int(getattr(self, k)):
                raise ValueError(f"the saved set's {k} {sd.get(k)} differs from this set's "
                                 f"{getattr(self, k)}")
        for k in self._TENSORS + ("count",):
            want = (self.groups,) if k == "count" else tuple(getattr(self, k).shape)
            if k not in sd or not torch.is_tensor(sd[k]) or tuple(sd[k].shape) != want or \
                    sd[k].dtype != (torch.int32 if k == "count" else getattr(self, k).dtype):
                raise ValueError(f"the saved set's {k} has another shape or type")

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        for k in self._TENSORS:
            getattr(self, k).copy_(sd[k])
        self._count2[:, self._cur].copy_(sd["count"])


class _PoolOfSet(MazePool):
    """MazePoolSet.pool(g): a MazePool whose arrays are the set's rows [g C, (g + 1) C) and whose
    counter is the set's pair g (read when used, so the view follows the set's record() calls)."""

    def __init__(self, pools, g):
        s, C = pools, pools.capacity
        self._set, self.group = s, g
        self.env, self.lib, self.device = s.env, s.lib, s.device
        self.capacity, self.pitch, self.words = C, s.pitch, s.words
        self.toroidal, self.enrich = s.toroidal, s.enrich
        for k in ("bits", "meta", "algo", "owner", "stamp"):
            setattr(self, k, getattr(s, k)[g * C:(g + 1) * C])
        self.errors = s.errors

    @property
    def _count2(self):
        return self._set._count2[self.group]

    @property
    def _cur(self):
        return self._set._cur

    def record(self, flags=None, stamp=0):
        raise TypeError("a pool of a MazePoolSet is filled by the set's record()")


def add_pool_arguments(ap, what="the run"):
    """--archive C and --explored-mazes N of the episodic trainers' command lines (mazerl.train's
    options and defaults: 0 = off, N default every held entry)."""
    ap.add_argument("--archive", type=int, default=0,
                    help=f"C > 0: keep the first C mazes {what} trains on (every instance's first "
                         "maze, then each winner's new one) in a MazePool and report the win rate "
                         "on them, the reference's test(n, new=False); 0 = off")
    ap.add_argument("--explored-mazes", type=int, default=None,
                    help="N: replay the pool's oldest N entries (default: all held; at most held)")


def check_pool_arguments(a):
    """mazerl.train's refusals of the two options, raised before any GPU call."""
    if a.archive < 0:
        raise ValueError("--archive must be >= 0")
    if a.explored_mazes is not None:
        if a.explored_mazes < 1:
            raise ValueError("--explored-mazes must be >= 1")
        if not a.archive:
            raise ValueError("--explored-mazes replays the pool: it needs --archive")


def instance_algorithms(env):
    """The algorithm id the handle holds for each instance (uint8 [B] device tensor, no host
    read): what a push records, taken from a one-slot archive that is dropped again."""
    a = MazeArchive(env, 1)
    a.record()
    return a.algo[:, 0].clone()
