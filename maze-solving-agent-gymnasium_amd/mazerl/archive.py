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

All archive memory is torch tensors owned by this object (the env handle keeps no pointer to
it), so an archive outlives its env, is saved by state_dict() and loads into another handle.
"""
import numpy as np
import torch

from . import _native as N

_FORMAT = "mazerl.MazeArchive/1"


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
        s = torch.as_tensor(slot).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        ids = None
        if env_ids is not None:
            ids = torch.as_tensor(env_ids).to(device=self.device, dtype=torch.int32) \
                .reshape(-1).contiguous()
            if ids.numel() != s.numel():
                raise ValueError("one slot per listed instance")
        elif s.numel() > env.num_envs:
            raise ValueError("more slots than instances")
        if env.device != self.device:
            raise ValueError("the archive and the env live on different devices")
        N.check(self.lib.mz_archive_load(
            env._h, None if ids is None else ids.data_ptr(), int(s.numel()), s.data_ptr(),
            self.words, self.bits.data_ptr(), self.meta.data_ptr(), self.algo.data_ptr(),
            self.errors.data_ptr(), self._stream()))

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
        info = [unpack_meta(m) for m in meta]
        D = max((x[0] for x in info), default=0)
        grids = np.zeros((len(lin), D, D), np.uint8)
        sg = np.zeros((len(lin), 4), np.int32)
        sizes = np.zeros(len(lin), np.int32)
        for j, (n, sr, sc, gr, gc, _) in enumerate(info):
            grids[j, :n, :n] = unpack_grid(bits[j], n, (gr, gc))
            sg[j] = (sr, sc, gr, gc)
            sizes[j] = n
        return grids, sg, sizes

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


def instance_algorithms(env):
    """The algorithm id the handle holds for each instance (uint8 [B] device tensor, no host
    read): what a push records, taken from a one-slot archive that is dropped again."""
    a = MazeArchive(env, 1)
    a.record()
    return a.algo[:, 0].clone()
