"""The inputs of tests/test_ppo_model.py and tests/test_ppo_exact.py, built once per process: the
CPU test checks the caps on left-out episodes / rows / columns on exactly the cases the GPU test
runs, and both share the model's results."""
import functools

import numpy as np

import ppo_model as M

REWARDS = [1.0, 0.45, -0.55, -1.0, -0.18126924692201818, -0.13929202357494222, -0.05]
FIN_LENS = [2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097]
SCAN_BS = [1, 64, 1023, 1024, 1025, 2048, 4099]
SCAN_PATTERNS = ["mix", "all", "edges", "none"]
SCAN_L = 6
ACT_BS = [1, 7, 8, 9, 4099]
ACT_L = 6
ACT_SEED, ACT_COUNTER = 0x5EED0DD5, 3
HEAD_BS = [1, 2, 37, 255, 256, 257, 1023, 1024, 1025, 2048]
HEAD_MODES = ["inside", "outside"]
CLIP, COEF = 0.3, 7e-3


# ---- scan ---------------------------------------------------------------------------------------
def scan_step(B, pattern, call):
    """(term, trunc, reward64) of one vector step; `call` 0 / 1 are the two consecutive calls."""
    rng = np.random.default_rng(1000 * B + 10 * SCAN_PATTERNS.index(pattern) + call)
    u = rng.random(B)
    if pattern == "mix":      # ~30 % done: 12 % terminated, 12 % truncated, 6 % both
        term, trunc = (u < 0.18), (u >= 0.12) & (u < 0.30)
    elif pattern == "all":
        term, trunc = (u < 0.5), (u >= 0.4)
    elif pattern == "edges":  # only the instances next to the kernel's chunk boundaries
        ids = np.array([i for k in range(1, 5) for i in (1024 * k - 1, 1024 * k) if i < B], int)
        term, trunc = np.zeros(B, bool), np.zeros(B, bool)
        term[ids[::2]] = True
        trunc[ids[1::2]] = True
    else:
        term, trunc = np.zeros(B, bool), np.zeros(B, bool)
    return term.astype(np.uint8), trunc.astype(np.uint8), rng.choice(REWARDS, B).astype(np.float64)


def scan_t0(B, pattern):
    rng = np.random.default_rng(77 * B + SCAN_PATTERNS.index(pattern))
    t = rng.integers(0, SCAN_L, B).astype(np.int32)
    if pattern == "edges":
        for i in range(1023, B, 1024):
            t[i:i + 2] = np.maximum(t[i:i + 2], 1)  # listed, not dropped as 1-step episodes
    return t


SCAN_STATE0 = dict(fill=12345, total=99999, stats=[7, 3, 2, 1])


# ---- finish -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def finish_list(name, gamma):
    """A hand-built finished list: B, L, ids / offs / lens, cap (capacity), alloc (pool rows
    allocated), rec_r float64 [B, L], rec_v float32 [B, L]."""
    rng = np.random.default_rng({"main": 11, "stride": 12, "edge": 13}[name])
    if name == "main":
        B, L, lens = 16, 4100, list(FIN_LENS)
        ids = [int(i) for i in rng.permutation(B)[:len(lens)]]
        offs, o = [], 5
        for n in lens:
            offs.append(o)
            o += n + 3  # gaps between the episodes' rows
        cap = alloc = o + 4
    elif name == "stride":
        B, L = 2100, 4
        lens = [int(n) for n in rng.integers(2, 5, B)]
        ids = [int(i) for i in rng.permutation(B)]
        offs = [int(x) for x in np.concatenate([[0], np.cumsum(lens)[:-1]]) + np.arange(B) // 7]
        cap = alloc = offs[-1] + lens[-1]
    else:  # zero rewards; an episode that ends on the capacity; one that ends one row past it
        B, L, lens, ids, cap = 4, 8, [5, 4, 3], [2, 0, 3], 20
        offs, alloc = [1, cap - 4, cap - 2], cap + 8
    assert ids != sorted(ids) and len(set(ids)) == len(ids)
    rec_r = rng.choice(REWARDS, (B, L)).astype(np.float64)
    rec_v = rng.standard_normal((B, L)).astype(np.float32)
    if name == "edge":
        rec_r[2, :5] = 0.0
    return dict(name=name, B=B, L=L, gamma=gamma, ids=ids, offs=offs, lens=lens, cap=cap,
                alloc=alloc, rec_r=rec_r, rec_v=rec_v)


@functools.lru_cache(maxsize=None)
def finish_model(name, gamma):
    """[(returns, advantages, clear)] per listed episode."""
    c = finish_list(name, gamma)
    return [M.finish(c["rec_r"][i, :n], c["rec_v"][i, :n], gamma) for i, n in zip(c["ids"], c["lens"])]


FINISH_LISTS = [("main", 0.9), ("main", 0.99), ("stride", 0.99), ("edge", 0.99)]


# ---- act ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def act_case(B):
    rng = np.random.default_rng(500 + B)
    L = ACT_L
    logits = (2.0 * rng.standard_normal((B, 4))).astype(np.float32)
    t = rng.integers(0, L, B).astype(np.int32)
    if B >= 7:
        logits[2, 1] = 30.0
        logits[4, 3] = -30.0
        t[1], t[3], t[5] = -1, L, L + 5  # outside the record: nothing written for these
    u24 = M.uniform24(ACT_SEED, ACT_COUNTER, B)
    return dict(B=B, L=L, logits=logits, t=t, u24=u24, model=M.act(logits, u24),
                value=rng.standard_normal(B).astype(np.float32),
                obs6=rng.random((B, 6)).astype(np.float32),
                bits=rng.integers(0, 2 ** 32, (B, 22), dtype=np.uint64).astype(np.uint32))


# ---- head loss ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def head_case(b, mode):
    """"inside": most ratios within [1 - clip, 1 + clip]; "outside": most beyond it."""
    rng = np.random.default_rng(900 + 2 * b + HEAD_MODES.index(mode))
    sz, sn = (0.05, 0.07) if mode == "inside" else (2.0, 2.0)
    logits = (sz * rng.standard_normal((b, 4))).astype(np.float32)
    action = rng.integers(0, 4, b).astype(np.int64)
    if b >= 37:  # saturated rows: softmax entries below the entropy's 1e-8
        logits[5], action[5] = [30.0, 0.0, 0.5, -0.5], 0
        logits[11], action[11] = [-30.0, 0.1, 0.2, 0.3], 1
        logits[20], action[20] = [0.0, 0.0, -30.0, 0.0], 2  # the drawn action is the vanishing one
    adv = rng.standard_normal(b).astype(np.float32)
    adv[::17] = 0.0
    z = logits.astype(np.float64)
    lsm = z - np.log(np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)) - z.max(1, keepdims=True)
    lp_new = lsm[np.arange(b), action]
    # (the vanishing action's log-prob of -31 is kept out of lp_old: as an old log-prob it would put
    # ratios of e^30 into every column and leave the sums to that one term)
    lp_old = (np.maximum(lp_new, -4.0)[rng.permutation(b)] + sn * rng.standard_normal(b)).astype(np.float32)
    c = dict(b=b, mode=mode, logits=logits, action=action, adv=adv, lp_old=lp_old,
             value=rng.standard_normal(b).astype(np.float32),
             ret=rng.standard_normal(b).astype(np.float32), coef=np.float32(COEF), clip=CLIP)
    c["model"] = M.head(logits, c["value"], action, lp_old, adv, c["ret"], c["coef"], CLIP)
    return c


def torch_head(c, dtype):
    """The package's own expressions on the CPU (ActorCriticNet.evaluate's three lines, the
    broadcast branch of ppo_losses, total = pl + 0.5 vl) with autograd: (total, dlogits, dvalue)
    as float64 numpy arrays."""
    import torch
    import torch.nn.functional as F
    from mazerl.agents.ppo import ppo_losses
    logits = torch.tensor(c["logits"], dtype=dtype, requires_grad=True)
    value = torch.tensor(c["value"], dtype=dtype).reshape(-1, 1).requires_grad_()
    act = torch.from_numpy(c["action"]).reshape(-1, 1)
    lp_old = torch.tensor(c["lp_old"], dtype=dtype).reshape(-1, 1)
    adv, ret = (torch.tensor(c[k], dtype=dtype) for k in ("adv", "ret"))
    coef = torch.tensor(float(c["coef"]), dtype=dtype)
    prob = F.softmax(logits, dim=-1)
    lp_new = F.log_softmax(logits, dim=-1).gather(1, act).squeeze(1)
    ent = -torch.sum(prob * torch.log(prob + 1e-8), dim=1)
    pl, vl = ppo_losses(lp_old, lp_new, adv, ent, ret, value, coef, clip=c["clip"])
    total = pl + 0.5 * vl
    total.backward()
    return (float(total.detach().double()), logits.grad.double().numpy(),
            value.grad.double().numpy().reshape(-1))


def pair_terms_left_out(c):
    """sum of the surrogate's column terms of the columns that are not clear, over b^2 (what the
    loss comparison subtracts from every side)."""
    m = c["model"]
    return float(m["part"][~m["clear"]].sum()) / (c["b"] * c["b"])
