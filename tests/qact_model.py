"""An exact CPU model of the bf16x3 acting forward (csrc/mz_qact.hip: k_qconv, k_qfc1, k_qact2),
its dropout masks and the synthetic states the CPU and GPU tests share. CPU only: numpy and torch
on the host, no library call.

The kernels split every GEMM operand x into hi = bf16(x) (round to nearest even) and
lo = bf16(x - hi) and sum hi*hi + hi*lo + lo*hi in f32. Every such product is exact in f32, so the
only thing between the kernels and `model_q(dtype=float64)` is the order of the f32 additions.
`model_q(dtype=float32)` accumulates the same products in f32 on the CPU in a fixed order of its
own (one accumulator per output, k after k — the same number on every machine): its distance
from the float64 model, E_acc, measures what an f32 accumulation order costs at this network's
scale, and the GPU tests' tolerance T_MODEL is derived from it.

Measured (tests/test_qact_model.py recomputes them; make_net: QNet seed 11, weights x 3; the 512
rows of synthetic_states(512, 5); row-relative: max_a |dQ| / max_a |Q| per row, the largest row):

                                        DQN       DDQN      DDQN, dropout (seed 77, counter 0, p 0.2)
  E_alg  f64 model   vs f64 network     1.9e-5    2.3e-5    -
         f32 network vs f64 network     1.9e-6    1.2e-6    -
  E_acc  f32 model   vs f64 model       7.9e-6    7.1e-6    8.2e-6
  mutation vs the unmutated f64 model
         obs_lo                         2.9e-4    2.6e-4
         fc1_chunk_lo                   8.4e-4    6.2e-4
         fc1_rows_lo                    1.7e-3    1.3e-3
         fc2_lohi                       4.8e-3    4.1e-3

T_MODEL = 4 x the largest E_acc (8.2e-6 -> 3.3e-5), rounded up to one significant digit: 4e-5.
The factor 4 covers the MFMA's own order (32-deep blocks, the three product passes interleaved
product-major), which is not the CPU's. The smallest mutation (2.6e-4) is 6.5 x T_MODEL.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

E_ACC = {"dqn": 7.9e-6, "ddqn": 7.1e-6, "ddqn_dropout": 8.2e-6}  # as measured, see above
T_MODEL = 4e-5

MUTATIONS = ("obs_lo", "fc1_chunk_lo", "fc1_rows_lo", "fc2_lohi")
CONV_OUT = 1568
M64 = (1 << 64) - 1


def split(x):
    """x (f32) -> hi = bf16(x), lo = bf16(x - hi), both as f32 (x = hi + lo + O(2^-17 x))."""
    x = x.to(torch.float32)
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def window(bits):
    """Packed windows (int32 [n, 22], bit i of the row = word i / 32, bit i % 32) -> f32
    [n, 3, 15, 15]; the pad bits 675..703 are ignored."""
    b = np.ascontiguousarray(torch.as_tensor(bits).cpu().numpy()).view(np.uint32)
    i = np.arange(675)
    w = (b[:, i // 32] >> (i % 32).astype(np.uint32)) & 1
    return torch.from_numpy(w.astype(np.float32).reshape(-1, 3, 15, 15))


def make_net(variant, seed=11, scale=3.0):
    """The Q-network every QAct test runs: the reference's sizes, weights of a trained net's
    scale, on the CPU in eval mode."""
    from mazerl.agents.nets import QNet
    torch.manual_seed(seed)
    net = QNet(variant=variant)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(scale)
    return net.eval()


def _x3(a, w, dtype, lo_a=True):
    """a [n, k] x w [m, k]^T as the kernels' three products, accumulated in `dtype`."""
    (ah, al), (wh, wl) = a, w
    if dtype == torch.float32:
        # one f32 accumulator per output, k after k, the three products of a k in the kernels'
        # order; each product is exact in f32, so every step is one rounding. An explicit order
        # (not a BLAS call's) so that E_acc is the same number on every machine.
        wht, wlt = wh.t().contiguous(), wl.t().contiguous()
        acc = torch.zeros(ah.shape[0], wh.shape[0], dtype=torch.float32)
        for k in range(ah.shape[1]):
            acc.addcmul_(ah[:, k:k + 1], wht[k])
            acc.addcmul_(ah[:, k:k + 1], wlt[k])
            if lo_a:
                acc.addcmul_(al[:, k:k + 1], wht[k])
        return acc
    ah, al, wh, wl = (t.to(dtype) for t in (ah, al, wh, wl))
    out = ah @ wh.t() + ah @ wl.t()
    return out + al @ wh.t() if lo_a else out


@torch.no_grad()
def model_q(net, win, obs6, keep=None, p=0.0, dtype=torch.float64, mutate=None):
    """Q [n, 4] (`dtype`) of the bf16x3 forward on windows win [n, 3, 15, 15] (0 / 1) and obs6
    [n, 6]: what the kernels compute up to the order of their f32 additions.

    keep [n, 32, 15, 15] (bool) with p: DDQN's train-mode dropout after the conv activation
    (keep_masks). dtype float64: the exact sums; float32: the same products accumulated in f32.
    mutate: one of MUTATIONS, a defect a rework of the kernels could plausibly have —
      obs_lo        the lo half of the obs6 chunk's A operand dropped
      fc1_chunk_lo  the lo image of one 32-wide K chunk of fc1 (pooled position 24) zeroed
      fc1_rows_lo   the lo image of 64 fc1 output rows (320..383) zeroed
      fc2_lohi      the lo*hi product missing in fc2
    """
    assert mutate is None or mutate in MUTATIONS
    f32 = torch.float32
    conv = net.conv[0]
    lin = [m for m in net.fc if isinstance(m, nn.Linear)]
    relu = isinstance(net.fc[3], nn.ReLU)
    win, obs6 = win.cpu().to(f32), obs6.cpu().to(f32)
    # conv: the window is exact in bf16, only the weights are split; the accumulator starts at
    # the bias; the kernel holds the result as f32
    ch, cl = split(conv.weight.detach().cpu())
    z = F.conv2d(win.to(dtype), ch.to(dtype), None, padding=1) + \
        F.conv2d(win.to(dtype), cl.to(dtype), None, padding=1) + \
        conv.bias.detach().cpu().to(dtype).view(1, -1, 1, 1)
    a = F.leaky_relu(z.to(f32), 0.01)
    if keep is not None:
        scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))  # the f32 the library passes
        a = a * torch.as_tensor(keep).to(f32) * float(scale)
    x = torch.cat((F.max_pool2d(a, 2, 2).flatten(1), obs6), 1)  # f32 [n, 1574], torch's order
    # fc1 on the f32 features
    xs, w1 = list(split(x)), list(split(lin[0].weight.detach().cpu()))
    if mutate == "obs_lo":
        xs[1][:, CONV_OUT:] = 0.0
    if mutate == "fc1_chunk_lo":  # the kernel's chunk q holds torch's features c * 49 + q
        w1[1][:, 24 + 49 * torch.arange(32)] = 0.0
    if mutate == "fc1_rows_lo":
        w1[1][320:384] = 0.0
    z = _x3(xs, w1, dtype) + lin[0].bias.detach().cpu().to(dtype)
    h1 = F.leaky_relu(z.to(f32), 0.01)
    # fc2 on the f32 h1
    z = _x3(split(h1), split(lin[1].weight.detach().cpu()), dtype, lo_a=mutate != "fc2_lohi") + \
        lin[1].bias.detach().cpu().to(dtype)
    h2 = F.relu(z.to(f32)) if relu else F.leaky_relu(z.to(f32), 0.01)
    # fc3 in plain precision on the f32 h2
    if dtype == f32:  # product rounded, then added, k after k (the fixed order again)
        w3t = lin[2].weight.detach().cpu().t().contiguous()
        q = torch.zeros(h2.shape[0], 4, dtype=f32)
        for k in range(h2.shape[1]):
            q += h2[:, k:k + 1] * w3t[k]
        return q + lin[2].bias.detach().cpu()
    return h2.to(dtype) @ lin[2].weight.detach().cpu().to(dtype).t() + \
        lin[2].bias.detach().cpu().to(dtype)


def row_dev(q, ref):
    """Per row: max_a |q - ref| / max_a |ref| (float64)."""
    q, ref = q.detach().cpu().double(), ref.detach().cpu().double()
    return (q - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-30)


def clear_rows(ref, tol=None):
    """Rows whose top-2 gap exceeds 2 tol max|Q|: there an argmax within tol of `ref` is ref's."""
    tol = T_MODEL if tol is None else tol
    ref = ref.detach().cpu().double()
    top2 = ref.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) > 2 * tol * ref.abs().amax(1)


def _lowbias32(x):
    x = x.astype(np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def drop_thresh(p):
    """The 16-bit threshold mz_qact derives from the f32 p: a draw below it drops."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def keep_masks(seed, counter, rows, p):
    """The kernel's keep decisions, bool [len(rows), 32, 15, 15] (row and column 14, which the
    pooling never reads, False). rows: the list positions (without a row list: the instances).

    Key as mz_qact: k = seed * 0x9E3779B97F4A7C15 + counter * 0xD1B54A32D192ED03 + 1 (mod 2^64),
    key = low 32 bits of k ^ (k >> 32). Per (row, channel pair, pooled position) one xorshift32
    stream of 4 draws, seeded from the (row, pair) base and the position: draw r (= 2 dy + dx)
    -> low half: the even channel, high half: the odd one; kept iff the 16-bit draw >= thresh."""
    thresh = drop_thresh(p)
    k = ((int(seed) & M64) * 0x9E3779B97F4A7C15 + (int(counter) & M64) * 0xD1B54A32D192ED03 + 1) & M64
    key = np.uint64((k ^ (k >> 32)) & 0xFFFFFFFF)
    rows = np.asarray(rows, dtype=np.uint64)
    n = rows.shape[0]
    rkey = _lowbias32(key ^ _lowbias32(rows))  # [n]
    base = _lowbias32(rkey[:, None] ^ np.arange(16, dtype=np.uint64)[None]) | 1  # [n, 16]
    keep = np.zeros((n, 32, 15, 15), bool)
    for qi in range(49):
        y, x = 2 * (qi // 7), 2 * (qi % 7)
        st = _lowbias32(base ^ np.uint64((qi * 0x9E3779B9) & 0xFFFFFFFF)) | 1
        for r in range(4):
            st ^= (st << 13) & 0xFFFFFFFF
            st ^= st >> 17
            st ^= (st << 5) & 0xFFFFFFFF
            keep[:, 0::2, y + (r >> 1), x + (r & 1)] = (st & 0xFFFF) >= thresh
            keep[:, 1::2, y + (r >> 1), x + (r & 1)] = (st >> 16) >= thresh
    return keep


def drop_fraction(keep):
    """The dropped share of the 14 x 14 positions the pooling reads."""
    return 1.0 - float(keep[:, :, :14, :14].mean())


def synthetic_states(n, seed):
    """bits int32 [n, 22], obs6 f32 [n, 6] (numpy), n >= 12. Windows random at density 0.3; row 0
    all zeros, row 1 all 675 bits; row 2 is row 3 with the pad bits 675..703 of word 21 set as
    well (the kernels must ignore them: the same Q bit for bit). obs6 uniform in [-1, 1]; rows
    4..7 carry values whose lo half matters (1 + 2^-9 and its negative: hi = +-1, lo = +-2^-9;
    3e-5: a small magnitude beside them) and zeros."""
    assert n >= 12
    rng = np.random.default_rng(seed)
    w = rng.random((n, 675)) < 0.3
    w[0] = False
    w[1] = True
    w[2] = w[3]
    padded = np.zeros((n, 704), np.uint64)
    padded[:, :675] = w
    padded[2, 675:] = 1
    words = (padded.reshape(n, 22, 32) << np.arange(32, dtype=np.uint64)).sum(2)
    bits = words.astype(np.uint32).view(np.int32)
    obs6 = rng.uniform(-1.0, 1.0, (n, 6)).astype(np.float32)
    obs6[2] = obs6[3]
    e = np.float32(1.0 + 2.0 ** -9)
    obs6[4] = [e, -e, 3e-5, 0.0, e, -e]
    obs6[5] = e
    obs6[6] = -e
    obs6[7] = [3e-5, 0.0, -3e-5, 0.0, 3e-5, 0.0]
    return np.ascontiguousarray(bits), obs6
