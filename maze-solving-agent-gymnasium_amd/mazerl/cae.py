"""Convolutional-autoencoder pre-training of the conv stem (train_CAE.py) on the GPU.

The reference trains `CAE(3, 32)` (lib/models/convolutional_autoencoder.py) on 400 distinct 15x15
mazes (generate_collection_of_mazes, lib/maze_generation.py:220-247) with
alpha * MSE + (1 - alpha) * (1 - SSIM), Adam(5e-3), CosineAnnealingLR(T_max=15, eta_min=1e-5)
stepped per epoch for 30 epochs, and saves `model.encoder` so that a Q-network's stem can start
from it. Here:

  collect_windows   the dataset: at 15x15 the Enrich window is the whole maze and reset() builds
                    `non_visited` as generate_collection_of_mazes does, so an element is the reset
                    window of a 15x15 instance, already packed in env.window_bits;
  cae_loss          stem forward (csrc/mz_stem.hip) -> mz_cae_loss (csrc/mz_cae.hip: decoder,
                    loss, dL/dfeat, decoder gradients, Y never in memory) -> stem backward;
  ssim              the same definition in torch ops (CPU / f32-window path);
  VectorCAETrainer  the recipe: seeded device shuffle, cae_loss's kernels, the flat one-launch
                    Adam (agents/flat.py FlatAdamW with weight_decay 0 and no clamp), torch's
                    CosineAnnealingLR values written to the device lr once per epoch;
  load_stem         hand the trained encoder to a net or learner of mazerl.agents.

SSIM is pytorch_msssim.ssim(Y, X, data_range=1) with its defaults *by definition* (11-tap
Gaussian, sigma 1.5, separable valid filtering, C1 = 0.01^2, C2 = 0.03^2, mean of the map, no
ReLU): that package is not a dependency, so parity with it is by the formula, not by a run.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N

FEAT = 1568
LD = FEAT + 6  # the stem's row: features | obs6 (unused here, zero)
C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- the loss in torch ops ---------------------------------------------------------------------
def gaussian_window(dtype=torch.float32, device=None):
    """g[k] ~ exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1."""
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype=dtype, device=device)


def _filter(x, g):
    c = x.shape[1]
    x = F.conv2d(x, g.view(1, 1, 11, 1).expand(c, 1, 11, 1), groups=c)
    return F.conv2d(x, g.view(1, 1, 1, 11).expand(c, 1, 1, 11), groups=c)


def ssim(Y, X):
    """SSIM(Y, X) of [n, c, h, w] images in [0, 1] (module docstring): a scalar."""
    g = gaussian_window(Y.dtype, Y.device)
    mu1, mu2 = _filter(Y, g), _filter(X, g)
    s1 = _filter(Y * Y, g) - mu1 * mu1
    s2 = _filter(X * X, g) - mu2 * mu2
    s12 = _filter(Y * X, g) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s1 + s2 + C2))
    return m.mean()


def unpack_windows(bits):
    """packed int32 [n, 22] -> f32 [n, 3, 15, 15] (bit ch*225 + r*15 + c of a sample)."""
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    x = (bits.unsqueeze(-1) >> sh) & 1
    return x.reshape(bits.shape[0], 22 * 32)[:, :675].reshape(-1, 3, 15, 15).to(torch.float32)


# ---- the HIP path ------------------------------------------------------------------------------
def _check_model(model):
    enc, dec = model.encoder[0], model.decoder[0]
    if tuple(enc.weight.shape) != (32, 3, 3, 3) or tuple(dec.weight.shape) != (32, 3, 2, 2) \
            or enc.bias is None or dec.bias is None:
        raise ValueError("the HIP path implements CAE(3, 32) on 15x15 windows")
    return enc, dec


def stem_features_only(bits, conv):
    """The encoder's output rows [n, 1574] (first 1,568 columns) from packed windows, no grad."""
    from .agents.stem import stem_features
    obs6 = torch.zeros(bits.shape[0], 6, dtype=torch.float32, device=bits.device)
    with torch.no_grad():
        return stem_features(bits, obs6, conv, 0.0, None, 0)


class _Buffers:
    """Per-batch-size scratch of one loss + gradient evaluation."""

    def __init__(self, n, dev, L):
        f32 = dict(dtype=torch.float32, device=dev)
        self.obs6 = torch.zeros(n, 6, **f32)
        self.feat = torch.empty(n, LD, **f32)
        self.code = torch.empty(n, FEAT, dtype=torch.uint8, device=dev)
        self.gfeat = torch.empty(n, LD, **f32)
        self.ws = torch.empty(max(1, L.mz_cae_workspace_floats(n)), **f32)
        self.sws = torch.empty(max(1, L.mz_stem_workspace_floats(n)), **f32)


def loss_and_grads(model, bits, alpha, grads=None, bufs=None):
    """loss3 = (loss, mse, ssim) f32 [3] on the device; with `grads` = (dw_enc, db_enc, dw_dec,
    db_dec) also the four parameter gradients, written there. Three or five launches."""
    enc, dec = _check_model(model)
    if not (bits.is_cuda and bits.dtype == torch.int32 and bits.dim() == 2 and bits.shape[1] == 22):
        raise ValueError("cae_loss takes packed int32 [n, 22] windows on the GPU")
    bits = bits.contiguous()
    n, dev = bits.shape[0], bits.device
    L = N.load()
    b = bufs if bufs is not None else _Buffers(n, dev, L)
    st = torch.cuda.current_stream(dev).cuda_stream
    ew, eb = enc.weight.detach(), enc.bias.detach()
    dw, db = dec.weight.detach(), dec.bias.detach()
    assert ew.is_contiguous() and dw.is_contiguous()
    loss3 = torch.empty(3, dtype=torch.float32, device=dev)
    N.check(L.mz_stem_forward(bits.data_ptr(), b.obs6.data_ptr(), n, ew.data_ptr(), eb.data_ptr(),
                              0.0, None, 0, b.feat.data_ptr(), LD,
                              b.code.data_ptr() if grads is not None else None, st))
    if grads is None:
        N.check(L.mz_cae_loss(bits.data_ptr(), b.feat.data_ptr(), LD, n, dw.data_ptr(),
                              db.data_ptr(), float(alpha), loss3.data_ptr(), None, LD, None, None,
                              b.ws.data_ptr(), st))
        return loss3
    g_ew, g_eb, g_dw, g_db = grads
    N.check(L.mz_cae_loss(bits.data_ptr(), b.feat.data_ptr(), LD, n, dw.data_ptr(), db.data_ptr(),
                          float(alpha), loss3.data_ptr(), b.gfeat.data_ptr(), LD, g_dw.data_ptr(),
                          g_db.data_ptr(), b.ws.data_ptr(), st))
    N.check(L.mz_stem_backward(bits.data_ptr(), b.code.data_ptr(), b.gfeat.data_ptr(), LD, n, 0.0,
                               b.sws.data_ptr(), g_ew.data_ptr(), g_eb.data_ptr(), st))
    return loss3


def _grad_outputs(model):
    """Where the four gradients go: the parameters' flat segments (agents/flat.py flatten_grads)
    when the model has them, else fresh tensors."""
    from .agents.flat import grad_segment
    enc, dec = model.encoder[0], model.decoder[0]
    ps = (enc.weight, enc.bias, dec.weight, dec.bias)
    segs = [grad_segment(p) for p in ps]
    if any(s is None for s in segs):
        segs = [torch.empty_like(p) for p in ps]
    return ps, segs


class _CAELossFn(torch.autograd.Function):
    """forward: the loss alone (stem forward, mz_cae_loss without gradients). backward: the
    gradient launches on the saved windows, like the stem's own autograd function — two forwards
    before a backward do not share any buffer."""

    @staticmethod
    def forward(ctx, bits, alpha, model, ew, eb, dw, db):
        ctx.bits, ctx.alpha, ctx.model = bits, alpha, model
        return loss_and_grads(model, bits, alpha)[0]

    @staticmethod
    def backward(ctx, g):
        model, bits = ctx.model, ctx.bits
        ctx.model = ctx.bits = None
        _, segs = _grad_outputs(model)
        loss_and_grads(model, bits, ctx.alpha, segs)  # dL/dp for an upstream gradient of 1
        for s in segs:
            s.mul_(g)
        return (None, None, None) + tuple(segs)


def cae_loss(model, bits, alpha=0.65):
    """alpha * MSE + (1 - alpha) * (1 - SSIM) of `model` on packed windows, a scalar with autograd:
    backward() computes the four parameter gradients at the parameters' values of that moment.
    With flattened parameters (agents/flat.py flatten_grads) they are written into the flat
    gradient segments and returned as views of them, so a parameter's .grad must be None when
    backward() runs (zero_grad(set_to_none=True) between steps): a .grad that already is the
    segment, as VectorCAETrainer keeps it for its own steps, would be added to itself."""
    enc, dec = _check_model(model)
    return _CAELossFn.apply(bits, float(alpha), model, enc.weight, enc.bias, dec.weight, dec.bias)


# ---- the dataset -------------------------------------------------------------------------------
def collect_windows(env, n, distinct=True, algorithms=("r-prim", "prim&kill", "dfs"), seed=0):
    """`n` packed reset windows [n, 22] int32 of a 15x15 Enrich `env`, generated one maze per
    instance without best-of selection, each maze's algorithm drawn uniformly from `algorithms`
    (generate_collection_of_mazes's random.choice). distinct: keep first occurrences in generation
    order (the reference's `not any(torch.equal(...))`), generating until there are n."""
    from .vector_env import ALGOS
    if env.maze_dim != 15 or not env.enrich or env.toroidal or env.window_bits is None:
        raise ValueError("collect_windows needs a euclidean 15x15 Enrich env with window_bits")
    ids = torch.tensor([ALGOS[a] for a in algorithms], dtype=torch.uint8)
    gen = torch.Generator().manual_seed(int(seed))
    B = env.num_envs
    seen, rows, rnd = set(), [], 0
    while len(rows) < n:
        algo = ids[torch.randint(len(ids), (B,), generator=gen)]
        env.generate(algorithm=algo, dim=15, seed=(int(seed) << 20) + rnd * B, candidates=1)
        env.reset()
        w = env.window_bits.cpu()
        for k in range(B):
            if len(rows) == n:
                break
            key = w[k].numpy().tobytes()
            if distinct and key in seen:
                continue
            seen.add(key)
            rows.append(w[k])
        rnd += 1
        if rnd > 64 + 8 * n:
            raise RuntimeError("could not collect enough distinct windows")
    return torch.stack(rows).to(env.device)


# ---- the trainer -------------------------------------------------------------------------------
class _CosineLR:
    """torch's CosineAnnealingLR values (its chained recurrence, which climbs back after T_max),
    from the scheduler itself on a one-element CPU optimizer."""

    def __init__(self, lr, t_max, eta_min):
        self._p = nn.Parameter(torch.zeros(1))
        self.opt = torch.optim.SGD([self._p], lr=lr)
        self.sched = torch.optim.lr_scheduler.CosineAnnealingLR(self.opt, T_max=t_max,
                                                                eta_min=eta_min)

    @property
    def lr(self):
        return float(self.opt.param_groups[0]["lr"])

    def step(self):
        self.opt.step()  # (keeps torch's "scheduler before optimizer" warning quiet)
        self.sched.step()
        return self.lr

    def state_dict(self):
        return {"sched": self.sched.state_dict(), "lr": self.lr}

    def load_state_dict(self, sd):
        self.sched.load_state_dict(sd["sched"])
        self.opt.param_groups[0]["lr"] = sd["lr"]


class VectorCAETrainer:
    """train_CAE.py on the GPU: `model` a CAE(3, 32) on the device, `windows` packed int32
    [N, 22]. Every step is five launches (stem forward, loss + decoder gradients, its reduce, stem
    backward + reduce) and one Adam launch over the flat parameter buffer."""

    def __init__(self, model, windows, batch_size=4, lr=5e-3, alpha=0.65, t_max=15, eta_min=1e-5,
                 seed=0):
        from .agents.flat import FlatAdamW, flatten_grads
        _check_model(model)
        self.model = model
        self.windows = windows.contiguous()
        dev = self.windows.device
        if dev.type != "cuda" or next(model.parameters()).device != dev:
            raise RuntimeError("VectorCAETrainer runs on the GPU (HIP); model and windows on it")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError("alpha outside [0, 1]")
        self.batch_size, self.alpha = int(batch_size), float(alpha)
        # Adam == AdamW without weight decay; no gradient clamp in the reference's script
        self.opt = FlatAdamW(model, lr, weight_decay=0.0, clamp=math.inf, write_grad=False)
        flatten_grads(model)
        self._ps, self._segs = _grad_outputs(model)
        for p, s in zip(self._ps, self._segs):
            p.grad = s  # the kernels write here; FlatAdamW then reads one contiguous gradient
        self.sched = _CosineLR(lr, t_max, eta_min)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(int(seed))
        self.epoch = 0
        self._bufs = {}
        self.L = N.load()

    def step(self, bits):
        """One Adam step on the batch `bits`; returns loss3 (loss, mse, ssim) on the device."""
        n = bits.shape[0]
        b = self._bufs.get(n)
        if b is None:
            b = self._bufs[n] = _Buffers(n, bits.device, self.L)
        loss3 = loss_and_grads(self.model, bits, self.alpha, self._segs, b)
        self.opt.step()
        return loss3

    def train(self, epochs):
        """`epochs` passes over the windows in a fresh seeded order each; per epoch
        {"epoch", "loss": mean batch loss, "lr": the rate after the scheduler's step, as the
        reference prints it}."""
        N_, bs = self.windows.shape[0], self.batch_size
        log = []
        for _ in range(int(epochs)):
            order = torch.randperm(N_, generator=self.gen, device=self.windows.device)
            data = self.windows[order]
            total = torch.zeros((), dtype=torch.float64, device=data.device)
            nb = 0
            for i in range(0, N_, bs):
                total += self.step(data[i:i + bs])[0]
                nb += 1
            lr = self.sched.step()
            self.opt.param_groups[0]["lr"].fill_(lr)  # the device scalar the Adam launch reads
            log.append({"epoch": self.epoch, "loss": float(total.item()) / nb, "lr": lr})
            self.epoch += 1
        return log

    @torch.no_grad()
    def evaluate(self, windows, batch_size=4):
        """train_CAE.py:61-73: per batch the cosine similarity between the flattened batch and the
        flattened round(Y), averaged over the batches."""
        sims = []
        for i in range(0, windows.shape[0], int(batch_size)):
            bits = windows[i:i + int(batch_size)].contiguous()
            x = unpack_windows(bits).reshape(1, -1)
            y = self.model(bits).round().reshape(1, -1)
            sims.append(F.cosine_similarity(x, y, dim=1))
        return float(torch.cat(sims).mean().item())

    def state_dict(self):
        return {"format": "mazerl.VectorCAETrainer/1",
                "model": {k: v.clone() for k, v in self.model.state_dict().items()},
                "exp_avg": self.opt.exp_avg.clone(), "exp_avg_sq": self.opt.exp_avg_sq.clone(),
                "step": self.opt._step_buf.clone(), "sched": self.sched.state_dict(),
                "epoch": self.epoch, "gen": self.gen.get_state(),
                "batch_size": self.batch_size, "alpha": self.alpha}

    def load_state_dict(self, sd):
        if sd.get("format") != "mazerl.VectorCAETrainer/1":
            raise ValueError("not a state_dict of a VectorCAETrainer")
        with torch.no_grad():
            for k, v in self.model.state_dict().items():
                v.copy_(sd["model"][k])  # in place: the parameters stay views of the flat buffer
        self.opt.exp_avg.copy_(sd["exp_avg"])
        self.opt.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.opt._step_buf.copy_(sd["step"])
        self.sched.load_state_dict(sd["sched"])
        self.opt.param_groups[0]["lr"].fill_(self.sched.lr)
        self.epoch = int(sd["epoch"])
        self.gen.set_state(sd["gen"].cpu())
        self.batch_size, self.alpha = int(sd["batch_size"]), float(sd["alpha"])


# ---- handing the encoder to a learner ----------------------------------------------------------
def _encoder_tensors(encoder):
    if isinstance(encoder, (str, bytes)) or hasattr(encoder, "__fspath__"):
        try:  # a state_dict, the documented format
            encoder = torch.load(encoder, map_location="cpu", weights_only=True)
        except Exception:  # a pickled module (the reference saves model.encoder whole): only
            # from a file you trust — unpickling runs what the file says
            encoder = torch.load(encoder, map_location="cpu", weights_only=False)
    if isinstance(encoder, nn.Module):
        conv = encoder.encoder[0] if hasattr(encoder, "encoder") else encoder[0]
        return conv.weight.detach(), conv.bias.detach()
    if isinstance(encoder, dict):
        for pre in ("encoder.0.", "0.", "conv.0."):
            if pre + "weight" in encoder:
                return encoder[pre + "weight"], encoder[pre + "bias"]
    raise ValueError("encoder: a CAE, its encoder Sequential, a state_dict of either, or a path")


def _stem_conv(net):
    conv = getattr(net, "conv", None)
    c0 = conv[0] if isinstance(conv, nn.Sequential) and len(conv) else None
    if not isinstance(c0, nn.Conv2d) or tuple(c0.weight.shape) != (32, 3, 3, 3) \
            or c0.padding != (1, 1) or c0.bias is None:
        raise ValueError("load_stem needs a net whose conv[0] is Conv2d(3, 32, 3, padding=1)")
    return c0


@torch.no_grad()
def load_stem(target, encoder):
    """Copy a trained encoder (a CAE, its `encoder` Sequential, a state_dict of either, or a path
    to one saved with torch.save) into the conv stem of `target`: a QNet (either variant),
    ActorCriticNet or PolicyNetwork, or a learner built on one (its `source` / `net` /
    `policy_net` / `agent` / `source_net`). In place (copy_), so flat-parameter views survive; a
    learner's target net and prepared acting weights are refreshed through its own sync path."""
    w, b = _encoder_tensors(encoder)
    if tuple(w.shape) != (32, 3, 3, 3) or tuple(b.shape) != (32,):
        raise ValueError(f"encoder stem of shape {tuple(w.shape)}: need [32, 3, 3, 3]")
    net = target
    if not isinstance(target, nn.Module):
        for name in ("source", "net", "policy_net", "agent", "source_net"):
            if isinstance(getattr(target, name, None), nn.Module):
                net = getattr(target, name)
                break
        else:
            raise ValueError("load_stem: no stem-bearing net on this learner")
    c0 = _stem_conv(net)
    if net is not target and hasattr(target, "finish"):
        target.finish()  # an overlapped learner: join its side stream first
    c0.weight.copy_(w.to(c0.weight.device))
    c0.bias.copy_(b.to(c0.bias.device))
    if net is target:
        return target
    if hasattr(target, "_sync_target"):  # VectorDQNLearner: target <- source
        target._sync_target()
    elif hasattr(target, "update_target"):  # the single-env DQN / DDQN agents
        target.update_target()
    heads = [getattr(target, "fused", None)] + list(getattr(target, "actor_fused", []))
    for h in heads:
        if h is not None and hasattr(h, "invalidate"):
            h.invalidate()  # prepared acting weights are rebuilt on the next act
    return target
