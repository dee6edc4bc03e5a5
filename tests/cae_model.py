"""A float64 model of the convolutional autoencoder and its loss, written from the definitions
(not from the product's code): the yardstick of tests/test_cae.py and tests/test_cae_gpu.py.

  X        [n, 3, 15, 15] binary (channel order wall, cell, non-visited).
  encoder  feat = MaxPool2(LeakyReLU_0.01(Conv3x3_pad1(X) + b)), [n, 32, 7, 7].
  decoder  z[o, 2i+a, 2j+b] = b[o] + sum_c feat[c, i, j] W[c, o, a, b]; row / column 14 = b[o];
           Y = 1 / (1 + exp(-z)).
  loss     alpha * mean((Y - X)^2) + (1 - alpha) * (1 - SSIM(Y, X)).
  SSIM     g[k] ~ exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, sum 1; F = valid filter down the rows
           then along the columns (15x15 -> 5x5), per channel; mu1 = F(Y), mu2 = F(X),
           s1 = F(YY) - mu1^2, s2 = F(XX) - mu2^2, s12 = F(YX) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2,
           map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * (2 s12 + C2) / (s1 + s2 + C2); the mean
           of the map over all 75 n entries, no ReLU.
  Adam     lr, betas (0.9, 0.999), eps 1e-8: m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
           p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps).

Gradients come from float64 autograd on these formulas. `torch_f32` evaluates the same model with
torch's own f32 modules and ops: its distance from the float64 model is what f32 costs, the unit
the kernels' tolerances are counted in.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
NAMES = ("encoder.0.weight", "encoder.0.bias", "decoder.0.weight", "decoder.0.bias")


def gaussian():
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def encode(X, we, be):
    a = F.conv2d(X, we, be, padding=1)
    a = torch.where(a > 0, a, a * 0.01)
    return F.max_pool2d(a, 2, 2)


def decode(feat, wd, bd):
    n = feat.shape[0]
    z = bd.view(1, 3, 1, 1).expand(n, 3, 15, 15).clone()
    t = torch.einsum("ncij,coab->noiajb", feat, wd).reshape(n, 3, 14, 14)
    z[:, :, :14, :14] = z[:, :, :14, :14] + t
    return 1.0 / (1.0 + torch.exp(-z))


def filt(x, g):
    x = (x.unfold(2, 11, 1) * g).sum(-1)   # [n, c, 5, 15]
    return (x.unfold(3, 11, 1) * g).sum(-1)  # [n, c, 5, 5]


def ssim_map(Y, X):
    g = gaussian().to(Y.dtype)
    mu1, mu2 = filt(Y, g), filt(X, g)
    s1 = filt(Y * Y, g) - mu1 * mu1
    s2 = filt(X * X, g) - mu2 * mu2
    s12 = filt(Y * X, g) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * (2 * s12 + C2) / (s1 + s2 + C2)


def loss_terms(Y, X, alpha):
    mse = ((Y - X) ** 2).mean()
    ss = ssim_map(Y, X).mean()
    return alpha * mse + (1 - alpha) * (1 - ss), mse, ss


def _params64(params):
    return [torch.as_tensor(np.asarray(params[k], dtype=np.float64)).clone().requires_grad_(True)
            for k in NAMES]


def evaluate(params, X, alpha):
    """Everything the kernels produce, in float64 numpy: Y, loss, mse, ssim, gfeat [n, 1568], the decoder's
    and the encoder's gradients. params: name -> array; X: [n, 3, 15, 15] of 0 / 1."""
    we, be, wd, bd = _params64(params)
    X = torch.as_tensor(np.asarray(X, dtype=np.float64))
    feat = encode(X, we, be)
    feat.retain_grad()
    Y = decode(feat, wd, bd)
    loss, mse, ss = loss_terms(Y, X, float(alpha))
    loss.backward()
    out = {"Y": Y, "loss": loss, "mse": mse, "ssim": ss, "feat": feat,
           "gfeat": feat.grad.reshape(X.shape[0], -1), "dw_dec": wd.grad, "db_dec": bd.grad,
           "dw_enc": we.grad, "db_enc": be.grad}
    return {k: v.detach().numpy() for k, v in out.items()}


def torch_f32(params, X, alpha, model_cls, ssim_fn):
    """The same quantities from torch's own f32 evaluation: the drop-in module `model_cls(3, 32)`
    (Conv2d, LeakyReLU, MaxPool2d, ConvTranspose2d, Sigmoid), mse_loss and `ssim_fn` in f32."""
    net = model_cls(3, 32)
    net.load_state_dict({k: torch.as_tensor(np.asarray(params[k], dtype=np.float32)) for k in NAMES})
    X = torch.as_tensor(np.asarray(X, dtype=np.float32))
    feat = net.encoder(X)
    feat.retain_grad()
    Y = net.decoder(feat)
    mse = F.mse_loss(Y, X)
    ss = ssim_fn(Y, X)
    loss = alpha * mse + (1 - alpha) * (1 - ss)
    loss.backward()
    enc, dec = net.encoder[0], net.decoder[0]
    out = {"Y": Y, "loss": loss, "mse": mse, "ssim": ss,
           "gfeat": feat.grad.reshape(X.shape[0], -1), "dw_dec": dec.weight.grad,
           "db_dec": dec.bias.grad, "dw_enc": enc.weight.grad, "db_enc": enc.bias.grad}
    return {k: v.detach().double().numpy() for k, v in out.items()}


def distance(a, ref):
    """max |a - ref| relative to ref's largest magnitude (0 / 0 = 0)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    m = float(np.max(np.abs(ref))) if ref.size else 0.0
    d = float(np.max(np.abs(a - ref))) if ref.size else 0.0
    return d / m if m > 0 else (0.0 if d == 0 else math.inf)


def adam_run(params, batches, alpha, lr=5e-3, b1=0.9, b2=0.999, eps=1e-8):
    """`len(batches)` Adam steps in float64 on the model: (losses [steps], final params)."""
    p = _params64(params)
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    losses = []
    for t, X in enumerate(batches, 1):
        X = torch.as_tensor(np.asarray(X, dtype=np.float64))
        for x in p:
            x.grad = None
        loss = loss_terms(decode(encode(X, p[0], p[1]), p[2], p[3]), X, float(alpha))[0]
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for x, mm, vv in zip(p, m, v):
                g = x.grad
                mm.mul_(b1).add_(g, alpha=1 - b1)
                vv.mul_(b2).addcmul_(g, g, value=1 - b2)
                x -= lr / (1 - b1 ** t) * mm / (vv.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    return np.array(losses), {k: x.detach().numpy() for k, x in zip(NAMES, p)}


def adam_run_f32(params, batches, alpha, model_cls, ssim_fn, lr=5e-3):
    """The same steps with torch's f32 modules and torch.optim.Adam."""
    net = model_cls(3, 32)
    net.load_state_dict({k: torch.as_tensor(np.asarray(params[k], dtype=np.float32)) for k in NAMES})
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    losses = []
    for X in batches:
        X = torch.as_tensor(np.asarray(X, dtype=np.float32))
        Y = net(X)
        loss = alpha * F.mse_loss(Y, X) + (1 - alpha) * (1 - ssim_fn(Y, X))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses, dtype=np.float64), \
        {k: v.detach().double().numpy() for k, v in net.state_dict().items()}


def random_params(seed, scale=1.0):
    """CAE(3, 32) parameters (f32 numpy) uniform in +-1 / sqrt(fan_in); `scale` multiplies the
    decoder's weights (x50 saturates Y)."""
    rng = np.random.default_rng(seed)
    u = lambda shape, fan: (rng.uniform(-1, 1, shape) / math.sqrt(fan)).astype(np.float32)  # noqa: E731
    return {"encoder.0.weight": u((32, 3, 3, 3), 27), "encoder.0.bias": u((32,), 27),
            "decoder.0.weight": (u((32, 3, 2, 2), 12) * np.float32(scale)),
            "decoder.0.bias": u((3,), 12)}


def pack(X):
    """[n, 3, 15, 15] of 0 / 1 -> packed int32 [n, 22] numpy (bit ch*225 + r*15 + c)."""
    x = np.asarray(X).reshape(len(X), -1).astype(np.uint64)
    x = np.concatenate([x, np.zeros((len(X), 22 * 32 - 675), np.uint64)], 1).reshape(len(X), 22, 32)
    words = (x << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return words.view(np.int32)
