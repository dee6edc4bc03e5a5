"""The autoencoder's HIP path (csrc/mz_cae.hip, mazerl/cae.py) against the float64 model of
tests/cae_model.py: the C entry points at the sample counts where the stem's group of 4, its
backward's chunk of 64 and a ragged tail change the launch, the reference's fixture end to end,
the trainer, load_stem on a DQN learner and a checkpoint round trip.

Tolerance. No number is fixed in advance: the unit is what f32 itself costs, the distance between
torch's own f32 evaluation of the model (cae_model.torch_f32: the drop-in module, mse_loss and
mazerl.cae.ssim on the CPU) and the float64 model on the same inputs, per tensor and relative to
that tensor's largest magnitude. The kernels get 4x that unit (differently associated 11-tap
filters and sample reductions, another expf). For Y, gfeat and the four parameter gradients the
unit is the case's own (same windows, same n, same alpha). For the three scalars loss, mse and ssim
one case's f32 distance is a single rounding's luck (it can be 0, which no f32 result could be
held to; over n = 1 .. 67 it varies 40 to 200-fold), so their unit is the largest over the sample
counts of the case set. alpha reaches the kernels as an f32, so every evaluation uses
float32(alpha).

Measured on an MI355X over n in {1, 3, 4, 5, 63, 64, 65, 67}, alpha in {0.65, 1, 0}, both pitches
(unit = the f32 yardstick, kernel = the kernels' distance, worst = the largest kernel / unit of any
single case):

            fixture and random windows                   constant footprints (sigma2^2 = 0)
  tensor    unit              kernels           worst    unit              kernels           worst
  y         9.5e-8 .. 1.9e-7  1.1e-7 .. 1.6e-7  1.19     9.6e-8 .. 1.5e-7  9.3e-8 .. 1.4e-7  1.10
  loss      5.7e-8 .. 1.2e-7  9.2e-10 .. 5.8e-8 0.95     1.3e-7 .. 6.2e-7  6.5e-10 .. 6.4e-8 0.49
  mse       8.8e-8 .. 1.1e-7  1.7e-9 .. 5.4e-8  0.52     1.3e-7            6.5e-10 .. 6.4e-8 0.49
  ssim      1.5e-7 .. 5.4e-6  6.8e-10 .. 1.1e-6 0.41     5.6e-6            9.4e-8 .. 1.6e-7  0.03
  gfeat     1.1e-7 .. 2.1e-7  7.2e-8 .. 1.7e-7  1.23     1.4e-7 .. 2.6e-5  1.1e-7 .. 4.7e-7  1.10
  dw_dec    9.0e-8 .. 5.8e-7  7.5e-8 .. 2.7e-7  1.47     1.5e-7 .. 9.8e-6  1.4e-7 .. 3.7e-7  1.20
  db_dec    3.6e-8 .. 8.7e-6  1.9e-8 .. 1.4e-6  1.45     8.8e-8 .. 4.1e-5  6.2e-9 .. 2.8e-7  0.34
  dw_enc    7.7e-8 .. 6.0e-7  5.8e-8 .. 1.6e-7  1.47     1.2e-7 .. 1.2e-5  6.0e-8 .. 4.0e-7  0.57
  db_enc    5.6e-8 .. 4.2e-7  3.9e-8 .. 2.6e-7  1.49     1.2e-7 .. 1.3e-5  3.6e-8 .. 4.1e-7  0.72

Decoder weights x50: worst single-case ratio 2.29 (db_enc, n = 4). 20 Adam steps: losses 4.5e-8
(unit 7.3e-8), parameters 1.3e-7 .. 2.7e-7 (units 1.3e-7 .. 7.2e-7). Fixture outputs through the
packed path: 1.16e-7 (unit 1.31e-7). Every test prints its figures before it asserts; DESIGN.md
section 6u has the table.

Memory contract: every output buffer is pre-filled with a NaN sentinel, padded to its pitch and
wrapped in guard rows; after the launches the sentinel must still stand in the pad columns and the
guards. The pad columns of the feature rows hold NaN too.
"""
import functools
import os

import numpy as np
import pytest
import torch

import cae_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SENT = 0x7FC0BEEF
NS = [1, 3, 4, 5, 63, 64, 65, 67]
ALPHAS = [0.65, 1.0, 0.0]
TENSORS = ("Y", "loss", "mse", "ssim", "gfeat", "dw_dec", "db_dec", "dw_enc", "db_enc")
MARGIN = 4.0


@pytest.fixture(autouse=True)
def _keep_qnet_numbering():
    """QNet numbers its instances (the number salts the dropout masks of its HIP stem) and tests
    later in a session regenerate those masks from it: the nets built here leave it as it was."""
    from mazerl.agents.nets import QNet
    n = QNet._count
    yield
    QNet._count = n


def _gold():
    return np.load(os.path.join(HERE, "golden", "cae.npz"))


def _cae():
    from mazerl.lib.models.convolutional_autoencoder import CAE
    return CAE


def _lib():
    from mazerl import _native as N
    return N, N.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Buf:
    """[rows, width] at row pitch ld inside guard rows, all NaN sentinel; `data` in the top left."""

    def __init__(self, rows, width=1, ld=None, data=None, guard=2):
        self.rows, self.width, self.ld, self.g = rows, width, ld or width, guard
        self.full = torch.full((rows + 2 * guard, self.ld), SENT, dtype=torch.int32,
                               device=DEV).view(torch.float32)
        if data is not None:
            self.body[:, :width] = data

    @property
    def body(self):
        return self.full[self.g:self.g + self.rows]

    @property
    def ptr(self):
        return self.body.data_ptr()

    def host(self):
        return self.body[:, :self.width].cpu().numpy().astype(np.float64)

    def raw(self):
        return self.body[:, :self.width].contiguous().view(torch.int32).cpu().numpy()

    def intact_outside(self):
        x = self.full.view(torch.int32).clone()
        x[self.g:self.g + self.rows, :self.width] = SENT
        return bool((x == SENT).all())


# ---- inputs ------------------------------------------------------------------------------------
def windows(kind, n):
    if kind == "fixture":
        x = _gold()["x"]
        return x[np.arange(n) % len(x)]
    rng = np.random.default_rng(77 + n)
    x = rng.integers(0, 2, (n, 3, 15, 15)).astype(np.uint8)
    if kind == "flat":  # constant filter footprints: sigma2^2 = 0 there
        x[:, 0] = 0
        x[:, 1] = 1
        x[:, 2, :11, :11] = np.arange(n).reshape(n, 1, 1) % 2
    return x


@functools.lru_cache(maxsize=None)
def reference(kind, n, alpha, scale=1.0):
    """(float64 model, torch f32) of one case, computed once."""
    from mazerl.cae import ssim
    a = float(np.float32(alpha))
    p = M.random_params(9, scale)
    x = windows(kind, n)
    return M.evaluate(p, x, a), M.torch_f32(p, x, a, _cae(), ssim)


SCALARS = ("loss", "mse", "ssim")


@functools.lru_cache(maxsize=None)
def scalar_units(kind, alpha, scale=1.0):
    """The three scalars' f32 yardstick: the largest torch-f32 distance over the case set's NS."""
    u = {k: 0.0 for k in SCALARS}
    for n in NS:
        ref, f32 = reference(kind, n, alpha, scale)
        for k in SCALARS:
            u[k] = max(u[k], M.distance(f32[k], ref[k]))
    return u


def units(kind, n, alpha, scale=1.0):
    """The f32 yardstick of one case: its own torch-f32 distance per tensor; the scalars pooled."""
    ref, f32 = reference(kind, n, alpha, scale)
    u = {k: M.distance(f32[k], ref[k]) for k in TENSORS}
    u.update(scalar_units(kind, alpha, scale))
    return u


def run_kernels(p, x, alpha, ld, ldg, grads=True):
    """stem forward -> mz_cae_decode, mz_cae_loss -> stem backward through the C ABI; returns
    name -> float64 numpy, and the raw int32 images of the outputs (bit comparisons)."""
    N, L = _lib()
    n = len(x)
    bits = _dev(M.pack(x))
    we, be, wd, bd = (_dev(p[k]) for k in M.NAMES)
    st = _stream()
    tmp = torch.empty(n, 1574, dtype=torch.float32, device=DEV)
    code = torch.empty(n, 1568, dtype=torch.uint8, device=DEV)
    obs6 = torch.zeros(n, 6, dtype=torch.float32, device=DEV)
    N.check(L.mz_stem_forward(bits.data_ptr(), obs6.data_ptr(), n, we.data_ptr(), be.data_ptr(),
                              0.0, None, 0, tmp.data_ptr(), 1574, code.data_ptr(), st))
    feat = Buf(n, 1568, ld, tmp[:, :1568])  # pad columns: NaN
    Y, loss3 = Buf(n, 675), Buf(1, 3)
    ws = Buf(1, L.mz_cae_workspace_floats(n))
    N.check(L.mz_cae_decode(feat.ptr, ld, n, wd.data_ptr(), bd.data_ptr(), Y.ptr, st))
    out = {}
    if not grads:
        N.check(L.mz_cae_loss(bits.data_ptr(), feat.ptr, ld, n, wd.data_ptr(), bd.data_ptr(),
                              alpha, loss3.ptr, None, ldg, None, None, ws.ptr, st))
        bufs = {"Y": Y, "loss3": loss3}
    else:
        gfeat, dwd, dbd = Buf(n, 1568, ldg), Buf(1, 384), Buf(1, 3)
        N.check(L.mz_cae_loss(bits.data_ptr(), feat.ptr, ld, n, wd.data_ptr(), bd.data_ptr(),
                              alpha, loss3.ptr, gfeat.ptr, ldg, dwd.ptr, dbd.ptr, ws.ptr, st))
        dwe, dbe = Buf(1, 864), Buf(1, 32)
        sws = Buf(1, max(1, L.mz_stem_workspace_floats(n)))
        N.check(L.mz_stem_backward(bits.data_ptr(), code.data_ptr(), gfeat.ptr, ldg, n, 0.0,
                                   sws.ptr, dwe.ptr, dbe.ptr, st))
        bufs = {"Y": Y, "loss3": loss3, "gfeat": gfeat, "dw_dec": dwd, "db_dec": dbd,
                "dw_enc": dwe, "db_enc": dbe}
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact_outside(), f"{k}: wrote outside its rows / columns"
    assert ws.intact_outside() and feat.intact_outside()
    out = {k: b.host() for k, b in bufs.items()}
    for j, k in enumerate(("loss", "mse", "ssim")):
        out[k] = out["loss3"][0, j]
    del out["loss3"]
    raw = {k: b.raw() for k, b in bufs.items()}
    return out, raw


def check(got, ref, unit, label):
    bad = []
    for k in got:
        d = M.distance(np.reshape(got[k], ref[k].shape), ref[k])
        print(f"{label} {k}: kernel {d:.3e} unit {unit[k]:.3e} ratio "
              f"{d / unit[k] if unit[k] else float('inf'):.2f}")
        assert np.isfinite(got[k]).all(), k
        if not d <= MARGIN * unit[k]:
            bad.append((k, d, unit[k]))
    assert not bad, f"{label}: beyond {MARGIN} x the f32 yardstick: {bad}"


# ---- the C ABI against the model ---------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("kind", ["fixture", "random"])
def test_kernels_against_model(kind, alpha):
    p = M.random_params(9)
    for n in NS:
        for ld, ldg in ((1574, 1574), (1600, 1632)):
            got, _ = run_kernels(p, windows(kind, n), alpha, ld, ldg)
            check(got, reference(kind, n, alpha)[0], units(kind, n, alpha),
                  f"{kind} a={alpha} n={n} ld={ld}")


@pytest.mark.parametrize("alpha", ALPHAS)
def test_constant_footprints(alpha):
    """Channels that are all 0 / all 1 and an 11x11 constant corner: sigma2^2 = 0 in the map."""
    p = M.random_params(9)
    for n in (1, 5, 67):
        got, _ = run_kernels(p, windows("flat", n), alpha, 1574, 1574)
        check(got, reference("flat", n, alpha)[0], units("flat", n, alpha), f"flat a={alpha} n={n}")


def test_saturated_decoder():
    """Decoder weights x50: Y reaches exactly 0 / 1 in f32 on part of the elements. Everything
    stays finite and within the yardstick of the model. dz is not an output, so in this mixed case
    the saturated elements' zero gradient is covered only through that tolerance; it is asserted
    exactly with the bias at +-1000 on top, where every element saturates and every gradient must
    be exactly 0."""
    p = M.random_params(9, 50.0)
    for n in (4, 67):
        got, _ = run_kernels(p, windows("random", n), 0.65, 1574, 1574)
        assert ((got["Y"] == 0.0) | (got["Y"] == 1.0)).any()
        assert got["Y"].min() >= 0.0 and got["Y"].max() <= 1.0
        check(got, reference("random", n, 0.65, 50.0)[0], units("random", n, 0.65, 50.0),
              f"x50 n={n}")
    q = dict(p)
    q["decoder.0.bias"] = np.array([1000.0, -1000.0, 1000.0], np.float32)
    got, _ = run_kernels(q, windows("random", 5), 0.65, 1574, 1574)
    assert ((got["Y"] == 0.0) | (got["Y"] == 1.0)).all()
    assert all(np.isfinite(got[k]) for k in ("loss", "mse", "ssim"))
    for k in ("gfeat", "dw_dec", "db_dec", "dw_enc", "db_enc"):
        assert (got[k] == 0.0).all(), k


def test_forward_only_and_identical_bits():
    p = M.random_params(9)
    for n in (3, 67):
        x = windows("random", n)
        a, ra = run_kernels(p, x, 0.65, 1600, 1574)
        b, rb = run_kernels(p, x, 0.65, 1600, 1574)
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k  # fixed-order sums: the same bits
        f, rf = run_kernels(p, x, 0.65, 1600, 1574, grads=False)
        assert np.array_equal(rf["loss3"], ra["loss3"]) and np.array_equal(rf["Y"], ra["Y"])


# ---- the fixture end to end --------------------------------------------------------------------
def _env(n):
    import mazerl
    return mazerl.VectorMazeEnv(n, 15, enrich=True, device=DEV, generate=False, window=False)


def test_fixture_end_to_end():
    from mazerl.cae import unpack_windows
    g = _gold()
    env = _env(8)
    env.load_mazes(g["grids"], g["start_goal"])
    env.reset()
    bits = env.window_bits.clone()
    assert np.array_equal(unpack_windows(bits).cpu().numpy(), g["x"].astype(np.float32))
    assert np.array_equal(bits.cpu().numpy(), M.pack(g["x"]))
    net = _cae()(3, 32)
    net.load_state_dict({k: torch.from_numpy(g["sd." + k]) for k in M.NAMES})
    y = net.to(DEV)(bits).cpu().numpy().astype(np.float64)
    ref = M.evaluate({k: g["sd." + k] for k in M.NAMES}, g["x"], 0.65)["Y"]
    unit = M.distance(g["y"], ref)  # the reference module's own f32 output against the model
    d = M.distance(y, ref)
    print(f"fixture Y: kernel {d:.3e} unit {unit:.3e}")
    assert d <= MARGIN * unit
    env.close()


# ---- the trainer -------------------------------------------------------------------------------
def _model(seed=0):
    torch.manual_seed(seed)
    return _cae()(3, 32)


def test_twenty_adam_steps_against_float64():
    from mazerl.cae import VectorCAETrainer, ssim
    net = _model(3)
    p = {k: v.numpy().copy() for k, v in net.state_dict().items()}
    x = np.concatenate([windows("fixture", 8), windows("random", 24)])
    batches = [x[4 * (k % 8):4 * (k % 8) + 4] for k in range(20)]
    a = float(np.float32(0.65))
    l64, p64 = M.adam_run(p, batches, a)
    l32, p32 = M.adam_run_f32(p, batches, a, _cae(), ssim)
    tr = VectorCAETrainer(net.to(DEV), _dev(M.pack(x)), batch_size=4, lr=5e-3, alpha=0.65)
    got = [tr.step(_dev(M.pack(b))) for b in batches]
    lk = torch.stack(got)[:, 0].cpu().numpy().astype(np.float64)
    pk = {k: v.cpu().numpy().astype(np.float64) for k, v in tr.model.state_dict().items()}
    bad = []
    rows = [("losses", lk, l32, l64)] + [(k, pk[k], p32[k], p64[k]) for k in M.NAMES]
    for name, k_, f_, r_ in rows:
        unit, d = M.distance(f_, r_), M.distance(k_, r_)
        print(f"20 steps {name}: kernel {d:.3e} unit {unit:.3e}")
        if not d <= MARGIN * unit:
            bad.append((name, d, unit))
    assert not bad, bad


def _collect(n, seed=1):
    from mazerl.cae import collect_windows
    env = _env(64)
    w = collect_windows(env, n, seed=seed)
    env.close()
    return w


def test_collect_windows_distinct_in_order():
    from mazerl.cae import unpack_windows
    w = _collect(64)
    assert w.shape == (64, 22) and w.dtype == torch.int32
    assert len({r.numpy().tobytes() for r in w.cpu()}) == 64
    x = unpack_windows(w).cpu().numpy()
    assert ((x[:, 0] + x[:, 1]).sum((1, 2)) == 224).all()  # wall + cell: all but the goal
    assert ((x[:, 1] - x[:, 2]).sum((1, 2)) == 0).all()    # non-visited: cells + goal - start
    env = _env(64)
    from mazerl.cae import collect_windows
    assert torch.equal(collect_windows(env, 40, seed=1), w[:40])  # generation order, seeded
    env.close()


def test_reduced_recipe_learns():
    """64 distinct windows, 48 / 16, batch 4, 10 epochs: the last epoch's mean loss below 0.1 x the
    first's, and the held-out similarity above 0.99 (the torch model alone, on the CPU: ratios
    0.061 to 0.065, similarity 0.9969)."""
    from mazerl.cae import VectorCAETrainer
    w = _collect(64)
    tr = VectorCAETrainer(_model(0).to(DEV), w[:48], batch_size=4, seed=0)
    log = tr.train(10)
    sim = tr.evaluate(w[48:], 4)
    print("recipe", [round(r["loss"], 5) for r in log], "sim", sim)
    assert [r["epoch"] for r in log] == list(range(10))
    assert log[-1]["loss"] < 0.1 * log[0]["loss"]
    assert sim > 0.99


def test_checkpoint_round_trip_resumes_to_identical_bits():
    from mazerl.cae import VectorCAETrainer
    w = _dev(M.pack(windows("fixture", 24)))
    a = VectorCAETrainer(_model(5).to(DEV), w, batch_size=4, seed=9)
    a.train(2)
    sd = a.state_dict()
    la = a.train(2)
    b = VectorCAETrainer(_model(6).to(DEV), w, batch_size=4, seed=1)
    b.load_state_dict(sd)
    lb = b.train(2)
    assert la == lb
    for (k, u), v in zip(a.model.state_dict().items(), b.model.state_dict().values()):
        assert torch.equal(u, v), k
    assert torch.equal(a.opt.exp_avg, b.opt.exp_avg)
    assert torch.equal(a.opt._step_buf, b.opt._step_buf)


def test_cae_loss_autograd_fills_the_gradients():
    from mazerl.cae import cae_loss
    x = windows("fixture", 5)
    net = _model(2)
    p = {k: v.numpy().copy() for k, v in net.state_dict().items()}
    ref = M.evaluate(p, x, float(np.float32(0.65)))
    net = net.to(DEV)
    loss = cae_loss(net, _dev(M.pack(x)), 0.65)
    (2.0 * loss).backward()
    assert abs(float(loss.detach()) - ref["loss"]) < 1e-6 * abs(ref["loss"])
    enc, dec = net.encoder[0], net.decoder[0]
    for g, k in ((enc.weight.grad, "dw_enc"), (enc.bias.grad, "db_enc"),
                 (dec.weight.grad, "dw_dec"), (dec.bias.grad, "db_dec")):
        assert M.distance(g.cpu().numpy() / 2.0, ref[k]) < 1e-5, k


def test_load_stem_into_a_dqn_learner():
    from mazerl.agents.dqn import VectorDQNLearner
    from mazerl.agents.nets import QNet
    from mazerl.cae import load_stem
    cae = _model(4)
    learner = VectorDQNLearner(16, DEV, variant="dqn", capacity=1024, batch_size=16, seed=3)
    bits = _dev(M.pack(windows("fixture", 16)))
    obs6 = torch.rand(16, 6, device=DEV)
    q_before = learner.fused(obs6, bits).clone()  # the acting weights are prepared now
    flat = learner.source._flat_params
    load_stem(learner, cae)
    assert learner.source._flat_params is flat
    from mazerl.agents.flat import _aliases
    assert _aliases(flat, list(learner.source.parameters()), learner.source._flat_sizes)
    for net in (learner.source, learner.target):
        assert torch.equal(net.conv[0].weight.cpu(), cae.encoder[0].weight)
        assert torch.equal(net.conv[0].bias.cpu(), cae.encoder[0].bias)
    for a, b in zip(learner.source.state_dict().values(), learner.target.state_dict().values()):
        assert torch.equal(a, b)
    ref = QNet(variant="dqn").to(DEV)  # a net that has the weights from the start
    ref.load_state_dict(learner.source.state_dict())
    head = learner._head(ref, 3)
    q = learner.fused(obs6, bits)
    assert torch.equal(q, head(obs6, bits))
    assert not torch.equal(q, q_before)
    with pytest.raises(ValueError):
        load_stem(learner, _cae()(3, 16))
