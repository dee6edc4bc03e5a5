"""The convolutional autoencoder without a GPU: the float64 model's own identities
(tests/cae_model.py), the drop-in CAE module against the reference's fixture
(tests/golden/cae.npz, written by tests/golden/make_golden_cae.py), the torch-op loss against the
model, load_stem on the three net classes, and the C entry points' refusals (which launch
nothing, so they need no device)."""
import os

import numpy as np
import pytest
import torch

import cae_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = 0x1000  # a non-NULL "device pointer": every call below is refused before it is used


@pytest.fixture(autouse=True)
def _keep_qnet_numbering():
    """QNet numbers its instances (the number salts the dropout masks of its HIP stem) and tests
    later in a session regenerate those masks from it: the nets built here leave it as it was."""
    from mazerl.agents.nets import QNet
    n = QNet._count
    yield
    QNet._count = n


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "cae.npz"))


def _cae():
    from mazerl.lib.models.convolutional_autoencoder import CAE
    return CAE


def test_gaussian_sums_to_one():
    from mazerl.cae import gaussian_window
    g = M.gaussian()
    assert g.shape == (11,) and abs(float(g.sum()) - 1.0) < 1e-15
    assert torch.equal(g, g.flip(0)) and int(g.argmax()) == 5
    w = gaussian_window(torch.float32)
    assert abs(float(w.double().sum()) - 1.0) < 1e-7
    assert np.allclose(w.double().numpy(), g.numpy(), rtol=0, atol=2 ** -25)


def test_ssim_of_identical_images_is_one(gold):
    from mazerl.cae import ssim
    X = torch.from_numpy(gold["x"].astype(np.float64))
    assert float(M.ssim_map(X, X).min()) == 1.0 and float(M.ssim_map(X, X).max()) == 1.0
    assert float(ssim(X.float(), X.float())) == 1.0
    R = torch.from_numpy(np.random.default_rng(5).integers(0, 2, (3, 3, 15, 15)).astype(np.float32))
    assert float(ssim(R, R)) == 1.0


def test_dropin_has_the_reference_layout_and_outputs(gold):
    net = _cae()(3, 32)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold["names"]]
    for k in sd:
        assert tuple(sd[k].shape) == gold["sd." + k].shape, k
    net.load_state_dict({k: torch.from_numpy(gold["sd." + k]) for k in sd})
    with torch.no_grad():
        y = net(torch.from_numpy(gold["x"]).float())
    assert y.shape == (8, 3, 15, 15)
    # the same torch modules on the same inputs: f32 rounding of another conv algorithm at most
    assert np.max(np.abs(y.numpy() - gold["y"])) <= 4 * 2.0 ** -24
    # and the float64 model is the same function
    ref = M.evaluate({k: gold["sd." + k] for k in M.NAMES}, gold["x"], 0.65)
    assert M.distance(gold["y"], ref["Y"]) < 1e-6


def test_fixture_tensors_are_the_grids_reset_planes(gold):
    g, sg, x = gold["grids"], gold["start_goal"], gold["x"]
    for k in range(len(g)):
        nv = (g[k] != 0).astype(np.uint8)
        nv[sg[k][0], sg[k][1]] = 0
        assert np.array_equal(x[k], np.stack([g[k] == 0, g[k] == 1, nv]).astype(np.uint8))
        assert g[k][sg[k][2], sg[k][3]] == 2


@pytest.mark.parametrize("alpha", [0.65, 1.0, 0.0])
def test_torch_path_agrees_with_the_model(gold, alpha):
    """The product's CPU path (CAE in f32 + mazerl.cae.ssim) is the model up to f32."""
    from mazerl.cae import ssim
    p = M.random_params(3)
    ref = M.evaluate(p, gold["x"], alpha)
    got = M.torch_f32(p, gold["x"], alpha, _cae(), ssim)
    for k in got:
        assert M.distance(got[k], ref[k]) < 2e-5, k


def test_pack_unpack_roundtrip(gold):
    from mazerl.cae import unpack_windows
    bits = torch.from_numpy(M.pack(gold["x"]))
    assert bits.shape == (8, 22) and bits.dtype == torch.int32
    assert np.array_equal(unpack_windows(bits).numpy(), gold["x"].astype(np.float32))


def _nets():
    from mazerl.agents.nets import QNet
    from mazerl.agents.ppo import ActorCriticNet
    from mazerl.agents.rf_agent import PolicyNetwork
    return [lambda: QNet(variant="dqn"), lambda: QNet(variant="ddqn"),
            lambda: ActorCriticNet(3, 6, 4, 32, 1024), lambda: PolicyNetwork(3, 6, 4, 32, 1024)]


@pytest.mark.parametrize("which", range(4))
def test_load_stem_into_every_net_class(tmp_path, which):
    from mazerl.cae import load_stem
    torch.manual_seed(11)
    cae = _cae()(3, 32)
    net = _nets()[which]()
    w_ptr = net.conv[0].weight.data_ptr()
    path = str(tmp_path / "enc.pth")
    torch.save(cae.encoder.state_dict(), path)
    for src in (cae, cae.encoder, cae.state_dict(), cae.encoder.state_dict(), path):
        with torch.no_grad():
            net.conv[0].weight.zero_()
        load_stem(net, src)
        assert torch.equal(net.conv[0].weight, cae.encoder[0].weight)
        assert torch.equal(net.conv[0].bias, cae.encoder[0].bias)
    assert net.conv[0].weight.data_ptr() == w_ptr  # copied in place


def test_load_stem_refuses_another_shape():
    from mazerl.agents.nets import QNet
    from mazerl.cae import load_stem
    with pytest.raises(ValueError):
        load_stem(QNet(variant="dqn"), _cae()(3, 16))
    with pytest.raises(ValueError):
        load_stem(QNet(h_channels=16, variant="dqn"), _cae()(3, 32))


def test_cosine_schedule_is_torchs():
    """The trainer's per-epoch rates are CosineAnnealingLR(T_max=15, eta_min=1e-5)'s own: down to
    eta_min at epoch 15 and back up to the base rate at 30."""
    from mazerl.cae import _CosineLR
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=5e-3)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=15, eta_min=1e-5)
    mine = _CosineLR(5e-3, 15, 1e-5)
    want, got = [], []
    for _ in range(30):
        opt.step()
        sch.step()
        want.append(opt.param_groups[0]["lr"])
        got.append(mine.step())
    assert got == want
    assert abs(got[14] - 1e-5) < 1e-12 and abs(got[29] - 5e-3) < 1e-9 and got[20] > got[16]


# ---- refusals of the C entry points (nothing is launched) --------------------------------------
def _lib():
    from mazerl import _native as N
    return N.load()


def _loss_args(**kw):
    a = dict(bits=FAKE, feat=FAKE, ld=1574, n=4, w=FAKE, b=FAKE, alpha=0.65, loss3=FAKE,
             gfeat=FAKE, ldg=1574, dw=FAKE, db=FAKE, ws=FAKE)
    a.update(kw)
    return (a["bits"], a["feat"], a["ld"], a["n"], a["w"], a["b"], a["alpha"], a["loss3"],
            a["gfeat"], a["ldg"], a["dw"], a["db"], a["ws"], None)


@pytest.mark.parametrize("bad", [dict(bits=None), dict(feat=None), dict(w=None), dict(b=None),
                                 dict(loss3=None), dict(ws=None), dict(n=0), dict(n=-3),
                                 dict(ld=1567), dict(ldg=1567), dict(alpha=-0.01),
                                 dict(alpha=1.01), dict(alpha=float("nan"))])
def test_loss_refusals(bad):
    L = _lib()
    assert L.mz_cae_loss(*_loss_args(**bad)) != 0
    assert L.mz_last_error()


@pytest.mark.parametrize("bad", [dict(feat=None), dict(w=None), dict(b=None), dict(out=None),
                                 dict(n=0), dict(ld=1567)])
def test_decode_refusals(bad):
    a = dict(feat=FAKE, ld=1568, n=2, w=FAKE, b=FAKE, out=FAKE)
    a.update(bad)
    assert _lib().mz_cae_decode(a["feat"], a["ld"], a["n"], a["w"], a["b"], a["out"], None) != 0


def test_workspace_size():
    L = _lib()
    assert L.mz_cae_workspace_floats(0) == 0 and L.mz_cae_workspace_floats(-1) == 0
    assert L.mz_cae_workspace_floats(1) >= 384 + 3 + 2
    assert L.mz_cae_workspace_floats(4096) == 4096 * L.mz_cae_workspace_floats(1)
