"""The float64 models of tests/learner_model.py against torch float64 on the CPU: autograd of the
reference expression (Linear(H, 4) after ReLU / LeakyReLU, gather, argmax / max, mse_loss) and
torch.optim.AdamW(foreach=False) with grad.clamp_. The GPU tests compare the HIP kernels with
these models; here the models themselves are pinned, on random rows and on the hand-made special
rows (ties, signed zeros, NaN, inf) the GPU tests use.

The models hold three constants as the f32 values the kernels use; torch is given the same ones
(the f32 slope and gamma; its gradients rescaled by f32(2 / b) / (2 / b)), so the comparison is at
float64 rounding level. AdamW's seven scalars are f32 casts of the doubles torch uses (relative
2^-24 each), so that comparison allows 16 * 2^-24 of each tensor's scale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import learner_model as M
import learner_util as U


def _torch_head(c, gradient):
    b, act, dbl = c["b"], c["act"], c["dbl"]
    t = lambda k, g=False: torch.tensor(c[k], dtype=torch.float64, requires_grad=g)  # noqa: E731
    z2s, w3s, b3s = t("z2s", True), t("w3s", True), t("b3s", True)
    fa = (lambda x: F.leaky_relu(x, float(np.float32(0.01)))) if act == 0 else torch.relu
    q = F.linear(fa(z2s), w3s, b3s)
    with torch.no_grad():
        q_t = F.linear(fa(t("z2t")), t("w3t"), t("b3t"))[:b]
        if dbl:
            v = q_t.gather(1, q[b:2 * b].max(1)[1].unsqueeze(1)).squeeze(1)
        else:
            v = q_t.max(1)[0]
        expected = v * float(np.float32(c["gamma"])) + t("reward")[:b]
    q_sa = q[:b].gather(1, torch.tensor(c["action"][:b]).view(-1, 1))
    loss = F.mse_loss(q_sa, expected.unsqueeze(1))
    loss.backward(gradient=torch.tensor(gradient, dtype=torch.float64))
    fix = float(np.float32(2.0 / b)) / (2.0 / b)
    return dict(diff=(q_sa.squeeze(1) - expected).detach().numpy(), loss=float(loss.detach()),
                q=q.detach().numpy(), q_t=q_t.numpy(), dz2=z2s.grad.numpy() * fix,
                dW=w3s.grad.numpy() * fix, db=b3s.grad.numpy() * fix)


def _same(x, y, what):
    # two float64 summation orders of <= 1,024 terms of magnitude <= ~30: far below 1e-12
    np.testing.assert_allclose(x, y, rtol=1e-11, atol=1e-12, equal_nan=True, err_msg=what)


def _check_head(c, grads=True):
    b, gradient = c["b"], 0.625
    ref = _torch_head(c, gradient)
    fw = M.head_forward(c["z2s"], c["w3s"], c["b3s"], c["z2t"], c["w3t"], c["b3t"], c["action"],
                        c["reward"], c["gamma"], b, c["act"], c["dbl"])
    _same(fw["q_s"], ref["q"][:b], "q_s")
    _same(fw["q_t"], ref["q_t"], "q_t")
    if c["dbl"]:
        _same(fw["q_n"], ref["q"][b:2 * b], "q_n")
    _same(fw["diff"], ref["diff"], "diff")
    _same(fw["loss"], ref["loss"], "loss")
    if "choice" in c:
        assert list(fw["choice"]) == list(c["choice"])
    dz2, dW, db = M.head_backward(gradient, fw["diff"], c["action"], b, c["z2s"], c["w3s"], c["act"])
    _same(dz2, ref["dz2"][:b], "dz2")
    assert not ref["dz2"][b:].any()  # the s' rows carry no gradient
    if grads:
        _same(dW, ref["dW"], "dW3")
        _same(db, ref["db"], "db3")
    return fw


@pytest.mark.parametrize("dbl", [0, 1])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("H,b", [(4, 1), (8, 5), (60, 17), (260, 16), (512, 67)])
def test_head_model_matches_torch_autograd(H, b, act, dbl):
    c = dict(U.head_case(H, b, act), dbl=dbl)
    _check_head(c)
    c = dict(U.head_case(H, b, act, missing_action=2), dbl=dbl)
    fw = _check_head(c)
    _, dW, db = M.head_backward(1.0, fw["diff"], c["action"], b, c["z2s"], c["w3s"], act)
    assert not dW[2].any() and db[2] == 0


@pytest.mark.parametrize("c", U.special_head_cases(), ids=lambda c: c["name"])
def test_head_model_special_rows_match_torch(c):
    """Ties (first maximum), signed zeros, NaN and inf rows: values and NaN positions as torch
    has them. fc3's weight / bias gradients are compared where every activation and diff is
    finite: torch's dense dq^T h spreads 0 * NaN over the other actions' rows of dW3, the gather
    form (the model's and the kernels') does not."""
    finite = all(np.isfinite(c[k]).all() for k in ("z2s", "z2t", "b3s"))
    fw = _check_head(c, grads=finite)
    if c["name"].startswith(("nan", "bias-nan", "qrows")):
        assert np.isnan(fw["loss"]) and np.isnan(fw["diff"]).any()
    if c["name"].startswith("inf"):
        assert np.isinf(fw["diff"][2]) and np.isinf(fw["loss"])


def test_head_model_activation_rules():
    nan, inf = float("nan"), float("inf")
    z = np.array([-inf, -1.0, -0.0, 0.0, 2.0, inf, nan], np.float32)
    g = np.full(7, 3.0)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    for act, fn in ((0, lambda x: F.leaky_relu(x, float(np.float32(0.01)))), (1, torch.relu)):
        zt.grad = None
        y = fn(zt)
        y.backward(torch.tensor(g))
        _same(M.act_forward(z, act), y.detach().numpy(), "forward")
        _same(M.act_backward(z, g, act), zt.grad.numpy(), "backward")


@pytest.mark.parametrize("dbl", [0, 1])
def test_q_loss_model_matches_torch(dbl):
    rng = np.random.default_rng(5 + dbl)
    b, rows = 67, 2 * 67 + 3
    q, qn, qt = (rng.standard_normal((n, 4)).astype(np.float32) for n in (rows, b, b))
    qn[:8, 2] = qn[:8, 0] = 3.0  # ties: the first maximum
    qn[3, 1] = qt[5, 2] = np.nan
    a = rng.integers(0, 4, b)
    r = rng.choice(U.REWARDS, b).astype(np.float32)
    qq = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(qt, dtype=torch.float64)
    v = tt.gather(1, torch.tensor(qn).double().argmax(1, keepdim=True)).squeeze(1) if dbl \
        else tt.max(1)[0]
    expected = v * float(np.float32(0.7)) + torch.tensor(r).double()
    q_sa = qq[:b].gather(1, torch.tensor(a).view(-1, 1))
    loss = F.mse_loss(q_sa, expected.unsqueeze(1))
    loss.backward(gradient=torch.tensor(0.625, dtype=torch.float64))
    out = M.q_loss_forward(q, qn if dbl else None, qt, a, r, 0.7, b)
    _same(out["diff"], (q_sa.squeeze(1) - expected).detach().numpy(), "diff")
    _same(out["loss"], float(loss.detach()), "loss")
    dq = M.q_loss_backward(0.625, out["diff"], a, b, rows)
    _same(dq, qq.grad.numpy() * (float(np.float32(2.0 / b)) / (2.0 / b)), "dq")


@pytest.mark.parametrize("gscale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("clamp", [1.0, 0.25])
def test_adamw_model_matches_torch_adamw(clamp, gscale):
    rng = np.random.default_rng(9)
    n, lr, wd = 4096, 1e-3, 1e-2
    p0 = rng.standard_normal(n).astype(np.float32)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([pt], lr=lr, weight_decay=wd, foreach=False)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(3):
        g = (rng.standard_normal(n) * (3.0 if step == 1 else 0.5)).astype(np.float32)
        g[:4] = [np.nan, np.inf, -np.inf, clamp]
        pt.grad = torch.tensor(g, dtype=torch.float64) * float(np.float32(gscale))
        pt.grad.clamp_(-clamp, clamp)  # average over ranks, then clamp
        opt.step()
        p, m, v, gc = M.adamw_step(p, g, m, v, lr, step, 0.9, 0.999, 1e-8, wd, clamp, gscale)
        st = opt.state[pt]
        _same(gc, pt.grad.numpy(), "clamped gradient")
        assert np.isnan(gc[0]) and gc[1] == clamp and gc[2] == -clamp
        for x, y, what in ((p, pt.detach().numpy(), "p"), (m, st["exp_avg"].numpy(), "m"),
                           (v, st["exp_avg_sq"].numpy(), "v")):
            assert np.isnan(x[0]) and np.isnan(y[0]), what
            np.testing.assert_allclose(x[1:], y[1:], rtol=16 * M.U32,
                                       atol=16 * M.U32 * np.abs(y[1:]).max(), err_msg=what)
        assert float(st["step"]) == step + 1


def test_near_tie_cap_is_zero_for_every_listed_case():
    """tests/test_head_loss_exact.py may leave out rows whose float64 top-two gap of q_n is within
    twice the Q tolerance; for its listed (H, b, act) no such row exists."""
    cases = [(H, b) for H in (4, 8, 60, 252, 256, 260, 512, 1024) for b in (1, 3, 4, 5, 15, 16, 17, 67)]
    for H, b in cases + [(8, 1029)]:
        for act in (0, 1):
            c = U.head_case(H, b, act)
            fw = M.head_forward(c["z2s"], c["w3s"], c["b3s"], c["z2t"], c["w3t"], c["b3t"],
                                c["action"], c["reward"], c["gamma"], b, act, 1)
            _, near = M.head_tolerances(fw, c["action"], c["reward"], c["gamma"], H, 1)
            assert int(near.sum()) == 0, (H, b, act)


def test_pack_windows_round_trip():
    from test_qfront import bits_to_window, random_bits
    w = U.make_batch(16, 33)[1]
    bits = U.pack_windows(w)
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (16, 22)
    assert torch.equal(bits_to_window(bits), torch.from_numpy(w))
    rb = random_bits(64, torch.Generator().manual_seed(2))  # bit 31 set: negative words
    assert torch.equal(U.pack_windows(bits_to_window(rb)), rb)
