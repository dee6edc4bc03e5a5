"""The fused Q head + loss (agents/dqn.py _HeadLossFn: mz_head_loss / mz_head_loss_backward, one
launch forward for both nets' last activation, fc3 and the loss; one launch + a column sum
backward) against the unfused path (the nets' own fc3 / activation launches, then mz_q_loss):
the loss and every source gradient agree to f32 tolerance (the dot products associate
differently), for DQN (LeakyReLU, max over the target's row) and DDQN (ReLU, the stacked [s; s']
pass and the argmax of the source's s' rows), with and without the flat gradient buffer
(agents/flat.py: fc3's weight and bias gradients land in their segments with one column sum)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _batch(b, seed):
    g = torch.Generator().manual_seed(seed)
    s6 = torch.rand(b, 6, generator=g).cuda()
    sw = torch.randint(0, 2 ** 31, (b, 22), generator=g, dtype=torch.int64)
    sw[:, 21] &= 7
    sw = sw.to(torch.int32).cuda()
    s6n = torch.rand(b, 6, generator=g).cuda()
    swn = torch.roll(sw, 1, 0).contiguous()
    a = torch.randint(0, 4, (b,), generator=g).cuda()
    r = (torch.rand(b, generator=g) - 0.5).cuda()
    return (s6, sw), a, r, (s6n, swn)


@pytest.mark.parametrize("flat", [False, True], ids=["grads", "flat-grads"])
@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
@pytest.mark.parametrize("b", [200, 1024])
def test_fused_head_matches_unfused(variant, flat, b):
    import mazerl.agents.dqn as D
    from mazerl.agents.flat import flatten_grads
    from mazerl.agents.nets import QNet
    torch.manual_seed(3)
    src0 = QNet(3, 6, 4, 32, 1024, variant).cuda()
    tgt0 = QNet(3, 6, 4, 32, 1024, variant).cuda()
    state, a, r, nxt = _batch(b, 11)
    out = {}
    for fused in (True, False):
        src, tgt = copy.deepcopy(src0), copy.deepcopy(tgt0)
        src.eval(); tgt.eval()  # Dropout(0.2) (DDQN) would draw per-net masks
        if flat:
            flatten_grads(src)
        D.FUSED_HEAD = fused
        try:
            loss = D.q_loss(src, tgt, state, a, r, nxt, 0.7, variant == "ddqn")
            src.zero_grad(set_to_none=True)
            loss.backward()
        finally:
            D.FUSED_HEAD = True
        torch.cuda.synchronize()
        out[fused] = (float(loss), [p.grad.detach().clone() for p in src.parameters()])
    (lf, gf), (lu, gu) = out[True], out[False]
    assert lf == pytest.approx(lu, rel=2e-5)
    names = [n for n, _ in src0.named_parameters()]
    for n, x, y in zip(names, gf, gu):
        torch.testing.assert_close(x, y, rtol=2e-4, atol=1e-6, msg=n)


@pytest.mark.parametrize("flat", ["grads", "flat-adjacent", "flat-apart"])
@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
@pytest.mark.parametrize("b", [5, 17])
@pytest.mark.parametrize("hidden", [8, 520])
def test_fused_head_through_autograd_matches_float64_net(hidden, b, variant, flat):
    """q_loss through _HeadLossFn at head widths other than 512 (H = 4: most lanes hold no column;
    H = 260: one full trip of the 256-column loop and a 4-column tail) and batch sizes that fill
    neither the forward's 4-row nor the backward's 16-row workgroups, against a float64 copy of the
    nets on the expanded windows: the loss (rel 1e-5) and the gradients of fc.0, fc.2 and fc.4
    (rtol 1e-4, atol 1e-5 x scale: the f32-versus-f64 tolerances of test_learner_overlap.py).
    conv.0's gradients are discontinuous near a pool tie and belong to test_stem.py. With flat
    gradients, both branches of _HeadLossFn.backward: fc3's bias segment right behind its weight's
    (one column sum into both), and apart from it."""
    import mazerl.agents.dqn as D
    from mazerl.agents.flat import flatten_grads, grad_segment
    from mazerl.agents.nets import QNet
    from test_stem import _close, _window
    torch.manual_seed(5)
    src = QNet(3, 6, 4, 32, hidden, variant).cuda().eval()
    tgt = QNet(3, 6, 4, 32, hidden, variant).cuda().eval()
    ref, reft = copy.deepcopy(src).double(), copy.deepcopy(tgt).double()
    state, a, r, nxt = _batch(b, 13)
    fc3 = src.fc[4]
    if flat != "grads":
        flatten_grads(src)
        if flat == "flat-apart":
            fc3.bias._grad_seg = (torch.zeros(4, device="cuda"), 0)
        gw, gb = grad_segment(fc3.weight), grad_segment(fc3.bias)
        assert (gb.data_ptr() == gw.data_ptr() + 16 * (hidden // 2)) == (flat == "flat-adjacent")
    dbl = variant == "ddqn"
    assert D._head_ok(src, tgt, state, a, r)  # the fused head route
    loss = D.q_loss(src, tgt, state, a, r, nxt, 0.7, dbl)
    assert isinstance(loss.grad_fn, D._HeadLossFn._backward_cls)
    loss.backward()
    wide = lambda s: (s[0].double(), _window(s[1].cpu()).cuda().double())  # noqa: E731
    loss_ref = D.q_loss(ref, reft, wide(state), a, r.double(), wide(nxt), 0.7, dbl)
    loss_ref.backward()
    torch.cuda.synchronize()
    assert float(loss) == pytest.approx(float(loss_ref), rel=1e-5)
    for (name, p), pr in zip(src.named_parameters(), ref.parameters()):
        if name.startswith("fc."):
            assert _close(p.grad, pr.grad.float(), 1e-4, 1e-5), name
    if flat != "grads":
        assert fc3.weight.grad.data_ptr() == gw.data_ptr()
        assert fc3.bias.grad.data_ptr() == gb.data_ptr()


def test_fused_head_loss_is_deterministic():
    """Two launches on the same rows give the same loss and gradients bit for bit (the loss and
    the fc3 gradient sums run in a fixed order: per block, then over blocks)."""
    import mazerl.agents.dqn as D
    from mazerl.agents.nets import QNet
    torch.manual_seed(4)
    src = QNet(3, 6, 4, 32, 1024, "ddqn").cuda().eval()
    tgt = QNet(3, 6, 4, 32, 1024, "ddqn").cuda().eval()
    state, a, r, nxt = _batch(1024, 12)
    res = []
    for _ in range(2):
        loss = D.q_loss(src, tgt, state, a, r, nxt, 0.7, True)
        src.zero_grad(set_to_none=True)
        loss.backward()
        res.append((loss.detach().clone(), [p.grad.clone() for p in src.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    for x, y in zip(res[0][1], res[1][1]):
        assert torch.equal(x, y)
