"""The bf16x3 acting forward (agents/qact.py QAct; csrc/mz_qact.hip k_qconv, k_qfc1, k_qact2)
against its exact CPU model (tests/qact_model.py) and over its launch edges.

tests/test_qact.py compares QAct with the f32 network at 2e-4: that bounds the algorithm. Here
the reference is the algorithm itself — the same hi / lo operands, the same three products,
summed in float64 — so only the order of the kernels' f32 additions is left, and the tolerance is
T_MODEL (4 x the measured cost of an f32 order, tests/test_qact_model.py), under which a dropped
lo operand, chunk, row block or product does not fit. Every launch geometry (1..5 chunk groups
per row tile, ragged tiles, n < 64), the device-side row count, the argmax contract and the
dropout key / row-list / p paths are run as well."""
import copy

import numpy as np
import pytest
import torch

import qact_model as M
from qact_model import T_MODEL

pytestmark = pytest.mark.gpu

STATES = 256  # the first rows of synthetic_states(512, 5): the rows tests/test_qact_model.py measures


class _Ctx:
    def __init__(self):
        bits, obs6 = M.synthetic_states(512, 5)
        self.bits_np, self.obs6_np = bits[:STATES], obs6[:STATES]
        self.win = M.window(self.bits_np)
        self.obs6_cpu = torch.from_numpy(self.obs6_np)
        self.bits = torch.from_numpy(self.bits_np).cuda()
        self.obs6 = self.obs6_cpu.cuda()
        self._net, self._model = {}, {}

    def net(self, variant):
        """(the CPU network the model reads, a fresh copy of it on the GPU in eval mode)"""
        if variant not in self._net:
            self._net[variant] = M.make_net(variant)
        return self._net[variant], copy.deepcopy(self._net[variant]).cuda().eval()

    def model(self, variant):
        """The float64 model's Q of all STATES rows, eval mode (computed once)."""
        if variant not in self._model:
            self._model[variant] = M.model_q(self.net(variant)[0], self.win, self.obs6_cpu)
        return self._model[variant]


@pytest.fixture(scope="module")
def ctx():
    return _Ctx()


def _within(q, model):
    dev = M.row_dev(q, model)
    print("kernel vs model: max", float(dev.max()), "of T_MODEL", T_MODEL)
    assert float(dev.max()) <= T_MODEL, float(dev.max())


@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
def test_kernel_matches_the_model(ctx, variant):
    """200 rows (three full tiles and 8 rows), eval mode: Q within T_MODEL of the model per row,
    the model's argmax on every clear row, greedy = argmax of the Q values, and the pad bits of
    the last window word ignored (row 2 = row 3 bit for bit)."""
    from mazerl.agents.qact import QAct
    n = 200
    _, net = ctx.net(variant)
    qa = QAct(net)
    q = qa(ctx.obs6[:n], ctx.bits[:n])
    g = qa.greedy(ctx.obs6[:n], ctx.bits[:n])
    torch.cuda.synchronize()
    model = ctx.model(variant)[:n]
    _within(q, model)
    clear = M.clear_rows(model)
    assert int((~clear).sum()) <= n // 100
    assert torch.equal(q.argmax(1).cpu()[clear], model.argmax(1)[clear])
    assert torch.equal(g, q.argmax(1))
    assert torch.equal(q[2], q[3])


def test_dropout_matches_the_model(ctx):
    """DDQN in train mode, 136 rows: the masks rebuilt from (seed, counter, list position, p) —
    a counter above 0, a seed above 2^32, another p, and a row list (masks keyed by position
    0..69 of the list, not by instance) — give the kernel's Q within T_MODEL."""
    from mazerl.agents.qact import QAct
    n = 136
    cpu_net, net = ctx.net("ddqn")
    net.train()
    qa = QAct(net, seed=77)
    obs6, bits = ctx.obs6[:n].contiguous(), ctx.bits[:n].contiguous()
    for seed, counter, p in ((77, 0, 0.2), (2 ** 40 + 5, 3, 0.2), (77, 1, 0.5)):
        qa.seed, qa.counter, qa.dropout.p = seed, counter, p
        q = qa(obs6, bits)
        torch.cuda.synchronize()
        assert qa.counter == counter + 1
        keep = M.keep_masks(seed, counter, np.arange(n), p)
        assert abs(M.drop_fraction(keep) - M.drop_thresh(p) / 65536) < 0.002
        model = M.model_q(cpu_net, ctx.win[:n], ctx.obs6_cpu[:n], keep=keep, p=p)
        print("seed", seed, "counter", counter, "p", p)
        _within(q, model)
        assert float(M.row_dev(model, ctx.model("ddqn")[:n]).min()) > 100 * T_MODEL  # masks matter
    # the row list: 100 distinct instances, 70 of them evaluated
    qa.seed, qa.counter, qa.dropout.p = 2 ** 40 + 5, 9, 0.2
    lst = np.random.default_rng(4).permutation(n)[:100].astype(np.int32)
    rows = torch.from_numpy(lst).cuda()
    count = torch.tensor([70], dtype=torch.int32, device="cuda")
    greedy = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    qout = torch.full((100, 4), float("nan"), device="cuda")
    qa.rows_greedy(obs6, bits, rows, count, greedy, qout)
    torch.cuda.synchronize()
    keep = M.keep_masks(2 ** 40 + 5, 9, np.arange(70), 0.2)
    assert abs(M.drop_fraction(keep) - M.drop_thresh(0.2) / 65536) < 0.002
    idx = torch.from_numpy(lst[:70].astype(np.int64))
    model = M.model_q(cpu_net, ctx.win[idx], ctx.obs6_cpu[idx], keep=keep, p=0.2)
    _within(qout[:70], model)
    assert bool(torch.isnan(qout[70:]).all())
    assert torch.equal(greedy[idx.cuda()], qout[:70].argmax(1))


def _groups(row_tiles):
    """mz_launch_qact's rule: chunk groups per row tile until the grid has ~512 workgroups."""
    g = 1
    while g < 5 and row_tiles * g < 512:
        g += 1
    return g


@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
def test_rows_do_not_depend_on_batch_or_position(ctx, variant):
    """Each output row is computed independently in a fixed K order: the Q of a state is the same
    bit for bit whatever the batch size, its tile, its place in the tile, and the number of
    chunk groups k_qconv's grid splits a tile into (all of 1..5 are run)."""
    from mazerl import _native
    from mazerl.agents.qact import QAct
    tiles = _native.load()._Z17mz_qact_row_tilesi
    _, net = ctx.net(variant)
    qa = QAct(net)
    obs6, bits = ctx.obs6[:192].contiguous(), ctx.bits[:192].contiguous()
    base = qa(obs6, bits)
    assert bool(torch.isfinite(base).all())
    seen = set()
    for n in (1, 63, 64, 65, 8192, 10981, 16384, 32769):
        idx = (7 * torch.arange(n, device="cuda")) % 192
        q = qa(obs6[idx].contiguous(), bits[idx].contiguous())
        assert q.shape == (n, 4)
        differ = int((q != base[idx]).any(1).sum())
        assert differ == 0, (n, differ, float((q - base[idx]).abs().max()))
        assert torch.equal(q, base[idx])
        assert tiles(n) == (n + 63) // 64
        seen.add(_groups(tiles(n)))
    assert [_groups(tiles(n)) for n in (8192, 10981, 16384, 32769)] == [4, 3, 2, 1]
    assert seen == {1, 2, 3, 4, 5}


def test_device_count_bounds_what_is_written(ctx):
    """A list of capacity 200 with the count read on the device: exactly min(count, 200) rows of
    q_out and their instances' greedy entries are written — none for 0, on and just past a tile
    boundary, and no further than the list when the count exceeds it."""
    from mazerl.agents.qact import QAct
    _, net = ctx.net("dqn")
    qa = QAct(net)
    lst = np.random.default_rng(8).permutation(STATES)[:200].astype(np.int32)
    rows = torch.from_numpy(lst).cuda()
    model = ctx.model("dqn")
    for c in (0, 1, 64, 128, 129, 500):
        m = min(c, 200)
        count = torch.tensor([c], dtype=torch.int32, device="cuda")
        greedy = torch.full((STATES,), -7, dtype=torch.int64, device="cuda")
        qout = torch.full((200, 4), float("nan"), device="cuda")
        qa.rows_greedy(ctx.obs6, ctx.bits, rows, count, greedy, qout)
        torch.cuda.synchronize()
        idx = torch.from_numpy(lst[:m].astype(np.int64))
        assert bool(torch.isfinite(qout[:m]).all()) and bool(torch.isnan(qout[m:]).all()), c
        if m:
            _within(qout[:m], model[idx])
        assert torch.equal(greedy[idx.cuda()], qout[:m].argmax(1)), c
        others = torch.ones(STATES, dtype=torch.bool, device="cuda")
        others[idx.cuda()] = False
        assert bool((greedy[others] == -7).all()), c
        assert int((greedy != -7).sum()) == m


ARGMAX_CASES = [([1.0, 1.0, 0.0, 0.0], 0), ([0.0, 2.0, 2.0, 1.0], 1), ([3.0, 3.0, 3.0, 3.0], 0),
                ([0.0, 1.0, float("nan"), 5.0], 2),
                ([0.0, float("nan"), float("nan"), float("inf")], 1),
                ([float("-inf")] * 4, 0)]


@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
def test_argmax_first_maximum_nan_as_maximum(ctx, variant):
    """torch.argmax's contract: the first maximum; a NaN counts as the maximum (the first NaN).
    With fc3's weight zero Q is b3 exactly, so ties and NaNs are placed at will."""
    from mazerl.agents.qact import QAct
    n = 65
    _, net = ctx.net(variant)
    with torch.no_grad():
        net.fc[4].weight.zero_()
    qa = QAct(net)
    obs6, bits = ctx.obs6[:n].contiguous(), ctx.bits[:n].contiguous()
    for b3, action in ARGMAX_CASES:
        b = torch.tensor(b3, dtype=torch.float32, device="cuda")
        assert int(torch.argmax(b)) == action  # the contract is torch's
        with torch.no_grad():
            net.fc[4].bias.copy_(b)
        q = qa(obs6, bits)
        g = qa.greedy(obs6, bits)
        torch.cuda.synchronize()
        assert torch.equal(q.view(torch.int32), b.view(torch.int32).expand(n, 4)), b3
        assert bool((g == action).all()), (b3, g.unique().tolist())


def test_weight_change_is_seen_without_invalidate(ctx):
    """An in-place update moves the parameter's _version: the next call rebuilds the hi / lo
    images by itself (invalidate() is for graph-replayed optimizers, which do not move it)."""
    from mazerl.agents.qact import QAct
    n = 65
    cpu_net, net = ctx.net("dqn")
    cpu_net = copy.deepcopy(cpu_net)
    qa = QAct(net)
    obs6, bits = ctx.obs6[:n].contiguous(), ctx.bits[:n].contiguous()
    q0 = qa(obs6, bits)
    _within(q0, ctx.model("dqn")[:n])
    with torch.no_grad():
        net.fc[0].weight.add_(0.01)
        cpu_net.fc[0].weight.add_(0.01)
    q1 = qa(obs6, bits)
    torch.cuda.synchronize()
    model1 = M.model_q(cpu_net, ctx.win[:n], ctx.obs6_cpu[:n])
    assert float(M.row_dev(model1, ctx.model("dqn")[:n]).min()) > 100 * T_MODEL  # a real change
    _within(q1, model1)


def test_empty_batch(ctx):
    from mazerl.agents.qact import QAct
    _, net = ctx.net("dqn")
    qa = QAct(net)
    q = qa(ctx.obs6[:0], ctx.bits[:0])
    g = qa.greedy(ctx.obs6[:0], ctx.bits[:0])
    assert q.shape == (0, 4) and q.is_cuda and g.shape == (0,) and g.dtype == torch.int64
