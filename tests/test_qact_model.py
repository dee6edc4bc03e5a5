"""The CPU model of the bf16x3 acting forward (tests/qact_model.py) pinned on the CPU: how far the
algorithm is from the f64 network (E_alg), what an f32 accumulation order costs (E_acc) and
hence the tolerance T_MODEL the GPU tests use (tests/test_qact_exact.py), that four plausible
kernel defects each exceed it, and that the argmax is decided on these inputs. Then the C entry
points' argument checks, which run before any GPU call, and QAct on an empty batch."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import qact_model as M

ROWS = 512
DROP = dict(seed=77, counter=0, p=0.2)


@pytest.fixture(scope="module")
def runs():
    """Per variant the four CPU runs on synthetic_states(512, 5), computed once, left unchanged."""
    bits, obs6 = M.synthetic_states(ROWS, 5)
    win, o6 = M.window(bits), torch.from_numpy(obs6)
    out = {"win": win, "obs6": o6}
    for v in ("dqn", "ddqn"):
        net = M.make_net(v)
        net64 = copy.deepcopy(net).double()
        with torch.no_grad():
            out[v] = dict(net=net, net64=net64((o6.double(), win.double())), net32=net((o6, win)),
                          m64=M.model_q(net, win, o6),
                          m32=M.model_q(net, win, o6, dtype=torch.float32))
    return out


def _max(q, ref):
    return float(M.row_dev(q, ref).max())


@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
def test_algorithm_error_between_f32_and_the_suite_bound(runs, variant):
    """E_alg: bf16x3 is within the suite's 2e-4 of the f64 network (tests/test_qact.py) and is
    not f32: its error exceeds the f32 network's own."""
    r = runs[variant]
    e_alg, e_f32 = _max(r["m64"], r["net64"]), _max(r["net32"], r["net64"])
    print(variant, "E_alg", e_alg, "f32 network", e_f32)
    assert e_alg <= 2e-4
    assert e_alg > e_f32


def test_t_model_rests_on_the_accumulation_error(runs):
    """T_MODEL = 4 x the largest E_acc (both variants, DDQN with dropout), rounded up to one
    significant digit; the values recorded beside it are the ones measured here."""
    net = runs["ddqn"]["net"]
    keep = M.keep_masks(DROP["seed"], DROP["counter"], np.arange(ROWS), DROP["p"])
    d64 = M.model_q(net, runs["win"], runs["obs6"], keep=keep, p=DROP["p"])
    d32 = M.model_q(net, runs["win"], runs["obs6"], keep=keep, p=DROP["p"], dtype=torch.float32)
    e_acc = {"dqn": _max(runs["dqn"]["m32"], runs["dqn"]["m64"]),
             "ddqn": _max(runs["ddqn"]["m32"], runs["ddqn"]["m64"]),
             "ddqn_dropout": _max(d32, d64)}
    print("E_acc", e_acc)
    worst = max(e_acc.values())
    assert 4 * worst <= M.T_MODEL
    # one significant digit, rounded up: the next smaller such number is below 4 x E_acc
    mag = 10.0 ** math.floor(math.log10(M.T_MODEL))
    assert abs(M.T_MODEL / mag - round(M.T_MODEL / mag)) < 1e-9
    assert M.T_MODEL - mag < 4 * worst
    for k, v in e_acc.items():  # the recorded figures are these
        assert abs(v - M.E_ACC[k]) <= 0.05 * M.E_ACC[k], (k, v)
    # dropout did something, and the mask's drop rate is the threshold's
    assert _max(d64, runs["ddqn"]["m64"]) > 1e-2
    assert abs(M.drop_fraction(keep) - M.drop_thresh(DROP["p"]) / 65536) < 0.002


@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_each_defect_exceeds_twice_the_tolerance(runs, variant, mutation):
    """Teeth: a kernel with this defect is at least 2 T_MODEL from the model on some row, so no
    f32 accumulation order (<= T_MODEL by the GPU test's bound) brings it back inside. Asserted
    on the first 200 rows, the ones test_qact_exact.py's comparison with the model runs."""
    r = runs[variant]
    dev = M.row_dev(M.model_q(r["net"], runs["win"], runs["obs6"], mutate=mutation), r["m64"])
    print(variant, mutation, float(dev.max()), float(dev[:200].max()))
    assert float(dev[:200].max()) >= 2 * M.T_MODEL


@pytest.mark.parametrize("variant", ["dqn", "ddqn"])
def test_argmax_is_decided_on_these_inputs(runs, variant):
    """At most 1 % of the rows have a top-2 gap within 2 T_MODEL max|Q| (where a result within
    T_MODEL could pick the other action); the f32 model picks the model's action on the rest."""
    r = runs[variant]
    clear = M.clear_rows(r["m64"])
    assert int((~clear).sum()) <= ROWS // 100
    assert torch.equal(r["m32"].argmax(1)[clear], r["m64"].argmax(1)[clear])


def test_synthetic_states_edges(runs):
    bits, obs6 = M.synthetic_states(ROWS, 5)
    b2, o2 = M.synthetic_states(ROWS, 5)
    assert np.array_equal(bits, b2) and np.array_equal(obs6, o2)  # the same inputs everywhere
    assert bits.dtype == np.int32 and bits.shape == (ROWS, 22)
    assert obs6.dtype == np.float32 and obs6.shape == (ROWS, 6)
    win = runs["win"]
    assert float(win[0].sum()) == 0 and float(win[1].sum()) == 675
    u = bits.view(np.uint32)
    assert (u[:, 21] >> 3).any(axis=0) and not (np.delete(u, 2, 0)[:, 21] >> 3).any()  # pads: row 2 only
    assert u[2, 21] >> 3 == (1 << 29) - 1 and np.array_equal(u[2, :21], u[3, :21])
    assert torch.equal(win[2], win[3]) and np.array_equal(obs6[2], obs6[3])
    assert abs(float(win[8:].mean()) - 0.3) < 0.01
    assert obs6.min() >= -1.0 - 2.0 ** -9 and obs6.max() <= 1.0 + 2.0 ** -9
    hi, lo = M.split(torch.from_numpy(obs6[4:8]))
    assert float(lo.abs().max()) == 2.0 ** -9 and float(hi[1, 0]) == 1.0
    for v in ("dqn", "ddqn"):  # the pad bits do not reach the model either
        assert torch.equal(runs[v]["m64"][2], runs[v]["m64"][3])


def test_split_is_bf16_round_to_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, -3e-5, 0.0, 0.1])
    hi, lo = M.split(x)
    assert hi[0] == 1.0 and hi[1] == 1.0 + 2.0 ** -6  # ties to even
    assert lo[0] == 2.0 ** -8 and lo[2] == 2.0 ** -9
    assert torch.equal(hi.view(torch.int32) & 0xFFFF, torch.zeros(6, dtype=torch.int32))
    assert torch.equal(lo.view(torch.int32) & 0xFFFF, torch.zeros(6, dtype=torch.int32))
    assert float(((hi.double() + lo.double() - x.double()).abs() / x.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16


# ---- the C entry points refuse bad arguments before any GPU call ---------------------------------
P = 0x10000  # a 16-byte aligned non-null address; never dereferenced: every call is refused or has n = 0
QACT_ARGS = ["bits", "obs6", "rows", "count", "n", "conv_w", "conv_b", "w1h", "w1l", "b1", "w2h",
             "w2l", "b2", "w3", "b3", "relu", "drop_p", "seed", "counter", "h1", "greedy", "q_out",
             "stream"]
QACT_REQUIRED = ["bits", "obs6", "conv_w", "conv_b", "w1h", "w1l", "b1", "w2h", "w2l", "b2", "w3",
                 "b3", "h1"]


def _qact(lib, **over):
    """mz_qact with well-formed arguments (n = 0: even an accepted call launches nothing) but
    for `over`."""
    a = {k: P for k in QACT_ARGS}
    a.update(n=0, relu=0, drop_p=0.0, seed=1, counter=0, stream=None)
    a.update(over)
    return lib.mz_qact(*[a[k] for k in QACT_ARGS])


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def _refused(lib, rc):
    assert rc != 0
    assert lib.mz_last_error()  # a text for the caller
    return lib.mz_last_error().decode()


def test_qact_refuses_bad_arguments(lib):
    assert _qact(lib) == 0  # the well-formed call (n = 0) is accepted: each refusal has one cause
    for k in QACT_REQUIRED:
        _refused(lib, _qact(lib, **{k: None}))
    _refused(lib, _qact(lib, n=-1))
    _refused(lib, _qact(lib, greedy=None, q_out=None))
    assert _qact(lib, greedy=None) == 0 and _qact(lib, q_out=None) == 0  # one output is enough
    assert "row list" in _refused(lib, _qact(lib, rows=None))  # a count without a row list
    assert _qact(lib, rows=None, count=None) == 0
    for p in (1.0, -0.1, float("nan")):
        assert "dropout" in _refused(lib, _qact(lib, drop_p=p))
    for k in ("q_out", "h1", "w1h", "w1l", "w2h", "w2l"):
        assert "aligned" in _refused(lib, _qact(lib, **{k: P + 8}))


def test_qact_prepare_refuses_bad_pointers(lib):
    for i in range(6):
        for bad in (None, P + 8, P + 4):
            a = [P] * 6 + [None]
            a[i] = bad
            _refused(lib, lib.mz_qact_prepare(*a))


def test_qact_workspace_size(lib):
    rt = lib._Z17mz_qact_row_tilesi  # the host function the launch sizes its grid with
    rt.restype, rt.argtypes = C.c_int, [C.c_int]
    assert lib.mz_qact_workspace_floats(0) == 0
    for n, tiles in ((1, 1), (64, 1), (65, 2)):
        assert rt(n) == tiles
        assert lib.mz_qact_workspace_floats(n) == n * 1024 + tiles * 50 * 64 * 32


def test_qact_empty_batch_makes_no_library_call():
    """An empty batch returns an empty result before anything is touched: an instance without a
    library, weights or device would fail on any further step."""
    from mazerl.agents.qact import QAct
    qa = object.__new__(QAct)
    bits, obs6 = torch.zeros(0, 22, dtype=torch.int32), torch.zeros(0, 6)
    q = qa(obs6, bits)
    assert q.shape == (0, 4) and q.dtype == torch.float32
    g = qa.greedy(obs6, bits)
    assert g.shape == (0,) and g.dtype == torch.int64
    rows, count = torch.zeros(0, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    greedy = torch.full((5,), -7, dtype=torch.int64)
    qa.rows_greedy(torch.zeros(5, 6), torch.zeros(5, 22, dtype=torch.int32), rows, count, greedy)
    assert bool((greedy == -7).all())
