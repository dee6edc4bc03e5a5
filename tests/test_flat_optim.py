"""FlatAdamW (agents/flat.py, csrc/mz_optim.hip: the reference's per-parameter
grad.clamp_(-1, 1) + torch.optim.AdamW step, dqn_agent.py:152-157, as one launch over a flat
buffer) against torch.optim.AdamW (single-tensor path) + clamp_ on the same QNet, with a cosine
schedule stepping the device-side lr. Same formula and operation order; torch's kernels may
contract multiply-adds, so params agree within rtol 1e-5 / atol 1e-6 after 25 steps and the
moments within rtol 1e-4 (relative to each tensor's scale)."""
import copy

import pytest
import torch
from torch.optim import lr_scheduler

pytestmark = pytest.mark.gpu


def test_flat_adamw_matches_torch_adamw_with_clamp():
    from mazerl.agents.flat import FlatAdamW
    from mazerl.agents.nets import QNet
    torch.manual_seed(0)
    A = QNet(variant="ddqn").cuda()
    B = copy.deepcopy(A)
    oa = FlatAdamW(A, lr=1e-3)
    ob = torch.optim.AdamW(B.parameters(), lr=1e-3, foreach=False)
    sa = lr_scheduler.CosineAnnealingLR(oa, T_max=7, eta_min=1e-5)
    sb = lr_scheduler.CosineAnnealingLR(ob, T_max=7, eta_min=1e-5)
    assert all(p.data_ptr() >= A._flat_params.data_ptr() for p in A.parameters())
    g = torch.Generator(device="cuda").manual_seed(1)
    for k in range(25):
        for pa, pb in zip(A.parameters(), B.parameters()):
            gr = torch.randn(pa.shape, device="cuda", generator=g) * (0.5 if k % 3 else 3.0)
            pa.grad = gr.clone()
            pb.grad = gr.clone()
        oa.step()
        for p in B.parameters():
            p.grad.data.clamp_(-1, 1)
        ob.step()
        if k % 4 == 3:
            sa.step()
            sb.step()
    torch.cuda.synchronize()
    assert float(oa.param_groups[0]["lr"]) == pytest.approx(ob.param_groups[0]["lr"], rel=1e-6)
    assert float(oa.step_t) == 25.0
    for (n, pa), pb in zip(A.named_parameters(), B.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-5, atol=1e-6), n
        assert torch.equal(pa.grad, pb.grad), n  # clamped in place, like clamp_
    off = 0
    for pb, n in zip(B.parameters(), oa.sizes):
        st = ob.state[pb]
        m = oa.exp_avg[off:off + pb.numel()].view_as(pb)
        v = oa.exp_avg_sq[off:off + pb.numel()].view_as(pb)
        assert torch.allclose(m, st["exp_avg"], rtol=1e-4, atol=1e-4 * float(st["exp_avg"].abs().max()))
        assert torch.allclose(v, st["exp_avg_sq"], rtol=1e-4, atol=1e-4 * float(st["exp_avg_sq"].abs().max()))
        off += n


def test_flat_params_survive_state_dict_and_copy():
    from mazerl.agents.flat import copy_flat, flatten_params
    from mazerl.agents.nets import QNet
    torch.manual_seed(0)
    A, B = QNet(variant="dqn").cuda(), QNet(variant="dqn").cuda()
    ref = {k: v.clone() for k, v in A.state_dict().items()}
    fa, fb = flatten_params(A), flatten_params(B)
    assert flatten_params(A) is fa  # idempotent
    for k, v in A.state_dict().items():
        assert torch.equal(v, ref[k]), k
    copy_flat(B, A)
    for (k, v), w in zip(B.state_dict().items(), A.state_dict().values()):
        assert torch.equal(v, w), k
    C = copy.deepcopy(A)  # deepcopy clones the parameters apart from the buffer
    fc = flatten_params(C)
    assert fc.data_ptr() != fa.data_ptr()
    assert all(torch.equal(x, y) for x, y in zip(C.parameters(), A.parameters()))


def test_flat_adamw_step_counts_are_independent_and_graph_safe():
    """The step count is a plain f32 [1] (include/mazerl.h mz_adamw_flat), advanced by a
    one-thread launch behind the update on the caller's stream. Two optimizers interleaved on
    two streams, eagerly and as captured-graph replays, each advance their own count by exactly
    one per step."""
    from mazerl.agents.flat import FlatAdamW
    from mazerl.agents.nets import QNet
    torch.manual_seed(3)
    A, B = QNet(variant="dqn").cuda(), QNet(variant="ddqn").cuda()
    oa, ob = FlatAdamW(A, lr=1e-3), FlatAdamW(B, lr=1e-3)
    assert oa._step_buf.numel() == 1 and ob._step_buf.numel() == 1
    for p in list(A.parameters()) + list(B.parameters()):
        p.grad = torch.randn_like(p) * 1e-3
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for k in range(7):
        with torch.cuda.stream(s1):
            oa.step()
        with torch.cuda.stream(s2):
            ob.step()
            ob.step()
    torch.cuda.synchronize()
    assert float(oa.step_t) == 7.0 and float(ob.step_t) == 14.0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            oa.step()
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(5):
        g.replay()
    ob.step()
    torch.cuda.synchronize()
    assert float(oa.step_t) == 12.0 and float(ob.step_t) == 15.0


def test_learner_gradients_land_in_the_flat_buffer():
    """VectorDQNLearner's backward writes every source-net gradient into its segment of ONE flat
    buffer (agents/flat.py flatten_grads: GraphSafeLinear's GEMM / column-sum outputs and the HIP
    stem's weight gradients, kept by autograd as .grad without a copy) — eager and captured — so
    FlatAdamW reads one contiguous gradient and a gradient all-reduce runs on it in place."""
    from mazerl import VectorMazeEnv
    from mazerl.agents.dqn import VectorDQNLearner
    from mazerl.agents.flat import grads_are_flat
    from test_learner_graph import _fill
    env = VectorMazeEnv(4, 21, enrich=True, device="cuda", seed=1)
    L = VectorDQNLearner(4, "cuda", variant="ddqn", batch_size=32, capacity=64, seed=3)
    _fill(L)
    for _ in range(5):  # 3 eager warm-up updates, the capture, a replay
        L.update(env.expand_window)
        torch.cuda.synchronize()
        assert grads_are_flat(L.source)
        g = L.source._flat_grads
        assert float(g.abs().sum()) > 0
        off = 0
        for p, n in zip(L.source.parameters(), L.source._flat_sizes):
            assert p.grad.data_ptr() == g.data_ptr() + 4 * off
            off += n
    assert L._graph is not None
    env.close()


# ---- mz_adamw_flat through the C ABI against the float64 model (tests/learner_model.py) ---------
# Bounds from rounding counts (u = 2^-24; the library is built without multiply-add contraction,
# so every f32 operation of k_adamw rounds once; the seven scalars are the same f32 values in the
# kernel and in the model):
#   g' = clamp(g * s)        one product: |dg| <= u |g s| (the clamp selects, it does not round);
#                            exact when s is a power of two
#   m' = m + w1 (g' - m)     dg (<= u |g'|), the difference, the product, the sum — each on a value
#                            <= |m| + |g'|: |dm| <= 4 u (|m| + |g'|)
#   v' = v b2 + w2 (g' g')   g' twice (2 u), g' g', w2 *, v b2, the sum, all terms >= 0: <= 5 u v'
#   p' = p decay - U,  U = step_size * (m' / denom),  denom = sqrt(v') / bc2_sqrt + eps:
#        p decay and the final difference: 3 u |p| (|U| << |p| or counted in the next term);
#        denom from v' (5 u / 2), sqrt, the division, the sum; then m' / denom and step_size *:
#        8 u |U|; and m's own error carried through: step_size * tol_m / denom.
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 1e-2


def _ulib():
    from mazerl import _native as N
    return N, N.load()


def _launch(L, p, m, v, grads, lens, lr, step, clamp, gscale, write_grad, off=0):
    import ctypes as C
    arr = (C.c_void_p * len(grads))(*[g if isinstance(g, int) else g.data_ptr() for g in grads])
    ln = (C.c_int64 * len(lens))(*lens)
    rc = L.mz_adamw_flat(p.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off, arr,
                         ln, len(lens), lr.data_ptr(), step.data_ptr(), B1, B2, EPS, WD, clamp,
                         gscale, write_grad, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _state(n, seed, gmul=1.0):
    import numpy as np
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    m = (0.3 * rng.standard_normal(n)).astype(np.float32)
    v = (0.1 * rng.standard_normal(n) ** 2).astype(np.float32)
    g = (gmul * rng.standard_normal(n)).astype(np.float32)
    return p, m, v, g


def _bits(t):
    return t.view(torch.int32)


def _check_step(p0, m0, v0, g0, got, lr, step, clamp, gscale):
    """got = (p, m, v, g) after one launch from the f32 state (p0, m0, v0, g0)."""
    import numpy as np
    import learner_model as M
    u = M.U32
    pm, mm, vm, gm = M.adamw_step(p0, g0, m0, v0, lr, step, B1, B2, EPS, WD, clamp, gscale)
    s = M.adamw_scalars(lr, step, B1, B2, EPS, WD)
    p, m, v, g = (x.cpu().numpy().astype(np.float64) for x in got)
    s32 = float(np.float32(gscale))
    tol_g = u * np.abs(g0.astype(np.float64) * s32)
    if float(np.log2(s32)).is_integer():
        tol_g = np.zeros_like(tol_g)  # a power of two scales exactly
    tol_m = 4 * u * (np.abs(m0) + np.abs(gm))
    denom = np.sqrt(vm) / s["bc2_sqrt"] + s["eps"]
    upd = s["step_size"] * mm / denom
    tol_p = 3 * u * np.abs(p0) + 8 * u * np.abs(upd) + s["step_size"] * tol_m / denom
    for name, x, ref, tol in (("g", g, gm, tol_g), ("m", m, mm, tol_m), ("v", v, vm, 5 * u * vm),
                              ("p", p, pm, tol_p)):
        err = np.abs(x - ref)
        worst = float(np.max(err / np.maximum(tol, 1e-300))) if tol.any() else float(err.max())
        print(f"  step {step} clamp {clamp} gscale {gscale:.4f} {name}: err/tol {worst:.3f}")
        assert np.all(err <= tol), (name, step, clamp, gscale, worst)


@pytest.mark.parametrize("gscale", [1.0, 0.125, 1.0 / 3.0])
@pytest.mark.parametrize("clamp", [1.0, 0.25])
def test_adamw_flat_one_step_matches_float64_model(clamp, gscale):
    """One launch from a random state (v >= 0; gradients on both sides of the clamp, before and
    after the scale) at step counts 0, 1, 999 and 10,000, then a second one after the device-side
    lr changed: every element of p, m, v and the written-back gradient within its bound, and the
    step count advanced by one per launch."""
    N, L = _ulib()
    n = 2052
    for step in (0, 1, 999, 10000):
        p0, m0, v0, g0 = _state(n, 17 + step, gmul=2.0)
        p, m, v, g = (torch.from_numpy(x).cuda() for x in (p0, m0, v0, g0))
        lr = torch.tensor(1e-3, dtype=torch.float32, device="cuda")
        st = torch.tensor([float(step)], dtype=torch.float32, device="cuda")
        N.check(_launch(L, p, m, v, [g], [n], lr, st, clamp, gscale, 1))
        assert float(st) == step + 1
        _check_step(p0, m0, v0, g0, (p, m, v, g), 1e-3, step, clamp, gscale)
        p1, m1, v1 = (x.cpu().numpy() for x in (p, m, v))
        g1 = _state(n, 99 + step, gmul=0.3)[3]
        g.copy_(torch.from_numpy(g1))
        lr.fill_(3.7e-4)  # the schedule writes the device-side lr between launches
        N.check(_launch(L, p, m, v, [g], [n], lr, st, clamp, gscale, 1))
        assert float(st) == step + 2
        _check_step(p1, m1, v1, g1, (p, m, v, g), 3.7e-4, step + 1, clamp, gscale)


@pytest.mark.parametrize("clamp", [1.0, 0.25])
def test_adamw_flat_clamp_and_special_values(clamp):
    """Gradients exactly at +-clamp, one ulp outside and inside, +-inf (clamped) and NaN (it
    propagates to p, m, v and the written gradient, as clamp_ followed by torch's step does); the
    scale applies before the clamp (average over ranks, then clamp)."""
    import numpy as np
    import learner_model as M
    N, L = _ulib()
    c = np.float32(clamp)
    up, dn = np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(0))
    g0 = np.array([c, -c, up, -up, dn, -dn, np.inf, -np.inf, np.nan, 0.0, -0.0, 8 * c],
                  dtype=np.float32)
    n = g0.size
    for gscale, want in ((1.0, [c, -c, c, -c, dn, -dn, c, -c, np.nan, 0.0, -0.0, c]),
                         (0.125, list(g0[:6] * np.float32(0.125)) + [c, -c, np.nan, 0.0, -0.0, c])):
        p0, m0, v0, _ = _state(n, 5)
        p, m, v, g = (torch.from_numpy(x).cuda() for x in (p0, m0, v0, g0))
        lr = torch.tensor(1e-3, dtype=torch.float32, device="cuda")
        st = torch.tensor([3.0], dtype=torch.float32, device="cuda")
        N.check(_launch(L, p, m, v, [g], [n], lr, st, clamp, gscale, 1))
        got = g.cpu().numpy()
        want = np.array(want, dtype=np.float32)
        assert np.array_equal(got, want, equal_nan=True), (gscale, got, want)
        pm, mm, vm, gm = M.adamw_step(p0, g0, m0, v0, 1e-3, 3, B1, B2, EPS, WD, clamp, gscale)
        assert np.array_equal(gm.astype(np.float32), want, equal_nan=True)
        for x, ref in ((p, pm), (m, mm), (v, vm)):
            x = x.cpu().numpy()
            assert np.array_equal(np.isnan(x), np.isnan(ref)) and np.isnan(x).sum() == 1
            assert np.isnan(x[8]) and np.all(np.isfinite(x[np.arange(n) != 8]))
        ok = np.arange(n) != 8
        keep = torch.from_numpy(np.flatnonzero(ok)).cuda()
        _check_step(p0[ok], m0[ok], v0[ok], g0[ok], tuple(x[keep] for x in (p, m, v, g)), 1e-3, 3,
                    clamp, gscale)


def test_adamw_flat_write_grad_off_leaves_the_gradient_alone():
    """write_grad = 0 (the learner's hot path): the gradient buffer is bit-identical afterwards
    and p, m, v are those of the write_grad = 1 launch, which leaves clamp(g * scale) behind."""
    import numpy as np
    N, L = _ulib()
    n = 1028
    p0, m0, v0, g0 = _state(n, 23, gmul=2.0)
    out = []
    for wg in (0, 1):
        p, m, v, g = (torch.from_numpy(x).cuda() for x in (p0, m0, v0, g0))
        lr = torch.tensor(1e-3, dtype=torch.float32, device="cuda")
        st = torch.tensor([7.0], dtype=torch.float32, device="cuda")
        N.check(_launch(L, p, m, v, [g], [n], lr, st, 1.0, 0.5, wg))
        out.append((p, m, v, g))
    assert np.array_equal(out[0][3].cpu().numpy().view(np.int32), g0.view(np.int32))
    assert np.array_equal(out[1][3].cpu().numpy(), np.clip(g0 * np.float32(0.5), -1, 1))
    for x, y in zip(out[0][:3], out[1][:3]):
        assert torch.equal(_bits(x), _bits(y))


SEG_LENS = [4, 4, 8, 2048, 4, 524288, 12, 4, 8, 1024, 4, 4, 16, 4, 260, 8]


@pytest.mark.parametrize("layout", ["separate", "one_allocation"])
def test_adamw_flat_sixteen_segments_equal_one(layout):
    """16 gradient segments (the maximum) whose addresses are not in segment order — separate
    allocations, or shuffled places inside one allocation — 527,700 elements: more than the grid's
    256 x 512 x 4, so the grid-stride loop wraps with segment boundaries inside the second trip.
    Bit-identical to one segment holding the concatenated gradient. 17 segments, a length that is
    no multiple of 4 and a misaligned gradient pointer are errors that leave the state alone."""
    import numpy as np
    N, L = _ulib()
    n = sum(SEG_LENS)
    assert len(SEG_LENS) == 16 and n > 256 * 512 * 4
    p0, m0, v0, g0 = _state(n, 31, gmul=1.5)
    order = np.random.default_rng(2).permutation(16)
    segs = [None] * 16
    if layout == "separate":
        for k in order:  # allocated out of order: the addresses do not follow the segment order
            segs[k] = torch.empty(SEG_LENS[k], dtype=torch.float32, device="cuda")
    else:
        pool = torch.from_numpy(_state(n + 16, 32)[3]).cuda()
        at = 0
        for k in order:
            segs[k] = pool[at:at + SEG_LENS[k]]
            at += SEG_LENS[k]
    addr = [s.data_ptr() for s in segs]
    assert addr != sorted(addr) and len(set(addr)) == 16
    off = np.concatenate(([0], np.cumsum(SEG_LENS)))
    for k in range(16):
        segs[k].copy_(torch.from_numpy(g0[off[k]:off[k + 1]]))
    res = []
    for grads, lens in ((segs, SEG_LENS), ([torch.from_numpy(g0).cuda()], [n])):
        p, m, v = (torch.from_numpy(x).cuda() for x in (p0, m0, v0))
        lr = torch.tensor(1e-3, dtype=torch.float32, device="cuda")
        st = torch.tensor([4.0], dtype=torch.float32, device="cuda")
        N.check(_launch(L, p, m, v, grads, lens, lr, st, 1.0, 1.0 / 3.0, 1))
        res.append((p, m, v, torch.cat(grads)))
    for x, y in zip(*res):
        assert torch.equal(_bits(x), _bits(y))
    _check_step(p0, m0, v0, g0, res[0], 1e-3, 4, 1.0, 1.0 / 3.0)
    # rejected arguments
    p, m, v, g = res[1]
    keep = [x.clone() for x in (p, m, v, g)]
    lr = torch.tensor(1e-3, dtype=torch.float32, device="cuda")
    st = torch.tensor([4.0], dtype=torch.float32, device="cuda")
    small = [g[4 * k:] for k in range(17)]
    assert _launch(L, p, m, v, small, [4] * 17, lr, st, 1.0, 1.0, 1) != 0
    assert _launch(L, p, m, v, [g], [6], lr, st, 1.0, 1.0, 1) != 0
    assert _launch(L, p, m, v, [g.data_ptr() + 4], [8], lr, st, 1.0, 1.0, 1) != 0
    assert float(st) == 4.0
    for x, y in zip((p, m, v, g), keep):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("k", [2, 8])
def test_adamw_flat_shards_equal_one_launch(k):
    """The data-parallel step updates an (offset, length) shard of the flat buffer per rank: k
    launches over the k shards (the step count put back before each, as every rank holds its own)
    equal one launch over the whole buffer bit for bit — through the ABI on offset pointers, then
    through FlatAdamW with opt.shard set (agents/flat.py's pointer arithmetic), with the
    all-reduce average as grad_scale and write_grad off as the learner runs it."""
    import copy

    import numpy as np
    from mazerl.agents.flat import FlatAdamW, flatten_grads, grad_segment
    N, L = _ulib()
    n = 8 * 260
    p0, m0, v0, g0 = _state(n, 41, gmul=1.5)
    lr = torch.tensor(1e-3, dtype=torch.float32, device="cuda")
    whole = [torch.from_numpy(x).cuda() for x in (p0, m0, v0, g0)]
    st = torch.tensor([5.0], dtype=torch.float32, device="cuda")
    N.check(_launch(L, *whole[:3], [whole[3]], [n], lr, st, 1.0, 1.0 / k, 0))
    parts = [torch.from_numpy(x).cuda() for x in (p0, m0, v0, g0)]
    ln = n // k
    for r in range(k):
        st.fill_(5.0)
        N.check(_launch(L, *parts[:3], [parts[3].data_ptr() + 4 * r * ln], [ln], lr, st, 1.0,
                        1.0 / k, 0, off=r * ln))
    assert float(st) == 6.0
    for x, y in zip(whole, parts):
        assert torch.equal(_bits(x), _bits(y))
    _check_step(p0, m0, v0, g0, parts[:3] + [torch.from_numpy(np.clip(
        g0 * np.float32(1.0 / k), -1, 1)).cuda()], 1e-3, 5, 1.0, 1.0 / k)
    assert np.array_equal(parts[3].cpu().numpy().view(np.int32), g0.view(np.int32))

    torch.manual_seed(6)
    A = torch.nn.Sequential(torch.nn.Linear(10, 12), torch.nn.Linear(12, 6)).cuda()
    B = copy.deepcopy(A)
    opts = []
    for net in (A, B):
        opt = FlatAdamW(net, lr=1e-3, write_grad=False)
        gbuf = flatten_grads(net)
        gbuf.copy_(torch.from_numpy(_state(gbuf.numel(), 43, gmul=1.5)[3]))
        for q in net.parameters():
            q.grad = grad_segment(q)
        opt.exp_avg.copy_(torch.from_numpy(_state(gbuf.numel(), 44)[1]))
        opt.exp_avg_sq.copy_(torch.from_numpy(_state(gbuf.numel(), 44)[2]))
        opt._step_buf.fill_(5.0)
        opt.grad_scale = 1.0 / k
        opts.append(opt)
    oa, ob = opts
    assert oa.flat.numel() % k == 0 and (oa.flat.numel() // k) % 4 == 0
    g_before, flat_before = B._flat_grads.clone(), oa.flat.clone()
    oa.step()
    ln = ob.flat.numel() // k
    for r in range(k):
        ob._step_buf.fill_(5.0)
        ob.shard = (r * ln, ln)
        ob.step()
    torch.cuda.synchronize()
    assert float(oa.step_t) == 6.0 and float(ob.step_t) == 6.0
    assert not torch.equal(oa.flat, flat_before)  # the step moved the parameters
    for x, y in ((oa.flat, ob.flat), (oa.exp_avg, ob.exp_avg), (oa.exp_avg_sq, ob.exp_avg_sq)):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(_bits(B._flat_grads), _bits(g_before))
