"""REINFORCE on the GPU (csrc/mz_reinforce.hip, trainers/reinforce_trainer.py) against the
reference's recorded run (tests/golden/reinforce.npz) and the torch expressions the kernels
replace. Tolerances are tests/test_ppo_gpu.py's for the same quantities.

Euclidean window mazes start at 15x15 (the reference's SimpleVariableMazeEnv.START_SHAPE; the env
refuses a smaller euclidean Enrich maze, which cannot hold the 15x15 window), so the euclidean
cases here use 15x15 and growth (15, 23)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_io as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    return G.load("reinforce.npz")


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _trainer(B, dims, toroidal=False, hidden=256, **kw):
    from mazerl.trainers.reinforce_trainer import VectorReinforceTrainer
    from mazerl.trainers.vector_trainer import make_env
    env = make_env(B, list(dims), toroidal=toroidal, device=DEV, done_list=False, reward64=True,
                   window=False, window_bits=True, max_dim=kw.pop("max_dim", None),
                   seed=kw.pop("env_seed", 0x5EED0000))
    kw.setdefault("bank", False)
    return env, VectorReinforceTrainer(env, DEV, hidden_dim=hidden, **kw)


# ---- mz_rf_act ------------------------------------------------------------------------------
def _rf_act(lib, logits, s6, bits, L, seed, counter, t, rs6, rw, ra, out, tau=2.0):
    from mazerl import _native as N
    N.check(lib.mz_rf_act(logits.data_ptr(), logits.stride(0), tau, s6.data_ptr(), bits.data_ptr(),
                          logits.shape[0], L, seed, counter, t.data_ptr(), rs6.data_ptr(),
                          rw.data_ptr(), ra.data_ptr(), out.data_ptr(), _stream()))


def test_act_records_at_the_step_index_only(lib):
    """B = 130 (two full waves of instances and a two-lane tail), L = 8, t[i] spread over 0..7:
    the recorded action is the stepped one, obs6 / bits at [i][t[i]] are the inputs' bits, no
    other slot is written, and the same (seed, counter) gives the same draws."""
    B, L = 130, 8
    g = torch.Generator(device=DEV).manual_seed(11)
    logits = torch.randn(B, 4, generator=g, device=DEV) * 2
    s6 = torch.rand(B, 6, generator=g, device=DEV)
    bits = torch.randint(-2**31, 2**31 - 1, (B, 22), generator=g, device=DEV, dtype=torch.int32)
    t = (torch.arange(B, device=DEV) % L).to(torch.int32)
    assert int(t.max()) == L - 1

    def run(counter):
        rs6 = torch.full((B, L, 6), -7.0, device=DEV)
        rw = torch.full((B, L, 22), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        ra = torch.full((B, L), -9, dtype=torch.int64, device=DEV)
        out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        _rf_act(lib, logits, s6, bits, L, 77, counter, t, rs6, rw, ra, out)
        torch.cuda.synchronize()
        return rs6, rw, ra, out

    rs6, rw, ra, out = run(3)
    ar = torch.arange(B, device=DEV)
    tl = t.long()
    assert bool(((out >= 0) & (out < 4)).all())
    assert torch.equal(ra[ar, tl], out.long())
    assert torch.equal(rs6[ar, tl], s6) and torch.equal(rw[ar, tl], bits)
    other = torch.ones(B, L, dtype=torch.bool, device=DEV)
    other[ar, tl] = False
    assert bool((rs6[other] == -7.0).all()) and bool((rw[other] == 0x5A5A5A5A).all())
    assert bool((ra[other] == -9).all())
    again = run(3)
    assert all(torch.equal(x, y) for x, y in zip((rs6, rw, ra, out), again))
    assert not torch.equal(run(4)[3], out)  # another counter: other draws (130 instances)
    # an index outside the record: the action is still drawn, nothing is recorded
    t_out = torch.full((B,), L, dtype=torch.int32, device=DEV)
    rs6b = torch.full((B, L, 6), -7.0, device=DEV)
    rwb = torch.zeros(B, L, 22, dtype=torch.int32, device=DEV)
    rab = torch.full((B, L), -9, dtype=torch.int64, device=DEV)
    outb = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _rf_act(lib, logits, s6, bits, L, 77, 3, t_out, rs6b, rwb, rab, outb)
    torch.cuda.synchronize()
    assert torch.equal(outb, out) and bool((rab == -9).all()) and bool((rs6b == -7.0).all())


def test_draws_follow_the_temperature_softmax(lib):
    """P(a) of mz_rf_act's draw == softmax(logits / 2)[a] (select_action, rf_agent.py:79-81):
    2^20 draws per logits row, chi-square against the float64 probabilities (p-value > 1e-6),
    with test_ppo_draws_follow_softmax_probabilities' rows; the -200 logit is never drawn."""
    from scipy.stats import chi2
    rows = torch.tensor([[0.0, 0.5, -1.0, 2.0], [3.0, 3.0, -200.0, 0.1], [-0.3, -0.3, -0.3, -0.3]],
                        device=DEV)
    B, K = 65536, 16
    s6 = torch.zeros(B, 6, device=DEV)
    bits = torch.zeros(B, 22, dtype=torch.int32, device=DEV)
    t = torch.zeros(B, dtype=torch.int32, device=DEV)
    rs6, rw = torch.zeros(B, 6, device=DEV), torch.zeros(B, 22, dtype=torch.int32, device=DEV)
    ra = torch.zeros(B, dtype=torch.int64, device=DEV)
    out = torch.zeros(B, dtype=torch.int32, device=DEV)
    for r in rows:
        logits = r.repeat(B, 1).contiguous()
        counts = torch.zeros(4, dtype=torch.int64, device=DEV)
        for c in range(K):
            _rf_act(lib, logits, s6, bits, 1, 77, c, t, rs6, rw, ra, out)
            counts += torch.bincount(out.long(), minlength=4)
        p = F.softmax(r.double() / 2, dim=-1).cpu().numpy()
        n = counts.cpu().numpy().astype(np.float64)
        assert n.sum() == B * K
        live = p > 1e-12
        assert n[~live].sum() == 0
        exp = p[live] * n.sum()
        stat = ((n[live] - exp) ** 2 / exp).sum()
        assert chi2.sf(stat, live.sum() - 1) > 1e-6, (r.tolist(), n, exp)


# ---- mz_ppo_scan + mz_rf_finish ---------------------------------------------------------------
def test_episode_finish_matches_reference_returns(fx):
    """The nine pool episodes (1, 2, 3, 63, 64, 65, 256, 257, 1000 steps: around one wave, around
    a workgroup's width, several rows per lane) on B = 11 instances, two of them mid-episode:
    adv within rtol 1e-5 / atol 2e-6 of the reference's get_returns output minus its float32
    mean; the length column is T on every row; every other column is the record, bit for bit;
    rows land in instance order; the 1-step episode is dropped and counted; the episode counter
    reads 8; a second round appends behind the first."""
    lens = [int(n) for n in fx["pool.lens"]]
    E = len(lens)
    B = E + 2
    roff = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    poff = np.concatenate([[0], np.cumsum([n if n > 1 else 0 for n in lens])]).astype(int)
    env, tr = _trainer(B, [35], update_rows=1 << 20)
    assert tr.L > max(lens) and tr.gamma == float(fx["gamma"])
    g = torch.Generator(device=DEV).manual_seed(5)
    tr.b_s6.copy_(torch.rand(tr.b_s6.shape, generator=g, device=DEV))
    tr.b_w.copy_(torch.randint(-2**31, 2**31 - 1, tr.b_w.shape, generator=g, device=DEV, dtype=torch.int32))
    tr.b_a.copy_(torch.randint(0, 4, tr.b_a.shape, generator=g, device=DEV))
    rew = torch.from_numpy(fx["pool.rewards"]).to(DEV)

    def round_(episodes):
        r64 = torch.zeros(B, dtype=torch.float64, device=DEV)
        term = torch.zeros(B, dtype=torch.uint8, device=DEV)
        trunc = torch.zeros(B, dtype=torch.uint8, device=DEV)
        t0 = torch.zeros(B, dtype=torch.int32)
        for i, k in episodes:
            n, sl = lens[k], slice(roff[k], roff[k + 1])
            tr.b_r[i, :n - 1] = rew[sl][:-1]
            t0[i] = n - 1
            r64[i] = rew[sl][-1]
            term[i] = 1  # every pool episode ends in the win reward
        t0[E], t0[E + 1] = 5, 0  # two instances mid-episode
        r64[E] = r64[E + 1] = 0.45
        tr.t.copy_(t0)
        tr._scan_finish(r64, term, trunc)
        torch.cuda.synchronize()
        t1 = tr.t.cpu()
        assert all(t1[i] == 0 for i, _ in episodes)
        assert t1[E] == 6 and t1[E + 1] == 1 and float(tr.b_r[E, 5]) == 0.45

    def check(episodes, base):
        o = base
        for i, k in episodes:
            n = lens[k]
            if n == 1:
                continue
            rows = slice(o, o + n)
            ret = torch.from_numpy(fx["pool.returns"][poff[k]:poff[k + 1]])
            torch.testing.assert_close(tr.p_adv[rows].cpu(), ret - ret.mean(), rtol=1e-5, atol=2e-6)
            assert bool((tr.p_len[rows] == n).all())
            assert torch.equal(tr.p_s6[rows], tr.b_s6[i, :n]) and torch.equal(tr.p_w[rows], tr.b_w[i, :n])
            assert torch.equal(tr.p_a[rows], tr.b_a[i, :n])
            o += n
        return o

    first = [(k, k) for k in range(E)]
    round_(first)
    fill = check(first, 0)
    assert int(tr.pool_fill) == fill == sum(n for n in lens if n > 1) == int(tr.pool_total)
    assert tr.stats.tolist() == [E, E, 1, 0] and int(tr.pool_episodes) == 8
    assert bool((tr.p_adv[fill:] == 0).all()) and bool((tr.p_len[fill:] == 0).all())
    second = [(3, 6), (0, 8), (7, 4), (5, 2)]  # instance order differs from fixture order
    round_(second)
    end = check(sorted(second), fill)
    assert int(tr.pool_fill) == end == int(tr.pool_total) and int(tr.pool_episodes) == 12
    check(first, 0)  # the first round's rows are untouched
    env.close()


def test_finish_writes_no_row_past_the_capacity(fx):
    """Two 64-step episodes against a pool of 100 rows: the first is pooled, the second is not
    written (and not counted); the fill the host checks reads 128 > capacity."""
    env, tr = _trainer(2, [15], update_rows=1 << 20, pool_capacity=100)
    r = torch.from_numpy(fx["ep3.rewards"]).to(DEV)
    for i in range(2):
        tr.b_r[i, :63] = r[:63]
    tr.t.fill_(63)
    tr.p_adv.fill_(-5.0)
    ones = torch.ones(2, dtype=torch.uint8, device=DEV)
    tr._scan_finish(r[63:64].repeat(2), ones, torch.zeros_like(ones))
    torch.cuda.synchronize()
    assert int(tr.pool_fill) == 128 and int(tr.pool_episodes) == 1
    assert bool((tr.p_adv[:64] != -5.0).all()) and bool((tr.p_adv[64:] == -5.0).all())
    with pytest.raises(RuntimeError, match="pool overflow"):
        tr._update()
    env.close()


# ---- mz_rf_head_loss --------------------------------------------------------------------------
def _head_inputs(b, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(b, 4, generator=g) * 3
    act = torch.randint(0, 4, (b,), generator=g)
    adv = torch.randn(b, generator=g)
    ln = torch.where(torch.arange(b) < (b + 1) // 2, 5, 64).to(torch.int32)  # two episodes' lengths
    # rows whose drawn action has p < 1e-10 (the +1e-10 decides the value and the gradient),
    # rows with adv = 0, and a row with p_a within 1e-9 of 1
    for j in range(0, b, 9):
        logits[j] = torch.tensor([40.0, 0.0, 0.0, -40.0])
        act[j] = 3
    adv[1::7] = 0.0
    if b > 20:
        logits[20] = torch.tensor([-30.0, 12.0, -30.0, -30.0])
        act[20] = 1
    return logits, act, adv, ln


def _head_ref(logits, act, adv, ln, E, tau, coef):
    x = logits.double().clone().requires_grad_()
    q = F.softmax(x / tau, dim=-1) + 1e-10
    l = torch.log(q)
    pg = -adv.double() * l.gather(1, act[:, None]).squeeze(1) / E
    en = -(coef / ln.double()) * (-(q * l).sum(1)) / E
    loss = (pg + en).sum()
    (gx,) = torch.autograd.grad(loss, x)
    return loss.detach(), gx, float((pg.abs().sum() + en.abs().sum()).detach())


@pytest.mark.parametrize("b,ldl,ldg", [(1, 4, 4), (37, 6, 5), (2048, 4, 4)])
@pytest.mark.parametrize("E", [1, 3])
def test_head_loss_matches_float64_autograd(lib, b, ldl, ldg, E):
    from mazerl import _native as N
    tau, coef = 2.0, 0.01
    logits, act, adv, ln = _head_inputs(b, 100 + b)
    ref_loss, ref_g, terms = _head_ref(logits, act, adv, ln, E, tau, coef)
    wide = torch.full((b, ldl), 1e30)
    wide[:, :4] = logits
    wide, actd, advd, lnd = wide.to(DEV), act.to(DEV), adv.to(DEV), ln.to(DEV)
    ep = torch.tensor([E], dtype=torch.int32, device=DEV)

    def launch():
        loss = torch.full((1,), -1.0, device=DEV)
        dl = torch.full((b, ldg), 7.0, device=DEV)
        N.check(lib.mz_rf_head_loss(wide.data_ptr(), ldl, actd.data_ptr(), advd.data_ptr(),
                                    lnd.data_ptr(), ep.data_ptr(), b, tau, coef, loss.data_ptr(),
                                    dl.data_ptr(), ldg, _stream()))
        torch.cuda.synchronize()
        return loss.cpu(), dl.cpu()

    loss, dl = launch()
    print(f"b={b} E={E}: loss {float(loss):.9g} ref {float(ref_loss):.9g} sum|terms| {terms:.6g}; "
          f"max|dlogits - ref| {float((dl[:, :4].double() - ref_g).abs().max()):.3g} "
          f"max|ref| {float(ref_g.abs().max()):.3g}")
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * terms
    torch.testing.assert_close(dl[:, :4].double(), ref_g, rtol=1e-4, atol=1e-6 * float(ref_g.abs().max()))
    assert bool((dl[:, 4:] == 7.0).all())  # the row stride's padding is not written
    rare = act == 3
    rare &= (logits == torch.tensor([40.0, 0.0, 0.0, -40.0])).all(1)
    if bool((rare & (adv != 0)).any()):  # d f / d x_3 = p_3 (g_3 - sum p g) / tau, g_3 ~ -adv 1e10
        sel = rare & (adv != 0)
        torch.testing.assert_close(dl[sel, 3].double(), ref_g[sel, 3], rtol=1e-4, atol=1e-30)
        assert bool((ref_g[sel, 3].abs() > 1e-10 * adv[sel].abs()).all())
    loss2, dl2 = launch()
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)  # fixed-order sums


def test_head_loss_function_backpropagates_the_kernel_gradient():
    """head_loss (the autograd.Function around mz_rf_head_loss) against reinforce_loss (the torch
    expression) through a layer: loss rel 1e-5, gradients rtol 1e-4."""
    from mazerl.agents.rf_agent import head_loss, reinforce_loss
    b, E = 37, 3
    logits, act, adv, ln = (x.to(DEV) for x in _head_inputs(b, 7))
    w = torch.randn(4, 4, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    ep = torch.tensor([E], dtype=torch.int32, device=DEV)
    out = []
    for fn, e in ((head_loss, ep), (reinforce_loss, E)):
        wp = w.clone().requires_grad_()
        loss = fn(logits @ wp * 0.2, act, adv, ln, e, 2.0, 0.01)
        (gw,) = torch.autograd.grad(2.0 * loss, wp)
        out.append((float(loss), gw))
    assert out[0][0] == pytest.approx(out[1][0], rel=1e-5, abs=1e-7)
    torch.testing.assert_close(out[0][1], out[1][1], rtol=1e-4, atol=1e-6 * float(out[1][1].abs().max()))


# ---- the update -------------------------------------------------------------------------------
def test_fixture_episodes_as_four_updates(fx):
    """The four fixture episodes through the records, mz_ppo_scan + mz_rf_finish and the update
    (E = 1; one chunk for the short episodes, batch_size 16 for the 64-step one: four accumulated
    chunks) on the fixture's net (4 conv channels, hidden 8): parameters rtol 1e-5 / atol 1e-5,
    the lr to 1e-12, as the CPU test."""
    from mazerl.agents.rf_agent import cosine_lr
    env, tr = _trainer(1, [15], hidden=8, h_channels=4, update_rows=1, lr=float(fx["lr"]),
                       gamma=float(fx["gamma"]))
    with torch.no_grad():
        tr.net.load_state_dict({str(k): torch.from_numpy(fx[f"init.{k}"]) for k in fx["names"]})
    one = torch.ones(1, dtype=torch.uint8, device=DEV)
    for e, T in enumerate(int(n) for n in fx["ep.lens"]):
        assert T < tr.L
        r = torch.from_numpy(fx[f"ep{e}.rewards"]).to(DEV)
        tr.b_s6[0, :T] = torch.from_numpy(fx[f"ep{e}.obs6"]).to(DEV)
        tr.b_w[0, :T] = torch.from_numpy(fx[f"ep{e}.bits"]).to(DEV)
        tr.b_a[0, :T] = torch.from_numpy(fx[f"ep{e}.actions"]).to(DEV)
        tr.b_r[0, :T - 1] = r[:-1]
        tr.t.fill_(T - 1)
        tr._scan_finish(r[-1:].clone(), one, torch.zeros_like(one))
        tr.batch_size = 16 if T == 64 else 2048
        tr._update()
        torch.cuda.synchronize()
        assert tr.updates == e + 1 and tr.last_update["episodes"] == 1
        assert tr.last_update["cols"][0].shape[0] == T == tr.rows_trained - sum(fx["ep.lens"][:e])
        assert int(tr.pool_fill) == 0 and int(tr.pool_episodes) == 0
        ret = torch.from_numpy(fx[f"ep{e}.returns"])
        torch.testing.assert_close(tr.last_update["cols"][3].cpu(), ret - ret.mean(), rtol=1e-5, atol=2e-6)
        assert abs(tr.last_update["lr"] - cosine_lr(e, float(fx["lr"]))) <= 1e-12
        assert abs(cosine_lr(tr.updates, tr.lr) - float(fx[f"ep{e}.lr_after"])) <= 1e-12
        assert float(tr.opt.lr_dev[0]) == pytest.approx(tr.last_update["lr"], rel=1e-6)
        for k, p in tr.net.named_parameters():
            torch.testing.assert_close(p.detach().cpu(), torch.from_numpy(fx[f"ep{e}.param.{k}"]),
                                       rtol=1e-5, atol=1e-5,
                                       msg=lambda m, k=k, e=e: f"episode {e} param {k}: {m}")
    env.close()


def test_one_instance_is_the_reference_step():
    """B = 1 on a 15x15 euclidean maze with an update after every episode: every update consumed
    one whole episode (E = 1), and redoing the updates with reinforce_loss + clip_grad_norm_(1.0)
    + torch AdamW at cosine_lr from the same starting parameters gives the trainer's parameters
    after each update (rtol 1e-5 / atol 1e-5)."""
    from mazerl.agents.rf_agent import PolicyNetwork, cosine_lr, reinforce_loss
    env, tr = _trainer(1, [15], update_rows=1, seed=3)
    ref = PolicyNetwork(3, 6, 4, 32, 256).to(DEV)
    ref.load_state_dict(tr.net.state_dict())
    opt = torch.optim.AdamW(ref.parameters(), tr.lr)
    steps = 0
    while tr.updates < 3 and steps < 4 * tr.L:
        before = tr.updates
        tr.vector_step()
        steps += 1
        if tr.updates == before:
            continue
        up = tr.last_update
        s6, bits, act, adv, ln = up["cols"]
        T = s6.shape[0]
        assert up["episodes"] == 1 and T >= 2 and bool((ln == T).all())
        for g in opt.param_groups:
            g["lr"] = cosine_lr(before, tr.lr)
        loss = reinforce_loss(ref((s6, bits)), act, adv, ln, 1)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt.step()
        assert float(up["loss"]) == pytest.approx(float(loss), rel=1e-4, abs=1e-6)
        for (k, p), q in zip(tr.net.named_parameters(), ref.parameters()):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-5,
                                       msg=lambda m, k=k, u=before: f"update {u} param {k}: {m}")
    assert tr.updates == 3, steps
    assert tr.rows_trained == tr.consumed and tr.episodes >= 3
    env.close()


# ---- end to end -------------------------------------------------------------------------------
def _e2e(kind, seed=0, env_seed=0x5EED0000):
    if kind == "euclidean":
        return _trainer(256, [15], max_dim=23, growth=(15, 23), curriculum="global", bank=True,
                        update_rows=2048, batch_size=1024, seed=seed, env_seed=env_seed)
    return _trainer(256, [17, 21], toroidal=True, update_rows=2048, batch_size=1024, seed=seed,
                    env_seed=env_seed)


@pytest.mark.parametrize("kind", ["euclidean", "toroidal"])
def test_vector_reinforce_trains_with_device_pool(kind):
    """300 vector steps of B = 256: updates fire from the one-step-late view of the pool total,
    each consumes every pooled episode (the pool is empty right after), the counters match the
    pool's rows, no parameter goes non-finite, and both evaluations run."""
    from mazerl.trainers.vector_trainer import evaluate
    env, tr = _e2e(kind)
    for _ in range(300):
        before, rows = tr.updates, tr.rows_trained
        tr.vector_step()
        if tr.updates > before:
            assert int(tr.pool_fill) == 0 and int(tr.pool_episodes) == 0
            up = tr.last_update
            assert tr.rows_trained - rows == up["cols"][0].shape[0] >= 2048
            ln, i, n_ep = up["cols"][4].cpu(), 0, 0
            while i < ln.numel():  # whole episodes only: T rows that carry the length T
                T = int(ln[i])
                assert T >= 2 and bool((ln[i:i + T] == T).all()) and i + T <= ln.numel()
                i, n_ep = i + T, n_ep + 1
            assert n_ep == up["episodes"]
    fill = int(tr.pool_fill)
    assert tr.updates >= 1 and tr.rows_trained == tr.consumed
    assert int(tr.pool_total) == tr.consumed + fill and 0 <= fill <= tr.cap
    assert tr.episodes > 0 and tr.stats.tolist()[3] == 0
    assert all(bool(torch.isfinite(p).all()) for p in tr.net.parameters())
    dims = [15, 19, 23] if kind == "euclidean" else [17, 21]
    for learner in (tr, tr.sampler()):
        rate, _ = evaluate(learner, 64, dims, toroidal=kind == "toroidal", device=DEV, seed=5)
        assert 0.0 <= rate <= 1.0
    env.close()


@pytest.mark.parametrize("kind", ["euclidean", "toroidal"])
def test_checkpoint_resume_is_bit_exact(kind, tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    envA, A = _e2e(kind, seed=1)
    A.train(120)
    assert A.updates > 0
    path = save_checkpoint(str(tmp_path / "rf.pt"), A)
    A.train(60)
    envB, Bt = _e2e(kind, seed=2, env_seed=0x5EED1111)
    load_checkpoint(path, Bt)
    Bt.train(60)
    torch.cuda.synchronize()
    assert A.updates == Bt.updates and A.counter == Bt.counter == 180 and A.consumed == Bt.consumed
    assert torch.equal(A.stats, Bt.stats) and torch.equal(A.t, Bt.t)
    for (ka, pa), (kb, pb) in zip(A.net.state_dict().items(), Bt.net.state_dict().items()):
        assert torch.equal(pa, pb), ka
    assert torch.equal(A.env.obs6, Bt.env.obs6) and torch.equal(A.env.window_bits, Bt.env.window_bits)
    assert torch.equal(A.env.reward64, Bt.env.reward64)
    for i in range(0, 256, 37):  # the mazes and the per-instance state behind the observations
        assert A.env.query(i) == Bt.env.query(i) and np.array_equal(A.env.grid(i), Bt.env.grid(i)), i
    fill = int(A.pool_fill)
    assert fill == int(Bt.pool_fill) and torch.equal(A.p_w[:fill], Bt.p_w[:fill])
    assert torch.equal(A.p_adv[:fill], Bt.p_adv[:fill]) and int(A.pool_episodes) == int(Bt.pool_episodes)
    envA.close()
    envB.close()
