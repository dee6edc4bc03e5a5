"""Prioritized replay windows in recurrent DQN populations: the three new entry points refuse bad
arguments with MZ_EINVAL before any GPU call (no device is needed: the pointers handed over are
never followed, some of them are garbage), the population's constructor refuses priority arguments
that break the rules, learner by learner, before it touches the env or the device, its footprint
counts the new buffers, and the command line sweeps the four settings per learner."""
import ctypes as C

import pytest

H, L = 32, 8
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from mazerl import _native
    return _native.load()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_uint64 * 64)()  # any non-null address: a refusal comes before any use of it
    yield C.addressof(buf)


def test_prio_entry_points_refuse_bad_arguments(lib, p):
    from mazerl import _native as N
    g = 0xDEAD0008  # garbage: following it would fault, so a clean MZ_EINVAL shows nothing ran
    store = lambda hid=H, P=3, b=4, Lr=L, T=3, cap=5, fin=p, flen=p, fcnt=p, prio=p, psum=p, \
        pmax=p, ring=p: lib.mz_drqn_pop_prio_store(hid, P, b, Lr, T, fin, flen, fcnt, cap, prio,  # noqa: E731
                                                   psum, pmax, ring, None)
    sample = lambda seed=p, cnt=p, burn=p, beta=p, due=p, hid=H, P=3, E=4, Lr=L, T=3, K=3, cap=5, \
        lens=p, prio=p, psum=p, wdir=p, off=p, tot=p, isw=p: lib.mz_drqn_pop_prio_sample(  # noqa: E731
            seed, cnt, burn, beta, due, hid, P, E, Lr, T, K, cap, lens, prio, psum, wdir, off, tot,
            isw, None)
    update = lambda alpha=p, eta=p, eps=p, due=p, hid=H, P=3, E=4, Lr=L, T=3, cap=5, wdir=p, off=p, \
        tot=p, qa=p, y=p, d=p, ep=p, isw=p, prio=p, psum=p, pmax=p: lib.mz_drqn_pop_prio_update(  # noqa: E731
            alpha, eta, eps, due, hid, P, E, Lr, T, cap, wdir, off, tot, qa, y, d, ep, isw, prio,
            psum, pmax, None)
    bad = [
        lambda: store(P=0), lambda: store(P=-1), lambda: store(b=0), lambda: store(hid=16),
        lambda: store(Lr=0), lambda: store(T=0), lambda: store(cap=0), lambda: store(fin=None),
        lambda: store(flen=None), lambda: store(fcnt=None), lambda: store(prio=None),
        lambda: store(psum=None), lambda: store(pmax=None), lambda: store(ring=None),
        lambda: store(cap=2 ** 33, T=8),                          # capacity W 2^30 >= 2^63
        lambda: store(P=0, fin=g, prio=g, psum=g, pmax=g, ring=g),
        lambda: sample(P=0), lambda: sample(hid=8), lambda: sample(E=0), lambda: sample(Lr=0),
        lambda: sample(T=0), lambda: sample(K=-3), lambda: sample(K=4), lambda: sample(cap=0),
        lambda: sample(seed=None), lambda: sample(cnt=None), lambda: sample(burn=None),
        lambda: sample(beta=None), lambda: sample(lens=None), lambda: sample(prio=None),
        lambda: sample(psum=None), lambda: sample(wdir=None), lambda: sample(off=None),
        lambda: sample(tot=None), lambda: sample(isw=None),
        lambda: sample(cap=2 ** 31, E=4, T=8, K=0),
        lambda: sample(K=4, seed=g, cnt=g, burn=g, beta=g, lens=g, prio=g, psum=g, wdir=g, isw=g),
        lambda: update(P=0), lambda: update(hid=16), lambda: update(E=0), lambda: update(Lr=0),
        lambda: update(T=0), lambda: update(cap=0), lambda: update(alpha=None),
        lambda: update(eta=None), lambda: update(eps=None), lambda: update(wdir=None),
        lambda: update(off=None), lambda: update(tot=None), lambda: update(qa=None),
        lambda: update(y=None), lambda: update(d=None), lambda: update(ep=None),
        lambda: update(isw=None), lambda: update(prio=None), lambda: update(psum=None),
        lambda: update(pmax=None), lambda: update(cap=2 ** 29, E=8, T=4),
        lambda: update(T=0, alpha=g, eta=g, eps=g, wdir=g, qa=g, d=g, prio=g, pmax=g),
    ]
    for k, f in enumerate(bad):
        assert f() == EINVAL, k
        with pytest.raises(ValueError):
            N.check(f())
    assert lib.mz_drqn_pop_prio_sample(p, p, p, None, p, H, 3, 4, L, 3, 3, 5, p, p, p, p, p, p, p,
                                       None) == EINVAL
    assert b"mz_drqn_pop_prio_sample: null pointer" in lib.mz_last_error()
    # the scalar fallbacks of the shared validators keep their ranges (the single entry points)
    assert lib.mz_drqn_prio_sample(1, 2, H, 4, L, 3, 3, 5, p, p, p, p, p, p, p, -0.5, None) == EINVAL
    assert lib.mz_drqn_prio_update(H, 4, L, 3, 5, p, p, p, p, p, p, p, p, 0.9, 1.5, 1e-3, p, p, p,
                                   None) == EINVAL
    assert lib.mz_drqn_prio_update(H, 4, L, 3, 5, p, p, p, p, p, p, p, p, 0.9, 0.9, 0.0, p, p, p,
                                   None) == EINVAL


class _Env:
    num_envs, max_dim, toroidal = 12, 9, False


def test_constructor_refuses_priority_arguments_that_break_the_rules():
    """All before the env or the device is touched."""
    from mazerl.trainers import VectorRecurrentDQNPopulation as Pop
    for kw in (dict(priority_alpha=0.9),                                  # no window
               dict(priority_alpha=[None, None, 0.9]),
               dict(window=4, priority_alpha=[None, 0.0, -0.1]),
               dict(window=4, priority_alpha=[None, 0.0, float("nan")]),
               dict(window=4, priority_alpha=0.9, priority_eta=1.5),
               dict(window=4, priority_alpha=0.9, priority_eta=[0.9, 0.9, -0.1]),
               dict(window=4, priority_alpha=0.9, priority_eps=0.0),
               dict(window=4, priority_alpha=0.9, priority_eps=[1e-3, -1.0, 1e-3]),
               dict(window=4, priority_alpha=0.9, priority_beta=-1.0),
               dict(window=4, priority_alpha=0.9, priority_beta=(0.4, 1.0, 0)),      # one schedule
               dict(window=4, priority_alpha=0.9, priority_beta=[0.4, (0.4, 1.0), 0.6]),
               dict(window=4, priority_alpha=0.9, priority_beta=[0.4, 0.6, (0.4, 1.0, 2.5)]),
               dict(window=4, priority_alpha=[None, 0.5, 0.9],
                    priority_beta=[0.4, (0.4, -1.0, 10), (0.4, 1.0, 10)])):
        with pytest.raises(ValueError, match="priority_alpha"):
            Pop(_Env(), "cuda", learners=3, **kw)
    for kw in (dict(priority_alpha=[0.5, 0.9]), dict(priority_alpha=0.9, priority_beta=[0.4, 0.6]),
               dict(priority_alpha=0.9, priority_eta=[0.9] * 4),
               dict(priority_alpha=0.9, priority_eps=[1e-3] * 2)):
        with pytest.raises(ValueError, match="3 learners"):
            Pop(_Env(), "cuda", learners=3, window=4, **kw)


def test_footprint_and_memory_error_count_the_priorities(monkeypatch):
    import torch
    from mazerl.trainers import VectorRecurrentDQNPopulation as Pop
    from mazerl.trainers.drqn_population import footprint
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (1 << 20, 1 << 30))
    kw = dict(learners=3, memory_size=100000, batch_size=4, window=4, initial_state="zero")
    with pytest.raises(MemoryError, match="mem_prio"):
        Pop(_Env(), "cuda", priority_alpha=[None, 0.0, 0.9], **kw)
    with pytest.raises(MemoryError) as e:
        Pop(_Env(), "cuda", priority_alpha=[None] * 3, **kw)
    assert "mem_prio" not in str(e.value)
    P, B, Lb, E, cap = 3, 12, 30, 4, 50
    plain, pr = footprint(P, B, Lb, E, cap, 4, False), footprint(P, B, Lb, E, cap, 4, False, True)
    assert set(pr) - set(plain) == {"prio"}
    # per learner: capacity x (8 windows x 4 B + an 8 B sum), prio_max, E weights, three float64
    assert pr["prio"] == P * (cap * (8 * 4 + 8) + 4 + E * 4 + 24)
    assert pr["total"] == plain["total"] + pr["prio"]
    assert all(pr[k] == plain[k] for k in plain if k != "total")


def test_command_line_sweeps_the_priority_settings():
    from mazerl.train_lstm_dqn import parse_args, parse_sweeps
    out = parse_sweeps(["priority-alpha=none,0,0.9"], None, 3)
    assert out == {"priority_alpha": [None, 0.0, 0.9]}
    out = parse_sweeps(["priority_alpha=0.5", "priority-beta=0.4,0.4:1:100,1", "priority-eta=0.5",
                        "priority-eps=0.01,0.02,0.03"], "1,2,3", 3)
    assert out == {"priority_alpha": [0.5] * 3, "priority_beta": [0.4, (0.4, 1.0, 100), 1.0],
                   "priority_eta": [0.5] * 3, "priority_eps": [0.01, 0.02, 0.03], "seed": [1, 2, 3]}
    with pytest.raises(ValueError, match="values must be"):
        parse_sweeps(["priority-alpha=none,zero,0.9"], None, 3)
    with pytest.raises(ValueError, match="values must be"):
        parse_sweeps(["priority-beta=0.4:1,0.6,0.6"], None, 3)
    with pytest.raises(ValueError, match="2 values for 3 learners"):
        parse_sweeps(["priority-alpha=none,0.9"], None, 3)
    with pytest.raises(ValueError, match="given twice"):
        parse_sweeps(["priority-alpha=0.9", "priority_alpha=0.5"], None, 3)
    base = ["--learners", "2", "--envs", "64"]
    a = parse_args(base + ["--window", "4", "--sweep", "priority-alpha=none,0.9",
                           "--priority-beta", "0.4,1,500", "--priority-eta", "0.5"])
    assert a.per_learner == {"priority_alpha": [None, 0.9]} and a.priority_alpha is None
    assert (a.priority_beta, a.priority_eta, a.priority_eps) == ((0.4, 1.0, 500), 0.5, 1e-3)
    for argv in (["--sweep", "priority-alpha=0.9"],                       # no --window
                 ["--window", "4", "--sweep", "priority-alpha=0.9,-1"],
                 ["--window", "4", "--sweep", "priority-alpha=0.9", "--priority-eta", "2"],
                 ["--window", "4", "--sweep", "priority-alpha=0.9", "--sweep", "priority-eps=1,0"],
                 ["--window", "4", "--priority-beta", "0.5"],             # no learner has an alpha
                 ["--window", "4", "--sweep", "priority-alpha=none", "--sweep", "priority-eta=0.5"],
                 ["--window", "4", "--sweep", "priority-alpha=none,x"]):
        with pytest.raises(SystemExit):
            parse_args(base + argv)
