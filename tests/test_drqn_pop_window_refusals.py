"""Replay windows in recurrent DQN populations: the four new entry points refuse bad arguments
with MZ_EINVAL before any GPU call (no device is needed: the pointers handed over are never
followed), the population's constructor refuses window arguments that break the rules before it
touches the env or the device, its MemoryError names the state memory, and the command line takes
--window / --burn-in / --initial-state with --learners."""
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


def test_window_entry_points_refuse_bad_arguments(lib, p):
    from mazerl import _native as N
    snap = lambda hidden=H, P=3, b=4, Lr=L, T=3, cap=5, fin=p, state=p, ring=p: \
        lib.mz_drqn_pop_snap_store(hidden, P, b, Lr, T, fin, p, p, p, cap, state, ring, None)  # noqa: E731
    sample = lambda seed=p, burn=p, hidden=H, P=3, E=4, Lr=L, T=3, K=6, cap=5, filled=5, wdir=p: \
        lib.mz_drqn_pop_window_sample(seed, p, burn, p, hidden, P, E, Lr, T, K, cap, filled, p, p,  # noqa: E731
                                      wdir, p, p, None)
    fwd = lambda params=p, hidden=H, target=1, P=3, E=2, Lr=L, T=3, K=6, cap=5, burn=p, stored=p, \
        state=p, stash=None, gamma=p: lib.mz_drqn_pop_window_forward(  # noqa: E731
            params, hidden, target, P, E, Lr, T, K, cap, gamma, burn, stored, p, p, p, state, p, p,
            p, p, stash, stash, stash, stash, stash, None)
    bwd = lambda params=p, hidden=H, P=3, E=2, Lr=L, T=3, K=6, cap=5, burn=p, grads=p, gpart=p: \
        lib.mz_drqn_pop_window_backward(params, hidden, P, E, Lr, T, K, cap, burn, p, p, p, p, p,  # noqa: E731
                                        p, p, p, gpart, grads, p, None)
    bad = [
        lambda: snap(hidden=16), lambda: snap(P=0), lambda: snap(b=0), lambda: snap(Lr=0),
        lambda: snap(T=0), lambda: snap(cap=0), lambda: snap(fin=None), lambda: snap(state=None),
        lambda: snap(ring=None),
        lambda: sample(seed=None), lambda: sample(burn=None), lambda: sample(wdir=None),
        lambda: sample(hidden=8), lambda: sample(P=0), lambda: sample(E=0), lambda: sample(Lr=0),
        lambda: sample(T=0), lambda: sample(K=-3), lambda: sample(K=4),  # K_max % T != 0
        lambda: sample(E=6),                                             # capacity < E
        lambda: sample(filled=3),                                        # E > min_filled
        lambda: fwd(params=None), lambda: fwd(hidden=16), lambda: fwd(P=0), lambda: fwd(E=0),
        lambda: fwd(Lr=0), lambda: fwd(T=0), lambda: fwd(K=-3), lambda: fwd(K=5), lambda: fwd(E=6),
        lambda: fwd(burn=None), lambda: fwd(stored=None),  # a state memory needs stored_dev
        lambda: fwd(target=0),                             # source mode needs its outputs
        lambda: fwd(target=0, stash=p, gamma=None),
        lambda: bwd(params=None), lambda: bwd(hidden=8), lambda: bwd(P=0), lambda: bwd(E=0),
        lambda: bwd(Lr=0), lambda: bwd(T=0), lambda: bwd(K=-3), lambda: bwd(K=7), lambda: bwd(E=6),
        lambda: bwd(burn=None), lambda: bwd(grads=None), lambda: bwd(gpart=None),
    ]
    for k, f in enumerate(bad):
        assert f() == EINVAL, k
        with pytest.raises(ValueError):
            N.check(f())


class _Env:
    num_envs, max_dim, toroidal = 12, 9, False


def test_constructor_refuses_window_arguments_that_break_the_rules():
    """All before the env or the device is touched."""
    from mazerl.trainers import VectorRecurrentDQNPopulation as Pop
    for kw in (dict(window=4, burn_in=3),                      # K_p no multiple of T
               dict(window=4, burn_in=[0, 4, 6]),
               dict(burn_in=4),                                # burn_in without window
               dict(burn_in=[0, 0, 4]),
               dict(window=0), dict(window=4, burn_in=-4), dict(window=4, burn_in=4.0),
               dict(window=4, initial_state="kept"),           # unknown initial_state
               dict(window=4, initial_state=["stored", "zero", "none"])):
        with pytest.raises(ValueError, match="window"):
            Pop(_Env(), "cuda", learners=3, **kw)
    with pytest.raises(ValueError, match="3 learners"):
        Pop(_Env(), "cuda", learners=3, window=4, burn_in=[0, 4])
    with pytest.raises(ValueError, match="3 learners"):
        Pop(_Env(), "cuda", learners=3, window=4, initial_state=["stored", "zero"])


def test_memory_error_names_the_state_memory(monkeypatch):
    import torch
    from mazerl.trainers import VectorRecurrentDQNPopulation as Pop
    from mazerl.trainers.drqn_population import footprint
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (1 << 20, 1 << 30))
    kw = dict(learners=3, memory_size=100000, batch_size=4)
    with pytest.raises(MemoryError, match="mem_state") as e:
        Pop(_Env(), "cuda", window=4, burn_in=4, initial_state=["stored", "zero", "zero"], **kw)
    assert "snap_rec" in str(e.value)
    for extra in (dict(), dict(window=4, initial_state="zero")):  # no state memory to name
        with pytest.raises(MemoryError) as e:
            Pop(_Env(), "cuda", **extra, **kw)
        assert "mem_state" not in str(e.value)
    # the accounting: P capacity ceil(L / T) snapshots of 256 B, B in flight; windowed row buffers
    P, B, Lb, E, cap = 3, 12, 30, 4, 50
    whole, zero = footprint(P, B, Lb, E, cap), footprint(P, B, Lb, E, cap, 4, False)
    st = footprint(P, B, Lb, E, cap, 4, True)
    assert set(whole) == {"replay", "records", "update", "total"}
    assert st["state"] == P * cap * 8 * 256 and st["snap_rec"] == B * 8 * 256
    assert zero["state"] == zero["snap_rec"] == 0 and zero["update"] == st["update"] < whole["update"]
    assert st["total"] == zero["total"] + st["state"] + st["snap_rec"]
    assert whole["replay"] == zero["replay"] and whole["records"] == zero["records"]


def test_command_line_windows_with_learners():
    from mazerl.train_lstm_dqn import parse_args
    a = parse_args(["--learners", "2", "--envs", "64", "--window", "4", "--burn-in", "4"])
    assert (a.window, a.burn_in, a.initial_state, a.per_learner) == (4, 4, "stored", {})
    a = parse_args(["--learners", "2", "--envs", "64", "--window", "4", "--sweep", "burn-in=0,4",
                    "--sweep", "initial-state=stored,zero", "--initial-state", "zero"])
    assert a.per_learner == {"burn_in": [0, 4], "initial_state": ["stored", "zero"]}
    a = parse_args(["--learners", "3", "--envs", "66", "--window", "2", "--sweep", "burn_in=4"])
    assert a.per_learner == {"burn_in": [4, 4, 4]}
    for argv in (["--window", "4", "--sweep", "window=4,8"],       # T is shared
                 ["--window", "4", "--sweep", "burn-in=3"],        # no multiple of T
                 ["--window", "4", "--sweep", "burn-in=0,6"],
                 ["--sweep", "burn-in=0,4"],                       # a burn-in without windows
                 ["--burn-in", "4"],
                 ["--window", "4", "--sweep", "initial-state=stored,kept"],
                 ["--window", "4", "--sweep", "burn-in=0,4,8"],    # three values, two learners
                 ["--window", "4", "--burn-in", "6"]):
        with pytest.raises(SystemExit):
            parse_args(["--learners", "2", "--envs", "64"] + argv)
    # without --learners the window options are the single trainer's, as before
    a = parse_args(["--envs", "64", "--window", "4", "--burn-in", "8", "--initial-state", "zero"])
    assert (a.learners, a.per_learner, a.window, a.burn_in) == (None, None, 4, 8)
