"""The population entry points of the recurrent DQN refuse bad arguments with MZ_EINVAL before any
GPU call (no device is needed: the pointers handed over are never followed), the population's
constructor refuses the coupling curriculum, and the command line parses --learners / --sweep /
--seeds and leaves the single-learner path alone."""
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


def test_population_entry_points_refuse_bad_arguments(lib, p):
    from mazerl import _native as N
    act = lambda params=p, hidden=H, P=3, b=4, obs=p, Lr=L, explore=4: lib.mz_drqn_pop_act(  # noqa: E731
        params, hidden, P, b, obs, Lr, p, explore, p, 0, p, p, p, p, p, p, None, None)
    store = lambda P=3, b=4, cap=5, mem=p: lib.mz_drqn_pop_store(  # noqa: E731
        p, p, P, b, L, p, p, p, p, p, p, cap, mem, p, p, p, None)
    sample = lambda P=3, E=4, cap=5, filled=5, seed=p: lib.mz_drqn_pop_sample(  # noqa: E731
        seed, p, p, P, E, L, cap, filled, p, p, p, p, p, p, None)
    fwd = lambda params=p, hidden=H, target=1, P=3, E=2, cap=5, stash=None: \
        lib.mz_drqn_pop_seq_forward(params, hidden, target, P, E, L, cap, p, p, p, p, p, p, p, p,  # noqa: E731
                                    p, stash, stash, stash, stash, stash, None)
    bwd = lambda params=p, hidden=H, P=3, E=2, cap=5, grads=p: lib.mz_drqn_pop_seq_backward(  # noqa: E731
        params, hidden, P, E, L, cap, p, p, p, p, p, p, p, p, p, p, grads, p, None)
    sync = lambda src=p, P=3, mask=p: lib.mz_drqn_pop_sync(src, p, mask, P, None)  # noqa: E731
    adam = lambda param=p, P=3, n=5252, clamp=1.0: lib.mz_adamw_pop(  # noqa: E731
        param, p, p, p, P, n, p, p, p, 0.9, 0.999, 1e-8, 1e-2, clamp, 1.0, 1, None)
    bad = [
        lambda: act(params=None), lambda: act(obs=None), lambda: act(hidden=16),
        lambda: act(P=0), lambda: act(b=0), lambda: act(Lr=-1), lambda: act(explore=5),
        lambda: lib.mz_drqn_pop_act(p, H, 3, 4, p, L, p, 4, p, 0, p, p, p, None, p, p, None, None),
        lambda: store(P=0), lambda: store(b=0), lambda: store(cap=0), lambda: store(mem=None),
        lambda: sample(P=0), lambda: sample(E=0), lambda: sample(E=6),  # capacity < E
        lambda: sample(filled=3),                                       # E > the smallest filled
        lambda: sample(seed=None),
        lambda: fwd(params=None), lambda: fwd(hidden=16), lambda: fwd(P=0), lambda: fwd(E=0),
        lambda: fwd(E=6), lambda: fwd(target=0),                        # source mode needs outputs
        lambda: bwd(params=None), lambda: bwd(hidden=8), lambda: bwd(P=0), lambda: bwd(E=0),
        lambda: bwd(E=6), lambda: bwd(grads=None),
        lambda: sync(src=None), lambda: sync(P=0), lambda: sync(mask=None),
        lambda: adam(param=None), lambda: adam(P=0), lambda: adam(n=5250), lambda: adam(n=0),
        lambda: adam(clamp=0.0),
    ]
    for k, f in enumerate(bad):
        assert f() == EINVAL, k
        with pytest.raises(ValueError):
            N.check(f())


def test_global_curriculum_and_uneven_blocks_are_refused():
    """Both are refused before the env or the device is touched."""
    from mazerl.trainers import VectorRecurrentDQNPopulation

    class Env:
        num_envs = 12

    for cur in (True, "global"):
        with pytest.raises(ValueError, match="couple"):
            VectorRecurrentDQNPopulation(Env(), "cuda", learners=3, curriculum=cur)
    with pytest.raises(ValueError, match="multiple"):
        VectorRecurrentDQNPopulation(Env(), "cuda", learners=5)
    with pytest.raises(ValueError, match="3 learners"):
        VectorRecurrentDQNPopulation(Env(), "cuda", learners=3, lr=[1e-3, 1e-4])


def test_command_line_sweeps():
    from mazerl.train_lstm_dqn import parse_args, parse_sweeps, spread
    a = parse_args(["--learners", "4", "--envs", "64", "--sweep", "lr=1e-3,3e-4,1e-4,3e-5",
                    "--sweep", "gamma=0.9", "--sweep", "target_update=5,6,7,8", "--seeds", "0,1,2,3"])
    assert a.per_learner == {"lr": [1e-3, 3e-4, 1e-4, 3e-5], "discount_factor": [0.9] * 4,
                             "target_update_frequency": [5, 6, 7, 8], "seed": [0, 1, 2, 3]}
    assert parse_sweeps(None, None, 3) == {}
    assert parse_sweeps(["eps-decay=200"], "7", 2) == {"epsilon_decay": [200.0, 200.0],
                                                       "seed": [7, 7]}
    for sweeps, seeds in ((["lr=1,2"], None), (["batch=3"], None), (["lr"], None),
                          (["lr=a"], None), (["lr=1", "lr=2"], None), (["seed=1"], "2"),
                          (None, "1,2")):
        with pytest.raises(ValueError):
            parse_sweeps(sweeps, seeds, 3)
    s = spread([0.5, 0.7, 0.9])
    assert s["mean"] == pytest.approx(0.7) and s["std"] == pytest.approx(0.2)
    assert (s["min"], s["max"]) == (0.5, 0.9) and spread([0.4])["std"] == 0.0


def test_command_line_without_learners_is_the_single_trainer(monkeypatch, capsys):
    """No --learners: the arguments of before, and main() builds VectorRecurrentDQNTrainer."""
    import mazerl.train_lstm_dqn as T
    a = T.parse_args(["--envs", "64", "--seed", "3"])
    assert a.learners is None and a.per_learner is None and a.seed == 3 and a.envs == 64
    for argv in (["--sweep", "lr=1e-3"], ["--seeds", "1,2"], ["--learners", "3", "--envs", "64"]):
        with pytest.raises(SystemExit):
            T.parse_args(argv)
    capsys.readouterr()
    built = []

    class Stop(Exception):
        pass

    class Env:
        def __init__(self, *a, **k):
            pass

    def single(*a, **k):
        built.append("single")
        raise Stop

    def population(a):
        built.append("population")

    monkeypatch.setattr(T, "VectorMazeEnv", Env)
    monkeypatch.setattr(T, "VectorRecurrentDQNTrainer", single)
    monkeypatch.setattr(T, "main_population", population)
    monkeypatch.setattr(T.torch.cuda, "current_device", lambda: 0)
    with pytest.raises(Stop):
        T.main(["--envs", "64"])
    T.main(["--envs", "64", "--learners", "2"])
    assert built == ["single", "population"]
