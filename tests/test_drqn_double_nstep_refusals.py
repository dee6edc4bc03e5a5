"""double_q and n_step without a GPU: the constructors' refusals (raised before anything touches a
device) and the command line's two flags and two sweeps."""
import pytest


def _trainer(**kw):
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    return VectorRecurrentDQNTrainer(None, "cpu", **kw)


class _Env:
    num_envs = 8


def _population(**kw):
    from mazerl.trainers.drqn_population import VectorRecurrentDQNPopulation
    return VectorRecurrentDQNPopulation(_Env(), "cpu", learners=4, **kw)


BAD = [dict(n_step=0), dict(n_step=-1), dict(n_step=1.5), dict(n_step=True), dict(n_step=None),
       dict(n_step="3"), dict(double_q=1), dict(double_q=0), dict(double_q=None),
       dict(double_q="yes"), dict(double_q=True, n_step=0)]


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_the_trainer_refuses(kw):
    with pytest.raises(ValueError, match="double_q: a bool; n_step: an int >= 1"):
        _trainer(**kw)


@pytest.mark.parametrize("kw", BAD + [dict(n_step=[1, 3, 0, 5]), dict(n_step=[1, 2.0, 3, 4]),
                                      dict(double_q=[True, False, 1, False]),
                                      dict(n_step=[1, True, 3, 5])], ids=str)
def test_the_population_refuses(kw):
    with pytest.raises(ValueError, match="double_q: a bool; n_step: an int >= 1"):
        _population(**kw)


@pytest.mark.parametrize("kw", [dict(n_step=[1, 3, 5]), dict(double_q=[True, False]),
                                dict(n_step=[1, 2, 3, 4, 5]), dict(double_q=[])], ids=str)
def test_the_population_refuses_a_list_of_the_wrong_length(kw):
    with pytest.raises(ValueError, match="values for 4 learners"):
        _population(**kw)


def test_the_checks_come_before_the_other_arguments_and_accept_the_valid_ones():
    from mazerl.trainers.drqn_trainer import check_returns
    for dq in (False, True):
        for n in (1, 2, 5, 1000):
            check_returns(dq, n)
    # a refused n_step is reported although the env is unusable: nothing was touched
    with pytest.raises(ValueError, match="n_step"):
        _trainer(n_step=0, window=4, burn_in=4)


def _parse(*argv):
    from mazerl.train_lstm_dqn import parse_args
    return parse_args(list(argv))


def test_cli_flags():
    a = _parse()
    assert a.double_q is False and a.n_step == 1
    a = _parse("--double-q", "--n-step", "5", "--window", "40", "--burn-in", "40")
    assert a.double_q is True and a.n_step == 5 and a.per_learner is None
    a = _parse("--n-step", "3")
    assert a.double_q is False and a.n_step == 3
    for argv in (["--n-step", "0"], ["--n-step", "-2"], ["--n-step", "1.5"], ["--n-step"],
                 ["--double-q", "1"]):
        with pytest.raises(SystemExit):
            _parse(*argv)


def test_cli_sweeps():
    a = _parse("--envs", "64", "--learners", "4", "--sweep", "double-q=0,1,0,1", "--sweep",
               "n-step=1,1,3,5")
    assert a.per_learner == {"double_q": [False, True, False, True], "n_step": [1, 1, 3, 5]}
    a = _parse("--envs", "64", "--learners", "4", "--double-q", "--sweep", "n_step=5")
    assert a.double_q is True and a.per_learner == {"n_step": [5, 5, 5, 5]}
    a = _parse("--envs", "64", "--learners", "2", "--sweep", "double-q=1", "--seeds", "3,4")
    assert a.per_learner == {"double_q": [True, True], "seed": [3, 4]}
    for sweeps in (["double-q=0,1,2,0"], ["double-q=yes,no,no,no"], ["n-step=1,0,3,5"],
                   ["n-step=1,2.5,3,5"], ["n-step=1,3,5"], ["double-q=0,1"],
                   ["n-step=1,3,5,7", "n-step=1"]):
        argv = ["--envs", "64", "--learners", "4"]
        for s in sweeps:
            argv += ["--sweep", s]
        with pytest.raises(SystemExit):
            _parse(*argv)
    with pytest.raises(SystemExit):  # a sweep needs a population
        _parse("--sweep", "n-step=3")
