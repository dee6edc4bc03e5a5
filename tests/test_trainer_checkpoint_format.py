"""The on-disk format of the three episode-recording trainers (trainers/episodic.py and its
subclasses): the key sets of state_dict(), written out here as the files of earlier versions hold
them, the live-row count of the records and the format strings. Smallest shapes the trainers
accept: 64 instances of 15x15 Enrich mazes (PPO, REINFORCE), of 9x9 plain mazes (recurrent DQN);
40 vector steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 40

FLAT_OPT = {"exp_avg", "exp_avg_sq", "step_t", "lr_dev"}
KEYS = {
    "ppo": dict(
        format="mazerl.VectorPPOTrainer/2",
        top={"format", "L", "cap", "schedule", "net", "opt", "t", "records", "pool_fill", "pool",
             "pool_total", "stats", "total_host", "counters", "env"},
        records={"b_s6", "b_w", "b_a", "b_lp", "b_v", "b_r"},
        pool={"p_s6", "p_w", "p_a", "p_lp", "p_adv", "p_ret"},
        opt=FLAT_OPT,
        counters={"seed", "counter", "consumed", "updates", "rows_trained", "calls"}),
    "reinforce": dict(
        format="mazerl.VectorReinforceTrainer/1",
        top={"format", "L", "cap", "schedule", "net", "opt", "t", "records", "pool_fill", "pool",
             "pool_total", "pool_episodes", "stats", "total_host", "counters", "env"},
        records={"b_s6", "b_w", "b_a", "b_r"},
        pool={"p_s6", "p_w", "p_a", "p_adv", "p_len"},
        opt=FLAT_OPT,
        counters={"seed", "counter", "sample_counter", "consumed", "updates", "rows_trained"}),
    "drqn": dict(
        format="mazerl.VectorRecurrentDQNTrainer/1",
        top={"format", "L", "capacity", "schedule", "source", "target", "opt", "h", "c", "t",
             "records", "ring", "mem", "mem_len", "mem_term", "stats", "pool", "loss", "counters",
             "env"},
        records={"rec_x", "rec_a", "rec_r"},
        pool=None,  # a tensor: mz_ppo_scan's two row counters
        opt={"exp_avg", "exp_avg_sq", "step", "lr"},
        counters={"seed", "steps_done", "counter", "updates", "filled"}),
}


def _mk(kind, growth=None, max_dim=None):
    """The trainer at its smallest shape; growth: a growth schedule (the env's pitch is then its
    largest size); max_dim: that pitch without a schedule."""
    import mazerl
    from mazerl.trainers.vector_trainer import make_env
    max_dim = growth[1] if growth else max_dim
    if kind == "drqn":
        from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
        env = mazerl.VectorMazeEnv(64, 9, enrich=False, device=DEV, seed=0x5EED0D00,
                                   max_dim=max_dim)
        return VectorRecurrentDQNTrainer(env, DEV, batch_size=4, memory_size=64, growth=growth)
    env = make_env(64, [15], device=DEV, done_list=False, reward64=True, window=False,
                   window_bits=True, max_dim=max_dim)
    if kind == "ppo":
        from mazerl.trainers.ppo_trainer import VectorPPOTrainer
        return VectorPPOTrainer(env, DEV, hidden_dim=64, batch_size=64, pool_size=256,
                                growth=growth)
    from mazerl.trainers.reinforce_trainer import VectorReinforceTrainer
    return VectorReinforceTrainer(env, DEV, hidden_dim=64, batch_size=64, update_rows=256,
                                  growth=growth)


def _growth(kind):
    return (9, 13) if kind == "drqn" else (15, 19)


@pytest.fixture(scope="module", params=list(KEYS))
def run(request):
    """(kind, the trainer after 40 vector steps, its state_dict): made once, left unchanged."""
    tr = _mk(request.param)
    tr.train(STEPS)
    yield request.param, tr, tr.state_dict()
    tr.env.close()


def test_state_dict_key_sets_and_format(run):
    kind, tr, sd = run
    want = KEYS[kind]
    assert sd["format"] == want["format"]
    assert set(sd) == want["top"]
    for part in ("records", "pool", "opt", "counters"):
        if want[part] is None:
            assert torch.is_tensor(sd[part]) and sd[part].shape == (2,)
        else:
            assert isinstance(sd[part], dict) and set(sd[part]) == want[part], part
    assert sd["schedule"] is None
    assert sd["counters"]["counter"] == STEPS and sd["L"] == tr.L


def test_records_hold_the_live_rows_only(run):
    kind, tr, sd = run
    n = int(sd["t"].sum())
    assert 0 < n < tr.env.num_envs * tr.L
    for k, v in sd["records"].items():
        assert v.shape[0] == n, k
        assert v.shape[1:] == getattr(tr, k).shape[2:], k


@pytest.mark.parametrize("kind", list(KEYS))
def test_growth_schedule_is_saved_as_a_dict_and_refused_by_a_trainer_without_one(kind):
    g = _growth(kind)
    tr = _mk(kind, growth=g)
    tr.train(4)
    sd = tr.state_dict()
    assert isinstance(sd["schedule"], dict) and sd["schedule"]["growth"] == list(g)
    assert set(sd) == KEYS[kind]["top"]
    plain = _mk(kind, max_dim=g[1])  # the same shape, no schedule
    assert plain.schedule is None and plain.L == tr.L
    with pytest.raises(ValueError, match="curriculum / growth differ"):
        plain.load_state_dict(sd)
    tr.env.close()
    plain.env.close()
