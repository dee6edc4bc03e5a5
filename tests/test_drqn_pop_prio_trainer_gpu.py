"""VectorRecurrentDQNPopulation with prioritized replay windows per learner on the GPU: 3 learners
x 64 instances of 9x9 plain mazes, E = 4, T = 4, K in {0, 4}, stored and zero state. Learner p is
defined as VectorRecurrentDQNTrainer with p's arguments on its block (an instance's mazes are keyed
by the env's seed + its index, so an env of 64 instances under seed + 64 p holds block p's mazes and
draws its replacements), which tests/test_drqn_prio_trainer_gpu.py and
tests/test_drqn_window_trainer_gpu.py hold to the models, so every comparison here is `==` on the
bits."""
import numpy as np
import pytest
import torch

from test_drqn_pop_window_trainer_gpu import _same

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIM, b, T, P = 9, 64, 4, 3
ENV_SEED = 0x5EED0D00
KW = dict(bank=False, memory_size=64, batch_size=4, epsilon_decay=200.0, window=T)
# learner 0 uniform, learner 1 uniform over the memory's windows (alpha 0) with a beta schedule,
# learner 2 R2D2's exponents with eta and eps of its own
PER = dict(seed=[0, 1, 2], lr=[1e-3, 2e-3, 1e-3], target_update_frequency=[2, 3, 4],
           priority_alpha=[None, 0.0, 0.9], priority_beta=[0.6, (0.4, 1.0, 5), 0.6],
           priority_eta=[0.9, 0.9, 0.5], priority_eps=[1e-3, 1e-3, 1e-2])
WINDOWS = {"K0-4-4": dict(burn_in=[0, 4, 4], initial_state=["stored", "stored", "zero"]),
           "K4-0-0": dict(burn_in=[4, 0, 0], initial_state=["zero", "stored", "stored"])}


def _env(B, seed=ENV_SEED):
    import mazerl
    return mazerl.VectorMazeEnv(B, DIM, toroidal=False, enrich=False, device=DEV, seed=seed)


def _pop(env_seed=ENV_SEED, **kw):
    from mazerl.trainers import VectorRecurrentDQNPopulation
    return VectorRecurrentDQNPopulation(_env(P * b, env_seed), DEV, learners=P, **{**KW, **kw})


def _single(p, per):
    from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer
    kw = dict(KW, **{k: v[p] for k, v in per.items()})
    return VectorRecurrentDQNTrainer(_env(b, ENV_SEED + p * b), DEV, **kw)


def _state(tr):
    """Everything a run is, learner by learner: test_drqn_pop_window_trainer_gpu's list and the
    priorities."""
    out = [tr.stats.clone()]
    for p in range(tr.P):
        s = slice(p * tr.b, (p + 1) * tr.b)
        out += [tr.src[p], tr.tgt[p], tr.exp_avg[p], tr.exp_avg_sq[p], tr.step[p], tr.ring[p],
                tr.mem[p], tr.mem_len[p], tr.mem_term[p], tr.h[:, s], tr.c[:, s], tr.t[s],
                tr.loss[p], tr.env.obs6[s]]
        if tr.stored[p]:
            out += [tr.mem_state[p, :int(tr.ring[p, 1]), 1:], tr.snap_rec[s]]
        if any(tr.prio):
            out += [tr.mem_prio[p], tr.mem_psum[p], tr.prio_max[p]]
        out.append(torch.tensor([tr.steps_done[p], tr.updates[p]]))
    return [t.clone() for t in out]


def _psum_holds(tr):
    return torch.equal(tr.mem_psum, tr.mem_prio.to(torch.int64).sum(dim=2))


@pytest.mark.parametrize("win", list(WINDOWS))
def test_learner_p_is_the_single_trainer_with_its_arguments_bit_for_bit(win):
    """A mixed population (alpha None, 0, 0.9; one beta a schedule that ends after 5 updates) run
    until every learner has updated at least 8 times (target syncs included): parameters, both
    Adam moments and the step count, mem, mem_len, mem_term and the ring, mem_prio, mem_psum and
    prio_max, the loss, the directory, the weights; mem_psum[p][slot] == mem_prio[p][slot].sum()
    after every step."""
    per = dict(PER, **WINDOWS[win])
    pop = _pop(**per)
    ones = [_single(p, per) for p in range(P)]
    assert pop.prio == [False, True, True] and pop.mem_prio.shape == (P, 64, pop.snaps)
    assert pop.prio_max.tolist() == [1 << 20] * P and bool((pop.isw == 1).all())
    assert ones[0].priority_alpha is None and ones[2].priority_alpha == 0.9
    for p, one in enumerate(ones):  # the same mazes to begin with
        assert torch.equal(one.env.obs6, pop.env.obs6[p * b:(p + 1) * b])
    for k in range(300):
        pop.vector_step()
        for one in ones:
            one.vector_step()
        assert _psum_holds(pop), k
        if min(pop.updates) >= 8:
            break
    print(f"vector steps {k + 1}, updates {pop.updates}, prio_max {pop.prio_max.tolist()}, "
          f"log {pop._log_fields()}")
    assert min(pop.updates) >= 8
    for p, one in enumerate(ones):
        s, o = slice(p * b, (p + 1) * b), one.opt
        pairs = [(pop.src[p], one.source_net._flat_params[:5252]),
                 (pop.tgt[p], one.target_net._flat_params[:5252]),
                 (pop.exp_avg[p], o.exp_avg[:5252]), (pop.exp_avg_sq[p], o.exp_avg_sq[:5252]),
                 (pop.step[p:p + 1], o._step_buf), (pop.ring[p], one.ring), (pop.mem[p], one.mem),
                 (pop.mem_len[p], one.mem_len), (pop.mem_term[p], one.mem_term),
                 (pop.h[:, s], one.h), (pop.c[:, s], one.c), (pop.t[s], one.t),
                 (pop.loss[p:p + 1], one.loss), (pop.rec_x[s], one.rec_x), (pop.rec_a[s], one.rec_a),
                 (pop.wdir[p], one.wdir), (pop.d_off[p], one.d_off), (pop.d_tot[p], one.d_tot),
                 (pop.qa[p], one.qa), (pop.d[p], one.d), (pop.gpart[p], one.gpart),
                 (pop.env.obs6[s], one.env.obs6)]
        if pop.stored[p]:
            pairs += [(pop.mem_state[p], one.mem_state), (pop.snap_rec[s], one.snap_rec)]
        if pop.prio[p]:
            pairs += [(pop.mem_prio[p], one.mem_prio), (pop.mem_psum[p], one.mem_psum),
                      (pop.prio_max[p:p + 1], one.prio_max), (pop.isw[p], one.isw)]
            assert pop.beta(p) == one.beta()
        for j, (x, y) in enumerate(pairs):
            assert _same([x], [y]), (p, j)
        assert (pop.steps_done[p], pop.updates[p], pop.filled[p]) == \
            (one.steps_done, one.updates, one.filled)
        assert pop.last_lr[p] == one.last_lr
    # the uniform learner's weights were never written, the others' were
    assert bool((pop.isw[0] == 1).all())
    m2 = pop.mem_prio[2]
    assert bool(((m2 != 0) & (m2 != 1 << 20)).any())  # alpha 0.9: masses that follow the residuals
    assert bool((pop.mem_prio[1][pop.mem_prio[1] != 0] == 1 << 20).all())  # alpha 0: every mass 1
    assert pop.beta(1) == 1.0  # the schedule ran out at this learner's own update 5
    log = pop._log_fields()
    assert log["prio_max"][0] is None and log["mean_weight"][0] is None
    assert log["prio_max"][1] == 1.0 and 0.0 < log["mean_weight"][2] <= 1.0
    for t in [pop] + ones:
        t.env.close()


def test_all_uniform_is_the_population_of_before():
    """Every alpha None, given as a value and as a list with the other three arguments set: the
    same bits over the same run as a population built without the arguments, no priority buffer,
    the same state dict key for key and bit for bit. Two entries of the env's own state dict are
    compared by what they do instead of by their bytes, since two envs of the same run do not share
    them: device_state, VectorMazeEnv's opaque copy of its handle, holds device scratch (tables and
    planes of cells no kernel reads), and outputs holds the last step's id lists in the order the
    env's atomics gave them. The population loads the other's checkpoint and both continue on the
    same bits."""
    kw = dict(seed=[3, 4, 5], lr=[1e-3, 2e-3, 1e-3], burn_in=[4, 0, 4],
              initial_state=["stored", "zero", "stored"])
    plain = _pop(**kw)
    none = _pop(priority_alpha=[None] * P, priority_beta=[0.4, (0.4, 1.0, 5), 1.0],
                priority_eta=0.5, priority_eps=[1e-2] * P, **kw)
    for _ in range(40):
        plain.vector_step()
        none.vector_step()
    assert min(plain.updates) > 4 and plain.updates == none.updates
    for tr in (plain, none):
        assert tr.priority_alpha is None and tr.prio == [False] * P and tr.upd.numel() == 5 * P
        assert not any(hasattr(tr, k) for k in ("mem_prio", "mem_psum", "prio_max", "isw",
                                                "beta_dev", "prio_alpha_dev"))
        assert "prio" not in tr.memory_bytes() and "prio_max" not in tr._log_fields()
    assert _same(_state(plain), _state(none))
    sa, sb = plain.state_dict(), none.state_dict()
    assert list(sa) == list(sb) and not {"priority", "mem_prio", "mem_psum", "prio_max"} & set(sa)

    def flat(v):
        if isinstance(v, dict):
            return [x for k in v for x in flat(v[k])]
        if isinstance(v, (list, tuple)):
            return [x for u in v for x in flat(u)]
        return [v]
    assert list(sa["env"]) == list(sb["env"])
    for k in sa:
        xs, ys = flat(sa[k]), flat(sb[k])
        if k == "env":
            xs, ys = (flat({j: v for j, v in sd[k].items() if j not in ("device_state", "outputs")})
                      for sd in (sa, sb))
        assert len(xs) == len(ys), k
        for x, y in zip(xs, ys):
            if torch.is_tensor(x):
                assert _same([x], [y]), k
            elif isinstance(x, np.ndarray):
                assert np.array_equal(x, y), k
            else:
                assert x == y, k
    none.load_state_dict(sa)
    for _ in range(10):
        plain.vector_step()
        none.vector_step()
    assert _same(_state(plain), _state(none))
    prio = _pop(priority_alpha=[None, 0.0, 0.9], **kw)
    assert set(prio.state_dict()) - set(sa) == {"priority", "mem_prio", "mem_psum", "prio_max"}
    assert prio.memory_bytes()["total"] == plain.memory_bytes()["total"] + prio.memory_bytes()["prio"]
    for t in (plain, none, prio):
        t.env.close()


def test_checkpoint_resume_same_seed_repeatability_and_mismatched_settings(tmp_path):
    from mazerl.checkpoint import load_checkpoint, save_checkpoint
    kw = dict(PER, **WINDOWS["K0-4-4"])
    tr, twin = _pop(**kw), _pop(**kw)
    for _ in range(30):
        tr.vector_step()
        twin.vector_step()
    assert min(tr.updates) > 4 and int((tr.t > 0).sum()) > 0
    assert _same(_state(tr), _state(twin))  # the same seeds: the same bits
    path = save_checkpoint(str(tmp_path / "pop.pt"), tr)
    tr2 = _pop(env_seed=0x5EED0D99, **dict(kw, seed=[8, 9, 10]))
    assert not _same(_state(tr), _state(tr2))
    load_checkpoint(path, tr2)
    assert _same(_state(tr), _state(tr2)) and tr2.seed == [0, 1, 2]
    for _ in range(15):  # past the end of learner 1's beta schedule or not: its own update count
        tr.vector_step()
        tr2.vector_step()
        twin.vector_step()
    assert tr.updates == tr2.updates and tr.steps_done == tr2.steps_done
    assert _same(_state(tr), _state(tr2)) and _same(_state(tr), _state(twin))
    assert torch.equal(tr.isw, tr2.isw) and torch.equal(tr.wdir, tr2.wdir) and _psum_holds(tr2)
    # a population with other per-learner settings refuses the checkpoint
    for other in (dict(priority_alpha=[None, 0.0, 0.8]), dict(priority_alpha=[0.0, 0.0, 0.9]),
                  dict(priority_alpha=[None, None, 0.9]), dict(priority_beta=[0.6, 0.4, 0.6]),
                  dict(priority_beta=[0.6, (0.4, 1.0, 6), 0.6]),
                  dict(priority_eta=[0.9, 0.9, 0.6]), dict(priority_eps=[1e-3, 2e-3, 1e-2]),
                  dict(priority_alpha=None)):
        tr3 = _pop(**dict(kw, **other))
        with pytest.raises(ValueError, match="prioritized replay"):
            load_checkpoint(path, tr3)
        tr3.env.close()
    # a checkpoint without the keys loads into an all-None population only
    kw0 = {k: v for k, v in kw.items() if not k.startswith("priority")}
    old = _pop(**kw0)
    for _ in range(12):
        old.vector_step()
    keyless = save_checkpoint(str(tmp_path / "old.pt"), old)
    with pytest.raises(ValueError, match="prioritized replay"):
        load_checkpoint(keyless, tr2)
    fresh = _pop(env_seed=0x5EED0D99, priority_alpha=[None] * P, **kw0)
    load_checkpoint(keyless, fresh)
    assert _same(_state(old), _state(fresh))
    for t in (tr, twin, tr2, old, fresh):
        t.env.close()
