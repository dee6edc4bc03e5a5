"""Two probes of VectorReinforceTrainer at 4,096 instances:
1. the win plumbing: the DQN exploration draw (mask-weighted random valid moves, env.act(eps=1))
   stepped through mz_ppo_scan / mz_rf_finish for 600 vector steps on 15x15 euclidean mazes;
2. the policy itself for 3,000 vector steps, euclidean 15x15 and toroidal 17 / 21: episodes, wins,
   updates and the mean step reward over the first and the last 100 vector steps.
One JSON line each (profiles/reinforce/probe.jsonl)."""
import json, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maze-solving-agent-gymnasium_amd"))
from mazerl.trainers.reinforce_trainer import VectorReinforceTrainer
from mazerl.trainers.vector_trainer import make_env

def mk(tor, dims, **kw):
    env = make_env(4096, dims, toroidal=tor, device="cuda", done_list=False, reward64=True, window=False, window_bits=True)
    return env, VectorReinforceTrainer(env, "cuda", bank=False, **kw)

# 1. plumbing: mask-weighted random valid moves (the DQN exploration draw) through scan / finish
env, tr = mk(False, [15], update_rows=1 << 30, pool_capacity=1 << 20)
for k in range(600):
    acts = env.act(eps=1.0, seed=5, counter=k)
    env.step(acts)
    tr._scan_finish()
    env.reset_done(regen_won=True)
print(json.dumps({"probe": "valid-move random walk, euclid 15", "episodes": tr.episodes, "wins": tr.wins}), flush=True)
env.close()
# 2. the policy itself, mean step reward early vs late, euclidean 15 and toroidal 17/21
for tor, dims in ((False, [15]), (True, [17, 21])):
    env, tr = mk(tor, dims)
    acc = []
    for k in range(3000):
        tr.vector_step()
        if k < 100 or k >= 2900:
            acc.append(env.reward64.mean())
    a = torch.stack(acc).cpu()
    print(json.dumps({"probe": "policy", "toroidal": tor, "episodes": tr.episodes, "wins": tr.wins, "updates": tr.updates,
                      "mean_step_reward_first100": float(a[:100].mean()), "mean_step_reward_last100": float(a[100:].mean())}), flush=True)
    env.close()
