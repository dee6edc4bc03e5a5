"""The recurrent DQN at 4,096 instances: the time of mz_drqn_act and of one update
(sample + target / source sequence forward + BPTT + FlatAdamW, E = 32 episodes) on 9x9 and 41x41
plain mazes, HIP-event timed over many launches after a warm-up.
One JSON line per size (profiles/lstm_dqn/probe.jsonl).
  exp_lstm_dqn_probe.py act LABEL   times mz_drqn_act alone at 4,096 and 65,536 instances: run
once per build of csrc/mz_drqn.hip with -DMZ_DRQN_ACT_PARTS=1 / 2 / 4 (threads per instance) loaded
through MZ_LIB_OVERRIDE (profiles/lstm_dqn/act_parts.jsonl)."""
import json, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maze-solving-agent-gymnasium_amd"))
import mazerl
from mazerl.trainers.drqn_trainer import VectorRecurrentDQNTrainer

def timed(f, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3  # us

if len(sys.argv) > 2 and sys.argv[1] == "act":
    for B in (4096, 65536):
        env = mazerl.VectorMazeEnv(B, 9, enrich=False, device="cuda", pos=False, done_list=False)
        tr = VectorRecurrentDQNTrainer(env, "cuda", batch_size=4, memory_size=8, train_every=10 ** 9, bank=False)
        for _ in range(20):
            tr._act()
        print(json.dumps({"probe": "mz_drqn_act", "build": sys.argv[2], "instances": B,
                          "act_us": round(timed(tr._act, 300), 2)}), flush=True)
        env.close()
    sys.exit(0)

for dim, fill_steps in ((9, 200), (41, 1800)):
    env = mazerl.VectorMazeEnv(4096, dim, enrich=False, device="cuda", pos=False, done_list=False)
    tr = VectorRecurrentDQNTrainer(env, "cuda", batch_size=32, memory_size=4096, train_every=10 ** 9, bank=False)
    for _ in range(fill_steps):
        tr.vector_step()
    count = int(tr.ring[1])
    tr.filled = count
    def act():
        tr._act()
        tr.counter -= 1; tr.steps_done -= 1
    def update():
        tr.sample(); tr.update(1e-3); tr.updates += 1
    for _ in range(20):
        act(); update()
    t_act, t_upd = timed(act, 200), timed(update, 50)
    lens = tr.mem_len[:count].float()
    print(json.dumps({"probe": "lstm-dqn", "dim": dim, "L": tr.L, "episodes_in_memory": count,
                      "mean_episode_steps": float(lens.mean()), "max_episode_steps": int(lens.max()),
                      "last_batch_steps": int(tr.d_tot[1]), "act_us": round(t_act, 1), "update_us": round(t_upd, 1)}), flush=True)
    env.close()
