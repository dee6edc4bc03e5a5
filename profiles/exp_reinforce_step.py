"""Vector steps of VectorReinforceTrainer at train_reinforce's defaults (4,096 euclidean instances,
growth 15 -> 35, global curriculum) for a rocprofv3 kernel trace:

  rocprofv3 --kernel-trace --stats -f csv -d OUT -o run -- python3 profiles/exp_reinforce_step.py 200

Prints the vector steps, updates and rows trained, so the trace's calls divide into launches per
vector step."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "maze-solving-agent-gymnasium_amd"))
from mazerl.trainers.reinforce_trainer import VectorReinforceTrainer  # noqa: E402
from mazerl.trainers.vector_trainer import make_env  # noqa: E402


def main(steps=200, envs=4096):
    dev = torch.device("cuda", 0)
    env = make_env(envs, [15], device=dev, done_list=False, reward64=True, window=False,
                   window_bits=True, max_dim=35)
    tr = VectorReinforceTrainer(env, dev, curriculum="global", growth=(15, 35))
    secs = tr.train(steps)
    print(json.dumps({"vector_steps": steps, "envs": envs, "seconds": secs, "updates": tr.updates,
                      "rows_trained": tr.rows_trained, "episodes": tr.episodes}), flush=True)
    env.close()


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:]))
