"""Pre-train the conv stem as the encoder of the convolutional autoencoder: the reference's
train_CAE.py on the GPU.

  python -m mazerl.train_cae                                   # the reference's recipe
  python -m mazerl.train_cae --mazes 64 --epochs 10 --save w   # a smaller run

The recipe: 400 distinct 15x15 mazes, each from an algorithm drawn among r-prim / prim&kill / dfs,
split 0.8 / 0.2, batch 4, 30 epochs of alpha * MSE + (1 - alpha) * (1 - SSIM) with alpha 0.65,
Adam(5e-3), CosineAnnealingLR(T_max=15, eta_min=1e-5) stepped per epoch. Prints one JSON line per
epoch ({"epoch", "loss", "lr"}) and a last one with the cosine similarity between the held-out
windows and the rounded reconstructions. With --save DIR writes DIR/CAE_(15, 15).pth (the model's
state_dict) and DIR/FeatureExtractor_(15, 15).pth (the encoder's): `mazerl.cae.load_stem` and
`python -m mazerl.train --stem` take either, and both load into the reference's modules.
"""
import argparse
import json
import os

import torch

from .cae import VectorCAETrainer, collect_windows
from .lib.models.convolutional_autoencoder import CAE
from .vector_env import VectorMazeEnv


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mazes", type=int, default=400, help="distinct mazes in the collection")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--alpha", type=float, default=0.65)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--save", default=None, help="directory for the two state_dicts")
    a = ap.parse_args(argv)
    if a.mazes < 2 or a.batch < 1 or a.epochs < 0:
        ap.error("--mazes >= 2, --batch >= 1, --epochs >= 0")
    dev = torch.device("cuda", torch.cuda.current_device())
    env = VectorMazeEnv(min(a.mazes, 1024), 15, enrich=True, device=dev, generate=False,
                        window=False)
    windows = collect_windows(env, a.mazes, seed=a.seed)
    env.close()
    # dataset.random_split(maze_set, [0.8, 0.2]): a seeded permutation, floor(0.8 n) to train
    g = torch.Generator().manual_seed(a.seed)
    perm = torch.randperm(a.mazes, generator=g).to(dev)
    n_train = max(1, min(a.mazes - 1, int(0.8 * a.mazes)))
    train, test = windows[perm[:n_train]], windows[perm[n_train:]]
    torch.manual_seed(a.seed)
    model = CAE(3, 32).to(dev)
    trainer = VectorCAETrainer(model, train, batch_size=a.batch, lr=a.lr, alpha=a.alpha,
                               seed=a.seed)
    log = []
    for _ in range(a.epochs):
        rec = trainer.train(1)[0]
        log.append(rec)
        print(json.dumps(rec), flush=True)
    sim = trainer.evaluate(test, a.batch)
    res = {"mazes": a.mazes, "train": n_train, "test": a.mazes - n_train, "batch": a.batch,
           "epochs": a.epochs, "final_loss": log[-1]["loss"] if log else None,
           "cosine_similarity": sim}
    if a.save:
        os.makedirs(a.save, exist_ok=True)
        cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}  # noqa: E731
        torch.save(cpu(model.state_dict()), os.path.join(a.save, "CAE_(15, 15).pth"))
        torch.save(cpu(model.encoder.state_dict()),
                   os.path.join(a.save, "FeatureExtractor_(15, 15).pth"))
        res["saved"] = a.save
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
