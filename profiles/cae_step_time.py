#!/usr/bin/env python3
"""One autoencoder training step at batch 4 and batch 4,096 on both paths: the HIP path
(VectorCAETrainer.step: stem forward, mz_cae_loss, stem backward, the flat Adam launch) and the
same module's torch-eager f32 path on expanded windows (CAE.forward, mse_loss, mazerl.cae.ssim,
backward, torch.optim.Adam). HIP events around `iters` steps after `warmup` steps; the two paths
are timed alternately, three rounds, and the median per step is reported. Prints one JSON line.
--path hip | eager times one path alone (the eager path's first steps compile MIOpen kernels for
a dozen small convolutions, minutes on a fresh machine; progress goes to stderr).

  python profiles/cae_step_time.py [--iters 200] [--eager-iters 20] [--warmup 30] [--path both]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "maze-solving-agent-gymnasium_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mazerl.cae import VectorCAETrainer, ssim, unpack_windows  # noqa: E402
from mazerl.lib.models.convolutional_autoencoder import CAE  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--eager-iters", type=int, default=20,
                    help="timed eager steps per round (a batch-4,096 eager step is ~0.65 s)")
    ap.add_argument("--path", default="both", choices=["both", "hip", "eager"])
    a = ap.parse_args()
    paths = ("hip", "eager") if a.path == "both" else (a.path,)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    out = {"iters": a.iters, "eager_iters": min(a.iters, a.eager_iters),
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for batch in (4, 4096):
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (batch, 22), device=dev, generator=g,
                             dtype=torch.int64).to(torch.int32)
        bits[:, 21] &= (1 << (675 - 21 * 32)) - 1
        x = unpack_windows(bits)
        torch.manual_seed(0)
        hip = VectorCAETrainer(CAE(3, 32).to(dev), bits, batch_size=batch)
        torch.manual_seed(0)
        net = CAE(3, 32).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=5e-3)

        def hip_step():
            hip.step(bits)

        def eager_step():
            y = net(x)
            loss = 0.65 * F.mse_loss(y, x) + 0.35 * (1 - ssim(y, x))
            opt.zero_grad()
            loss.backward()
            opt.step()

        steps = {"hip": hip_step, "eager": eager_step}
        for k in paths:
            t0 = time.time()
            for _ in range(a.warmup):
                steps[k]()
            torch.cuda.synchronize()
            print(f"batch {batch} {k}: warm-up {time.time() - t0:.1f} s", file=sys.stderr,
                  flush=True)
        runs = {k: [] for k in paths}
        for _ in range(3):
            for k in paths:
                runs[k].append(timed(steps[k], a.iters if k == "hip" else
                                     min(a.iters, a.eager_iters)))
        rec = {}
        for k in paths:
            rec[f"{k}_us"] = statistics.median(runs[k])
            rec[f"{k}_runs_us"] = runs[k]
        out[f"batch_{batch}"] = rec
        print(f"batch {batch}: {json.dumps(rec)}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
