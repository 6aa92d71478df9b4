#!/usr/bin/env python
"""One WGAN-GP critic step (dg_critic_step: the three-batch forward and backward, both sets of weight gradients, the tangent pass,
the reduction with Adam) of the reference's mnist_discriminator at its training shape, net_dim 128 and batch 50.  tflib's initial
weights, synthetic images; --warmup steps, then the median over --repeat windows of --steps steps each, every window ending in a
device synchronise.

    python tools/critic_time.py [--net_dim 128] [--batch 50] [--steps 20] [--repeat 5]      -> ms per step, steps/s and one JSON line
    rocprofv3 --kernel-trace --stats -d out -- python tools/critic_time.py --repeat 1          (the per-kernel split, a run of its own)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--net_dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--penalty_axes", default="reference", choices=["reference", "image"])
    args = ap.parse_args()
    import torch
    from defensegan_amd import critic
    c = critic.mnist_discriminator(net_dim=args.net_dim)
    c.init_like_tflib(seed=0)
    rs = np.random.RandomState(0)
    B = args.batch
    real = torch.from_numpy(rs.uniform(0, 1, (B, 28, 28, 1)).astype(np.float32)).cuda()
    fake = torch.from_numpy(rs.uniform(0, 1, (B, 28, 28, 1)).astype(np.float32)).cuda()
    alpha = torch.from_numpy(rs.uniform(0, 1, B).astype(np.float32)).cuda()
    cost = torch.empty(3, dtype=torch.float32, device=real.device)
    for _ in range(args.warmup):
        c.step(real, fake, alpha, penalty_axes=args.penalty_axes, cost=cost)
    times = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            c.step(real, fake, alpha, penalty_axes=args.penalty_axes, cost=cost)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / args.steps)
    ms = 1e3 * float(np.median(times))
    print("%.3f ms per critic step, %.1f steps/s (net_dim %d, batch %d)" % (ms, 1e3 / ms, args.net_dim, B))
    print(json.dumps({"net_dim": args.net_dim, "batch": B, "steps": args.steps, "repeat": args.repeat, "ms_per_step": ms,
                      "steps_per_s": 1e3 / ms, "spread_ms": [1e3 * min(times), 1e3 * max(times)], "cost": [float(v) for v in cost.cpu()]}))
    c.close()


if __name__ == "__main__":
    main()
