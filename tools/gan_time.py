#!/usr/bin/env python
"""One iteration of the WGAN-GP training loop (DefenseGANBase.train_gan) at the reference's shape -- generator NET_DIM 64, critic
net_dim 64, batch 50, 5 critic steps: ms per generator step (generate + critic seed + dg_gen_step), ms per critic step (generate +
dg_critic_step), ms per full iteration (1 + critic_iters), and the split of the generator step into forward, seed (the critic's
forward and backward, timed around the calls), backward, weight gradients and Adam plus refresh from the engine's profile hooks.
Synthetic weights and images; --warmup steps, then the median over --repeat windows of --steps steps, every window ending in a
device synchronise.

    python tools/gan_time.py [--net_dim 64] [--critic_dim 64] [--batch 50] [--steps 20] [--repeat 5]     -> text and one JSON line
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = (("forward", ("F1", "F2", "F3", "T5f")), ("backward", ("G5seed", "B5", "B3", "B2", "B1")), ("weight gradients", ("W",)),
          ("adam + refresh", ("ADAM", "REFRESH")))


def group_of(name):
    for g, prefixes in GROUPS:
        if any(name.startswith(p) for p in prefixes):
            return g
    return "other"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--net_dim", type=int, default=64)
    ap.add_argument("--critic_dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--critic_iters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch
    from defensegan_amd import critic, synth
    from defensegan_amd.gan import MnistDefenseGAN
    B = args.batch
    g = MnistDefenseGAN(cfg={"USE_BN": False, "NET_DIM": args.net_dim, "BATCH_SIZE": B, "CRITIC_ITERS": args.critic_iters}, test_mode=False)
    g.set_weights(synth.make_weights("mnist", seed=0, gain=1.0, net_dim=args.net_dim))
    g._ensure_handle()
    c = critic.mnist_discriminator(net_dim=args.critic_dim)
    c._device = g._device
    c.init_like_tflib(seed=0)
    g._critic = c
    rs = np.random.RandomState(0)
    real = torch.from_numpy(rs.uniform(0, 1, (B, 28, 28, 1)).astype(np.float32)).cuda()
    alpha = torch.from_numpy(rs.uniform(0, 1, B).astype(np.float32)).cuda()
    z = g.init_latents(B, seed=1, std=1.0)
    cost = torch.empty(3, dtype=torch.float32, device=real.device)

    def gen_step():
        g.generator_step(z)

    def critic_step():
        c.step(real, g.generate(z), alpha, cost=cost)

    def seed_only():
        g._critic_seed(g.generate(z))

    def iteration():
        gen_step()
        for _ in range(args.critic_iters):
            critic_step()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        times = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / args.steps)
        return 1e3 * float(np.median(times))

    out = {"net_dim": args.net_dim, "critic_dim": args.critic_dim, "batch": B, "critic_iters": args.critic_iters,
           "ms_generator_step": timed(gen_step), "ms_critic_step": timed(critic_step), "ms_iteration": timed(iteration),
           "ms_seed": timed(seed_only)}
    # the split of dg_gen_step's own launches
    g.profile_enable(1)
    g.profile_reset()
    zz, dy = z, g._critic_seed(g.generate(z))[1]
    g.profile_reset()
    n = 10
    for _ in range(n):
        g.generator_step(zz, dy)
    torch.cuda.synchronize()
    split, kernels = {}, {}
    for e in g.profile_read():
        split[group_of(e["name"])] = split.get(group_of(e["name"]), 0.0) + e["ms"] / n
        kernels[e["name"]] = e["ms"] / n
    g.profile_enable(0)
    out["split_ms"] = split
    out["kernels_ms"] = kernels
    print("%.3f ms per generator step (of which %.3f ms generate + critic seed), %.3f ms per critic step, %.3f ms per iteration (1 + %d)"
          % (out["ms_generator_step"], out["ms_seed"], out["ms_critic_step"], out["ms_iteration"], args.critic_iters))
    for k, v in sorted(split.items(), key=lambda kv: -kv[1]):
        print("  %-18s %.3f ms" % (k, v))
    for k, v in sorted(kernels.items(), key=lambda kv: -kv[1])[:8]:
        print("    %-44s %.3f ms" % (k, v))
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
