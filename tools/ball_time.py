#!/usr/bin/env python
"""PGD on 10 000 MNIST-shaped images at nb_iter 10, ord inf and ord 2 in the same process: what the per-image norms of the L2 step
(defensegan_amd/csrc/dg_ball.hip) cost beside the L-infinity step.  Model F with fixed random weights, synthetic images; one warm-up
call per setting, then the median of --repeat timed calls (each one dg_pgd / dg_pgd_ball call, synchronised).

    python tools/ball_time.py [--images 10000] [--nb_iter 10] [--repeat 5]      -> one JSON line
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
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--nb_iter", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch
    from defensegan_amd import network_builder as nb
    m = nb.model_f()
    m.init_like_reference(seed=1)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (args.images, 28, 28, 1)).astype(np.float32)).cuda()
    y = rs.randint(0, 10, args.images).astype(np.int32)
    atk = nb.ProjectedGradientDescent(m)
    settings = {"inf": dict(eps=0.3, eps_iter=0.05), "2": dict(eps=2.0, eps_iter=0.5, ord=2)}
    out = {"images": args.images, "nb_iter": args.nb_iter, "repeat": args.repeat}
    for name, kw in settings.items():
        times = []
        for i in range(args.repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            atk.generate(x, y, nb_iter=args.nb_iter, clip_min=0.0, clip_max=1.0, **kw)
            torch.cuda.synchronize()
            if i:
                times.append(time.perf_counter() - t0)
        out["seconds_ord_" + name] = float(np.median(times))
        out["spread_ord_" + name] = [float(min(times)), float(max(times))]
    out["ord_2_over_inf"] = out["seconds_ord_2"] / out["seconds_ord_inf"]
    print(json.dumps(out))
    m.close()


if __name__ == "__main__":
    main()
