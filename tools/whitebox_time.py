#!/usr/bin/env python
"""Times one run of the white-box flow (defensegan_amd.whitebox.whitebox) at the reference's shape on synthetic MNIST-shaped data:
classifier F trained for 10 epochs of batch 128 on 50 000 images, then the iterative L-infinity attack (eps 0.3, eps_iter 0.05,
nb_iter 10) on the test images and the evaluation -- once without the projection (defense_type none, attack pgd, 10 000 test
images, no generator) and once with it (defense_type defense_gan, attack bpda on 1 000 test images: every iteration and the
evaluation go through gan.reconstruct with synthetic generator weights, R = 10 restarts of L = 200 steps).  Prints one JSON line per
setting with the seconds per phase; every phase ends in a device synchronise.

    python tools/whitebox_time.py [--settings none,defense_gan] [--train 50000] [--tests 10000] [--gan_tests 1000] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ("training", "attack", "evaluation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="none,defense_gan")
    ap.add_argument("--train", type=int, default=50000, help="images the classifier trains on")
    ap.add_argument("--tests", type=int, default=10000, help="test images without the projection")
    ap.add_argument("--gan_tests", type=int, default=1000, help="test images with the projection")
    ap.add_argument("--nb_iter", type=int, default=10)
    ap.add_argument("--rec_iters", type=int, default=200)
    ap.add_argument("--rec_rr", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()
    import torch
    from defensegan_amd import network_builder as nb, synth, whitebox
    from defensegan_amd.gan import MnistDefenseGAN
    rs = np.random.RandomState(0)
    x_tr, y_tr = rs.uniform(0, 1, (a.train, 28, 28, 1)).astype(np.float32), rs.randint(0, 10, a.train)
    x_te, y_te = rs.uniform(0, 1, (a.tests, 28, 28, 1)).astype(np.float32), rs.randint(0, 10, a.tests)
    rows = []
    for setting in a.settings.split(","):
        gan, attack, n_te = None, "pgd", a.tests
        if setting == "defense_gan":
            gan = MnistDefenseGAN(cfg={"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": 64}, test_mode=True, rec_rr=a.rec_rr,
                                  rec_iters=a.rec_iters, rec_lr=10.0)
            assert gan.set_weights(synth.make_weights("mnist", seed=1234, gain=2.0, bias_range=0.1)) == []
            gan.reconstruct(x_te[:128])                                   # warm-up: tuning, code objects
            attack, n_te = "bpda", min(a.gan_tests, a.tests)
        model = nb.model_f()
        model.init_like_reference(seed=0)
        model.input_gradient(x_te[:128], labels=y_te[:128])              # warm-up of the classifier kernels and workspaces
        torch.cuda.synchronize()
        phases = {}
        t0 = time.perf_counter()
        acc, _, _ = whitebox.whitebox(gan, model, (x_tr, y_tr, x_te[:n_te], y_te[:n_te]), attack_type=attack, defense_type=setting,
                                      attack_params={"nb_iter": a.nb_iter}, phases=phases)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        row = {"setting": setting, "attack": attack, "train_images": a.train, "test_images": n_te, "nb_iter": a.nb_iter,
               "rec_rr": a.rec_rr if gan else None, "rec_iters": a.rec_iters if gan else None,
               "seconds": {k: round(phases.get(k, 0.0), 3) for k in PHASES}, "total_s": round(total, 3), "accuracy_under_attack": acc}
        rows.append(row)
        print(json.dumps(row), flush=True)
        model.close()
        if gan is not None:
            gan.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
