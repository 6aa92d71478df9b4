#!/usr/bin/env python
"""Times one run of the black-box flow (defensegan_amd.blackbox.blackbox) at the reference's shape on synthetic MNIST-shaped data:
oracle F trained for 10 epochs of batch 128 on 50 000 images, substitute E, holdout 150, 6 augmentations (150 -> 4800 images),
10 epochs each, lmbda 0.1, FGSM eps 0.3 on the 1850 test images behind the holdout -- once without the projection
(defense_type none, no generator) and once with it (defense_type defense_gan: the adversary's queries and the final
evaluation go through gan.reconstruct with synthetic generator weights, R = 10 restarts of L = 200 steps).  Prints one JSON line
per setting with the seconds per phase; every phase ends in a device synchronise.

    python tools/blackbox_time.py [--settings none,defense_gan] [--train 50000] [--rec_iters 200] [--rec_rr 10] [--json out.json]
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

PHASES = ("oracle training", "substitute training", "augmentation", "labelling", "attack", "evaluation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--settings", default="none,defense_gan")
    ap.add_argument("--train", type=int, default=50000, help="images the oracle trains on")
    ap.add_argument("--rec_iters", type=int, default=200)
    ap.add_argument("--rec_rr", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()
    import torch
    from defensegan_amd import blackbox, network_builder as nb, synth
    from defensegan_amd.gan import MnistDefenseGAN
    rs = np.random.RandomState(0)
    x_tr, y_tr = rs.uniform(0, 1, (a.train, 28, 28, 1)).astype(np.float32), rs.randint(0, 10, a.train)
    x_te, y_te = rs.uniform(0, 1, (2000, 28, 28, 1)).astype(np.float32), rs.randint(0, 10, 2000)
    rows = []
    for setting in a.settings.split(","):
        gan = None
        if setting == "defense_gan":
            gan = MnistDefenseGAN(cfg={"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": 64}, test_mode=True, rec_rr=a.rec_rr,
                                  rec_iters=a.rec_iters, rec_lr=10.0)
            assert gan.set_weights(synth.make_weights("mnist", seed=1234, gain=2.0, bias_range=0.1)) == []
            gan.reconstruct(x_te[:128])                                   # warm-up: tuning, code objects
        bb, sub = nb.model_f(), nb.model_e()
        for m, s in ((bb, 0), (sub, 1)):                                  # warm-up of the classifier kernels and workspaces
            m.init_like_reference(seed=s)
            m.class_gradient(x_te[:128], y_te[:128])
        torch.cuda.synchronize()
        phases = {}
        t0 = time.perf_counter()
        acc = blackbox.blackbox(gan, bb, sub, (x_tr, y_tr, x_te, y_te), defense_type=setting, phases=phases)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        row = {"setting": setting, "projection": gan is not None, "oracle_train_images": a.train,
               "rec_rr": a.rec_rr if gan else None, "rec_iters": a.rec_iters if gan else None,
               "seconds": {k: round(phases.get(k, 0.0), 3) for k in PHASES}, "total_s": round(total, 3),
               "accuracies": {k: acc[k] for k in ("bbox", "sub", "bbox_on_sub_adv_ex")}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for m in (bb, sub):
            m.close()
        if gan is not None:
            gan.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
