#!/usr/bin/env python
"""Times one epoch of classifier training (utils_tf.model_train -> one dg_clf_train call) at whitebox's parameters (whitebox.py:
120-170: batch 128, Adam at lr 0.001) on 50 000 synthetic MNIST-shaped images already on the device, for models F, A and B with
adversarial training (fgsm_eps_tr 0.15) off and on.  A 10-step epoch of the same shape warms up first (workspace, code objects);
the timed epoch ends in a device synchronise.  Prints one line per setting: s/epoch, images/s, and the FLOPs per image from the
layer shapes (2 x multiply-adds: forward, input gradient and weight gradient per step; the adversarial half adds two forwards,
two input gradients and one weight gradient).

    python tools/train_time.py [--models F,A,B] [--adv off,on] [--images 50000]
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


def forward_flops(model):
    from defensegan_amd import network_builder as nb
    _, H, W, Cc = model.input_shape
    shape, flat, fwd = (H, W, Cc), None, 0
    for l in model.layers:
        if isinstance(l, nb.Conv2D):
            out = nb.conv_output_shape(shape, l)
            fwd += 2 * l.kernel_shape[0] * l.kernel_shape[1] * shape[2] * out[0] * out[1] * out[2]
            shape = out
        elif isinstance(l, nb.Flatten):
            flat = int(np.prod(shape))
        elif isinstance(l, nb.Linear):
            fwd += 2 * flat * l.num_hid
            flat = l.num_hid
    return fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="F,A,B")
    ap.add_argument("--adv", default="off,on")
    ap.add_argument("--images", type=int, default=50000)
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()
    import torch
    from defensegan_amd import network_builder as nb
    from defensegan_amd import utils_tf
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (a.images, 28, 28, 1)).astype(np.float32)).to(dev)
    y = rs.randint(0, 10, a.images).astype(np.int32)
    args = {"nb_epochs": 1, "batch_size": 128, "learning_rate": 0.001}
    rows = []
    for name in a.models.split(","):
        for adv in a.adv.split(","):
            eps = 0.15 if adv == "on" else None
            m = nb.MODELS[name]()
            m.init_like_reference(seed=0)
            utils_tf.model_train(m, x[:1280], y[:1280], args=args, adv_eps=eps)             # warm-up
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            utils_tf.model_train(m, x, y, args=args, adv_eps=eps)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            fwd = forward_flops(m)
            per_img = (8 if eps else 3) * fwd
            row = {"model": name, "adv_tr": bool(eps), "images": a.images, "s_per_epoch": round(dt, 3),
                   "images_per_s": round(a.images / dt, 1), "mflop_per_image": round(per_img / 1e6, 2),
                   "tflops": round(per_img * a.images / dt / 1e12, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            m.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
