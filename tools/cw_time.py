#!/usr/bin/env python
"""Times one dg_cw call of configs[4]'s shape: 10 000 MNIST-shaped images, the white-box parameters (whitebox.py:201-209:
binary_search_steps 1, max_iterations 100, learning_rate 10, initial_const 100), models F and A (init_like_reference), batch_size
50 and 128, abort_early off (fixed work) and on.  A short call of the same shape warms up (workspace, code objects); the timed
call is bracketed by device events on a synchronised stream.  Prints one line per setting: ms per iteration, images/s and the
iteration's FLOP count from the layer shapes (forward + backward to the input; the CW kernels' elementwise work not counted).

    python tools/cw_time.py [--models F,A] [--images 10000] [--iters 100] [--batch-sizes 50,128]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def iteration_flops(model):
    """FLOPs per image of one CW iteration: 2 x (multiply-adds of the forward) for the forward, the same for the input
    gradient (every Conv2D / Linear, the first one included, is differentiated to its input)."""
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
    return 2 * fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="F,A")
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch-sizes", default="50,128")
    a = ap.parse_args()
    import torch
    from defensegan_amd import network_builder as nb
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, (a.images, 28, 28, 1)).astype(np.float32)).to(dev)
    for name in a.models.split(","):
        m = nb.MODELS[name]()
        m.init_like_reference(seed=ord(name))
        cw = nb.CarliniWagnerL2(m)
        fl = iteration_flops(m)
        for bs in [int(b) for b in a.batch_sizes.split(",")]:
            for abort in (False, True):
                kw = dict(batch_size=bs, learning_rate=10.0, binary_search_steps=1, initial_const=100.0, abort_early=abort)
                cw.generate(x, max_iterations=2, **kw)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, l2, cls = cw.generate(x, max_iterations=a.iters, return_info=True, **kw)
                e1.record()
                torch.cuda.synchronize(dev)
                ms = e0.elapsed_time(e1)
                ok = int((cls != -1).sum())
                print("model %s batch_size %d abort_early %d: %.1f ms total, %.3f ms/iteration, %.0f images/s, %.1f MFLOP/image/iteration "
                      "(%.1f TFLOP/s classifier-equivalent), %d/%d succeeded" %
                      (name, bs, abort, ms, ms / a.iters, a.images / (ms / 1e3), fl / 1e6, fl * a.images * a.iters / (ms / 1e3) / 1e12,
                       ok, a.images), flush=True)
        m.close()


if __name__ == "__main__":
    main()
