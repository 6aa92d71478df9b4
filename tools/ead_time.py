#!/usr/bin/env python
"""Times one dg_ead call against one dg_cw call at configs[4]'s classifier shape: the same MNIST-shaped images, the same
max_iterations, binary_search_steps 1, abort_early off, in the same process.  A short call of each warms up (workspace, code objects);
each timed call is bracketed by device events on a synchronised stream.  Prints ms per iteration and images/s for both, and the ratio.

Expectation, derived: an EAD iteration is one more classifier forward over B rows than a CW iteration (the slack and the iterate go
through one forward of 2 B rows), plus three small element-wise passes, so the ratio should stay under 2.

Measured on one MI355X (defaults: 10 000 images, 100 iterations, batch_size 128): model F 367.0 ms/iteration (272 images/s) against
dg_cw's 340.2 (294 images/s), ratio 1.079; model A 887.7 against 831.2 ms/iteration, ratio 1.068 ("Elastic net").

    python tools/ead_time.py [--models F,A] [--images 10000] [--iters 100] [--batch-size 128]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="F,A")
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=128)
    a = ap.parse_args()
    import torch
    from defensegan_amd import network_builder as nb
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, (a.images, 28, 28, 1)).astype(np.float32)).to(dev)
    for name in a.models.split(","):
        m = nb.MODELS[name]()
        m.init_like_reference(seed=ord(name))
        cw, ead = nb.CarliniWagnerL2(m), nb.ElasticNetMethod(m)
        common = dict(batch_size=a.batch_size, binary_search_steps=1, abort_early=False, initial_const=100.0)
        cw_kw = dict(common, learning_rate=10.0)
        ead_kw = dict(common, learning_rate=0.1, beta=1e-2)
        ead.generate(x, max_iterations=2, **ead_kw)
        cw.generate(x, max_iterations=2, **cw_kw)
        ms_e, (_, _, cls_e) = timed(lambda: ead.generate(x, max_iterations=a.iters, return_info=True, **ead_kw), dev)
        ms_c, (_, _, cls_c) = timed(lambda: cw.generate(x, max_iterations=a.iters, return_info=True, **cw_kw), dev)
        for what, ms, cls in (("dg_ead", ms_e, cls_e), ("dg_cw ", ms_c, cls_c)):
            print("model %s %s batch_size %d: %.1f ms total, %.3f ms/iteration, %.0f images/s, %d/%d succeeded" %
                  (name, what, a.batch_size, ms, ms / a.iters, a.images / (ms / 1e3), int((cls != -1).sum()), a.images), flush=True)
        print("model %s: dg_ead / dg_cw = %.3f per iteration" % (name, ms_e / ms_c), flush=True)
        m.close()


if __name__ == "__main__":
    main()
