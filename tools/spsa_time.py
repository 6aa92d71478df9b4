#!/usr/bin/env python
"""Times one SPSA attack (network_builder.SPSA) on the DEFENDED model: model F (init_like_reference) behind the projection with
synthetic generator weights, 20 synthetic MNIST-shaped images, R = 10 restarts of L = 200 steps, spsa_samples = 32, 5 iterations --
5 x 65 + 1 = 326 projected queries per image.  The run is a child process under `timeout -k 10`; nothing is retried.  The child
warms up with a one-iteration attack of the same shape (tuning, code objects, workspaces), then brackets the timed attack with
device events and every projection inside it with a pair of its own; it prints one JSON line: the seconds, the queries per second
and the share of the time spent outside dg_reconstruct (the two SPSA kernels, the classifier, tracking, the host loop).

    python tools/spsa_time.py [--images 20] [--nb_iter 5] [--spsa_samples 32] [--rec_rr 10] [--rec_iters 200] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(a):
    import torch
    from defensegan_amd import network_builder as nb, synth
    from defensegan_amd.gan import MnistDefenseGAN
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.uniform(0, 1, (a.images, 28, 28, 1)).astype(np.float32)).to(dev)
    y = rs.randint(0, 10, a.images)
    gan = MnistDefenseGAN(cfg={"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": 64}, test_mode=True, rec_rr=a.rec_rr, rec_iters=a.rec_iters,
                          rec_lr=10.0)
    assert gan.set_weights(synth.make_weights("mnist", seed=1234, gain=2.0, bias_range=0.1)) == []
    m = nb.model_f()
    m.init_like_reference(seed=ord("F"))
    m.add_rec_model(gan, None, 50)

    class Timed(nb.SpsaDeviceOps):
        pairs = []

        def project(self, q, seed, first_row, row_step=None):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rec = super().project(q, seed, first_row, row_step)
            e1.record()
            self.pairs.append((e0, e1))
            return rec
    ops = Timed(m)
    atk = nb.SPSA(m, ops=ops)
    kw = dict(eps=0.3, eps_iter=0.05, spsa_samples=a.spsa_samples, delta=0.01, clip_min=0.0, clip_max=1.0, seed=1)
    atk.generate(x, y, nb_iter=1, **kw)
    torch.cuda.synchronize(dev)
    del ops.pairs[:]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    _, first, queries = atk.generate(x, y, nb_iter=a.nb_iter, return_info=True, **kw)
    t1.record()
    torch.cuda.synchronize(dev)
    total = t0.elapsed_time(t1) / 1e3
    proj = sum(e0.elapsed_time(e1) for e0, e1 in ops.pairs) / 1e3
    row = {"images": a.images, "nb_iter": a.nb_iter, "spsa_samples": a.spsa_samples, "rec_rr": a.rec_rr, "rec_iters": a.rec_iters,
           "queries_per_image": queries, "engine_calls": len(ops.pairs), "seconds": round(total, 3),
           "queries_per_s": round(a.images * queries / total, 1), "seconds_in_dg_reconstruct": round(proj, 3),
           "share_outside_dg_reconstruct": round(1.0 - proj / total, 4), "images_with_a_successful_iterate": int((first > 0).sum())}
    print(json.dumps(row), flush=True)
    m.close()
    gan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--nb_iter", type=int, default=5)
    ap.add_argument("--spsa_samples", type=int, default=32)
    ap.add_argument("--rec_rr", type=int, default=10)
    ap.add_argument("--rec_iters", type=int, default=200)
    ap.add_argument("--limit", type=int, default=300, help="seconds the run may take before it is ended")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "1", "--images", str(a.images),
           "--nb_iter", str(a.nb_iter), "--spsa_samples", str(a.spsa_samples), "--rec_rr", str(a.rec_rr), "--rec_iters", str(a.rec_iters)]
    rc = subprocess.call(cmd)
    if rc != 0:
        print("exit status %d" % rc, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
