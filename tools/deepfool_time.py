#!/usr/bin/env python
"""Times DeepFool on 1000 MNIST-shaped images, model F (init_like_reference), the defaults (nb_candidate 10, overshoot 0.02, max_iter 50):

  device     one dg_deepfool call (attacks.DeepFool.generate, batch_size = the image count): seconds, images/s, mean iterations
  composed   the same schedule composed from Python out of MLP.class_gradient (one dg_clf_class_gradient call per candidate and
             iteration), MLP.get_logits and torch ops, with one host read per iteration to learn who is still active and the active
             images gathered before every call.  It uses nothing this attack added, so it runs on an older checkout as well.
  paths      (--paths) one dg_deepfool call at B = 100 through the product library (replicated rows: one backward of B nc rows) and
             through the measurement build (nc backwards of B rows): the measurement behind the choice in dg_deepfool.hip.

A short call of the same shape warms up (workspace, code objects); every timed run is bracketed by device events on a synchronised
stream.  Prints one JSON line per figure.

    python tools/deepfool_time.py [--images 1000] [--model F] [--paths] [--skip-composed]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def composed(m, t, nb_candidate=10, overshoot=0.02, max_iter=50, lo=0.0, hi=1.0):
    """DeepFool's schedule from the calls that existed before dg_deepfool; device tensors in and out: (x_adv, iters)."""
    import torch
    n = int(t.shape[0])
    z = m.get_logits(t)
    cand = torch.sort(z, dim=1, descending=True, stable=True)[1][:, :nb_candidate].to(torch.int32).contiguous()
    orig = cand[:, 0].to(torch.int64)
    r = torch.zeros_like(t)
    adv = t.clone()
    active = torch.ones(n, dtype=torch.bool, device=t.device)
    iters = torch.zeros(n, dtype=torch.int32, device=t.device)
    for _ in range(int(max_iter)):
        idx = active.nonzero().flatten()                           # the host read of the iteration
        if idx.numel() == 0:
            break
        a, c = adv[idx].contiguous(), cand[idx]
        zc = m.get_logits(a).gather(1, c.to(torch.int64))
        g = [m.class_gradient(a, c[:, j].contiguous(), of_probs=False) for j in range(nb_candidate)]
        w = (torch.stack(g[1:], dim=1) - g[0].unsqueeze(1)).reshape(idx.numel(), nb_candidate - 1, -1)
        wn = w.norm(dim=2)
        pert = torch.where(wn > 0, ((zc[:, 1:] - zc[:, :1]).abs() + 1e-5) / wn, torch.full_like(wn, float("inf")))
        best, js = pert.min(dim=1)
        rows = torch.arange(idx.numel(), device=t.device)
        r[idx] = r[idx] + ((best / wn[rows, js]).reshape(-1, 1) * w[rows, js]).reshape(a.shape)
        adv[idx] = torch.clamp(t[idx] + r[idx], lo, hi)
        iters[idx] += 1
        active[idx] = m.get_logits(adv[idx].contiguous()).argmax(dim=1) == orig[idx]
    return torch.clamp(t + (1.0 + overshoot) * r, lo, hi), iters


def timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--model", default="F")
    ap.add_argument("--paths", action="store_true", help="also time the two gradient paths at B = 100")
    ap.add_argument("--skip-composed", action="store_true")
    a = ap.parse_args()
    import torch
    from defensegan_amd import _native, network_builder as nb
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, (a.images, 28, 28, 1)).astype(np.float32)).to(dev)
    m = nb.MODELS[a.model]()
    m.init_like_reference(seed=ord(a.model))

    def line(what, sec, iters, n):
        print(json.dumps({"what": what, "model": a.model, "images": n, "seconds": round(sec, 5), "images_per_s": round(n / sec, 1),
                          "mean_iters": round(float(iters.float().mean()), 3), "max_iters": int(iters.max())}), flush=True)

    adv_dev = None
    if hasattr(nb, "DeepFool"):
        atk = nb.DeepFool(m)
        atk.generate(x, max_iter=2, batch_size=a.images)
        sec, (adv_dev, _, it, _) = timed(lambda: atk.generate(x, batch_size=a.images, return_info=True), dev)
        line("device", sec, it, a.images)
    if not a.skip_composed:
        composed(m, x[:64], max_iter=2)
        sec, (adv_c, it) = timed(lambda: composed(m, x), dev)
        line("composed", sec, it, a.images)
        if adv_dev is not None:
            print(json.dumps({"what": "device against composed", "max_abs_difference": float((adv_dev - adv_c).abs().max())}), flush=True)
    if a.paths and hasattr(nb, "DeepFool"):
        xb = x[:100].contiguous()
        for what, lib in (("replicated rows, B 100", _native.load()), ("nc backwards, B 100", _native.load(measure=True))):
            o = torch.empty_like(xb)
            it = torch.empty(100, dtype=torch.int32, device=dev)
            s = torch.cuda.current_stream(dev).cuda_stream

            def go(max_iter=50):
                _native.check(lib.dg_deepfool(m._handle, xb.data_ptr(), 100, 10, 0.02, max_iter, 0.0, 1.0, o.data_ptr(), None, it.data_ptr(), None, s), lib)
            go(2)
            best = min(timed(go, dev)[0] for _ in range(3))
            line(what, best, it, 100)
    m.close()


if __name__ == "__main__":
    main()
