#!/usr/bin/env python
"""Times the saliency-map attack on 1000 MNIST-shaped images, model F (init_like_reference), theta 1, gamma 0.1 (39 iterations at most),
on the logits unless --of_probs:

  device     one dg_jsma call (attacks.SaliencyMapMethod.generate, batch_size = the image count): seconds, images/s, mean iterations,
             success rate
  composed   the same schedule composed from Python out of the calls that existed before dg_jsma: MLP.get_logits, one
             MLP.class_gradient call per class and iteration (a = the target's, b = the sum of the others'), and the frameworks' pair
             search in torch -- the [chunk, F, F] tables of sums, masks and scores, the first maximum of the flat index -- in chunks of
             --chunk images so that the tables fit memory, with one host read per iteration to learn who is still active and the active
             images gathered before every call.

A short call of the same shape warms up (workspace, code objects); every timed run is bracketed by device events on a synchronised
stream.  Prints one JSON line per figure, the ratio, and the largest difference between the two results (torch's arg-max does not
promise the first index among equal scores, and the composed b is a sum of class gradients where the device seeds one backward: an
image whose two best pairs are closer than that rounding may take another pair).

    python tools/jsma_time.py [--images 1000] [--model F] [--gamma 0.1] [--of_probs] [--chunk 32] [--skip-composed]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pair_search(a, b, dom, theta, chunk):
    """The frameworks' pair search: a, b [n, F] float32, dom [n, F] bool on the device.  (p, q, found) [n]."""
    import torch
    n, F = a.shape
    tri = torch.triu(torch.ones(F, F, dtype=torch.bool, device=a.device), 1)
    ps, qs, fs = [], [], []
    for s in range(0, n, chunk):
        aa, bb, dd = a[s:s + chunk], b[s:s + chunk], dom[s:s + chunk]
        A = aa[:, :, None] + aa[:, None, :]
        Bs = bb[:, :, None] + bb[:, None, :]
        adm = ((A > 0) & (Bs < 0)) if theta > 0 else ((A < 0) & (Bs > 0))
        adm &= dd[:, :, None] & dd[:, None, :] & tri
        S = torch.where(adm, -(A * Bs), torch.zeros_like(A)).reshape(aa.shape[0], -1)
        best, flat = S.max(dim=1)
        ps.append(flat // F)
        qs.append(flat % F)
        fs.append(best > 0)
    return torch.cat(ps), torch.cat(qs), torch.cat(fs)


def composed(m, t, target, theta=1.0, max_iters=39, lo=0.0, hi=1.0, of_probs=False, chunk=32):
    """The saliency-map schedule from the calls that existed before dg_jsma; device tensors in and out: (x_adv, iters)."""
    import torch
    n, nc = int(t.shape[0]), int(m.nb_classes)
    adv = t.clone()
    flat = adv.view(n, -1)
    dom = (t.view(n, -1) < hi) if theta > 0 else (t.view(n, -1) > lo)
    active = torch.ones(n, dtype=torch.bool, device=t.device)
    iters = torch.zeros(n, dtype=torch.int32, device=t.device)
    tgt = target.to(torch.int64)
    for _ in range(int(max_iters)):
        idx = active.nonzero().flatten()                           # the host read of the iteration
        if idx.numel() == 0:
            break
        x = adv[idx].contiguous()
        z = m.get_logits(x)
        o = torch.softmax(z, dim=1) if of_probs else z
        go = (o.argmax(dim=1) != tgt[idx]) & (dom[idx].sum(dim=1) >= 2) & ~torch.isnan(o).any(dim=1)
        active[idx] = go
        idx, x = idx[go], x[go].contiguous()
        if idx.numel() == 0:
            break
        g = torch.stack([m.class_gradient(x, torch.full((idx.numel(),), j, dtype=torch.int32, device=t.device), of_probs=of_probs)
                         .reshape(idx.numel(), -1) for j in range(nc)], dim=0)                      # [classes, n, F]
        hot = torch.nn.functional.one_hot(tgt[idx], nc).t().to(g.dtype).unsqueeze(2)                # [classes, n, 1]
        a, b = (g * hot).sum(dim=0), (g * (1 - hot)).sum(dim=0)
        p, q, found = pair_search(a, b, dom[idx], theta, chunk)
        active[idx] = found
        idx, p, q = idx[found], p[found], q[found]
        for f in (p, q):
            flat[idx, f] = torch.clamp(flat[idx, f] + theta, lo, hi)
            dom[idx, f] = False
        iters[idx] += 1
    return adv, iters


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
    ap.add_argument("--theta", type=float, default=1.0)
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--of_probs", action="store_true", help="differentiate the softmax outputs (cleverhans' default), not the logits")
    ap.add_argument("--chunk", type=int, default=32, help="images per [chunk, F, F] table of the composed pair search")
    ap.add_argument("--skip-composed", action="store_true")
    a = ap.parse_args()
    import torch
    from defensegan_amd import network_builder as nb
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, (a.images, 28, 28, 1)).astype(np.float32)).to(dev)
    m = nb.MODELS[a.model]()
    m.init_like_reference(seed=ord(a.model))
    own = m.get_logits(x).argmax(dim=1)
    r = torch.from_numpy(np.random.RandomState(1).randint(0, m.nb_classes - 1, a.images)).to(dev)
    target = ((own + 1 + r) % m.nb_classes).to(torch.int32)
    atk = nb.SaliencyMapMethod(m)
    max_iters = atk.max_iters(28 * 28, a.gamma)

    def line(what, sec, adv, iters):
        ok = m.get_logits(adv).argmax(dim=1) == target
        print(json.dumps({"what": what, "model": a.model, "images": a.images, "of_probs": bool(a.of_probs), "max_iters": max_iters,
                          "seconds": round(sec, 5), "images_per_s": round(a.images / sec, 1), "mean_iters": round(float(iters.float().mean()), 3),
                          "success_rate": round(float(ok.float().mean()), 4)}), flush=True)

    par = dict(y_target=target, theta=a.theta, gamma=a.gamma, of_probs=a.of_probs, batch_size=a.images, return_info=True)
    atk.generate(x, **dict(par, gamma=2.1 * 2 / 784))                                              # two iterations: the warm-up
    sec_d, (adv_d, it_d, _, _) = timed(lambda: atk.generate(x, **par), dev)
    line("device", sec_d, adv_d, it_d)
    if not a.skip_composed:
        composed(m, x[:64], target[:64], a.theta, 2, of_probs=a.of_probs, chunk=a.chunk)
        sec_c, (adv_c, it_c) = timed(lambda: composed(m, x, target, a.theta, max_iters, of_probs=a.of_probs, chunk=a.chunk), dev)
        line("composed", sec_c, adv_c, it_c)
        same = (adv_d == adv_c).reshape(a.images, -1).all(dim=1)
        print(json.dumps({"what": "device against composed", "composed_over_device": round(sec_c / sec_d, 2),
                          "max_abs_difference": float((adv_d - adv_c).abs().max()), "images_with_the_same_x_adv": int(same.sum()),
                          "images_with_the_same_iters": int((it_d == it_c).sum())}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
