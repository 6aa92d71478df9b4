#!/usr/bin/env python
"""Times the latent-space attack (network_builder.LatentAttack, dg_latent_attack) on the shipped MNIST sizes: 100 synthetic images
x R = 10 restarts x 100 Adam iterations, a Conv2D / ReLU / Linear classifier, synthetic generator weights.  Two forms of the same
schedule:

    device     ONE dg_latent_attack call (nb_iter + 1 forwards, nb_iter backwards, margin / distance / Adam / tracker on the device)
    composed   the same iteration issued from Python through the public calls: gan.generate, model.get_logits, the margin and
               the hinge's seed in torch, model.backward (dg_clf_backward), gan.generator_gradient (dg_gen_param_gradient,
               weight gradients included: the public call has no form without them), torch.optim.Adam on z, tracking in torch

Each form is warmed up with one short call of the same shape (tuning, code objects, workspaces), then timed over 5 windows with
device events; the median window is reported as ms per iteration and images per second, and the ratio composed / device.

    python tools/latent_attack_time.py [--images 100] [--rec_rr 10] [--nb_iter 100] [--windows 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def composed(gan, model, x, lab, R, nb_iter, lr, c, kappa, z0):
    """The definition of DESIGN.md section 7, one public call per step; returns (x_adv, best_iter)."""
    import torch
    N, B = int(z0.shape[0]), int(x.shape[0])
    z = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    xr = x.repeat_interleave(R, dim=0)
    rows = lab.long().repeat_interleave(R)
    idx = torch.arange(N, device=x.device)
    best_d = torch.full((B,), float("inf"), device=x.device)
    best_it = torch.full((B,), -1, dtype=torch.int32, device=x.device)
    x_adv = torch.empty_like(x)
    for k in range(nb_iter + 1):
        with torch.no_grad():
            y = gan.generate(z.detach())
            Z = model.get_logits(y)
            own = Z[idx, rows]
            other, o = Z.scatter(1, rows[:, None], float("-inf")).max(dim=1)
            m = own - other
            d = ((y - xr) ** 2).reshape(N, -1).mean(dim=1)
            # tracking: per image the success of the smallest distance so far, else the final iterate's smallest margin
            dd = torch.where(m < -kappa, d, torch.full_like(d, float("inf"))).reshape(B, R)
            dmin, r = dd.min(dim=1)
            take = dmin < best_d
            if k == nb_iter:
                none = (best_it < 0) & ~take
                r = torch.where(none, m.reshape(B, R).argmin(dim=1), r)
                take = take | none
                best_it = torch.where(take & ~none, torch.full_like(best_it, k), best_it)
            else:
                best_it = torch.where(take, torch.full_like(best_it, k), best_it)
            best_d = torch.where(take, dmin, best_d)
            pick = y.reshape(B, R, *y.shape[1:])[torch.arange(B, device=x.device), r]
            x_adv = torch.where(take[:, None, None, None], pick, x_adv)
            if k == nb_iter:
                break
            on = (m + kappa > 0).float() * c
            dl = torch.zeros_like(Z)
            dl[idx, rows] = on
            dl[idx, o] = -on
            dy = model.backward(y, dl) + (y - xr) * (2.0 / 784.0)
            _, _, dz = gan.generator_gradient(z.detach(), dy, sync=False)
        z.grad = dz
        opt.step()
    return x_adv, best_it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--rec_rr", type=int, default=10)
    ap.add_argument("--nb_iter", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    import torch
    from defensegan_amd import network_builder as nb, synth
    from defensegan_amd.gan import MnistDefenseGAN
    dev = torch.device("cuda", 0)
    gan = MnistDefenseGAN(cfg={"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": 64}, test_mode=True, rec_rr=a.rec_rr, rec_iters=200, rec_lr=10.0)
    assert gan.set_weights(synth.make_weights("mnist", seed=1234, gain=2.0, bias_range=0.1)) == []
    gan._ensure_handle()
    model = nb.MLP([nb.Conv2D(64, (5, 5), (2, 2), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(10)], device=gan._device)
    model.init_like_reference(seed=0)
    rs = np.random.RandomState(0)
    B, R, N = a.images, a.rec_rr, a.images * a.rec_rr
    x = gan.generate(torch.from_numpy((rs.standard_normal((B, 128)) / np.sqrt(128)).astype(np.float32)).to(dev))
    lab = model.get_logits(x).argmax(dim=1).to(torch.int32)
    z0 = gan.init_latents(N, seed=1)
    atk = nb.LatentAttack(model, gan)
    lr, c, kappa = 0.05, 1.0, 0.0

    def timed(fn):
        fn(2)                                               # warm-up of the same shape
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(a.nb_iter)
            e1.record()
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), out

    t_dev, out = timed(lambda n: atk.call(x, lab, R, n, lr, c, kappa, z0=z0))
    t_py, (xa, bi) = timed(lambda n: composed(gan, model, x, lab, R, n, lr, c, kappa, z0))
    row = {"images": B, "rec_rr": R, "nb_iter": a.nb_iter, "windows": a.windows,
           "device_ms_per_iteration": round(t_dev / a.nb_iter, 4), "device_images_per_s": round(B / (t_dev / 1e3), 1),
           "composed_ms_per_iteration": round(t_py / a.nb_iter, 4), "composed_images_per_s": round(B / (t_py / 1e3), 1),
           "composed_over_device": round(t_py / t_dev, 3),
           "successes_device": int((out["best_iter"] >= 0).sum()), "successes_composed": int((bi >= 0).sum())}
    print(json.dumps(row), flush=True)
    model.close()
    gan.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
