"""float64 reference of the latent-space attack (defensegan_amd/csrc/dg_latent.hip), written from its definition (DESIGN.md section
7, "The latent-space attack") and independently of the device code: the generator is ``oracle.torch_ref.TorchGenerator`` through
tests/support/generator_reference.py, the classifier a few lines of torch here, every gradient autograd's, Adam
``critic_reference.adam_update``, the tracker plain NumPy.

    one iteration   y = G(z), Z = logits(y), m = Z[label] - max_{c != label} Z[c] (first maximum, index o),
                    d = mean_pixels (y - x)^2, f = d + c max(m + kappa, 0), dz = d(sum_j f_j)/dz, z <- Adam(z, dz)
    tracker         a row (k, r) succeeds when m < -kappa; per image the success of the smallest d (ties: earliest k, then
                    smallest r); with none, the smallest-margin row of the final iterate (smallest r) and best_iter = -1

Recorded draws (CASES): generator weights are generator_reference.weights(latent, 64); a case's (classifier seed, draw seed) is the
first pair ``find_case`` accepts: for every teacher-forced step k = 0, 1, 2 of the float64 run, a float32 CPU run of the same step
from the same z_k agrees with float64 on every ReLU gate of the generator and the classifier, on o_j and on the sign of
m_j + kappa, and float32 alone uses at most HALF of each bound the GPU test applies (dz: 1e-4 of the largest entry; margin, dist:
1e-5 relative), and no margin is a cancellation of more than MAX_CONDITION = 10: (|Z[label]| + |Z[o]|) / |m| stays below it
(the cases of MARGIN_ABS take an absolute margin bound instead and have no cancellation rule: see there).  tests/test_latent_cpu.py re-derives every recorded pair; no device output is stored anywhere.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.support import critic_reference as CR
from tests.support import generator_reference as GR

DZ_TOL, SCALAR_TOL = 1e-4, 1e-5
KINDS = {
    # a three-class classifier of one Linear layer
    "lin3": [("flatten",), ("linear", 3)],
    # two classes, the fewest the attack accepts: o is the only other class
    "lin2": [("flatten",), ("linear", 2)],
    # Conv2D / ReLU / Linear, 10 classes: the convolution of generator_reference.fixed_critic (8 channels, 5x5, stride 2, SAME)
    "conv10": [("conv", 8, (5, 5), (2, 2), "SAME"), ("relu",), ("flatten",), ("linear", 10)],
}
# teacher-forced cases: name -> (latent, classifier kind, B, R, c, kappa); lr, betas as the attack's defaults
CASES = {
    "conv_3x2": (128, "conv10", 3, 2, 1.0, 0.5),
    "lin_7x1_l64": (64, "lin3", 7, 1, 1.0, 0.0),
    "conv_1x1": (128, "conv10", 1, 1, 1.0, 0.0),
    "lin_1x10": (128, "lin3", 1, 10, 2.0, 0.25),
}
# Cases whose margin takes the ABSOLUTE bound.  The margin is the difference of two logits, each a float32 sum of 784 products, and
# cannot be more exact than they are: MARGIN_ABS_TOL of |Z[label]| + |Z[o]| (1e-6: a tenth of the relative bound at its largest
# admitted cancellation of 10, so never wider than the relative bound on the draws that rule admits).  With ten restarts of one image
# some margin always nearly cancels -- where an attack's margin crosses zero -- and no draw among 16 x 16 seeds meets the
# cancellation rule; under this bound those rows are checked, not excluded.
MARGIN_ABS = ("lin_1x10",)
MARGIN_ABS_TOL = 1e-6
# name -> the first (classifier seed, draw seed) find_case accepts (tests/test_latent_cpu.py re-derives each)
SEEDS = {"conv_3x2": (8, 4), "lin_7x1_l64": (6, 4), "conv_1x1": (0, 0), "lin_1x10": (1, 5)}
# shares of the (dz, margin, dist) bounds that float32 on the CPU uses for the recorded draws, as found with them (one machine):
# conv_3x2 0.010 / 0.129 / 0.012, lin_7x1_l64 0.011 / 0.213 / 0.010, conv_1x1 0.008 / 0.110 / 0.007, lin_1x10 0.011 / 0.233 (of its absolute bound) / 0.013.
LR, BETA1, BETA2 = 0.05, 0.9, 0.999
MAX_SEEDS = 16
MAX_SHARE = 0.5
MAX_CONDITION = 10.0
# the attack of the "it attacks" test: 10-class classifier, B = 8, R = 2, 30 iterations
ATTACK = dict(latent=128, kind="conv10", B=8, R=2, nb_iter=30, c=1.0, kappa=0.0, lr=0.05)
ATTACK_SEED = 0


def _same(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def classifier(kind, seed):
    """(layers, [(W, b)]) float32 arrays in the reference layouts ([kh,kw,cin,cout], [in,out]); unit-variance logits, small biases."""
    rs = np.random.RandomState(1000 + seed)
    layers, params, shape, flat = KINDS[kind], [], (28, 28, 1), None
    for L in layers:
        if L[0] == "conv":
            (kh, kw), (sh, sw) = L[2], L[3]
            W = rs.standard_normal((kh, kw, shape[2], L[1])) / np.sqrt(kh * kw * shape[2])
            params.append((W.astype(np.float32), rs.uniform(-0.1, 0.1, L[1]).astype(np.float32)))
            shape = (-(-shape[0] // sh), -(-shape[1] // sw), L[1])
        elif L[0] == "flatten":
            flat = int(np.prod(shape))
        elif L[0] == "linear":
            W = 4.0 * rs.standard_normal((flat, L[1])) / np.sqrt(flat)
            params.append((W.astype(np.float32), rs.uniform(-0.1, 0.1, L[1]).astype(np.float32)))
            flat = L[1]
    return layers, params


def mlp_layers(kind):
    """The same classifier as network_builder layers."""
    from defensegan_amd import network_builder as nb
    out = []
    for L in KINDS[kind]:
        out.append({"conv": lambda: nb.Conv2D(L[1], L[2], L[3], L[4]), "relu": nb.ReLU, "flatten": nb.Flatten,
                    "linear": lambda: nb.Linear(L[1])}[L[0]]())
    return out


def logits(layers, params, y, dtype=torch.float64, pre=None):
    """y [N,28,28,1] tensor -> Z [N, classes]; ``pre`` receives every ReLU's input."""
    h, it = y, iter(params)
    for L in layers:
        if L[0] == "conv":
            W, b = next(it)
            (kh, kw), (sh, sw) = L[2], L[3]
            t = h.permute(0, 3, 1, 2)
            if L[4] == "SAME":
                pt, pb = _same(t.shape[2], kh, sh)
                pl, pr = _same(t.shape[3], kw, sw)
                t = F.pad(t, (pl, pr, pt, pb))
            W = torch.as_tensor(np.asarray(W, np.float64)).to(dtype)
            h = F.conv2d(t, W.permute(3, 2, 0, 1), torch.as_tensor(np.asarray(b, np.float64)).to(dtype), stride=(sh, sw)).permute(0, 2, 3, 1)
        elif L[0] == "linear":
            W, b = next(it)
            h = h @ torch.as_tensor(np.asarray(W, np.float64)).to(dtype) + torch.as_tensor(np.asarray(b, np.float64)).to(dtype)
        elif L[0] == "relu":
            if pre is not None:
                pre.append(h.detach().double().numpy())
            h = torch.relu(h)
        elif L[0] == "flatten":
            h = h.reshape(h.shape[0], -1)
        else:
            raise ValueError(L)
    return h


def margin_of(Z, labels):
    """(m [N], o [N]) from logits Z [N, n] (NumPy) and the per-row labels: o = the FIRST maximum among the other classes."""
    Z = np.asarray(Z)
    N, n = Z.shape
    m, o = np.empty(N, Z.dtype), np.empty(N, np.int64)
    for j in range(N):
        best, oj = None, -1
        for c in range(n):
            if c == labels[j]:
                continue
            if oj < 0 or Z[j, c] > best:
                best, oj = Z[j, c], c
        m[j], o[j] = Z[j, labels[j]] - best, oj
    return m, o


def hinge_seed(m, o, labels, n, c, kappa):
    """dlogits [N, n]: (+c at the label, -c at o) where m + kappa > 0, else all zero."""
    g = np.zeros((len(m), n), np.float64)
    for j in range(len(m)):
        if m[j] + kappa > 0:
            g[j, labels[j]] += c
            g[j, o[j]] -= c
    return g


def iteration(gen_params, clf, x, labels, R, z, c, kappa, dtype=torch.float64):
    """One evaluated iterate at z [B R, latent]: dict of y, Z, margin, other, dist, f, dlogits, dy, dz (arrays, float64 views of
    ``dtype`` arithmetic), and the ReLU inputs of both networks (gates).  dz = d(sum_j f_j)/dz by autograd."""
    layers, cparams = clf
    g = GR._gen(gen_params, dtype)
    rows = np.repeat(np.asarray(labels, np.int64), R)
    xt = torch.as_tensor(np.asarray(x, np.float64)).to(dtype).repeat_interleave(R, dim=0)
    zt = torch.as_tensor(np.asarray(z, np.float64)).to(dtype).clone().requires_grad_(True)
    y = g.forward(zt)
    y.retain_grad()
    pre = []
    Z = logits(layers, cparams, y, dtype, pre)
    m_np, o = margin_of(Z.detach().numpy(), rows)
    idx = torch.arange(len(rows))
    m = Z[idx, torch.as_tensor(rows)] - Z[idx, torch.as_tensor(o)]
    d = ((y - xt) ** 2).reshape(len(rows), -1).mean(dim=1)
    active = torch.as_tensor((m_np + kappa > 0).astype(np.float64)).to(dtype)
    f = d + c * (m + kappa) * active
    f.sum().backward()
    return {"y": y.detach().double().numpy(), "Z": Z.detach().double().numpy(), "margin": m.detach().double().numpy(), "other": o,
            "dist": d.detach().double().numpy(), "f": f.detach().double().numpy(),
            "dlogits": hinge_seed(m_np, o, rows, Z.shape[1], c, kappa), "dy": y.grad.double().numpy(), "dz": zt.grad.double().numpy(),
            "gates": [a for a in GR.preacts(gen_params, np.asarray(z, np.float64), dtype)] + pre}


def track(margins, dists, kappa):
    """The tracker on the sequences margins, dists [K, B, R] of the evaluated iterates (the last one is the final iterate):
    (best_dist, best_margin, best_iter, best_row), each [B].

    Non-finite values:
      - a row whose margin is NaN is never a success and never the smallest margin;
      - a successful row whose distance is NaN is never taken (an image whose only successes have NaN distances has no success
        and takes the no-success branch, where that row may well hold the smallest margin);
      - if every margin of the final iterate is NaN, the result is row 0 (of the final iterate, best_iter = -1);
      - +inf distances and margins compare as numbers (an +inf distance is taken while there is no success yet, an +inf margin is
        the smallest only among +inf and NaN margins: the smallest r of the +inf ones)."""
    margins, dists = np.asarray(margins), np.asarray(dists)
    K, B, R = margins.shape
    bd, bm = np.empty(B, margins.dtype), np.empty(B, margins.dtype)
    bi, br = np.full(B, -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        for k in range(K):
            for r in range(R):
                d = dists[k, b, r]
                if margins[k, b, r] < -kappa and d == d and (bi[b] < 0 or d < bd[b]):
                    bd[b], bm[b], bi[b], br[b] = d, margins[k, b, r], k, r
        if bi[b] < 0:
            r = -1
            for q in range(R):
                mq = margins[K - 1, b, q]
                if mq == mq and (r < 0 or mq < margins[K - 1, b, r]):
                    r = q
            r = max(r, 0)
            bd[b], bm[b], br[b] = dists[K - 1, b, r], margins[K - 1, b, r], r
    return bd, bm, bi, br


def run(gen_params, clf, x, labels, R, z0, nb_iter, lr=LR, c=1.0, kappa=0.0, b1=BETA1, b2=BETA2):
    """The whole attack in float64: z [nb_iter + 1, N, latent] (z[k] = the iterate judged by forward k), the steps' dicts, the
    traces margin, dist [nb_iter + 1, N], and the tracker's result with x_adv."""
    z = np.asarray(z0, np.float64)
    m, v = np.zeros_like(z), np.zeros_like(z)
    zs, its = [], []
    for k in range(nb_iter + 1):
        it = iteration(gen_params, clf, x, labels, R, z, c, kappa)
        zs.append(z)
        its.append(it)
        if k < nb_iter:
            z, m, v = CR.adam_update(z, it["dz"], m, v, k + 1, lr, b1, b2)
    B = len(labels)
    margin = np.stack([it["margin"] for it in its])
    dist = np.stack([it["dist"] for it in its])
    bd, bm, bi, br = track(margin.reshape(-1, B, R), dist.reshape(-1, B, R), kappa)
    x_adv = np.stack([its[bi[b] if bi[b] >= 0 else nb_iter]["y"][b * R + br[b]] for b in range(B)])
    return {"z": np.stack(zs), "steps": its, "margin": margin, "dist": dist, "best_dist": bd, "best_margin": bm, "best_iter": bi,
            "best_row": br, "x_adv": x_adv}


# ---------------------------------------------------------------------- recorded draws
def draw(latent, B, R, seed):
    """(x [B,28,28,1] in (0, 1), labels [B] filled by the caller's class count, z0 [B R, latent] at the projection's std)."""
    rs = np.random.RandomState(5000 + seed)
    x = (1.0 / (1.0 + np.exp(-rs.standard_normal((B, 28, 28, 1))))).astype(np.float32)
    z0 = (rs.standard_normal((B * R, latent)) / np.sqrt(latent)).astype(np.float32)
    return x, rs.randint(0, 1 << 30, B), z0


def margin_scale(it, labels, R, absolute):
    """Per row what the margin's error is measured against: SCALAR_TOL |m|, or MARGIN_ABS_TOL (|Z[label]| + |Z[o]|)."""
    rows = np.arange(len(it["margin"]))
    lab = np.repeat(np.asarray(labels, np.int64), R)
    if absolute:
        return MARGIN_ABS_TOL * (np.abs(it["Z"][rows, lab]) + np.abs(it["Z"][rows, it["other"]]))
    return SCALAR_TOL * np.abs(it["margin"])


def shares(gen_params, clf, x, labels, R, z, c, kappa, absolute=False):
    """What float32 on the CPU costs at z against float64, as shares of the GPU test's bounds (dz, margin, dist), or None where
    the two disagree on a gate, on o_j or on the sign of m_j + kappa (or a gate lies within 1e-6 of zero)."""
    a = iteration(gen_params, clf, x, labels, R, z, c, kappa, torch.float64)
    b = iteration(gen_params, clf, x, labels, R, z, c, kappa, torch.float32)
    for p, q in zip(a["gates"], b["gates"]):
        if np.abs(p).min() <= GR.MIN_MARGIN or ((p > 0) != (q > 0)).any():
            return None
    if (a["other"] != b["other"]).any() or ((a["margin"] + kappa > 0) != (b["margin"] + kappa > 0)).any():
        return None
    if (np.abs(a["margin"] + kappa) <= GR.MIN_MARGIN).any():
        return None
    # the margin is a difference of two logits: a relative bound on it is a bound on float32 arithmetic only while the cancellation
    # stays small (critic_reference.conditioning's rule: at 10, 1e-5 of the margin is 1e-6 of the logits it is formed from)
    rows = np.arange(len(a["margin"]))
    lab = np.repeat(np.asarray(labels, np.int64), R)
    if not absolute and ((np.abs(a["Z"][rows, lab]) + np.abs(a["Z"][rows, a["other"]])) / np.abs(a["margin"]) > MAX_CONDITION).any():
        return None
    return (float(np.abs(a["dz"] - b["dz"]).max() / (DZ_TOL * np.abs(a["dz"]).max())),
            float((np.abs(a["margin"] - b["margin"]) / margin_scale(a, labels, R, absolute)).max()),
            float((np.abs(a["dist"] - b["dist"]) / (SCALAR_TOL * np.abs(a["dist"]))).max()))


@functools.lru_cache(maxsize=None)
def case_inputs(name, clf_seed, draw_seed):
    latent, kind, B, R, c, kappa = CASES[name]
    clf = classifier(kind, clf_seed)
    x, _, z0 = draw(latent, B, R, draw_seed)
    gp = GR.weights(latent, 64)
    # the label of an image = the classifier's float64 prediction on its FIRST restart's G(z0): that row starts with m > 0, so the
    # classification term and the classifier's backward are in play from step 0
    y0 = GR._gen(gp, torch.float64).forward(torch.as_tensor(z0[::R].astype(np.float64)))
    labels = logits(clf[0], clf[1], y0).argmax(dim=1).numpy().astype(np.int32)
    return gp, clf, x, labels, z0


def accepted_case(name, clf_seed, draw_seed, steps=3):
    """The worst shares over the teacher-forced steps k < ``steps`` of the float64 run, or None (see the module docstring)."""
    latent, kind, B, R, c, kappa = CASES[name]
    gp, clf, x, labels, z0 = case_inputs(name, clf_seed, draw_seed)
    ref = run(gp, clf, x, labels, R, z0, steps, c=c, kappa=kappa)
    worst = np.zeros(3)
    for k in range(steps):
        s = shares(gp, clf, x, labels, R, ref["z"][k], c, kappa, name in MARGIN_ABS)
        if s is None or max(s) > MAX_SHARE:
            return None
        worst = np.maximum(worst, s)
    return tuple(float(w) for w in worst)


def find_case(name):
    """The first (classifier seed, draw seed), draw seeds innermost, that accepted_case accepts, with its shares."""
    for cs in range(MAX_SEEDS):
        for ds in range(MAX_SEEDS):
            s = accepted_case(name, cs, ds)
            if s is not None:
                return (cs, ds), s
    raise AssertionError("no accepted (classifier seed, draw seed) for %s" % name)


# ---------------------------------------------------------------------- the attack that has to succeed
@functools.lru_cache(maxsize=None)
def attack_inputs(seed):
    """x = G(z_true) of the synthetic generator, labels = the classifier's own float64 predictions on it, z0 a fresh draw."""
    a = ATTACK
    gp, clf = GR.weights(a["latent"], 64), classifier(a["kind"], seed)
    rs = np.random.RandomState(7000 + seed)
    z_true = (rs.standard_normal((a["B"], a["latent"])) / np.sqrt(a["latent"])).astype(np.float32)
    x = GR._gen(gp, torch.float64).forward(torch.as_tensor(z_true.astype(np.float64)))
    labels = logits(clf[0], clf[1], x).argmax(dim=1).numpy().astype(np.int32)
    z0 = (rs.standard_normal((a["B"] * a["R"], a["latent"])) / np.sqrt(a["latent"])).astype(np.float32)
    return gp, clf, x.numpy().astype(np.float32), labels, z0


@functools.lru_cache(maxsize=None)
def attack_reference(seed):
    a = ATTACK
    gp, clf, x, labels, z0 = attack_inputs(seed)
    return run(gp, clf, x, labels, a["R"], z0, a["nb_iter"], lr=a["lr"], c=a["c"], kappa=a["kappa"])


# ---------------------------------------------------------------------- many rows: selected, not searched (tests/test_gpu_latent_regimes.py)
# A batch of 260 rows is never accepted whole by ``shares`` (its number of gates grows with the rows), but the attack has no
# reduction across rows: a row's y, Z, m, d and dz depend on that row's (x_i, label_i, z_j) alone, so rows can be selected, as
# generator_reference.draw_rows selects them for the generator's training step.
# name -> latent, classifier kind, B, R, c, kappa, labels (None: drawn), classifier seed, draw seed.  The draw seed is the first one, at
# classifier seed 0, for which the case is served within the pool cap AND float32 on the CPU uses at most MAX_SHARE of each bound
# (find_case's rule; the margin's bound is the tight one: draw seeds 0, 1, 2 of lin2_3x3 measure 1.16, 1.01, 1.82 of it and seed 0 of
# lin_130x2_l64 0.58 -- the float32 error of a logit, about 1e-6, against 1e-5 of a margin of a few tenths).  As found (one machine):
# conv_4x65 0.009 / 0.112 / 0.016 of the dz / margin / dist bounds from a pool of 4 blocks, lin_130x2_l64 0.008 / 0.489 / 0.018 from
# 9 blocks, lin2_3x3 0.010 / 0.479 / 0.013 from 2 blocks.  tests/test_latent_regimes_cpu.py re-checks each.
REGIME_CASES = {
    # row 256 = the first thread of the margin kernel's second workgroup, restart 61 of image 3; labels hold classes 0 and 9
    "conv_4x65": dict(latent=128, kind="conv10", B=4, R=65, c=1.0, kappa=1.0, labels=(0, 5, 3, 9), clf_seed=0, seed=0),
    # many images, few restarts
    "lin_130x2_l64": dict(latent=64, kind="lin3", B=130, R=2, c=1.0, kappa=0.25, labels=None, clf_seed=0, seed=1),
    # two classes
    "lin2_3x3": dict(latent=128, kind="lin2", B=3, R=3, c=1.0, kappa=0.0, labels=(0, 1, 0), clf_seed=0, seed=3),
}
REGIME_STEPS = 2            # teacher-forced steps k = 0, 1


def _row_eval(gp, clf, x_rows, lab_rows, z, c, kappa, dtype, want_dz=False):
    """One forward (and, with want_dz, backward) of the rows z [n, latent] in ``dtype`` arithmetic: per-row nearest-to-zero
    pre-activation of every ReLU layer (generator: Linear, Generator.2, Generator.3; then the classifier's), the signs' bytes, Z, m,
    o, and dz.  The generator's layers are restated as generator_reference.preacts restates them; ``regime_case`` checks the y of
    the selected rows against TorchGenerator.forward through ``iteration``."""
    layers, cparams = clf
    g = GR._gen(gp, dtype)
    n = len(z)
    zt = torch.as_tensor(np.asarray(z, np.float64)).to(dtype).clone().requires_grad_(want_dz)
    gates = []
    a = zt @ g.W + g.b
    gates.append(a)
    h = torch.relu(a).view(-1, 4, 4, g.W.shape[1] // 16).permute(0, 3, 1, 2)
    for (w, b, used, act, _bn) in g.layers:
        hin = h.shape[-1]
        a = F.conv_transpose2d(h, w, bias=b, stride=2, padding=1)[..., :2 * hin, :2 * hin]
        if act == "relu":
            gates.append(a[..., :used, :used])
            h = torch.relu(a)[..., :used, :used]
        else:
            h = torch.sigmoid(a)
    y = h.permute(0, 2, 3, 1)
    pre = []
    Z = logits(layers, cparams, y, dtype, pre)
    gates = [t.detach().double().numpy().reshape(n, -1) for t in gates] + [p.reshape(n, -1) for p in pre]
    Zn = Z.detach().double().numpy()
    m, o = margin_of(Zn, lab_rows)
    out = {"gates": gates, "Z": Zn, "margin": m, "other": o, "y": y.detach().double().numpy()}
    if want_dz:
        idx = torch.arange(n)
        xt = torch.as_tensor(np.asarray(x_rows, np.float64)).to(dtype)
        mt = Z[idx, torch.as_tensor(np.asarray(lab_rows, np.int64))] - Z[idx, torch.as_tensor(o)]
        d = ((y - xt) ** 2).reshape(n, -1).mean(dim=1)
        active = torch.as_tensor((m + kappa > 0).astype(np.float64)).to(dtype)
        (d + c * (mt + kappa) * active).sum().backward()
        out["dz"] = zt.grad.double().numpy()
    return out


def _runner_up_gap(Z, lab_rows, o):
    """Per row Z[o] - (the largest logit among the classes other than the label and o); +inf with two classes."""
    Z = np.array(Z, np.float64)
    rows = np.arange(len(Z))
    top = Z[rows, o].copy()
    Z[rows, lab_rows] = -np.inf
    Z[rows, o] = -np.inf
    return top - Z.max(axis=1)


def regime_draw(name):
    """(x [B,28,28,1], labels [B] int32, rs): the images and labels of a regime case and the stream its z blocks are drawn from."""
    p = REGIME_CASES[name]
    rs = np.random.RandomState(9000 + p["seed"])
    x = (1.0 / (1.0 + np.exp(-rs.standard_normal((p["B"], 28, 28, 1))))).astype(np.float32)
    n = KINDS[p["kind"]][-1][1]
    labels = np.asarray(p["labels"], np.int32) if p["labels"] is not None else rs.randint(0, n, p["B"]).astype(np.int32)
    return x, labels, rs


def regime_scale(it, lab_rows):
    """Per row what the margin's error is measured against: SCALAR_TOL |m| where the cancellation (|Z[label]| + |Z[o]|) / |m| is at
    most MAX_CONDITION, MARGIN_ABS_TOL (|Z[label]| + |Z[o]|) otherwise (the two meet at MAX_CONDITION).  Returns (scale, absolute)."""
    rows = np.arange(len(it["margin"]))
    mag = np.abs(it["Z"][rows, lab_rows]) + np.abs(it["Z"][rows, it["other"]])
    absolute = mag > MAX_CONDITION * np.abs(it["margin"])
    return np.where(absolute, MARGIN_ABS_TOL * mag, SCALAR_TOL * np.abs(it["margin"])), absolute


@functools.lru_cache(maxsize=None)
def regime_case(name):
    """The selected B x R batch of a regime case, its teacher-forced states and float64 iterations.

    The pool grows by blocks of B R rows drawn at the projection's std from one stream; row q of a block is a candidate restart of
    image q // R.  A candidate is judged at both teacher-forced steps: at z_0 = its draw and at z_1 = float32(Adam in float64 from
    z_0 with the float64 dz).  It is kept when, at both,
      - float64 and float32 on the CPU agree on every ReLU gate of the generator and the classifier, on o_j and on the sign of
        m_j + kappa, and
      - every float64 gate value lies farther from zero than ROW_MARGIN_FACTOR times the largest |float32 - float64| difference
        of its layer over the pool (generator_reference._select_rows's rule); m_j + kappa is treated as one more gate with the
        margins' differences, and Z[o] stands above the next other logit by more than ROW_MARGIN_FACTOR times twice the largest
        logit difference.
    Image i takes its first R kept candidates.  At most ROW_POOL_CAP blocks are drawn: this is a condition, not a tuning knob.

    Returns gp, clf, x, labels, lab_rows, R, c, kappa, z / m / v [2] float32 (the states the device is given at k = 0, 1), its [2]
    (``iteration`` in float64 at those float32 z), scale / absolute [2] (``regime_scale``), shares [3] (float32 on the CPU as
    shares of the dz / margin / dist bounds, the worst over both steps), info (pool, blocks, kept, hinge_on [2])."""
    p = REGIME_CASES[name]
    B, R, c, kappa, latent = p["B"], p["R"], p["c"], p["kappa"], p["latent"]
    N = B * R
    gp, clf = GR.weights(latent, 64), classifier(p["kind"], p["clf_seed"])
    x, labels, rs = regime_draw(name)
    lab_rows = np.repeat(labels.astype(np.int64), R)
    x_rows = np.repeat(x.astype(np.float64), R, axis=0)
    zero = np.zeros((N, latent))
    pool_z, near, agree, diffs = [], [], [], None
    for blocks in range(1, GR.ROW_POOL_CAP + 1):
        z0 = (rs.standard_normal((N, latent)) / np.sqrt(latent)).astype(np.float32)
        a = _row_eval(gp, clf, x_rows, lab_rows, z0, c, kappa, torch.float64, want_dz=True)
        z1 = CR.adam_update(z0.astype(np.float64), a["dz"], zero, zero, 1, LR, BETA1, BETA2)[0].astype(np.float32)
        blk_near, blk_agree, blk_diff = [], np.ones(N, bool), []
        for zk, a64 in ((z0, a), (z1, None)):
            if a64 is None:
                a64 = _row_eval(gp, clf, x_rows, lab_rows, zk, c, kappa, torch.float64)
            a32 = _row_eval(gp, clf, x_rows, lab_rows, zk, c, kappa, torch.float32)
            for g64, g32 in zip(a64["gates"], a32["gates"]):
                blk_near.append(np.abs(g64).min(axis=1))
                blk_diff.append(float(np.abs(g64 - g32).max()))
                blk_agree &= ((g64 > 0) == (g32 > 0)).all(axis=1)
            blk_near.append(np.abs(a64["margin"] + kappa))
            blk_diff.append(float(np.abs(a64["margin"] - a32["margin"]).max()))
            blk_near.append(_runner_up_gap(a64["Z"], lab_rows, a64["other"]))
            blk_diff.append(2.0 * float(np.abs(a64["Z"] - a32["Z"]).max()))
            blk_agree &= (a64["other"] == a32["other"]) & ((a64["margin"] + kappa > 0) == (a32["margin"] + kappa > 0))
        pool_z.append(z0)
        near.append(np.stack(blk_near))
        agree.append(blk_agree)
        # the two steps share one margin per layer
        half = len(blk_diff) // 2
        d = np.maximum(blk_diff[:half], blk_diff[half:])
        diffs = d if diffs is None else np.maximum(diffs, d)
        margins = GR.ROW_MARGIN_FACTOR * np.concatenate([diffs, diffs])
        keep = np.stack(agree) & (np.stack(near) > margins[None, :, None]).all(axis=1)          # [blocks, N]
        per_image = keep.reshape(blocks, B, R).transpose(1, 0, 2).reshape(B, blocks * R)         # image i: block-major candidates
        if (per_image.sum(axis=1) >= R).all():
            break
    else:
        raise AssertionError("%s: %d blocks of %d rows do not yield %d kept restarts for every image" % (name, GR.ROW_POOL_CAP, N, R))
    zs = np.stack(pool_z).reshape(blocks, B, R, latent).transpose(1, 0, 2, 3).reshape(B, blocks * R, latent)
    z0 = np.ascontiguousarray(np.stack([zs[i][np.flatnonzero(per_image[i])[:R]] for i in range(B)]).reshape(N, latent))
    # the teacher-forced states and the float64 iterations, through ``iteration`` (TorchGenerator.forward, autograd)
    it0 = iteration(gp, clf, x, labels, R, z0.astype(np.float64), c, kappa)
    z1, m1, v1 = CR.adam_update(z0.astype(np.float64), it0["dz"], zero, zero, 1, LR, BETA1, BETA2)
    z = [z0, z1.astype(np.float32)]
    m = [np.zeros((N, latent), np.float32), m1.astype(np.float32)]
    v = [np.zeros((N, latent), np.float32), v1.astype(np.float32)]
    its = [it0, iteration(gp, clf, x, labels, R, z[1].astype(np.float64), c, kappa)]
    assert np.abs(its[0]["y"] - _row_eval(gp, clf, x_rows, lab_rows, z0, c, kappa, torch.float64)["y"]).max() <= 1e-12
    scale, absolute, worst, hinge_on = [], [], np.zeros(3), []
    for k in range(REGIME_STEPS):
        a, b = its[k], iteration(gp, clf, x, labels, R, z[k].astype(np.float64), c, kappa, torch.float32)
        for g64, g32 in zip(a["gates"], b["gates"]):
            assert ((g64 > 0) == (g32 > 0)).all(), "the selected rows disagree on a gate"
        assert (a["other"] == b["other"]).all() and ((a["margin"] + kappa > 0) == (b["margin"] + kappa > 0)).all()
        s, ab = regime_scale(a, lab_rows)
        scale.append(s)
        absolute.append(ab)
        hinge_on.append(int((a["margin"] + kappa > 0).sum()))
        worst = np.maximum(worst, [np.abs(a["dz"] - b["dz"]).max() / (DZ_TOL * np.abs(a["dz"]).max()),
                                   (np.abs(a["margin"] - b["margin"]) / s).max(),
                                   (np.abs(a["dist"] - b["dist"]) / (SCALAR_TOL * np.abs(a["dist"]))).max()])
    info = {"pool": blocks * N, "blocks": blocks, "kept": float(keep.mean()), "hinge_on": hinge_on,
            "absolute": [int(ab.sum()) for ab in absolute]}
    return {"gp": gp, "clf": clf, "x": x, "labels": labels, "lab_rows": lab_rows, "R": R, "c": c, "kappa": kappa, "z": z, "m": m, "v": v,
            "its": its, "scale": scale, "absolute": absolute, "shares": tuple(float(w) for w in worst), "info": info}


# ---------------------------------------------------------------------- the tracker past 64 restarts
# B = 3 images of the 10-class classifier (seed 0), R restarts.  The synthetic generator's images all fall into one class (4, with
# margins of 0.2 to 1.0 at the draw), so the labels decide the branch: image 0 (label 1, margins -1.0 .. -0.2 at the draw) has a
# few successes at kappa 0.9 and gains more as the hinge pushes; image 1 (label 4) cannot reach m < -0.9 in three small steps and
# stays on the no-success branch; image 2 (label 7, margins below -1.9) succeeds in every row, and its LAST restart starts at the z
# its x was generated from, so that its distance is the smallest by orders of magnitude: a winner at r = R - 1 >= 64.
TRACKER = dict(latent=128, kind="conv10", clf_seed=0, B=3, labels=(1, 4, 7), nb_iter=3, lr=0.01, c=2.0, kappa=0.9)


@functools.lru_cache(maxsize=None)
def tracker_inputs(R):
    """(gp, clf, x [3,28,28,1], labels [3], z0 [3 R, latent]) of the R > 64 tracker case."""
    t = TRACKER
    gp, clf = GR.weights(t["latent"], 64), classifier(t["kind"], t["clf_seed"])
    rs = np.random.RandomState(9500 + R)
    x = (1.0 / (1.0 + np.exp(-rs.standard_normal((t["B"], 28, 28, 1))))).astype(np.float32)
    z_true = (rs.standard_normal((1, t["latent"])) / np.sqrt(t["latent"])).astype(np.float32)
    z0 = (rs.standard_normal((t["B"] * R, t["latent"])) / np.sqrt(t["latent"])).astype(np.float32)
    x[2] = GR._gen(gp, torch.float64).forward(torch.as_tensor(z_true.astype(np.float64))).numpy()[0].astype(np.float32)
    z0[3 * R - 1] = z_true[0]
    return gp, clf, x, np.asarray(t["labels"], np.int32), z0


@functools.lru_cache(maxsize=None)
def tracker_reference(R):
    t = TRACKER
    gp, clf, x, labels, z0 = tracker_inputs(R)
    return run(gp, clf, x, labels, R, z0, t["nb_iter"], lr=t["lr"], c=t["c"], kappa=t["kappa"])
