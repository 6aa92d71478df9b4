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
    (best_dist, best_margin, best_iter, best_row), each [B]."""
    margins, dists = np.asarray(margins), np.asarray(dists)
    K, B, R = margins.shape
    bd, bm = np.empty(B, margins.dtype), np.empty(B, margins.dtype)
    bi, br = np.full(B, -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        for k in range(K):
            for r in range(R):
                if margins[k, b, r] < -kappa and (bi[b] < 0 or dists[k, b, r] < bd[b]):
                    bd[b], bm[b], bi[b], br[b] = dists[k, b, r], margins[k, b, r], k, r
        if bi[b] < 0:
            r = 0
            for q in range(1, R):
                if margins[K - 1, b, q] < margins[K - 1, b, r]:
                    r = q
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
