"""CPU restatement of the WGAN-GP critic (the reference's models/gan.py:167-199 and models/dataset_models.py:74-97) in float64
torch, written independently of the device code (defensegan_amd/csrc/dg_critic.hip): the gradient penalty is differentiated by
autograd through ``autograd.grad(..., create_graph=True)`` -- a real double backward -- while the device uses the closed form for
piecewise-linear critics (one masked tangent pass plus weight-gradient products).  Also TF Adam with free betas and the helpers
the tests use to keep LeakyReLU inputs away from zero, where float32 and float64 decide the slope differently.

    layers = describe(critic)              # ("conv", ch, (kh, kw), (sh, sw), pad) / ("leakyrelu",) / ("flatten",) / ("linear", n)
    terms, grads, slopes = param_gradient(layers, params, real, fake, alpha, lam=10.0, axes=0)
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.support.train_reference import _same, as_params, describe  # noqa: F401  (describe: re-exported)

EPS = 1e-8
SLOPE = 0.2


def forward(layers, params, x, pre=None):
    """x [B,H,W,C] float64 tensor -> D(x) [B].  ``pre``: a list that receives every activation layer's input."""
    h, it = x, iter(params)
    for L in layers:
        kind = L[0]
        if kind == "conv":
            W, b = next(it)
            (kh, kw), (sh, sw), pad = L[2], L[3], L[4]
            t = h.permute(0, 3, 1, 2)
            if pad == "SAME":
                pt, pb = _same(t.shape[2], kh, sh)
                pl, pr = _same(t.shape[3], kw, sw)
                t = F.pad(t, (pl, pr, pt, pb))
            h = F.conv2d(t, W.permute(3, 2, 0, 1), b, stride=(sh, sw)).permute(0, 2, 3, 1)
        elif kind == "linear":
            W, b = next(it)
            h = h @ W + b
        elif kind == "leakyrelu":
            if pre is not None:
                pre.append(h)
            h = torch.where(h > 0, h, SLOPE * h)          # the tie at 0 takes the slope 0.2, as TF's MaximumGrad decides it
        elif kind == "relu":
            if pre is not None:
                pre.append(h)
            h = torch.where(h > 0, h, torch.zeros_like(h))
        elif kind == "flatten":
            h = h.reshape(h.shape[0], -1)
        else:
            raise ValueError("not a critic layer: %r" % (L,))
    return h.reshape(-1)


def slopes_of(g, axes):
    """s from g [B,H,W,C]: axes 0 sums over H alone ([B,W,C], the reference's reduction_indices=[1]); 1 over H, W, C ([B]).
    Where the sum is 0, s = 0 with a zero gradient (the project's departure from TF's NaN)."""
    ss = (g * g).sum(dim=1) if axes == 0 else (g * g).sum(dim=(1, 2, 3))
    pos = ss > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, ss, torch.ones_like(ss))), torch.zeros_like(ss))


def cost_terms(layers, p, real, fake, alpha, lam, axes):
    """(cost, w, P, slopes) as tensors; differentiable with respect to the parameters p."""
    xhat = (real + alpha.reshape(-1, 1, 1, 1) * (fake - real)).detach().requires_grad_(True)
    (g,) = torch.autograd.grad(forward(layers, p, xhat).sum(), xhat, create_graph=True)
    s = slopes_of(g, axes)
    P = ((s - 1.0) ** 2).mean()
    w = forward(layers, p, fake).mean() - forward(layers, p, real).mean()
    return w + lam * P, w, P, s


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def param_gradient(layers, params, real, fake, alpha, lam=10.0, axes=0, dtype=np.float64):
    """((cost, w, P) floats, [(dW, db)], slopes array).  ``dtype`` float32 runs the same computation in float32 (to measure what
    the number format alone costs)."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    p = [(torch.tensor(np.asarray(W, np.float64), dtype=td, requires_grad=True), torch.tensor(np.asarray(b, np.float64), dtype=td, requires_grad=True))
         for W, b in params]
    cost, w, P, s = cost_terms(layers, p, _t(real).to(td), _t(fake).to(td), _t(alpha).to(td), lam, axes)
    flat = [t for pair in p for t in pair]
    g = torch.autograd.grad(cost, flat, allow_unused=True)
    g = [torch.zeros_like(t) if q is None else q for q, t in zip(g, flat)]
    grads = [(g[2 * i].double().numpy(), g[2 * i + 1].double().numpy()) for i in range(len(p))]
    return (float(cost.item()), float(w.item()), float(P.item())), grads, s.detach().double().numpy()


def cost_of(layers, params, real, fake, alpha, lam=10.0, axes=0):
    """The cost as a plain function of the parameters (for finite differences)."""
    with torch.enable_grad():
        return float(cost_terms(layers, as_params(params), _t(real), _t(fake), _t(alpha), lam, axes)[0].item())


# ---------------------------------------------------------------------- the derivation of the issue, in NumPy-style steps
def derived_gradient(layers, params, real, fake, alpha, lam=10.0, axes=0):
    """The penalty's parameter gradient by the closed form the device uses -- slopes m_j frozen at xhat's pre-activations,
    a_j from the ordinary backward, v = dP/dg, the masked bias-free tangent pass u_j, dP/dC_j = wgrad(u_{j-1}, a_j) -- each product
    taken with a first-order autograd call on frozen masks (no create_graph anywhere).  Returns lam * dP/dparams as [(dW, db)]."""
    p = as_params(params)
    xhat = (_t(real) + _t(alpha).reshape(-1, 1, 1, 1) * (_t(fake) - _t(real)))
    pre = []
    forward(layers, p, xhat, pre=pre)
    masks = [torch.where(h > 0, torch.ones_like(h), torch.full_like(h, SLOPE if L[0] == "leakyrelu" else 0.0))
             for h, L in zip(pre, [L for L in layers if L[0] in ("leakyrelu", "relu")])]

    def linear_net(x, weights, outs=None):
        """The critic with its activations replaced by the frozen masks and no biases: linear in x and in every weight."""
        h, wi, mi = x, 0, 0
        for L in layers:
            if L[0] == "conv":
                (kh, kw), (sh, sw), pad = L[2], L[3], L[4]
                t = h.permute(0, 3, 1, 2)
                if pad == "SAME":
                    pt, pb = _same(t.shape[2], kh, sh)
                    pl, pr = _same(t.shape[3], kw, sw)
                    t = F.pad(t, (pl, pr, pt, pb))
                h = F.conv2d(t, weights[wi].permute(3, 2, 0, 1), None, stride=(sh, sw)).permute(0, 2, 3, 1)
                wi += 1
            elif L[0] == "linear":
                h = h @ weights[wi]
                wi += 1
            elif L[0] in ("leakyrelu", "relu"):
                h = masks[mi] * h
                mi += 1
            elif L[0] == "flatten":
                h = h.reshape(h.shape[0], -1)
        return h.reshape(-1)

    Ws = [W.detach() for W, _ in p]
    x0 = xhat.detach().requires_grad_(True)
    (g,) = torch.autograd.grad(linear_net(x0, Ws).sum(), x0)              # g = C_1^T a_1
    s = slopes_of(g, axes)
    n = float(s.numel())
    ratio = torch.where(s > 0, (s - 1.0) / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))
    v = (2.0 / n) * (ratio.unsqueeze(1) if axes == 0 else ratio.reshape(-1, 1, 1, 1)) * g
    # sum_b D_lin(v_b) is bilinear in (v, C_j) along the frozen masks: its C_j-gradient is wgrad(u_{j-1}, a_j)
    Wg = [W.detach().clone().requires_grad_(True) for W in Ws]
    dW = torch.autograd.grad(linear_net(v.detach(), Wg).sum(), Wg)
    return [(lam * d.numpy(), np.zeros(np.shape(b))) for d, (_, b) in zip(dW, params)]


# ---------------------------------------------------------------------- TF Adam with free betas, and the trajectory
def adam_update(p, g, m, v, t, lr, beta1, beta2, dtype=np.float64):
    """tf.train.AdamOptimizer's step t (from 1): (p, m, v).  In ``dtype`` float32 it is the device's arithmetic: 1 - beta is
    formed in that type, lr_t in float64 and then rounded."""
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    b1, b2 = dtype(beta1), dtype(beta2)
    m = b1 * m + (dtype(1) - b1) * g
    v = b2 * v + (dtype(1) - b2) * (g * g)
    lr_t = dtype(lr * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t))
    return p - lr_t * m / (np.sqrt(v) + dtype(EPS)), m, v


def train(layers, params, batches, lr=1e-4, beta1=0.5, beta2=0.9, lam=10.0, axes=0):
    """One Adam step per (real, fake, alpha) of ``batches`` from fresh moments, in float64: (costs [n, 3], params)."""
    costs, params, _ = train_safe(layers, params, lambda k, attempt: batches[k], len(batches), lr, beta1, beta2, lam, axes, min_margin=None)
    return costs, params


# ---------------------------------------------------------------------- keeping away from the kinks
def margin(layers, params, real, fake, alpha):
    """The smallest non-zero |activation input| of the float64 forwards of fake, real and xhat.  An input closer to zero than
    float32 rounding is decided one way in float64 and the other in float32, and the two gradients then differ by that unit's
    whole term; exact zeros (a zero patch under zero biases) take the slope 0.2 on both sides and do not count."""
    p = as_params(params)
    real, fake, alpha = _t(real), _t(fake), _t(alpha)
    xhat = real + alpha.reshape(-1, 1, 1, 1) * (fake - real)
    out = np.inf
    with torch.no_grad():
        for x in (fake, real, xhat):
            pre = []
            forward(layers, p, x, pre=pre)
            for h in pre:
                a = h.abs()
                a = a[a > 0]
                if a.numel():
                    out = min(out, float(a.min()))
    return out


def conditioning(layers, params, real, fake, alpha, lam=10.0, axes=0):
    """How much of the cost terms is cancellation, on the float64 reference alone: (|mean D(fake)| + |mean D(real)|) / |w| and
    (|w| + lam P) / |cost| (each 1 where its denominator is exactly 0, as it is for w when real == fake).  A relative bound on w or
    on the cost is a bound on float32 arithmetic only while these stay small: at 10, 1e-5 of the term is 1e-6 of what was summed."""
    p = as_params(params)
    with torch.enable_grad():
        cost, w, P, _ = cost_terms(layers, p, _t(real), _t(fake), _t(alpha), lam, axes)
    cost, w, P = float(cost.item()), float(w.item()), float(P.item())
    with torch.no_grad():
        df, dr = float(forward(layers, p, _t(fake)).mean()), float(forward(layers, p, _t(real)).mean())
    return ((abs(df) + abs(dr)) / abs(w) if w != 0 else 1.0), ((abs(w) + lam * P) / abs(cost) if cost != 0 else 1.0)


def safe_batch(layers, params, draw, min_margin=1e-6, max_tries=200, max_condition=None, lam=10.0, axes=(0,)):
    """draw(attempt) -> (real, fake, alpha); the first draw whose margin is at least ``min_margin`` (None: the first draw) and, with
    ``max_condition``, whose conditioning() stays below it for every one of ``axes``; and the attempt it took."""
    if min_margin is None:
        return draw(0), 0
    for attempt in range(max_tries):
        batch = draw(attempt)
        if margin(layers, params, *batch) < min_margin:
            continue
        if max_condition is None or all(max(conditioning(layers, params, *batch, lam=lam, axes=a)) <= max_condition for a in axes):
            return batch, attempt
    raise RuntimeError("no batch with a margin of %g in %d draws" % (min_margin, max_tries))


def train_safe(layers, params, draw, n_steps, lr=1e-4, beta1=0.5, beta2=0.9, lam=10.0, axes=0, min_margin=1e-6):
    """train(), but step k's batch is safe_batch(draw(k, attempt)) at the float64 parameters of that step.  Returns
    (costs [n, 3], params, batches): the batches are what the device run is then given."""
    params = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in params]
    mom = [[np.zeros_like(W), np.zeros_like(b)] for W, b in params]
    vel = [[np.zeros_like(W), np.zeros_like(b)] for W, b in params]
    costs, batches = [], []
    for k in range(n_steps):
        batch, _ = safe_batch(layers, params, lambda a: draw(k, a), min_margin)
        batches.append(batch)
        terms, grads, _ = param_gradient(layers, params, *batch, lam=lam, axes=axes)
        costs.append(terms)
        nxt = []
        for i, (pair, gpair) in enumerate(zip(params, grads)):
            new = []
            for j in range(2):
                q, mom[i][j], vel[i][j] = adam_update(pair[j], gpair[j], mom[i][j], vel[i][j], k + 1, lr, beta1, beta2)
                new.append(q)
            nxt.append(tuple(new))
        params = nxt
    return np.asarray(costs), params, batches


def discriminate(layers, params, x):
    with torch.no_grad():
        return forward(layers, as_params(params), _t(x)).numpy()
