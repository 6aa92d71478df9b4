"""CPU restatement of cleverhans' CarliniWagnerL2 (the reference's --attack_type cw, whitebox.py:201-209) in float64 torch,
written independently of the device code (defensegan_amd/csrc/dg_cw.hip): the logits come from F.conv2d / matmul with explicit
asymmetric SAME padding, the input gradient from autograd, the loss gradient from the TF rules stated in DESIGN.md section 7.

    out = cw_l2(layers_of(model), params, x, labels, targeted=False, batch_size=..., ...)
    out["x_adv"], out["best_l2"], out["best_class"], out["const"], out["abort_iters"]   # abort_iters[outer][chunk]: iteration or None

With ``trace=True`` the result also holds out["trace"]: how close every decision of the run came to flipping, in float64 (NaN
where an iteration did not take the decision: after a stop, and the best tracking of the stopping iteration itself).

    success_margin [N, outer, iteration]   |Z'_t - max_{k != t} Z'_k|: the top entry of Z' against the runner-up when the label is
                                           on top, against the label's entry when it is not (Z' = Z with the label moved by kappa)
    arg_margin     [N, outer, iteration]   |arg|, arg = real - oth + kappa (targeted: oth - real + kappa), whose sign gates the seed
    check_margin   [outer][chunk]          one |L - 0.9999 prev| / prev per check the chunk made
    step_success   [N, outer] bool         the outer step ended in success (what the constant update saw)
    max_logit      [N]                     the largest |Z| the run saw
"""
import numpy as np
import torch
import torch.nn.functional as F

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def layers_of(model):
    """The layer description of tests/test_classifier.py::_layers_of (copied, not imported from a test file)."""
    from defensegan_amd import network_builder as nb
    out = []
    for l in model.layers:
        if isinstance(l, nb.Conv2D):
            out.append(("conv", l.output_channels, l.kernel_shape, l.strides, l.padding))
        elif isinstance(l, nb.Linear):
            out.append(("linear", l.num_hid))
        else:
            out.append((l.__class__.__name__.lower(),))
    return out


def _same(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def logits(layers, params, x):
    """x [B,H,W,C] float64 tensor -> logits [B, n] (the layer before Softmax), differentiable."""
    h = x.permute(0, 3, 1, 2)
    it = iter(params)
    flat = False
    for L in layers:
        kind = L[0]
        if kind == "conv":
            W, b = next(it)
            (kh, kw), (sh, sw), pad = L[2], L[3], L[4]
            if pad == "SAME":
                pt, pb = _same(h.shape[2], kh, sh)
                pl, pr = _same(h.shape[3], kw, sw)
                h = F.pad(h, (pl, pr, pt, pb))
            K = torch.as_tensor(np.asarray(W, np.float64)).permute(3, 2, 0, 1)
            h = F.conv2d(h, K, torch.as_tensor(np.asarray(b, np.float64)), stride=(sh, sw))
        elif kind == "linear":
            W, b = next(it)
            h = h @ torch.as_tensor(np.asarray(W, np.float64)) + torch.as_tensor(np.asarray(b, np.float64))
        elif kind == "relu":
            h = torch.relu(h)
        elif kind == "flatten":
            h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)         # NHWC row-major, as the reference's Flatten
            flat = True
        elif kind == "softmax":
            break
    assert flat or h.dim() == 2
    return h


def to_img(t, lo, hi):
    return (t + 1) / 2 * (hi - lo) + lo


def loss1_and_seed(Z, t, const, confidence, targeted):
    """Per image: loss1 = const * max(0, real - oth + k) (targeted: oth - real + k) and dloss1/dZ by TF's rules: nothing where the
    argument is <= 0 (Maximum's tie goes to the constant), the max's share split evenly over its maximisers (_MaxGrad), none
    of it to the label's own entry.  Z [B, n] float64 tensor, t [B] ints, const [B]."""
    B, n = Z.shape
    onehot = torch.zeros(B, n, dtype=Z.dtype)
    onehot[torch.arange(B), torch.as_tensor(t)] = 1
    real = (onehot * Z).sum(1)
    o = (1 - onehot) * Z - onehot * 10000
    oth = o.max(1).values
    arg = (oth - real + confidence) if targeted else (real - oth + confidence)
    c = torch.as_tensor(np.asarray(const, np.float64))
    loss1 = c * torch.clamp(arg, min=0)
    sel = (o == oth[:, None]).to(Z.dtype)
    share = sel / sel.sum(1, keepdim=True) * (1 - onehot)
    sgn = -1.0 if targeted else 1.0
    active = (arg > 0).to(Z.dtype) * c
    seed = active[:, None] * (sgn * onehot - sgn * share)
    return loss1, seed


def step_values(layers, params, w, timg, other, t, const, confidence, targeted, lo, hi):
    """The values one iteration reads (from the pre-update w): newimg, l2, logits, loss1 and dLoss/dw."""
    u = (w + timg).requires_grad_(False)
    newimg = to_img(torch.tanh(u), lo, hi).detach().requires_grad_(True)
    Z = logits(layers, params, newimg)
    loss1, seed = loss1_and_seed(Z.detach(), t, const, confidence, targeted)
    Z.backward(seed)
    d = newimg - other
    l2 = (d * d).reshape(len(d), -1).sum(1).detach()
    gimg = newimg.grad + 2 * d.detach()
    g = gimg * (hi - lo) / 2 * (1 - torch.tanh(u) ** 2)
    return newimg.detach(), l2, Z.detach(), loss1, g


def total_loss(layers, params, w, timg, other, t, const, confidence, targeted, lo, hi):
    """sum (loss1 + l2) as a plain function of w (for finite differences)."""
    newimg = to_img(torch.tanh(w + timg), lo, hi)
    Z = logits(layers, params, newimg)
    loss1, _ = loss1_and_seed(Z, t, const, confidence, targeted)
    return float((loss1.sum() + ((newimg - other) ** 2).sum()).item())


def adam_step(w, m, v, g, lr, step):
    """TF Adam: step counts from 1."""
    m = BETA1 * m + (1 - BETA1) * g
    v = BETA2 * v + (1 - BETA2) * g * g
    lr_t = lr * np.sqrt(1 - BETA2 ** step) / (1 - BETA1 ** step)
    return w - lr_t * m / (torch.sqrt(v) + EPS) if isinstance(w, torch.Tensor) else w - lr_t * m / (np.sqrt(v) + EPS), m, v


def abort_check_iterations(max_iterations):
    every = (max_iterations // 10) or 1
    return [i for i in range(max_iterations) if i % every == 0]


def const_update(bestscore, t, const, lower, upper, targeted):
    """cleverhans' binary search over the constant after one outer step (per image, float64 arrays; returns new copies)."""
    const, lower, upper = np.array(const, np.float64), np.array(lower, np.float64), np.array(upper, np.float64)
    for e in range(len(const)):
        ok = bestscore[e] != -1 and ((bestscore[e] == t[e]) if targeted else (bestscore[e] != t[e]))
        if ok:
            upper[e] = min(upper[e], const[e])
            if upper[e] < 1e9:
                const[e] = (lower[e] + upper[e]) / 2
        else:
            lower[e] = max(lower[e], const[e])
            if upper[e] < 1e9:
                const[e] = (lower[e] + upper[e]) / 2
            else:
                const[e] *= 10
    return const, lower, upper


def success_margin(Z, t, confidence, targeted):
    """|Z'_t - max_{k != t} Z'_k| per image: how far the success decision on Z' is from flipping."""
    Zp = Z.clone()
    idx = torch.arange(len(Z))
    tt = torch.as_tensor(t)
    Zp[idx, tt] += -confidence if targeted else confidence
    own = Zp[idx, tt].clone()
    Zp[idx, tt] = -float("inf")
    return (own - Zp.max(1).values).abs().numpy()


def arg_margin(Z, t, confidence, targeted):
    """|arg| per image, arg being the hinge's argument (its sign decides whether loss1 has a gradient at all)."""
    idx = torch.arange(len(Z))
    tt = torch.as_tensor(t)
    real = Z[idx, tt]
    o = Z.clone()
    o[idx, tt] = -10000.0
    oth = o.max(1).values
    return ((oth - real + confidence) if targeted else (real - oth + confidence)).abs().numpy()


# The four places of the setup and the loop a mutated reference patches (tests/test_cw_cpu.py); cw_l2 looks them up at call time.
def to_tanh_space(xc, lo, hi):
    """timg: the image clipped to [lo, hi], scaled to (-1, 1) * 0.999999, through atanh."""
    u = torch.clamp((xc - lo) / (hi - lo), 0, 1)
    return torch.atanh((u * 2 - 1) * 0.999999)


def own_label(Z):
    """The label of a call without y / y_target: the model's own FIRST argmax (numpy's argmax takes the first of a tie)."""
    return np.argmax(Z, axis=1)


def rearm(prev, stopped):
    """The chunk's abort state at the start of an outer step: (prev, the iteration that stopped it), whatever the last step left."""
    return 1e6, None


def step_bestscore(bestscore, stopped):
    """The bestscore the constant update sees after an outer step that stopped at ``stopped`` (None: it ran to the end)."""
    return bestscore


def _success(Z, t, confidence, targeted):
    Zp = Z.clone()
    idx = torch.arange(len(Z))
    Zp[idx, torch.as_tensor(t)] += -confidence if targeted else confidence
    am = Zp.argmax(1).numpy()
    return (am == t) if targeted else (am != t)


def cw_l2(layers, params, x, labels=None, targeted=False, batch_size=1, confidence=0.0, learning_rate=5e-3, binary_search_steps=5,
          max_iterations=1000, abort_early=True, initial_const=1e-2, clip_min=0.0, clip_max=1.0, trace=False):
    x = torch.as_tensor(np.asarray(x, np.float64))
    N = len(x)
    lo, hi = float(clip_min), float(clip_max)
    if labels is None:
        with torch.no_grad():
            t_all = own_label(logits(layers, params, x).numpy())
    else:
        t_all = np.asarray(labels)
        if t_all.ndim > 1:
            t_all = t_all.argmax(-1)
    every = (max_iterations // 10) or 1
    repeat = binary_search_steps >= 10
    x_adv = torch.clamp(x, lo, hi).clone()
    o_bestl2 = np.full(N, 1e10)
    o_bestscore = np.full(N, -1, np.int64)
    const_all = np.full(N, float(initial_const))
    abort_iters = [[None] * ((N + batch_size - 1) // batch_size) for _ in range(binary_search_steps)]
    tr = {"success_margin": np.full((N, binary_search_steps, max_iterations), np.nan),
          "arg_margin": np.full((N, binary_search_steps, max_iterations), np.nan),
          "check_margin": [[[] for _ in abort_iters[0]] for _ in range(binary_search_steps)],
          "step_success": np.zeros((N, binary_search_steps), bool), "max_logit": np.zeros(N)}
    for ci, s in enumerate(range(0, N, batch_size)):
        sl = slice(s, min(s + batch_size, N))
        xc, t = x[sl], t_all[sl]
        timg = to_tanh_space(xc, lo, hi)
        other = to_img(torch.tanh(timg), lo, hi)
        n = len(xc)
        prev, stopped = 1e6, None
        lower, upper, const = np.zeros(n), np.full(n, 1e10), np.full(n, float(initial_const))
        for outer in range(binary_search_steps):
            bestl2, bestscore = np.full(n, 1e10), np.full(n, -1, np.int64)
            if repeat and outer == binary_search_steps - 1:
                const = upper.copy()
            w = torch.zeros_like(xc)
            m, v = torch.zeros_like(xc), torch.zeros_like(xc)
            prev, stopped = rearm(prev, stopped)
            abort_iters[outer][ci] = stopped
            for i in range(max_iterations if stopped is None else 0):
                newimg, l2, Z, loss1, g = step_values(layers, params, w, timg, other, t, const, confidence, targeted, lo, hi)
                w, m, v = adam_step(w, m, v, g, learning_rate, i + 1)
                tr["arg_margin"][sl, outer, i] = arg_margin(Z, t, confidence, targeted)
                tr["max_logit"][sl] = np.maximum(tr["max_logit"][sl], Z.abs().max(1).values.numpy())
                if abort_early and i % every == 0:
                    L = float((loss1 + l2).sum())
                    tr["check_margin"][outer][ci].append(abs(L - 0.9999 * prev) / prev)
                    if L > prev * 0.9999:
                        abort_iters[outer][ci] = stopped = i
                        break
                    prev = L
                tr["success_margin"][sl, outer, i] = success_margin(Z, t, confidence, targeted)
                succ = _success(Z, t, confidence, targeted)
                score = Z.argmax(1).numpy()
                l2n = l2.numpy()
                for e in range(n):
                    if l2n[e] < bestl2[e] and succ[e]:
                        bestl2[e], bestscore[e] = l2n[e], score[e]
                    if l2n[e] < o_bestl2[s + e] and succ[e]:
                        o_bestl2[s + e], o_bestscore[s + e] = l2n[e], score[e]
                        x_adv[s + e] = newimg[e]
            bestscore = step_bestscore(bestscore, stopped)
            tr["step_success"][sl, outer] = (bestscore != -1) & ((bestscore == t) if targeted else (bestscore != t))
            const, lower, upper = const_update(bestscore, t, const, lower, upper, targeted)
        const_all[sl] = const
    out = {"x_adv": x_adv.numpy(), "best_l2": o_bestl2, "best_class": o_bestscore, "const": const_all, "abort_iters": abort_iters,
           "labels": t_all}
    if trace:
        out["trace"] = tr
    return out
