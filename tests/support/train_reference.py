"""CPU restatement of classifier training (cleverhans utils_tf.model_train as the reference uses it, whitebox.py:120-170), in
float64 torch, written independently of the device code (defensegan_amd/csrc/dg_clf_train.hip): the training-phase forward with
given Dropout masks, all parameter gradients by autograd, the adversarial step, TF Adam, and the Philox4x32-10 mask generator the
device draws its masks from (so that both sides use the same masks, bit for bit).

    layers = describe(model)                       # ("conv", ch, (kh, kw), (sh, sw), pad) / ("linear", n) / ("dropout", keep) / ...
    masks = step_masks(layers, (28, 28, 1), B, seed, step, pass_)
    loss, grads, x_adv = param_gradient(layers, params, x, labels, seed, step, adv_eps=0.15)
"""
import numpy as np
import torch
import torch.nn.functional as F

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
_M32 = np.uint64(0xFFFFFFFF)


def describe(model):
    """The model's layers as plain tuples (Dropout carries its keep probability)."""
    from defensegan_amd import network_builder as nb
    out = []
    for l in model.layers:
        if isinstance(l, nb.Conv2D):
            out.append(("conv", l.output_channels, l.kernel_shape, l.strides, l.padding))
        elif isinstance(l, nb.Linear):
            out.append(("linear", l.num_hid))
        elif isinstance(l, nb.Dropout):
            out.append(("dropout", float(l.prob)))
        else:
            out.append((l.__class__.__name__.lower(),))
    return out


# ---------------------------------------------------------------------- Philox4x32-10 masks
def philox4x32_10(ctr, key):
    """ctr [N, 4] (uint32 values), key (k0, k1) -> [N, 4] uint64 arrays holding uint32 words (Random123's Philox4x32-10)."""
    c = [np.asarray(ctr[:, i], np.uint64) & _M32 for i in range(4)]
    k0, k1 = np.uint64(key[0]) & _M32, np.uint64(key[1]) & _M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _M32, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(c, axis=1)


def uniforms(n, seed, step, pass_, layer):
    """The n float32 uniforms in [0, 1) of one layer's mask: element 4 q + r takes word r of Philox(counter = (q, layer | pass << 16,
    step lo, step hi), key = (seed lo, seed hi)), u = (word >> 8) * 2^-24."""
    nq = (n + 3) // 4
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((nq, 4), np.uint64)
    ctr[:, 0] = np.arange(nq, dtype=np.uint64)
    ctr[:, 1] = (int(layer) | (int(pass_) << 16)) & 0xFFFFFFFF
    ctr[:, 2] = step & 0xFFFFFFFF
    ctr[:, 3] = step >> 32
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]
    return (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_mask(keep, n, seed, step, pass_, layer):
    """TF's mask: floor(keep + u) in float32 (0 or 1)."""
    return np.floor(np.float32(keep) + uniforms(n, seed, step, pass_, layer)).astype(np.float32)


def _same(n, k, s):
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def feature_counts(layers, input_shape):
    """Per layer: the features per image of its output (NHWC)."""
    H, W, Cc = input_shape
    out, flat = [], None
    for L in layers:
        if L[0] == "conv":
            (kh, kw), (sh, sw) = L[2], L[3]
            if L[4] == "SAME":
                H, W = -(-H // sh), -(-W // sw)
            else:
                H, W = (H - kh) // sh + 1, (W - kw) // sw + 1
            Cc = L[1]
        elif L[0] == "flatten":
            flat = H * W * Cc
        elif L[0] == "linear":
            flat = L[1]
        out.append(flat if flat is not None else H * W * Cc)
    return out


def step_masks(layers, input_shape, B, seed, step, pass_):
    """{layer index: mask [B, features]} of every Dropout layer for one forward pass (0 clean, 1 FGSM-inner, 2 adversarial)."""
    feats = feature_counts(layers, input_shape)
    return {j: dropout_mask(L[1], B * feats[j], seed, step, pass_, j).reshape(B, feats[j])
            for j, L in enumerate(layers) if L[0] == "dropout"}


# ---------------------------------------------------------------------- training-phase forward, loss, gradients
def logits(layers, params, x, masks=None, pre=None):
    """x [B,H,W,C] float64 tensor (NHWC) -> logits (the Softmax layer's input).  ``params``: list of (W, b) float64 tensors.
    ``masks``: {layer: [B, features] array} for the training phase (Dropout y = (x / keep) * mask); None: evaluation.
    ``pre``: a list that receives every ReLU / LeakyReLU layer's input."""
    h = x
    it = iter(params)
    for j, L in enumerate(layers):
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
        elif kind == "relu":
            if pre is not None:
                pre.append(h)
            h = torch.relu(h)
        elif kind == "leakyrelu":
            if pre is not None:
                pre.append(h)
            h = torch.where(h > 0, h, 0.2 * h)            # the tie at 0 takes the slope 0.2, as TF's MaximumGrad decides it
        elif kind == "flatten":
            h = h.reshape(h.shape[0], -1)
        elif kind == "dropout":
            if masks is not None:
                m = torch.as_tensor(masks[j], dtype=h.dtype).reshape(h.shape)
                h = (h / L[1]) * m
        elif kind == "softmax":
            break
    return h


def mean_ce(z, labels):
    """Mean cross-entropy over the batch.  A negative label marks an image without a label (what dg_clf_train's gather makes of an
    index outside the set): it adds nothing to the sum, and the divisor stays the batch size."""
    y = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    if bool((y < 0).any()):
        y = torch.where(y < 0, torch.full_like(y, -1), y)
        return F.cross_entropy(z, y, ignore_index=-1, reduction="sum") / z.shape[0]
    return F.cross_entropy(z, y)


def as_params(params, requires_grad=False):
    return [(torch.tensor(np.asarray(W, np.float64), requires_grad=requires_grad),
             torch.tensor(np.asarray(b, np.float64), requires_grad=requires_grad)) for W, b in params]


def fgsm_inner(layers, params_t, x, eps, lo, hi, masks):
    """whitebox.py:147-163: FGM (ord inf) on the model's own first argmax, in the training phase with its own masks; stopped."""
    xin = x.detach().clone().requires_grad_(True)
    z = logits(layers, [(W.detach(), b.detach()) for W, b in params_t], xin, masks)
    y = z.detach().argmax(dim=1)
    ce = F.cross_entropy(z, y, reduction="sum")
    (g,) = torch.autograd.grad(ce, xin)
    return torch.clamp(x + eps * torch.sign(g), lo, hi).detach()


def param_gradient(layers, params, x, labels, seed, step, adv_eps=0.0, lo=0.0, hi=1.0, x_adv=None):
    """One training step's loss and gradient: loss = mean CE (clean, masks of pass 0), or (clean + adversarial) / 2 with the FGSM
    inputs (inner pass 1, outer pass 2).  ``x_adv`` given: use it instead of the inner FGSM (to compare gradients without the
    float64 / float32 sign differences of near-zero input gradients).  Returns (loss float, [(dW, db)] float64, x_adv or None)."""
    x = torch.as_tensor(np.asarray(x, np.float64))
    B, shape = x.shape[0], tuple(x.shape[1:])
    p = as_params(params, requires_grad=True)
    loss = mean_ce(logits(layers, p, x, step_masks(layers, shape, B, seed, step, 0)), labels)
    xa = None
    if adv_eps > 0:
        xa = (fgsm_inner(layers, p, x, adv_eps, lo, hi, step_masks(layers, shape, B, seed, step, 1)) if x_adv is None
              else torch.as_tensor(np.asarray(x_adv, np.float64)))
        loss = (loss + mean_ce(logits(layers, p, xa, step_masks(layers, shape, B, seed, step, 2)), labels)) / 2
    flat = [t for pair in p for t in pair]
    g = torch.autograd.grad(loss, flat)
    grads = [(g[2 * i].numpy(), g[2 * i + 1].numpy()) for i in range(len(p))]
    return float(loss.item()), grads, (None if xa is None else xa.numpy())


def relu_margins(layers, params, x, masks=None):
    """Per image: the smallest non-zero |ReLU input| of the float64 forward.  The gradient jumps where a ReLU input crosses zero:
    an input closer to zero than float32 rounding of the sum that forms it (about 1e-7 for the unit-norm weight columns of the
    zoo) is decided one way in float64 and the other way in float32, and a float32 gradient then differs from the float64 one by
    that activation's whole term.  A comparison of the two is meaningful only at inputs whose margin is well above that; exact
    zeros (a zero image under zero biases) are "not > 0" on both sides and do not count."""
    pre = []
    logits(layers, as_params(params), torch.as_tensor(np.asarray(x, np.float64)), masks, pre=pre)
    out = np.full(len(x), np.inf)
    for h in pre:
        a = np.abs(h.numpy()).reshape(len(x), -1)
        out = np.minimum(out, np.where(a > 0, a, np.inf).min(axis=1))
    return out


def loss_of(layers, params, x, labels, masks):
    """The clean loss as a plain function of the parameters (for finite differences)."""
    z = logits(layers, as_params(params), torch.as_tensor(np.asarray(x, np.float64)), masks)
    return float(mean_ce(z, labels).item())


# ---------------------------------------------------------------------- TF Adam and the trajectory
def adam_update(p, g, m, v, t, lr, dtype=np.float64):
    """TF AdamOptimizer's step t (from 1): returns (p, m, v).  1 - beta enters as the constants 0.1 and 0.001, as the device
    (and dg_cw) writes them: in float32, 1 - 0.999f is 0.0010000467, not 0.001f."""
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    b1, b2, eps = dtype(BETA1), dtype(BETA2), dtype(EPS)
    m = b1 * m + dtype(0.1) * g
    v = b2 * v + dtype(0.001) * (g * g)
    lr_t = dtype(lr * np.sqrt(1 - BETA2 ** t) / (1 - BETA1 ** t))
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def train(layers, params, X, labels, idx, batch_size, lr, seed, adv_eps=0.0, lo=0.0, hi=1.0):
    """len(idx) / batch_size Adam steps from fresh moments (model_train's loop body); step s uses X[idx[s*bs:(s+1)*bs]] and the
    masks of (seed, s).  Returns (losses, params) in float64."""
    params = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in params]
    mom = [(np.zeros_like(W), np.zeros_like(b)) for W, b in params]
    vel = [(np.zeros_like(W), np.zeros_like(b)) for W, b in params]
    losses = []
    for s in range(len(idx) // batch_size):
        sel = np.asarray(idx[s * batch_size:(s + 1) * batch_size])
        loss, grads, _ = param_gradient(layers, params, X[sel], np.asarray(labels)[sel], seed, s, adv_eps, lo, hi)
        losses.append(loss)
        nxt = []
        for i, ((W, b), (gW, gb)) in enumerate(zip(params, grads)):
            W, mW, vW = adam_update(W, gW, mom[i][0], vel[i][0], s + 1, lr)
            b, mb, vb = adam_update(b, gb, mom[i][1], vel[i][1], s + 1, lr)
            mom[i], vel[i] = (mW, mb), (vW, vb)
            nxt.append((W, b))
        params = nxt
    return np.asarray(losses), params


# ---------------------------------------------------------------------- the weight-gradient planner, restated
# dg_clf_train.hip's geometry() and slot_plan(): a layer's weight gradient is a GEMM [M + 1, K] x [K, N] (row M: the bias) in
# 64 x 64 output tiles; the reduction axis K = B * output positions is cut into `slots` runs of Kc terms, each walked in chunks
# of 16.  Restated so that the tests can say which regime of the kernel each of their cases reaches, and pick the images that
# sit on a slot boundary.
WT, WKC = 64, 16


def wgrad_shapes(layers, input_shape):
    """Per Conv2D / Linear layer: (kind, M, N, positions): M = kh * kw * cin (Linear: its inputs), N = its outputs, positions =
    oh * ow output positions per image (Linear: 1)."""
    H, W, Cc = input_shape
    out, flat = [], None
    for L in layers:
        if L[0] == "conv":
            (kh, kw), (sh, sw) = L[2], L[3]
            M = kh * kw * Cc
            if L[4] == "SAME":
                H, W = -(-H // sh), -(-W // sw)
            else:
                H, W = (H - kh) // sh + 1, (W - kw) // sw + 1
            Cc = L[1]
            out.append(("conv", M, Cc, H * W))
        elif L[0] == "flatten":
            flat = H * W * Cc
        elif L[0] == "linear":
            out.append(("linear", flat, L[1], 1))
            flat = L[1]
    return out


def slot_plan(M, N, K):
    """(tiles, S, Kc, slots): about 1024 workgroups per layer, at least 64 terms per slot, at most 256 slots."""
    tiles = -(-(M + 1) // WT) * -(-N // WT)
    S = max(1, 1024 // tiles)
    S = min(S, max(1, K // 64), 256)
    Kc = -(-K // S)
    return tiles, S, Kc, -(-K // Kc)


REGIMES = ("linear layer with >= 2 slots of >= 2 chunks", "256-slot cap", "slot start off a chunk boundary", "slots < S", "K < 16",
           "K a multiple of 16", "ragged last M-tile", "ragged last N-tile", "N < 4")


def regimes(kind, M, N, positions, B):
    """The regimes of REGIMES that one layer's weight gradient reaches at batch size B."""
    K = B * positions
    _, S, Kc, slots = slot_plan(M, N, K)
    hit = {"linear layer with >= 2 slots of >= 2 chunks": kind == "linear" and slots >= 2 and Kc > WKC,
           "256-slot cap": S == 256,
           "slot start off a chunk boundary": slots >= 2 and Kc % WKC != 0,
           "slots < S": slots < S,
           "K < 16": K < WKC,
           "K a multiple of 16": K % WKC == 0,
           "ragged last M-tile": M + 1 > WT and (M + 1) % WT != 0,
           "ragged last N-tile": N > WT and N % WT != 0,
           "N < 4": N < 4}
    return {r for r in REGIMES if hit[r]}


def boundary_images(layers, input_shape, B):
    """The images whose terms lie next to a slot boundary in some layer: image 0 and B - 1 (the first and last k), and for each
    layer's first and last boundary kb = z * Kc the image holding term kb - 1 and the one holding kb (the same image when the
    boundary cuts inside it, as Kc = 98 cuts the 196 positions of a 14 x 14 output)."""
    out = {0, B - 1}
    for kind, M, N, pos in wgrad_shapes(layers, input_shape):
        _, _, Kc, slots = slot_plan(M, N, B * pos)
        for z in {1, slots - 1} - {0}:
            out |= {(z * Kc - 1) // pos, (z * Kc) // pos}
    return sorted(out)


# ---------------------------------------------------------------------- the cases of tests/test_gpu_train_shapes.py
def shape_model(key):
    """A letter of network_builder.MODELS at its full width, or "A16c": model A with 16 filters and 2 classes on 64 x 64 x 3."""
    from defensegan_amd import network_builder as nb
    if key == "A16c":
        return nb.model_a(nb_filters=16, nb_classes=2, input_shape=(None, 64, 64, 3))
    return nb.MODELS[key]()


# (model, batch size, adv_eps) of the weight-gradient value checks: E (Linear only) and F (convolutions) over the batch sizes,
# D, Y, Q, Z at a small and at the shipped batch size, the colour model.  tests/test_train_cpu.py asserts that every regime of
# REGIMES is reached by a layer of one of them.
BATCH_SIZES = (1, 16, 17, 64, 100, 128, 130, 200)
GRADIENT_CASES = ([(name, B, 0.0) for name in "EF" for B in BATCH_SIZES] + [("E", 128, 0.15), ("F", 128, 0.15)] +
                  [("D", 5, 0.0), ("D", 128, 0.0), ("Y", 3, 0.0), ("Y", 128, 0.0), ("Q", 3, 0.0), ("Q", 128, 0.0), ("Z", 3, 0.0),
                   ("Z", 128, 0.0), ("A16c", 37, 0.15)])
