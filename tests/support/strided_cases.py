"""The cases of tests/test_gpu_strided.py, fixed on the CPU (tests/test_strided_cpu.py asserts what their choice promises), and the
float32 restatement the spread-logit check is set against.  Nothing here touches a device.

Two tiny models, with n classes:

    "lin"   Flatten, Linear(n), Softmax                          on 3 x 3 x 1
    "mlp"   Flatten, Linear(16), ReLU, Linear(n), Softmax        on 4 x 4 x 1

n in WIDTHS: 2, and 63 / 64 / 65 / 130 around the 64 lanes that jac_seed_kernel and pgd_track_kernel stride the classes over (one
trip, exactly one trip, one class in the second trip, a third trip).  B in BATCHES: 67 is more than one 64-row block of the
kernels that use one thread per row.  Weights are bpda_reference.init_params (normal, normalised per output unit, small biases).
Every image keeps its float64 ReLU inputs MARGIN from zero and its two largest logits GAP of the largest |logit| apart, so that
neither a ReLU nor an arg-max is decided differently in float32.

The grid caps, read from the launchers (tests/test_strided_cpu.py checks them against the source text):

    BPDA_TRACK_CAP  1024 workgroups, one image each        dg_bpda_track:  grid = B < 1024 ? B : 1024
    PGD_TRACK_CAP   4096 workgroups of 4 images = 16384    pgd_track:      grid = (B + 3) / 4 < 4096 ? (B + 3) / 4 : 4096
    BALL_CAP        65536 workgroups, one image each       ball_grid:      B < 65536 ? B : 65536
"""
import functools

import numpy as np

from tests.support import blackbox_reference as BR
from tests.support import bpda_reference as R
from tests.support import train_reference as TR

WIDTHS = (2, 63, 64, 65, 130)
BATCHES = (1, 5, 67)
KINDS = ("lin", "mlp")
MARGIN = 1e-6                  # tests/test_gpu_blackbox.py: float64 ReLU inputs stay this far from zero
GAP = 1e-4                     # the two largest float64 logits differ by this share of the largest |logit|: ~100 float32 roundings of it
SPREAD = 30.0                  # the spread models' median logit range per row
SPREAD_TWO = 8.0               # with two classes the range IS the gap between them: at 30 p_c rounds to 1, the saturated case of
                               # tests/test_gpu_blackbox.py; at 8 it is 1 - 3e-4

BPDA_TRACK_CAP = 1024
PGD_TRACK_CAP = 4096 * 4
BALL_CAP = 65536
CAP_SOURCES = (("dg_bpda.hip", "const int grid = B < 1024 ? B : 1024;"),
               ("dg_pgd.hip", "const int grid = (B + 3) / 4 < 4096 ? (B + 3) / 4 : 4096;"),
               ("dg_pgd.hip", "b += (long long)gridDim.x * 4"),
               ("dg_ball.hip", "unsigned ball_grid(int B) { return (unsigned)(B < 65536 ? B : 65536); }"))


def model(kind, n, shape=None):
    """The network_builder.MLP of the case (no device is touched before its first use)."""
    from defensegan_amd import network_builder as nb
    if kind == "lin":
        return nb.MLP([nb.Flatten(), nb.Linear(n), nb.Softmax()], (None,) + (shape or (3, 3, 1)))
    return nb.MLP([nb.Flatten(), nb.Linear(16), nb.ReLU(), nb.Linear(n), nb.Softmax()], (None,) + (shape or (4, 4, 1)))


def as64(params):
    return [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in params]


def logits64(layers, params, x):
    import torch
    with torch.no_grad():
        return TR.logits(layers, TR.as_params(params), torch.as_tensor(np.asarray(x, np.float64))).numpy()


def top_gap(z):
    """[B]: (largest - second largest logit) / largest |logit|."""
    s = np.sort(z, axis=1)
    return (s[:, -1] - s[:, -2]) / np.abs(z).max(axis=1)


def _draw(m, layers, params, n_images, seed):
    rs = np.random.RandomState(seed)
    shape = tuple(m.input_shape[1:])
    x = rs.uniform(0, 1, (n_images,) + shape).astype(np.float32)
    for _ in range(40):
        bad = (TR.relu_margins(layers, params, x) < MARGIN) | (top_gap(logits64(layers, params, x)) < GAP)
        if not bad.any():
            return x
        x[bad] = rs.uniform(0, 1, (int(bad.sum()),) + shape).astype(np.float32)
    raise AssertionError("no batch with every ReLU input %g from zero and every arg-max decided" % MARGIN)


@functools.lru_cache(maxsize=None)
def case(kind, n, spread=False):
    """dict(layers, params (float32), p64, x [67, ...] float32 in [0, 1], y [67] int32 labels, z [67, n] float64 logits), computed once
    and never modified: rows [:B] are the case of batch size B (every kernel works on an image alone).  ``spread``: the last Linear
    layer times the factor that brings the median logit range of a row to SPREAD, then, for n > 64, the column of image 0's largest
    logit swapped with column 64, so that one image's mass sits on the only class of n = 65's second lane trip."""
    m = model(kind, n)
    layers = TR.describe(m)
    params = R.init_params(m, 1000 * n + len(kind))
    if spread:
        x0 = _draw(m, layers, as64(params), max(BATCHES), seed=7 * n + 1)
        z = logits64(layers, as64(params), x0)
        f = np.float32((SPREAD if n > 2 else SPREAD_TWO) / np.median(z.max(axis=1) - z.min(axis=1)))
        W, b = params[-1][0] * f, params[-1][1] * f
        if n > 64:
            top = int(z[0].argmax())
            W[:, [top, 64]], b[[top, 64]] = W[:, [64, top]], b[[64, top]]
        params = params[:-1] + [(np.ascontiguousarray(W, np.float32), np.ascontiguousarray(b, np.float32))]
    p64 = as64(params)
    x = _draw(m, layers, p64, max(BATCHES), seed=7 * n + 1)
    z = logits64(layers, p64, x)
    y = np.random.RandomState(n).randint(0, n, len(x)).astype(np.int32)
    for a in (x, y, z):
        a.setflags(write=False)
    return dict(layers=layers, params=params, p64=p64, x=x, y=y, z=z)


def spread_classes(z):
    """The classes the spread check differentiates: in the second lane trip (c >= 64) when there is one.  Even images take the
    largest logit of that range (mass to differentiate), odd images a seeded draw from it."""
    n = z.shape[1]
    first = 64 if n > 64 else 0
    rs = np.random.RandomState(n + 5)
    c = rs.randint(first, n, len(z))
    c[::2] = first + z[::2, first:].argmax(axis=1)
    return c.astype(np.int32)


# ---------------------------------------------------------------------- float32, in the kernels' documented order
def _fma32(a, b, c):
    """float32(a * b + c) with one rounding: the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def linear32(x, W, b):
    """clf_linear_kernel: acc = bias[o]; acc = fma(x[k], W[k, o], acc) for k in order."""
    acc = np.broadcast_to(b.astype(np.float32), (len(x), W.shape[1])).copy()
    for k in range(W.shape[0]):
        acc = _fma32(x[:, k:k + 1], W[k:k + 1, :], acc)
    return acc


def linear_bwd32(g, W):
    """clf_linear_bwd_kernel: dx[b, i] = fma(g[b, o], W[i, o], acc) for o in order, from 0."""
    acc = np.zeros((len(g), W.shape[0]), np.float32)
    for o in range(W.shape[1]):
        acc = _fma32(g[:, o:o + 1], W[:, o][None, :], acc)
    return acc


def _butterfly_sum32(lanes):
    """[B, 64] float32 -> [B]: s += shfl_xor(s, d) for d = 32 .. 1, every lane at once; lane 0's value."""
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, idx ^ d]).astype(np.float32)
    return lanes[:, 0]


def softmax_seed32(z, classes):
    """jac_seed_kernel in NumPy float32: the classes strided over 64 lanes (lane l sums exp(z_k - m) for k = l, l + 64, ... in order),
    the lane sums through the butterfly, inv = 1 / s, p_c = exp(z_c - m) * inv, seed_k = (delta_kc - p_c) * (exp(z_k - m) * inv).
    A class outside [0, n) gives a zero row."""
    z = np.asarray(z, np.float32)
    B, n = z.shape
    classes = np.asarray(classes)
    m = z.max(axis=1, keepdims=True)
    e = np.exp((z - m).astype(np.float32)).astype(np.float32)
    lanes = np.zeros((B, 64), np.float32)
    for k in range(n):
        lanes[:, k % 64] = (lanes[:, k % 64] + e[:, k]).astype(np.float32)
    inv = (np.float32(1.0) / _butterfly_sum32(lanes)).astype(np.float32)[:, None]
    p = (e * inv).astype(np.float32)
    valid = (classes >= 0) & (classes < n)
    safe = np.where(valid, classes, 0)
    onehot = np.zeros((B, n), np.float32)
    onehot[np.arange(B), safe] = 1
    seed = ((onehot - p[np.arange(B), safe][:, None]).astype(np.float32) * p).astype(np.float32)
    seed[~valid] = 0
    return seed


def class_gradient32(kind, params, x, classes):
    """d softmax(logits(x))[b, classes[b]] / dx of the two models in float32, every sum in the device's documented order."""
    p = [(np.asarray(W, np.float32), np.asarray(b, np.float32)) for W, b in params]
    h = np.asarray(x, np.float32).reshape(len(x), -1)
    if kind == "lin":
        return linear_bwd32(softmax_seed32(linear32(h, *p[0]), classes), p[0][0]).reshape(np.shape(x))
    a = np.maximum(linear32(h, *p[0]), np.float32(0))
    g = linear_bwd32(softmax_seed32(linear32(a, *p[1]), classes), p[1][0])
    g = np.where(a > 0, g, np.float32(0))                       # the ReLU fused into the first Linear: out > 0
    return linear_bwd32(g, p[0][0]).reshape(np.shape(x))


# ---------------------------------------------------------------------- best tracking on prescribed predictions, long batches
TRACK_PATTERNS = ("first at 1", "first at 3", "never", "at 1, undone at 2 and 3", "at 2, undone at 3")


def track_case(B, row_elems, seed=0):
    """Prescribed predictions for three dg_bpda_track calls: image b follows TRACK_PATTERNS[b % 5], so that every pattern sits below
    the grid cap, in the second pass and among the last three images of B = 2 * cap + 3.  -> (labels [B] int32, preds {k: [B] int32},
    iterates [x_0 .. x_3] float32 [B, row_elems], want_first [B]): want_first written out per pattern, not computed by track()."""
    rs = np.random.RandomState(seed + row_elems)
    labels = rs.randint(0, 10, B).astype(np.int32)
    wrong = ((labels + 1 + rs.randint(0, 9, B)) % 10).astype(np.int32)
    pat = np.arange(B) % 5
    hits = {1: (pat == 0) | (pat == 3), 2: pat == 4, 3: (pat == 1) | (pat == 0)}       # pattern 0 is wrong again at 3: nothing changes
    preds = {k: np.where(hits[k], wrong, labels).astype(np.int32) for k in (1, 2, 3)}
    iterates = [rs.standard_normal((B, row_elems)).astype(np.float32) for _ in range(4)]
    want_first = np.array([1, 3, -1, 1, 2], np.int32)[pat]
    return labels, preds, iterates, want_first
