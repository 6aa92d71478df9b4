"""The Carlini-Wagner edge cases shared by tests/test_cw_cpu.py (which asserts, on the float64 reference alone, the properties
they were chosen for: decidable, and sensitive to the bug each is meant to catch) and tests/test_gpu_cw_edges.py (which compares
the device with the reference on them).  Models, images, labels, parameters and seeds live here; nothing here touches a device.

    a  confidence    model F, 16 images, kappa 0.5 / 5.0, 5 / 20 iterations, untargeted and targeted
    b  ties          the 60-pixel model T whose last layer has columns 1 = 2 and 3 = 4 = 5; labels 0, and the model's own labels
                     (model U = T with class 0 moved down) at kappa 0.5 and at kappa 0, where the first-argmax rule decides
    c  clip edges    T and F, ranges [0, 1] and [-1, 1], pixels below, above and exactly on the bounds; the degenerate schedules
    d  abort         model F, 20 images in chunks of 8, three outer steps with abort_early on, 30 and 7 iterations
    e  chunking      the runs of (a) at other batch sizes (bit-identity on the device; the reference has nothing to add)
    f  bad labels    labels outside the classes through the C ABI; the reference runs the two good rows, which carry their own
                     classes 3 and 1

Gates of tests/test_gpu_cw.py, which the GPU tests use and the sensitivity assertions scale by ten.
"""
import functools

import numpy as np

from tests.support import cw_reference as R

L2_RTOL = 1e-3            # best_l2
PIXEL_ATOL = 1e-4         # |x_adv - ref| on at least PIXEL_SHARE of the pixels
PIXEL_SHARE = 0.999
CONST_RTOL = 1e-12        # final_const
IMAGE_MARGIN = 1e-4       # an image is undecidable below this share of its largest |logit| (success and arg margins)
CHECK_MARGIN = 1e-5       # a chunk is undecidable below this (abort checks)

TIE_SHAPE = (6, 5, 2)     # 60 pixels: fewer than one workgroup, no multiple of 64
TIE_GROUPS = ((1, 2), (3, 4, 5))
TIE_OWN_SHIFT = -1.0


def model(name, input_shape=None):
    """The case's model as a network_builder.MLP (no device is touched before its first use)."""
    from defensegan_amd import network_builder as nb
    if name in "TU":
        return nb.MLP([nb.Flatten(), nb.Linear(32), nb.ReLU(), nb.Linear(6)], (None,) + TIE_SHAPE)
    return nb.MODELS[name]()


@functools.lru_cache(maxsize=None)
def params(name):
    """float32 (W, b) pairs.  F and A: MLP.init_like_reference(seed=ord(name)) (its own code, the installation on the device
    left out), the last layer times 16 so that kappa = 0.5 and 5 both lie inside the range the logits move through in 20
    iterations.  T: a normalised Linear, then six columns that share a common part, so that the groups stay close and the top
    changes hands within the first iterations; class 0 starts a little ahead."""
    if name == "U":                               # T with class 0 moved down: the tied groups are on top of most images
        (W1, b1), (W2, b2) = params("T")
        return [(W1, b1), (W2, b2 + np.array([TIE_OWN_SHIFT, 0, 0, 0, 0, 0], np.float32))]
    if name == "T":
        rs = np.random.RandomState(60)
        W1 = rs.standard_normal((60, 32))
        W1 = (W1 / np.sqrt(np.square(W1).sum(axis=0, keepdims=True))).astype(np.float32)
        b1 = rs.uniform(-0.1, 0.1, 32).astype(np.float32)
        W2 = (rs.standard_normal((32, 1)) + 0.3 * rs.standard_normal((32, 6))).astype(np.float32)
        b2 = np.array([0.05, 0.0, 0.0, 0.0, 0.0, 0.0], np.float32)
        for g in TIE_GROUPS:
            W2[:, g[1:]] = W2[:, g[:1]]
        return [(W1, b1), (W2, b2)]
    m = model(name)
    m.set_weights = lambda p: None
    p = m.init_like_reference(seed=ord(name))
    return p[:-1] + [(p[-1][0] * np.float32(16), p[-1][1])]


def params64(name):
    return [(W.astype(np.float64), b.astype(np.float64)) for W, b in params(name)]


def reference_logits(name, x):
    import torch
    with torch.no_grad():
        return R.logits(R.layers_of(model(name)), params64(name), torch.as_tensor(np.asarray(x, np.float64))).numpy()


def _edge_pixels(x, lo, hi, rs):
    """In each image a fifth of the pixels below lo, a fifth above hi, a tenth exactly lo and a tenth exactly hi."""
    flat = x.reshape(len(x), -1)
    P = flat.shape[1]
    for row in flat:
        idx = rs.permutation(P)
        a, b, c, d = idx[:P // 5], idx[P // 5:2 * (P // 5)], idx[2 * (P // 5):2 * (P // 5) + P // 10], idx[-(P // 10):]
        row[a] = lo - rs.uniform(0.01, 0.5, len(a))
        row[b] = hi + rs.uniform(0.01, 0.5, len(b))
        row[c] = lo
        row[d] = hi
    return x


@functools.lru_cache(maxsize=None)
def images(name, n, seed, lo=0.0, hi=1.0, edges=False):
    shape = TIE_SHAPE if name in "TU" else (28, 28, 1)
    rs = np.random.RandomState(seed)
    x = rs.uniform(lo, hi, (n,) + shape).astype(np.float32)
    if edges:
        x = _edge_pixels(x, np.float32(lo), np.float32(hi), rs)
    x.setflags(write=False)
    return x


def own_labels(name, x):
    return reference_logits(name, x).argmax(axis=1)


def targets(name, x):
    """The runner-up class of every image: the target a few iterations can reach."""
    return np.argsort(reference_logits(name, x), axis=1)[:, -2]


# ---------------------------------------------------------------------- the cases: name -> (model, x, labels, targeted, parameters)
_A = dict(batch_size=16, learning_rate=0.01, binary_search_steps=1, abort_early=False, initial_const=100.0)
_B = dict(batch_size=16, learning_rate=0.1, binary_search_steps=1, abort_early=False, initial_const=100.0)
_C = {"T": dict(_B, learning_rate=0.2), "F": dict(_A, learning_rate=0.03)}      # five iterations must bring successes AND failures
_D = dict(batch_size=8, binary_search_steps=3, abort_early=True)
_D_SEARCH = {30: dict(learning_rate=0.01, initial_const=0.3), 7: dict(learning_rate=0.012, initial_const=0.3)}
TIE_OWN_CONFIDENCE = 0.5      # with the model's own labels the label sits in a tied group: arg = kappa exactly, so kappa is not 0

A_NAMES = tuple("a-%s-k%s-i%d" % (m, k, i) for m in ("untargeted", "targeted") for k in ("0.5", "5.0") for i in (5, 20))
B_NAMES = tuple("b-i%d" % i for i in (1, 2, 3, 6))
C_NAMES = tuple("c-%s-%s" % (m, r) for m in ("T", "F") for r in ("01", "11"))
D_NAMES = ("d-i30", "d-i7")
OWN_K0 = "b-own-k0"
NAMES = A_NAMES + B_NAMES + ("b-own",) + C_NAMES + D_NAMES + ("f-good",)
BAD_LABELS = (-1, 10, 3, 0x7fffffff, 1)       # case f, model F (10 classes): rows 0, 1 and 3 are outside the classes


def case(name):
    """-> dict(model=, x=, labels= (None: the model's own), targeted=, kw= (the parameters of cw_l2 / generate))."""
    part = name.split("-")
    if part[0] == "a":
        x = images("F", 16, 5)
        targeted = part[1] == "targeted"
        kw = dict(_A, confidence=float(part[2][1:]), max_iterations=int(part[3][1:]))
        return dict(model="F", x=x, labels=targets("F", x) if targeted else own_labels("F", x), targeted=targeted, kw=kw)
    if name == "b-own":
        return dict(model="U", x=images("U", 16, 61), labels=None, targeted=False,
                    kw=dict(_B, confidence=TIE_OWN_CONFIDENCE, max_iterations=10))
    if name == OWN_K0:          # not in NAMES: its tied images sit at arg = 0 exactly, see tied_own()
        return dict(model="U", x=images("U", 16, 61), labels=None, targeted=False, kw=dict(_B, confidence=0.0, max_iterations=6))
    if part[0] == "b":
        return dict(model="T", x=images("T", 16, 61), labels=np.zeros(16, np.int64), targeted=False,
                    kw=dict(_B, max_iterations=int(part[1][1:])))
    if part[0] == "c":
        lo, hi = (0.0, 1.0) if part[2] == "01" else (-1.0, 1.0)
        x = images(part[1], 16, 62, lo, hi, True)
        kw = dict(_C[part[1]], max_iterations=5, clip_min=lo, clip_max=hi)
        return dict(model=part[1], x=x, labels=own_labels(part[1], np.clip(x, lo, hi)) if part[1] == "F" else np.zeros(16, np.int64),
                    targeted=False, kw=kw)
    if part[0] == "d":
        return dict(model="F", x=images("F", 20, 7), labels=own_labels("F", images("F", 20, 7)), targeted=False,
                    kw=dict(_D, max_iterations=int(part[1][1:]), **_D_SEARCH[int(part[1][1:])]))
    if name == "f-good":
        return dict(model="F", x=bad_label_images()[[2, 4]], labels=np.array(BAD_LABELS)[[2, 4]], targeted=False,
                    kw=dict(_A, batch_size=1, binary_search_steps=2, max_iterations=5))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def image_of_class(name, cls, seed):
    """One float32 image that the model puts into ``cls`` by a margin: uniform images all fall into classes 0 and 3 of model F, so
    the image is what a targeted reference attack with kappa = 2 makes of a uniform one."""
    x0 = images(name, 1, seed)
    out = R.cw_l2(R.layers_of(model(name)), params64(name), x0.astype(np.float64), labels=np.array([cls]), targeted=True, batch_size=1,
                  confidence=2.0, learning_rate=0.05, binary_search_steps=1, max_iterations=40, abort_early=False, initial_const=100.0)
    assert out["best_class"][0] == cls
    return out["x_adv"].astype(np.float32)[0]


@functools.lru_cache(maxsize=None)
def bad_label_images():
    """Five images for BAD_LABELS: the good rows 2 and 4 are images whose own classes ARE 3 and 1, so that their attacks run
    through all 2 x 5 iterations instead of succeeding on the spot."""
    x = np.array(images("F", 5, 8))
    pool = images("F", 16, 8)
    x[2] = pool[np.flatnonzero(own_labels("F", pool) == BAD_LABELS[2])[1]]
    x[4] = image_of_class("F", BAD_LABELS[4], 8)
    x.setflags(write=False)
    return x


def bad_label_case():
    """Case f as the C ABI gets it: five images, BAD_LABELS, the parameters of "f-good"."""
    return dict(model="F", x=bad_label_images(), labels=np.array(BAD_LABELS, np.int64).astype(np.int32), good=[2, 4], bad=[0, 1, 3],
                kw=case("f-good")["kw"])


def tied_own(ref):
    """[N] bool: the images of a y=None run on model U whose own label sits in a tied group.  At kappa = 0 their arg and success
    margins are 0 by construction, not by accident: the label's twin has the same logit bit for bit, in float64 and on the
    device alike, so the decision is exact on both sides and these images are compared although decidable() leaves them out."""
    return ref["labels"] != 0


def run(name, **override):
    """cw_l2 on the case, with its trace; ``override`` replaces parameters (the CPU tests ask what kappa = 0 would have done)."""
    c = case(name)
    kw = dict(c["kw"], **override)
    return R.cw_l2(R.layers_of(model(c["model"])), params64(c["model"]), c["x"].astype(np.float64), labels=c["labels"],
                   targeted=c["targeted"], trace=True, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of the case, computed once and shared (do not modify it)."""
    return run(name)


def decidable(ref):
    """-> (keep [N] bool, chunks_ok bool): images whose smallest success / arg margin stays above IMAGE_MARGIN of their largest
    |logit|, and whether every abort check of every chunk stays above CHECK_MARGIN."""
    tr = ref["trace"]
    N = len(ref["best_l2"])
    both = np.concatenate([tr["success_margin"].reshape(N, -1), tr["arg_margin"].reshape(N, -1)], axis=1)
    smallest = np.where(np.isnan(both), np.inf, both).min(axis=1) if both.shape[1] else np.full(N, np.inf)
    keep = smallest >= IMAGE_MARGIN * tr["max_logit"]
    checks = [m for step in tr["check_margin"] for chunk in step for m in chunk]
    return keep, all(m >= CHECK_MARGIN for m in checks)


def stops(ref):
    """abort_iters as the device returns chunk_stop: -1 for None."""
    return [[-1 if s is None else s for s in row] for row in ref["abort_iters"]]


def differs(ref, other, batch_size, factor=10.0):
    """[N] bool: the images on which ``other`` misses the GPU test's gates by more than ``factor`` times (a non-finite value misses
    any gate; a chunk whose stop iterations differ counts with all its images)."""
    N = len(ref["best_l2"])
    out = ref["best_class"] != other["best_class"]
    with np.errstate(invalid="ignore"):
        out |= ~(np.abs(other["best_l2"] - ref["best_l2"]) <= factor * L2_RTOL * np.abs(ref["best_l2"]))
        far = ~(np.abs(other["x_adv"] - ref["x_adv"]) <= factor * PIXEL_ATOL)
        out |= far.reshape(N, -1).mean(axis=1) > min(factor * (1 - PIXEL_SHARE), 1.0)
        out |= ~(np.abs(other["const"] - ref["const"]) <= factor * CONST_RTOL * np.abs(ref["const"]))
    a, b = np.array(stops(ref)), np.array(stops(other))
    if a.size:
        out |= np.repeat((a != b).any(axis=0), batch_size)[:N]
    return out
