"""CPU restatement of the SPSA attack ("SPSA"), NumPy, written independently of the device code
(defensegan_amd/csrc/dg_spsa.hip, network_builder.SPSA).  The direction bits are Philox4x32-10 (bpda_reference.philox4x32_10,
pinned there by known answers); the queries are float32, exactly as the device forms them; margins, estimate and loop are float64.

    u = directions(B, P, n, seed, first_image, k)                  # [B, n, P] of +-1
    q = queries(x_k, n, delta, seed, first_image, k, lo, hi)       # [B, 2n+1, P] float32
    out = spsa(logits_of, x, y, eps, eps_iter, nb_iter, n, delta, lo, hi, seed)
"""
import numpy as np

from tests.support.bpda_reference import philox4x32_10, step_rule, track

SPSA_TAG = 0x53505341          # "SPSA": word 3 of the direction counter


# ---------------------------------------------------------------------- directions and queries
def direction_bits(n_images, P, n, seed, first_image=0, k=0):
    """bool [n_images, n, P]: bit (i & 31) of word (e & 3) of Philox(key = (seed lo, seed hi), counter = (e >> 2, g,
    k ceil(n / 32) + (i >> 5), SPSA_TAG)), g = first_image + row.  Written image by image, group by group."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    groups, nq = (n + 31) // 32, (P + 3) // 4
    if first_image + n_images > 2 ** 32 or k * groups + groups > 2 ** 32:
        raise ValueError("the counter words would wrap")
    out = np.empty((n_images, n, P), bool)
    for r in range(n_images):
        for grp in range(groups):
            ctr = np.zeros((nq, 4), np.uint64)
            ctr[:, 0] = np.arange(nq, dtype=np.uint64)
            ctr[:, 1] = first_image + r
            ctr[:, 2] = k * groups + grp
            ctr[:, 3] = SPSA_TAG
            words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:P]
            for i in range(32 * grp, min(n, 32 * grp + 32)):
                out[r, i] = ((words >> np.uint64(i & 31)) & np.uint64(1)).astype(bool)
    return out


def directions(n_images, P, n, seed, first_image=0, k=0):
    """float64 [n_images, n, P]: +1 where the bit is set, else -1."""
    return np.where(direction_bits(n_images, P, n, seed, first_image, k), 1.0, -1.0)


def queries(x_k, n, delta, seed, first_image, k, lo, hi):
    """float32 [B, 2n+1, P]: row 0 the iterate itself, rows 1 + 2i / 2 + 2i = clip(x_k +- delta u_i), one float32 rounding each."""
    x_k = np.asarray(x_k, np.float32)
    B, P = x_k.shape[0], int(np.prod(x_k.shape[1:]))
    xf = x_k.reshape(B, 1, P)
    d = np.where(direction_bits(B, P, n, seed, first_image, k), np.float32(delta), -np.float32(delta)).astype(np.float32)
    q = np.empty((B, 2 * n + 1, P), np.float32)
    q[:, 0] = xf[:, 0]
    q[:, 1::2] = np.clip(xf + d, np.float32(lo), np.float32(hi))
    q[:, 2::2] = np.clip(xf - d, np.float32(lo), np.float32(hi))
    return q


# ---------------------------------------------------------------------- loss, estimate
def margins(Z, y):
    """L = max_{j != y} Z_j - Z_y per query, float64; Z [B, Q, classes], y [B].  The maximum propagates NaN.  A label outside
    [0, classes) gives L = 0 for every query of the image."""
    Z = np.asarray(Z, np.float64)
    B, Q, C = Z.shape
    out = np.zeros((B, Q))
    for b in range(B):
        if 0 <= int(y[b]) < C:
            rest = np.delete(Z[b], int(y[b]), axis=1)
            with np.errstate(invalid="ignore"):
                out[b] = rest.max(axis=1) - Z[b, :, int(y[b])]
    return out


def delta_losses(Z, y):
    """dL_i = L(q+_i) - L(q-_i) [B, n] float64; a pair whose dL is not finite AS A FLOAT32 (NaN, +-inf, inf - inf, beyond float32's
    range) contributes 0."""
    L = margins(Z, y)
    with np.errstate(invalid="ignore", over="ignore"):
        d = L[:, 1::2] - L[:, 2::2]
        bad = ~np.isfinite(d.astype(np.float32))
    return np.where(bad, 0.0, d)


def estimate(dL, u, delta):
    """ghat [B, P] = (1 / (2 delta n)) sum_i dL_i u_i, float64 (delta as the float32 the device is handed)."""
    n = dL.shape[1]
    return np.einsum("bi,bip->bp", dL, u) / (2.0 * float(np.float32(delta)) * n)


def estimate_bound(dL, delta):
    """Per image, what a fixed-order float32 evaluation may differ from ``estimate`` by: (n + 2) 2^-24 sum_i |dL_i| / (2 delta n)
    -- dL's one rounding, n - 1 additions, the product with the scale and the scale's own rounding."""
    n = dL.shape[1]
    return (n + 2) * 2.0 ** -24 * np.abs(dL).sum(axis=1) / (2.0 * float(np.float32(delta)) * n)


# ---------------------------------------------------------------------- the loop
def spsa(logits_of, x, y, eps, eps_iter, nb_iter, n, delta, lo, hi, seed, first_image=0):
    """``logits_of(q [N, P] float32, what)`` -> [N, classes] is the attacked model (``what`` = the iteration k, or "closing").
    Returns a dict: x_adv, first_success, queries (per image), iterates [x_0 .. x_nb_iter], grads, margin0 {j: the margins of
    iterate j's own query 0, j = 1 .. nb_iter}."""
    x = np.asarray(x, np.float64)
    B, P = x.shape[0], int(np.prod(x.shape[1:]))
    xf = x.reshape(B, P)
    lo = -np.inf if lo is None else lo
    hi = np.inf if hi is None else hi
    x_k = np.clip(xf, lo, hi)
    iterates, grads, preds, margin0 = [x_k], [], {}, {}
    y = np.asarray(y)

    def judge(Z0, j):
        preds[j] = np.asarray(Z0, np.float64).argmax(axis=1)          # first maximum
        margin0[j] = margins(np.asarray(Z0)[:, None, :], y)[:, 0]

    for k in range(nb_iter):
        q = queries(x_k.astype(np.float32), n, delta, seed, first_image, k, lo, hi)
        Z = np.asarray(logits_of(q.reshape(-1, P), k), np.float64).reshape(B, 2 * n + 1, -1)
        if k > 0:
            judge(Z[:, 0], k)
        g = estimate(delta_losses(Z, y), directions(B, P, n, seed, first_image, k), delta)
        grads.append(g)
        x_k = step_rule(xf, x_k, g, eps, eps_iter, lo, hi)
        iterates.append(x_k)
    judge(logits_of(x_k.astype(np.float32), "closing"), nb_iter)
    x_adv, first = track(preds, y, iterates)
    shape = x.shape
    return {"x_adv": x_adv.reshape(shape), "first_success": first, "queries": nb_iter * (2 * n + 1) + 1,
            "iterates": [v.reshape(shape) for v in iterates], "grads": grads, "margin0": margin0, "preds": preds}


# ---------------------------------------------------------------------- the GPU cases, fixed on the CPU (tests/test_spsa_cpu.py)
# Kernel cases of tests/test_gpu_spsa.py: a second Philox group with one live direction, an image index and an iteration other than 0.
KERNEL = dict(B=3, n=33, first_image=5, k=2, delta=0.01, seed=(7 << 32) | 0x5EED, lo=0.0, hi=1.0, classes=10)


def kernel_inputs(P, case=KERNEL):
    """(x_cur [B, P], x_orig [B, P], Z [B (2n+1), classes], y [B]) float32 / int32: x_cur holds elements AT both clip bounds (so
    the queries' clip is live) and within eps of x_orig; the logits are random (teacher-forced); image 1's label is out of range."""
    rs = np.random.RandomState(1000 + P)
    B = case["B"]
    x_orig = rs.uniform(0.0, 1.0, (B, P)).astype(np.float32)
    x_cur = np.clip(x_orig + rs.uniform(-0.1, 0.1, (B, P)), 0.0, 1.0).astype(np.float32)
    x_cur[:, 0::7] = 0.0
    x_cur[:, 3::7] = 1.0
    Z = (3.0 * rs.standard_normal((B * (2 * case["n"] + 1), case["classes"]))).astype(np.float32)
    y = np.array([4, case["classes"], 9], np.int32)
    return x_cur, x_orig, Z, y


# The composition case: a bare Flatten + Linear classifier over 5 x 5 x 1 inputs in which EVERY value is a dyadic rational with few
# bits -- x on the 1/64 grid, W in eighths, delta = 1/64, eps_iter = 1/16, n = 4 so that 1 / (2 delta n) = 8 -- so float32 and
# float64 compute the same logits, margins, estimate and iterates exactly, and no margin of a judged iterate is 0.
COMPOSE = dict(B=6, n=4, classes=3, nb_iter=4, delta=1.0 / 64, eps=0.1875, eps_iter=0.0625, lo=0.0, hi=1.0, seed=(3 << 32) | 99)


def compose_inputs(case=COMPOSE):
    """(x [B,5,5,1] float32, y [B] int32, W [25, classes] float32, b [classes] float32)."""
    rs = np.random.RandomState(77)
    x = (rs.randint(8, 57, (case["B"], 5, 5, 1)) / 64.0).astype(np.float32)
    W = (rs.randint(-8, 9, (25, case["classes"])) / 8.0).astype(np.float32)
    b = (rs.randint(-4, 5, case["classes"]) / 8.0).astype(np.float32)
    y = (x.reshape(case["B"], 25).astype(np.float64) @ W + b).argmax(axis=1).astype(np.int32)       # the clean prediction
    return x, y, W, b
