"""CPU restatement of the BPDA/EOT projected sign-gradient attack ("BPDA/EOT"), float64 NumPy, written
independently of the device code (defensegan_amd/csrc/dg_bpda.hip, network_builder.BPDA).  The projection and the classifier's
input gradient are the oracle's (oracle/defensegan_oracle.py, oracle/classifier_oracle.py); the latents of every projection are
handed in as z0 blocks, one per seed, so the latents' generator is not restated (the GPU tests fetch the blocks with
dg_init_latents).  The one generator restated here is the ``rand_init`` draw's Philox4x32-10.

    ops = oracle_ops(gan_params, "mnist", layers, clf_params, y, z0_of_seed, R, L, lr)
    out = bpda(ops, x, y, eps, eps_iter, nb_iter, m, lo, hi, seed)        # x_adv, first_success, iterates, grads, seeds
"""
import numpy as np

NOISE_TAG = 0x42504441
_M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------- the definition
def step_rule(x, x_k, g, eps, eps_iter, lo, hi):
    """x_{k+1} = clip(x + clamp(x_k + eps_iter sign(g) - x, -eps, eps), lo, hi); np.sign(0) = 0."""
    return np.clip(x + np.clip(x_k + eps_iter * np.sign(g) - x, -eps, eps), lo, hi)


def eot_sum(grads):
    """g_0 + g_1 + ... + g_{m-1}, in that order: a sum, not a mean."""
    acc = np.array(grads[0], np.float64, copy=True)
    for g in grads[1:]:
        acc = acc + g
    return acc


def seed_schedule(seed, nb_iter, m):
    """([[seed + k m + s for s < m] for k < nb_iter], seed + nb_iter m)."""
    return [[seed + k * m + s for s in range(m)] for k in range(nb_iter)], seed + nb_iter * m


def track(preds_of_iterate, labels, iterates):
    """Best tracking.  preds_of_iterate[j], j = 1 .. nb_iter: the defended predictions [n] on iterate j; iterates[j] = x_j.
    Returns (x_adv, first_success): per image the first iterate whose prediction is not the label, or the last one and -1."""
    nb_iter = len(iterates) - 1
    labels = np.asarray(labels)
    first = np.full(len(labels), -1, np.int32)
    x_adv = np.array(iterates[nb_iter], copy=True)
    for j in range(1, nb_iter + 1):
        hit = (first < 0) & (np.asarray(preds_of_iterate[j]) != labels)
        x_adv[hit] = iterates[j][hit]
        first[hit] = j
    return x_adv, first


def bpda(ops, x, y, eps, eps_iter, nb_iter, m, lo, hi, seed, x_init=None, noise=None):
    """ops.project(x_k, seed) -> rec, ops.gradient(rec) -> d CE / d rec, ops.predict(rec) -> [n] classes.  ``noise``: the
    rand_init draw (rand_noise).  Returns a dict: x_adv, first_success, iterates [x_0 .. x_nb_iter], grads [g_0 .. g_{nb_iter-1}],
    seeds (every projection's seed in call order)."""
    x = np.asarray(x, np.float64)
    lo = -np.inf if lo is None else lo
    hi = np.inf if hi is None else hi
    if x_init is not None:
        x_k = np.asarray(x_init, np.float64)
    elif noise is not None:
        x_k = np.clip(x + np.asarray(noise, np.float64).reshape(x.shape), lo, hi)
    else:
        x_k = np.clip(x, lo, hi)
    sched, final = seed_schedule(seed, nb_iter, m)
    iterates, grads, preds, used = [x_k], [], {}, []
    for k in range(nb_iter):
        gs = []
        for s in range(m):
            rec = ops.project(x_k, sched[k][s])
            used.append(sched[k][s])
            if s == 0 and k > 0:
                preds[k] = ops.predict(rec)              # the defended view of iterate k, at no extra projection
            gs.append(ops.gradient(rec))
        g = eot_sum(gs)
        grads.append(g)
        x_k = step_rule(x, x_k, g, eps, eps_iter, lo, hi)
        iterates.append(x_k)
    preds[nb_iter] = ops.predict(ops.project(x_k, final))
    used.append(final)
    x_adv, first = track(preds, y, iterates)
    return {"x_adv": x_adv, "first_success": first, "iterates": iterates, "grads": grads, "seeds": used, "preds": preds}


# ---------------------------------------------------------------------- the rand_init draw
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


def rand_noise(n_images, row_elems, eps, seed, first_image=0):
    """float32 [n_images, row_elems]: element e of global image i takes word e % 4 of Philox(key = (seed lo, seed hi), counter =
    (e // 4, i lo, i hi, NOISE_TAG)); u = (word >> 8) 2^-24; noise = float32(eps) * (2 u - 1).  Written image by image."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (row_elems + 3) // 4
    out = np.empty((n_images, row_elems), np.float32)
    for r in range(n_images):
        i = first_image + r
        ctr = np.zeros((nq, 4), np.uint64)
        ctr[:, 0] = np.arange(nq, dtype=np.uint64)
        ctr[:, 1] = i & 0xFFFFFFFF
        ctr[:, 2] = i >> 32
        ctr[:, 3] = NOISE_TAG
        words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:row_elems]
        u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        out[r] = np.float32(eps) * (np.float32(2.0) * u - np.float32(1.0))
    return out


# ---------------------------------------------------------------------- the oracle behind ops, and the shared test case
class oracle_ops(object):
    """project = the float64 projection loop from the z0 block of the seed, gradient = the oracle's cross-entropy input
    gradient for the labels y, predict = first argmax of the oracle's logits."""

    def __init__(self, gan_params, arch, layers, clf_params, y, z0_of_seed, R, L, lr, momentum=0.7):
        self.p, self.arch, self.layers, self.y, self.z0, self.R, self.L, self.lr, self.mom = gan_params, arch, layers, np.asarray(y), z0_of_seed, R, L, lr, momentum
        self.cp = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in clf_params]

    def project(self, x_k, seed):
        from oracle import defensegan_oracle as O
        z0 = np.asarray(self.z0[seed], np.float64)
        return O.reconstruct(self.p, x_k, z0, self.R, self.L, lr=self.lr, momentum=self.mom, arch=self.arch, dtype=np.float64)["rec"]

    def gradient(self, rec):
        from oracle import classifier_oracle as CO
        return CO.input_gradient(self.layers, self.cp, rec, self.y)

    def predict(self, rec):
        from oracle import classifier_oracle as CO
        return CO.forward(self.layers, self.cp, rec)[0].argmax(axis=1)


def layers_of(model):
    """The model's layers as the oracle's tuples."""
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


def init_params(model, seed):
    """Fixed random classifier weights without touching the device: normal, normalised per output unit, small random biases."""
    rs = np.random.RandomState(seed)
    out = []
    for ws, bs in model.param_shapes():
        W = rs.standard_normal(ws)
        W = W / np.sqrt(1e-7 + np.square(W).sum(axis=tuple(range(len(ws) - 1)), keepdims=True))
        out.append((W.astype(np.float32), (0.1 * rs.standard_normal(bs)).astype(np.float32)))
    return out


# The teacher-forced GPU case, fixed on the CPU (tests/test_bpda_cpu.py asserts what the choice promises): MNIST generator at
# gain 2.0 (the contractive regime), clean in-range targets, R = 2, L = 5, lr 10 as the short-horizon golden files; classifier F.
CASE = dict(arch="mnist", wseed=1234, gain=2.0, bias_range=0.1, B=7, R=2, L=5, lr=10.0, clf="F", clf_seed=70, x_seed=31, seed=4100,
            eps=0.3, eps_iter=0.05, lo=0.0, hi=1.0)


def case_inputs(case=CASE):
    """(gan_params, x [B,H,W,C] float32, y [B] int32, model (no device touched), clf_params)."""
    from defensegan_amd import network_builder as nb, synth
    from tests.helpers import clean_targets
    p = synth.make_weights(case["arch"], seed=case["wseed"], gain=case["gain"], bias_range=case["bias_range"])
    x, _ = clean_targets(p, case["arch"], case["B"], case["x_seed"])
    shape = (None,) + tuple(x.shape[1:])
    model = nb.MODELS[case["clf"]](input_shape=shape)
    y = np.random.RandomState(case["x_seed"] + 1).randint(0, 10, case["B"]).astype(np.int32)
    return p, x, y, model, init_params(model, case["clf_seed"])


def host_z0_blocks(seeds, n_rows, latent, salt=0):
    """N(0, 1/latent) blocks from NumPy, for CPU runs of the reference (the device draws other values for the same seeds)."""
    return {s: (np.random.RandomState((s + salt) % (2 ** 32)).standard_normal((n_rows, latent)) * np.sqrt(1.0 / latent)).astype(np.float32)
            for s in seeds}


def undecided_fraction(g):
    """Share of pixels whose sign a float32 run may take differently: |g| <= 1e-4 max|g| (tests/test_classifier.py's FGSM rule)."""
    g = np.abs(np.asarray(g))
    return float((g <= 1e-4 * g.max()).mean())
