"""The attacks on the classifier container of network_builder.py, where the reference takes them from ``cleverhans.attacks``:
FastGradientMethod and CarliniWagnerL2 (the reference's own), ElasticNetMethod (the L1 attack), ProjectedGradientDescent, and the three that see or get round the
defense -- BPDA, SPSA, LatentAttack --, DeepFool with the ``robustness`` it measures, and SaliencyMapMethod (the L0 attack).  Every ``generate`` is the same host-side front end (the functions up to ``_pack``) around
one or a few device calls; the arithmetic runs in the HIP library.  ``network_builder.X`` keeps resolving every name here."""
from __future__ import annotations

import numpy as np

from . import _native, network_builder as nb
from .network_builder import MLP

_L1_ITERATIVE_NOTE = ("ord = 1 is not implemented for the iterative attacks: the projection onto an L1 ball needs a sort per image; "
                      "ord = np.inf and ord = 2 are")


def _attack_ord(ord, allowed, who):
    """``ord`` as np.inf, 1 or 2 ('inf' and float('inf') are np.inf); anything else, or a value not in ``allowed``, is refused."""
    if isinstance(ord, str):
        ord = {"inf": np.inf, "1": 1, "2": 2}.get(ord.lower(), ord)
    if not isinstance(ord, str) and ord in (np.inf, 1, 2):
        ord = np.inf if ord == np.inf else int(ord)
        if ord in allowed:
            return ord
        if ord == 1:
            raise NotImplementedError("%s: %s" % (who, _L1_ITERATIVE_NOTE))
    raise ValueError("%s: ord must be one of %s, got %r" % (who, ", ".join("np.inf" if a == np.inf else str(a) for a in allowed), ord))


# ---------------------------------------------------------------------- the front end of every generate
_ptr = lambda t: t.data_ptr() if t is not None else None


def _labels(y, n, dev, required=True, range_words=None, nb_classes=None):
    """int32 labels on ``dev`` from class indices or one-hot rows (NumPy, tensor or list); None for ``y`` None unless ``required``.
    ``n``: the length asked for (None: unchecked, FGSM).  ``range_words``: None -- no range check: on the device an index outside
    [0, nb_classes) means a zero gradient or a zero step --, or whose words refuse such an index: 'cw', or any other name ('latent', 'jsma') for the plain words."""
    import torch
    if y is None and not required:
        return None
    yy = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y)
    if yy.ndim > 1:
        yy = yy.argmax(axis=-1)                                    # one-hot labels as cleverhans takes them
    bad_shape = n is not None and yy.shape != (n,)
    bad_range = range_words is not None and not bad_shape and bool((yy < 0).any() or (yy >= nb_classes).any())
    if range_words == "cw" and (bad_shape or bad_range):
        raise ValueError("labels must be %d class indices in [0, %d) or one-hot rows" % (n, nb_classes))
    if bad_shape:
        raise ValueError("y must be %d class indices or one-hot rows" % n)
    if bad_range:
        raise ValueError("y holds a class index outside [0, %d)" % nb_classes)
    return torch.from_numpy(np.ascontiguousarray(yy.astype(np.int32))).to(dev)


def _clip_bounds(clip_min, clip_max, ordered=True):
    """``(lo, hi)`` as floats, None = unbounded; ``ordered`` refuses lo > hi and a NaN bound (FGSM never has)."""
    lo = float("-inf") if clip_min is None else float(clip_min)
    hi = float("inf") if clip_max is None else float(clip_max)
    if ordered and not lo <= hi:
        raise ValueError("clip_min must not exceed clip_max")
    return lo, hi


def _check_iterative(nb_iter=None, eps=0.0, eps_iter=0.0, batch_size=None, rand_init=False, x_init=None):
    """The budget of an iterative attack, checked before the device is touched; what a caller leaves out is not checked."""
    if nb_iter is not None and int(nb_iter) < 1:
        raise ValueError("nb_iter must be >= 1, got %d" % int(nb_iter))
    if not (float(eps) >= 0 and float(eps_iter) >= 0):
        raise ValueError("eps and eps_iter must be >= 0")
    if rand_init and x_init is not None:
        raise ValueError("give rand_init or x_init, not both")
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")


def _start_point(t, x_init, rand_init, eps, seed, ord, lo, hi, clone=False):
    """x_0 for the images ``t`` on their device: ``x_init`` as given, unclipped (``clone``: in a buffer of its own, for BPDA, which
    swaps and writes its iterates); with ``rand_init`` clip(x + noise), noise = ``bpda_rand_noise(n, P, eps, seed)`` -- through
    ``ball_project_noise`` for ord = 2 -- drawn on the host; else clip(x)."""
    import torch
    _check_iterative(rand_init=rand_init, x_init=x_init)
    if x_init is not None:
        x0 = nb._to_device(x_init, t.device)
        if tuple(x0.shape) != tuple(t.shape):
            raise ValueError("x_init must have x's shape")
        return x0.clone() if clone else x0
    if not rand_init:
        return torch.clamp(t, lo, hi)
    noise = bpda_rand_noise(int(t.shape[0]), int(t[0].numel()), eps, seed)
    noise = noise if ord == np.inf else ball_project_noise(noise, eps)
    return torch.clamp(t + torch.from_numpy(noise).to(t.device).view_as(t), lo, hi)


def _chunks(n, step=None):
    """[(a, b), ...]: [0, n) in runs of ``step`` (None: one run)."""
    step = n if step is None else int(step)
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def _pack(was_numpy, return_info, x_adv, *info):
    """What generate returns: ``x_adv``, or with ``return_info`` the tuple ``(x_adv,) + info``; NumPy where NumPy came in (a dict
    of tensors value by value, what is no tensor as it is), else the tensors as they are, not waited for."""
    import torch

    def out(v):
        if isinstance(v, dict):
            return {k: out(u) for k, u in v.items()}
        return v.cpu().numpy() if was_numpy and isinstance(v, torch.Tensor) else v
    return (out(x_adv),) + tuple(out(v) for v in info) if return_info else out(x_adv)


def ball_project_noise(noise, eps):
    """The ``rand_init`` draw for ord = 2: ``noise`` [n, P] (``bpda_rand_noise``, uniform in the L-infinity cube) scaled per image by
    ``min(1, eps / max(1e-12, ||noise||_2))`` onto the L2 ball, in float32 on the host (the norm in float64, rounded once)."""
    noise = np.asarray(noise, np.float32)
    norm = np.sqrt(np.square(noise.astype(np.float64)).sum(axis=1))
    scale = np.minimum(1.0, float(eps) / np.maximum(1e-12, norm)).astype(np.float32)
    return noise * scale[:, None]


def _row_norms(v, w, ord=2):
    """[n] float32 on the device: the per-image ``ord``-norm of ``v - w`` (of ``v`` when ``w`` is None), ``dg_row_norms``; device
    tensors [n, ...] on torch's current stream, not waited for."""
    import torch
    n = int(v.shape[0])
    out = torch.empty(n, dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        _native.check(_native.load().dg_row_norms(v.data_ptr(), w.data_ptr() if w is not None else None, n, int(v.numel() // n), int(ord),
                                                  out.data_ptr(), torch.cuda.current_stream(v.device).cuda_stream))
    return out


class FastGradientMethod(object):
    """The cleverhans attack object the reference instantiates (whitebox.py:198-200, blackbox.py:530-534) with ord = inf:
    ``adv = clip(x + eps * sign(grad_x CE(model(x), y)), clip_min, clip_max)``; without ``y`` the model's own prediction is
    the label (cleverhans' default).  ``ord`` 1 and 2 are cleverhans' as well, the norm per image over its H W C elements
    (``dg_fgm``): ``adv = clip(x + eps * g / max(1e-12, sum|g|), ...)`` and ``adv = clip(x + eps * g / max(1e-12, sqrt(sum g^2)), ...)``;
    a zero gradient gives a zero step.  ``sess`` / ``back`` are accepted for signature compatibility and ignored.

    White-box use on a DEFENDED model (whitebox.py:185-200 attaches the reconstruction layer first, then builds the attack
    on that model): the gradient through the projection is identically zero in the reference, so ``generate`` returns
    ``clip(x, clip_min, clip_max)`` -- reproduced here, with a warning."""

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    def generate(self, x, eps=0.3, ord=np.inf, y=None, clip_min=None, clip_max=None, **kwargs):
        import torch
        ord = _attack_ord(ord, (np.inf, 1, 2), "FastGradientMethod")
        m = self.model
        dev = nb._ready(m, weights=False)
        t, was_numpy = nb._images(m, x, dev)
        lo, hi = _clip_bounds(clip_min, clip_max, ordered=False)
        if m.rec_layer is not None:
            import warnings
            warnings.warn(nb._REC_GRADIENT_NOTE, stacklevel=2)
            return _pack(was_numpy, False, torch.clamp(t, lo, hi))             # x + eps * sign(0)
        lab = _labels(y, None, dev, required=False)
        out = torch.empty_like(t)
        fn, norm = (_native.load().dg_fgsm, ()) if ord == np.inf else (_native.load().dg_fgm, (int(ord),))
        with torch.cuda.device(dev):
            _native.check(fn(m._handle, t.data_ptr(), _ptr(lab), int(t.shape[0]), float(eps), *norm, lo, hi, out.data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream))
        return _pack(was_numpy, False, out)


_CW_REC_NOTE = (
    "CarliniWagnerL2 on a model with the Defense-GAN reconstruction layer attached (add_rec_model) is not implemented: in the "
    "reference the gradient through ReconstructionLayer is identically zero (network_builder.py:266-271), so the attack "
    "there reduces to repeated defended evaluations of the tanh round trip of x, whose per-iteration latent draws cannot be "
    "pinned.  Build the attack before add_rec_model, or on a model without it (no_rec), as bench.py's --strong flow does for "
    "FGSM.  The white-box attack that does use the defense is BPDA (L-infinity, projected sign gradient).")


class CarliniWagnerL2(object):
    """cleverhans' CarliniWagnerL2 (the reference's ``--attack_type cw``, whitebox.py:201-209), restated and run as ONE
    asynchronous device call (``dg_cw``; the algorithm is in defensegan_amd/csrc/dg_cw.hip's header comment and DESIGN.md
    section 7).  ``sess`` / ``back`` are accepted for signature compatibility and ignored.

    ``generate(x, y=None, y_target=None, **params)``: NumPy in gives NumPy out, a torch tensor in gives a tensor out (on the
    caller's current stream, not waited for); ``y`` / ``y_target`` one-hot or class indices; without either the label is the
    model's own first argmax on ``x``.  ``return_info=True`` also returns ``(best_l2, best_class)`` (1e10 / -1 where no step
    succeeded); ``return_search=True`` then also ``(final_const [B] float64, chunk_stop [binary_search_steps, chunks] int32)``:
    the constants after the last binary-search update and the iteration at whose check each chunk stopped (-1: it ran to
    max_iterations).  ``nb_classes`` and ``feed`` are accepted and ignored.

    ``abort_early`` changes which iterations count, not how long the call takes: a stopped chunk skips the attack's own
    kernels, but the classifier's forward and backward keep running over every image until max_iterations.

    The defaults are those of cleverhans 2.x ``generate`` as remembered (batch_size=1, confidence=0, learning_rate=5e-3,
    binary_search_steps=5, max_iterations=1000, abort_early=True, initial_const=1e-2, clip_min=0, clip_max=1): nothing in the
    reference pins them (cleverhans is an empty, un-pinned submodule).  Only the white-box setting is pinned:
    ``binary_search_steps=1, max_iterations=100, learning_rate=10, initial_const=100, batch_size=BATCH_SIZE`` and no clip
    bounds, so CelebA inputs are clipped to [0, 1] as well -- a quirk of the reference kept here.

    A model with the reconstruction layer attached raises NotImplementedError (see _CW_REC_NOTE)."""

    DEFAULTS = dict(batch_size=1, confidence=0.0, learning_rate=5e-3, binary_search_steps=5, max_iterations=1000, abort_early=True,
                    initial_const=1e-2, clip_min=0.0, clip_max=1.0)

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    def generate(self, x, y=None, y_target=None, return_info=False, return_search=False, nb_classes=None, feed=None, **params):
        import torch
        unknown = set(params) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown CarliniWagnerL2 parameters: %s" % sorted(unknown))
        p = dict(self.DEFAULTS, **params)
        m = self.model
        if m.rec_layer is not None:
            raise NotImplementedError(_CW_REC_NOTE)
        if y is not None and y_target is not None:
            raise ValueError("give y or y_target, not both")
        dev = nb._ready(m)
        t, was_numpy = nb._images(m, x, dev, batch="B")
        B = int(t.shape[0])
        if B == 0:
            raise ValueError("x holds no images")
        targeted = y_target is not None
        lab = _labels(y_target if targeted else y, B, dev, required=False, range_words="cw", nb_classes=m.nb_classes)
        out = torch.empty_like(t)
        best_l2 = torch.empty(B, dtype=torch.float32, device=dev)
        best_class = torch.empty(B, dtype=torch.int32, device=dev)
        nsteps, chunks = max(int(p["binary_search_steps"]), 0), -(-B // max(int(p["batch_size"]), 1))
        final_const = torch.empty(B, dtype=torch.float64, device=dev)
        chunk_stop = torch.empty(nsteps, chunks, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _native.check(_native.load().dg_cw(
                m._handle, t.data_ptr(), _ptr(lab), B, 1 if targeted else 0, int(p["batch_size"]),
                float(p["confidence"]), float(p["learning_rate"]), int(p["binary_search_steps"]), int(p["max_iterations"]),
                1 if p["abort_early"] else 0, float(p["initial_const"]), float(p["clip_min"]), float(p["clip_max"]), out.data_ptr(),
                best_l2.data_ptr(), best_class.data_ptr(), final_const.data_ptr() if return_search else None,
                chunk_stop.data_ptr() if return_search else None, stream))
        return _pack(was_numpy, return_info, out, best_l2, best_class, *((final_const, chunk_stop) if return_search else ()))


EAD_RULES = {"EN": 0, "L1": 1}                # dg_ead's decision_rule


class ElasticNetMethod(object):
    """The elastic-net attack (Chen et al. 2018, EAD; cleverhans' ``ElasticNetMethod``), the suite's L1 attack: Carlini-Wagner's loss
    plus ``beta * ||x_adv - clip(x)||_1``, minimised by iterative shrinkage-thresholding (``fista``: with the FISTA extrapolation) at
    the rate ``learning_rate * sqrt(1 - i / max_iterations)``, restated and run as ONE asynchronous device call (``dg_ead``; the
    algorithm is in defensegan_amd/csrc/dg_ead.hip's header comment and DESIGN.md section 7, "Elastic net").  It needs no L1
    projection, so no sort.  ``sess`` / ``back`` are accepted for signature compatibility and ignored.

    ``generate(x, y=None, y_target=None, **params)`` has ``CarliniWagnerL2.generate``'s conventions: NumPy in gives NumPy out, a torch
    tensor in gives a tensor out (on the caller's current stream, not waited for); ``y`` / ``y_target`` one-hot or class indices;
    without either the label is the model's own first argmax on ``x``.  ``decision_rule`` ranks the successful iterates: "EN" by
    ``||d||_2^2 + beta ||d||_1``, "L1" by ``||d||_1``, d = iterate - clip(x).  ``return_info=True`` also returns ``(best_dist,
    best_class)``: the rule's criterion at ``x_adv`` and its class (1e10 / -1 where no iterate succeeded; ``x_adv`` is then clip(x)
    bit for bit); ``return_search=True`` then also ``(final_const [B] float64, chunk_stop [binary_search_steps, chunks] int32)`` as
    CarliniWagnerL2's.  ``nb_classes`` and ``feed`` are accepted and ignored.  As for CarliniWagnerL2, ``abort_early`` changes which
    iterations count, not how long the call takes.

    The defaults are those of cleverhans' ``ElasticNetMethod`` as remembered (batch_size=1, confidence=0, beta=1e-3,
    decision_rule="EN", fista=True, learning_rate=1e-2, binary_search_steps=9, max_iterations=1000, abort_early=False,
    initial_const=1e-3, clip_min=0, clip_max=1): nothing in the reference pins them (cleverhans is an empty, un-pinned submodule).

    ``decision_rule`` outside {"EN", "L1"} and ``beta < 0`` are a ValueError before any device work; an unknown keyword is a
    TypeError.  A model with the reconstruction layer attached raises NotImplementedError, for _CW_REC_NOTE's reason: the
    reference's gradient through ReconstructionLayer is identically zero."""

    DEFAULTS = dict(batch_size=1, confidence=0.0, beta=1e-3, decision_rule="EN", fista=True, learning_rate=1e-2, binary_search_steps=9,
                    max_iterations=1000, abort_early=False, initial_const=1e-3, clip_min=0.0, clip_max=1.0)

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    @classmethod
    def parse_params(cls, params):
        """DEFAULTS overlaid with ``params``, checked on the host; ``decision_rule`` comes back as dg_ead's integer."""
        unknown = set(params) - set(cls.DEFAULTS)
        if unknown:
            raise TypeError("unknown ElasticNetMethod parameters: %s" % sorted(unknown))
        p = dict(cls.DEFAULTS, **params)
        if p["decision_rule"] not in EAD_RULES:
            raise ValueError("decision_rule must be 'EN' or 'L1', got %r" % (p["decision_rule"],))
        if not float(p["beta"]) >= 0:
            raise ValueError("beta must be >= 0, got %r" % (p["beta"],))
        if int(p["max_iterations"]) < 1:
            raise ValueError("max_iterations must be >= 1, got %d" % int(p["max_iterations"]))
        if int(p["batch_size"]) < 1:
            raise ValueError("batch_size must be >= 1")
        if not float(p["clip_min"]) < float(p["clip_max"]):
            raise ValueError("clip_min must be below clip_max")
        p["decision_rule"] = EAD_RULES[p["decision_rule"]]
        return p

    def generate(self, x, y=None, y_target=None, return_info=False, return_search=False, nb_classes=None, feed=None, **params):
        import torch
        p = self.parse_params(params)
        m = self.model
        if m.rec_layer is not None:
            raise NotImplementedError("ElasticNetMethod: " + _CW_REC_NOTE)
        if y is not None and y_target is not None:
            raise ValueError("give y or y_target, not both")
        dev = nb._ready(m)
        t, was_numpy = nb._images(m, x, dev, batch="B")
        B = int(t.shape[0])
        if B == 0:
            raise ValueError("x holds no images")
        targeted = y_target is not None
        lab = _labels(y_target if targeted else y, B, dev, required=False, range_words="cw", nb_classes=m.nb_classes)
        out = torch.empty_like(t)
        best_dist = torch.empty(B, dtype=torch.float32, device=dev)
        best_class = torch.empty(B, dtype=torch.int32, device=dev)
        nsteps, chunks = max(int(p["binary_search_steps"]), 0), -(-B // int(p["batch_size"]))
        final_const = torch.empty(B, dtype=torch.float64, device=dev)
        chunk_stop = torch.empty(nsteps, chunks, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _native.check(_native.load().dg_ead(
                m._handle, t.data_ptr(), _ptr(lab), B, 1 if targeted else 0, int(p["batch_size"]), float(p["confidence"]), float(p["beta"]),
                p["decision_rule"], 1 if p["fista"] else 0, float(p["learning_rate"]), int(p["binary_search_steps"]),
                int(p["max_iterations"]), 1 if p["abort_early"] else 0, float(p["initial_const"]), float(p["clip_min"]), float(p["clip_max"]),
                out.data_ptr(), best_dist.data_ptr(), best_class.data_ptr(), final_const.data_ptr() if return_search else None,
                chunk_stop.data_ptr() if return_search else None, stream))
        return _pack(was_numpy, return_info, out, best_dist, best_class, *((final_const, chunk_stop) if return_search else ()))


# ---------------------------------------------------------------------- the attack that sees the defense: BPDA / EOT
BPDA_NOISE_TAG = 0x42504441          # "BPDA": word 3 of the rand_init counter (the latents' draw has 0 there, dg_small.hip)
BPDA_DEFAULT_SEED = 11241990         # model_eval_gan's default: without ``seed`` iteration 0 sees the evaluation's own latents


def _philox4x32_10(ctr, key):
    """Random123's Philox4x32-10 on the host: ctr [N, 4] uint32 values, key (k0, k1) -> [N, 4] uint64 arrays holding uint32
    words.  The generator of the latent init and of Dropout (csrc/dg_shared_math.h), restated for the one draw made on the host."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(ctr[:, i], np.uint64) & M for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, axis=1)


def bpda_rand_noise(n_images: int, row_elems: int, eps: float, seed: int, first_image: int = 0) -> np.ndarray:
    """The ``rand_init`` draw of BPDA, float32 [n_images, row_elems] in [-eps, eps): element e of the image with GLOBAL index
    i = first_image + row takes word e % 4 of Philox4x32-10(key = (seed lo, seed hi), counter = (e // 4, i lo, i hi,
    BPDA_NOISE_TAG)); u = (word >> 8) * 2^-24 in [0, 1); noise = float32(eps) * (2 u - 1), one float32 rounding (2 u - 1 is exact).
    Keyed by the image, so the draw does not depend on how the images are batched.  Drawn once per attack, on the host."""
    n_images, row_elems, seed = int(n_images), int(row_elems), int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (row_elems + 3) // 4
    img = (np.arange(n_images, dtype=np.uint64) + np.uint64(int(first_image)))[:, None]
    ctr = np.empty((n_images, nq, 4), np.uint64)
    ctr[:, :, 0] = np.arange(nq, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = img & np.uint64(0xFFFFFFFF)
    ctr[:, :, 2] = img >> np.uint64(32)
    ctr[:, :, 3] = BPDA_NOISE_TAG
    words = _philox4x32_10(ctr.reshape(-1, 4), (seed & 0xFFFFFFFF, seed >> 32)).reshape(n_images, nq * 4)[:, :row_elems]
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (np.float32(eps) * (np.float32(2.0) * u - np.float32(1.0))).astype(np.float32)


def bpda_seed_schedule(seed: int, nb_iter: int, eot_samples: int):
    """``(per_iteration, final)``: ``per_iteration[k][s] = seed + k * eot_samples + s`` is the latent seed of EOT sample s of
    iteration k, ``final = seed + nb_iter * eot_samples`` that of the projection that judges the last iterate."""
    m = int(eot_samples)
    return [[int(seed) + k * m + s for s in range(m)] for k in range(int(nb_iter))], int(seed) + int(nb_iter) * m


class _AttackDeviceOps(object):
    """What the device operations of the iterative attacks on a (defended) model share: the classifier, its projection's model (or
    None), the device; the prediction on a batch; the best tracking."""

    def __init__(self, model: MLP):
        self.device = nb._ready(model)
        self.model, self.gan = model, (model.rec_layer.rec_model if model.rec_layer is not None else None)

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def predict(self, rec):
        """[B] int32: the classifier's first argmax on ``rec`` (dg_eval_batch)."""
        return self.model.eval_batch(rec, None, None, sync=False)[1]

    def track(self, preds, labels, k, x_iter, x_best, first_success):
        """dg_bpda_track: images still without a success take iterate k as their best, and k as their first success where
        ``preds != labels``."""
        import torch
        B = int(preds.shape[0])
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_bpda_track(
                preds.data_ptr(), labels.data_ptr(), B, int(k), x_iter.data_ptr(), x_best.data_ptr(), first_success.data_ptr(),
                int(x_iter.numel() // B), self._stream()))


class BpdaDeviceOps(_AttackDeviceOps):
    """The device operations ``BPDA.generate`` is made of (``step_ball`` and ``dist`` only with ``ord = 2``), on tensors of the classifier's device and torch's current stream;
    none of them waits for the device.  (``BPDA`` takes any object with these methods and a ``device``: the tests drive the loop
    with a recording stand-in.)  ``predict`` and ``track`` are the base class's."""

    def project(self, x, seed, first_row):
        """gan.reconstruct: latents drawn as dg_init_latents does for (seed, first_row + row)."""
        return self.gan.reconstruct(x, seed=int(seed), first_row=int(first_row))

    def step(self, rec, labels, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, clip_min, clip_max, x_next, ord=np.inf):
        """dg_bpda_step: the classifier's input gradient at ``rec``, then ``gsum += g`` (accumulate_only) or the projected sign
        step of ``gsum + g`` from ``x_cur`` around ``x_orig`` into ``x_next``.  With ``ord`` = 2 dg_bpda_step_ball: the L2 step."""
        import torch
        fn, norm = (_native.load().dg_bpda_step, ()) if ord == np.inf else (_native.load().dg_bpda_step_ball, (int(ord),))
        with torch.cuda.device(self.device):
            _native.check(fn(self.model._handle, rec.data_ptr(), labels.data_ptr(), int(rec.shape[0]), _ptr(x_cur), _ptr(x_orig), _ptr(gsum),
                             1 if accumulate_only else 0, float(eps), float(eps_iter), *norm, float(clip_min), float(clip_max), _ptr(x_next),
                             self._stream()))

    def step_ball(self, rec, labels, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, ord, clip_min, clip_max, x_next):
        """``step`` with the L2 step (``ord`` = 2) in the projected sign step's place, under the name and with the argument order
        ``BPDA.generate`` asks of its operations for ord = 2."""
        self.step(rec, labels, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, clip_min, clip_max, x_next, ord)

    def dist(self, x_adv, x_orig):
        """dg_row_norms: [n] float32, the per-image L2 distance of ``x_adv`` from ``x_orig``."""
        return _row_norms(x_adv, x_orig, 2)


class BPDA(object):
    """The white-box attack that uses the defense: BPDA with EOT (Athalye, Carlini, Wagner 2018), L-infinity, on a model with
    the Defense-GAN projection attached (``add_rec_model``).  Not in the reference, whose attacks differentiate through
    ``ReconstructionLayer`` and see a zero gradient (_REC_GRADIENT_NOTE).  The projection runs for real in the forward pass and
    counts as the identity in the backward pass; the gradient is summed over ``eot_samples`` projections with fresh latents:

        x_0 = clip(x)            (``rand_init``: clip(x + bpda_rand_noise(...)); or ``x_init`` as given)
        for k < nb_iter:   g_k = sum_{s < m} grad_r CE(logits(r), y) at r = reconstruct(x_k; latents of seed + k m + s)
                           x_{k+1} = clip(x + clamp(x_k + eps_iter sign(g_k) - x, -eps, eps), clip_min, clip_max),  sign(0) = 0

    Best tracking on the device: iterate k + 1 succeeds for an image when the defended prediction on it is not ``y``; that
    prediction is read off the next iteration's first projection (s = 0), the last iterate's off one more projection with seed
    ``seed + nb_iter m`` -- ``nb_iter * m + 1`` projections in all, enqueued with no host read in between.  ``generate`` returns
    per image the first successful iterate, or the last iterate; ``return_info=True`` adds ``first_success`` [n] int32 (the
    iterate's index in 1 .. nb_iter, or -1).

    ``ord = 2`` (default np.inf) bounds the perturbation in L2 instead, every norm per image over its H W C elements:
    ``u = g_k / max(1e-12, ||g_k||)``, ``d = (x_k + eps_iter u) - x``, ``x_{k+1} = clip(x + d min(1, eps / max(1e-12, ||d||)), ...)``
    (``dg_bpda_step_ball``; a zero gradient gives a zero step); ``rand_init`` then draws ``ball_project_noise(bpda_rand_noise(...))``,
    the same draw scaled onto the L2 ball on the host; and ``return_info=True`` returns a third value, ``dist`` [n] float32, the
    distance ``||x_adv - x||_2`` (``dg_row_norms``).  ``ord = 1`` raises NotImplementedError: its projection needs a sort.

    ``x`` NumPy or a device tensor [n, H, W, C] in generator range (NumPy in gives NumPy out; a tensor gives tensors on the
    caller's current stream, not waited for); ``y`` class indices or one-hot rows, required.  ``seed`` defaults to
    BPDA_DEFAULT_SEED.  The latents of image i are rows ``i * rec_rr + r`` of the seeded stream and every classifier output is
    one thread's fixed-order sum, so the result does not depend on ``batch_size``, bit for bit: ``batch_size`` (default: the
    reconstruction layer's) only bounds the images per engine call, and consecutive batches are coalesced into engine calls as
    in ``gan_defense.model_eval_gan``.  With a USE_BN generator the rows of an engine call share its Batchnorm statistics: the
    calls are then cut on ``batch_size`` exactly, and the result DOES depend on it.

    A bare model raises ValueError: projected gradient descent on an undefended classifier is ``ProjectedGradientDescent``.  A
    reconstruction layer with a fixed ``z_init`` is refused as well (the attack draws fresh latents for every projection)."""

    def __init__(self, model: MLP, back="tf", sess=None, ops=None):
        self.model = model
        self._ops = ops

    def generate(self, x, y, eps=0.3, eps_iter=0.05, nb_iter=10, eot_samples=1, clip_min=None, clip_max=None, rand_init=False,
                 seed=None, x_init=None, batch_size=None, return_info=False, ord=np.inf):
        import torch
        from . import gan_defense
        ord = _attack_ord(ord, (np.inf, 2), "BPDA")
        m = self.model
        rl = m.rec_layer
        if rl is None:
            raise ValueError("BPDA attacks a model with the Defense-GAN projection attached (add_rec_model); projected gradient "
                             "descent on a bare classifier (PGD-on-bare) is ProjectedGradientDescent")
        if rl.z_init is not None:
            raise ValueError("BPDA draws fresh latents for every projection; the reconstruction layer has a fixed z_init")
        nb_iter, mm = int(nb_iter), int(eot_samples)
        if mm < 1:
            raise ValueError("eot_samples must be >= 1, got %d" % mm)
        bs = batch_size or rl.batch_size or None                   # None: all images
        _check_iterative(nb_iter, eps, eps_iter, bs, rand_init, x_init)
        lo, hi = _clip_bounds(clip_min, clip_max)
        seed = BPDA_DEFAULT_SEED if seed is None else int(seed)
        ops = self._ops if self._ops is not None else BpdaDeviceOps(m)
        dev = ops.device
        t, was_numpy = nb._images(m, x, dev, batch="n", nonempty=True)
        n = int(t.shape[0])
        lab = _labels(y, n, dev)
        x_cur = _start_point(t, x_init, rand_init, eps, seed, ord, lo, hi, clone=True)
        gan = rl.rec_model
        R = int(gan.rec_rr)
        cuts = _chunks(n, gan_defense.engine_step(gan.reconstruct, int(bs or n), R, n))
        step, norm = (ops.step, ()) if ord == np.inf else (ops.step_ball, (ord,))
        x_next, x_best = torch.empty_like(x_cur), torch.empty_like(x_cur)
        first_success = torch.full((n,), -1, dtype=torch.int32, device=dev)
        gsum = torch.empty_like(x_cur) if mm > 1 else None
        seeds, final_seed = bpda_seed_schedule(seed, nb_iter, mm)
        for k in range(nb_iter):
            if gsum is not None:
                gsum.zero_()
            for s in range(mm):
                for a, b in cuts:
                    rec = ops.project(x_cur[a:b], seeds[k][s], a * R)
                    if s == 0 and k > 0:                           # rec_{k,0} is the defended view of iterate k
                        ops.track(ops.predict(rec), lab[a:b], k, x_cur[a:b], x_best[a:b], first_success[a:b])
                    gs = gsum[a:b] if gsum is not None else None
                    step(rec, lab[a:b], x_cur[a:b], t[a:b], gs, s < mm - 1, eps, eps_iter, *norm, lo, hi, x_next[a:b])
            x_cur, x_next = x_next, x_cur
        for a, b in cuts:
            rec = ops.project(x_cur[a:b], final_seed, a * R)
            ops.track(ops.predict(rec), lab[a:b], nb_iter, x_cur[a:b], x_best[a:b], first_success[a:b])
        return _pack(was_numpy, return_info, x_best, first_success, *((ops.dist(x_best, t),) if ord == 2 and return_info else ()))


class ProjectedGradientDescent(object):
    """Projected gradient descent (Madry et al. 2018), L-infinity, on a BARE classifier: ``BPDA`` with the identity as the projection
    and ``eot_samples = 1``, run as ONE asynchronous device call per ``batch_size`` images (``dg_pgd``, defensegan_amd/csrc/dg_pgd.hip):

        x_0 = clip(x)            (``rand_init``: clip(x + bpda_rand_noise(...)); or ``x_init`` as given)
        for k < nb_iter:   g_k = grad_x CE(logits(x_k), y)                     (``input_gradient``'s bits)
                           x_{k+1} = clip(x + clamp(x_k + eps_iter sign(g_k) - x, -eps, eps), clip_min, clip_max),  sign(0) = 0

    Best tracking as BPDA's: iterate k + 1 succeeds for an image when the model's prediction on it is not ``y``; ``generate``
    returns per image the first successful iterate, or the last one; ``return_info=True`` adds ``first_success`` [n] int32 (the
    iterate's index in 1 .. nb_iter, or -1).  The prediction is read off the logits the next iteration's forward keeps:
    ``nb_iter + 1`` forwards and ``nb_iter`` backwards in all.

    ``ord = 2`` (default np.inf) is the L2 attack, as ``BPDA``'s: the step ``u = g_k / max(1e-12, ||g_k||)``, ``d = (x_k + eps_iter u) - x``,
    ``x_{k+1} = clip(x + d min(1, eps / max(1e-12, ||d||)), ...)`` with every norm per image (``dg_pgd_ball``, still one device call);
    ``rand_init`` draws ``ball_project_noise(bpda_rand_noise(...))`` on the host; ``return_info=True`` returns a third value, ``dist`` [n]
    float32 = ``||x_adv - x||_2`` (``dg_row_norms``).  ``ord = 1`` raises NotImplementedError: its projection needs a sort.

    ``x`` NumPy or a device tensor [n, H, W, C] (NumPy in gives NumPy out; a tensor gives tensors on the caller's current stream,
    not waited for); ``y`` class indices or one-hot rows, required; a class index outside [0, nb_classes) gives that image a zero
    gradient (training's policy): it stays at x_0.  ``seed`` (default BPDA_DEFAULT_SEED) keys the ``rand_init`` draw, by the
    image.  ``batch_size`` only bounds the images per device call (default: all): every output element is one thread's
    fixed-order arithmetic on its own image, so the result does not depend on it, bit for bit.

    A model with the reconstruction layer attached raises ValueError: the attack that uses the defense is ``BPDA``."""

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    def generate(self, x, y, eps=0.3, eps_iter=0.05, nb_iter=10, clip_min=None, clip_max=None, rand_init=False, seed=None, x_init=None,
                 batch_size=None, return_info=False, ord=np.inf):
        import torch
        ord = _attack_ord(ord, (np.inf, 2), "ProjectedGradientDescent")
        m = self.model
        if m.rec_layer is not None:
            raise ValueError("ProjectedGradientDescent attacks a bare classifier; this model has the Defense-GAN projection attached "
                             "(add_rec_model), through which the gradient is identically zero: use BPDA")
        nb_iter = int(nb_iter)
        _check_iterative(nb_iter, eps, eps_iter, batch_size, rand_init, x_init)
        lo, hi = _clip_bounds(clip_min, clip_max)
        seed = BPDA_DEFAULT_SEED if seed is None else int(seed)
        dev = nb._ready(m)
        t, was_numpy = nb._images(m, x, dev, batch="n", nonempty=True)
        n = int(t.shape[0])
        lab = _labels(y, n, dev)
        x0 = _start_point(t, x_init, rand_init, eps, seed, ord, lo, hi)
        x_adv = torch.empty_like(t)
        first_success = torch.empty(n, dtype=torch.int32, device=dev)
        fn, norm = (_native.load().dg_pgd, ()) if ord == np.inf else (_native.load().dg_pgd_ball, (ord,))
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            for a, b in _chunks(n, batch_size):
                _native.check(fn(m._handle, t[a:b].data_ptr(), x0[a:b].data_ptr(), lab[a:b].data_ptr(), b - a, float(eps), float(eps_iter),
                                 nb_iter, *norm, lo, hi, x_adv[a:b].data_ptr(), first_success[a:b].data_ptr(), stream))
        return _pack(was_numpy, return_info, x_adv, first_success, *((_row_norms(x_adv, t, 2),) if ord == 2 and return_info else ()))


# ---------------------------------------------------------------------- the score-based black-box attack: SPSA
class SpsaDeviceOps(_AttackDeviceOps):
    """The device operations ``SPSA.generate`` is made of, on tensors of the classifier's device and torch's current stream; none
    of them waits for the device.  (``SPSA`` takes any object with these methods and a ``device``: the tests drive the loop with a
    recording stand-in.)  ``predict`` and ``track`` are the base class's."""

    def queries(self, x_cur, n, delta, seed, first_image, k, clip_min, clip_max, q):
        """dg_spsa_queries: the 2 n + 1 queries of every image of ``x_cur`` [B, ...] into ``q`` [B (2 n + 1), ...]."""
        import torch
        B = int(x_cur.shape[0])
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_spsa_queries(
                x_cur.data_ptr(), B, int(x_cur.numel() // B), int(n), float(delta), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image), int(k),
                float(clip_min), float(clip_max), q.data_ptr(), self._stream()))

    def project(self, q, seed, first_row, row_step=None):
        """The defended model's projection of ``q``: row j takes the latents ``first_row + j * row_step + r``, r < rec_rr, of the
        stream of ``seed``.  ``row_step`` None = rec_rr, consecutive rows: one ``gan.reconstruct``; any other step (the closing
        pass, whose images lie 2 n + 1 queries apart) draws each row's latents with ``init_latents`` and hands them over as z0 --
        the values ``reconstruct`` would have drawn.  On a bare model: the identity."""
        import torch
        if self.gan is None:
            return q
        R = int(self.gan.rec_rr)
        if row_step is None or int(row_step) == R or int(q.shape[0]) == 1:
            return self.gan.reconstruct(q, seed=int(seed), first_row=int(first_row))
        z0 = torch.cat([self.gan.init_latents(R, seed=int(seed), first_row=int(first_row) + j * int(row_step)) for j in range(int(q.shape[0]))])
        return self.gan.reconstruct(q, z_init_val=z0, seed=int(seed))

    def logits(self, rec):
        """[B, classes] float32: the classifier's logits on ``rec`` (dg_clf_forward)."""
        import torch
        B = int(rec.shape[0])
        out = torch.empty(B, self.model.nb_classes, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_clf_forward(self.model._handle, rec.data_ptr(), B, out.data_ptr(), None, self._stream()))
        return out

    def step(self, logits, labels, n, delta, seed, first_image, k, x_cur, x_orig, eps, eps_iter, clip_min, clip_max, x_next, out_grad=None):
        """dg_spsa_step: margins, the estimate and the projected sign step from ``x_cur`` around ``x_orig`` into ``x_next``."""
        import torch
        B = int(x_cur.shape[0])
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_spsa_step(
                logits.data_ptr(), labels.data_ptr(), B, int(logits.shape[1]), int(x_cur.numel() // B), int(n), float(delta),
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image), int(k), x_cur.data_ptr(), x_orig.data_ptr(), float(eps), float(eps_iter),
                float(clip_min), float(clip_max), x_next.data_ptr(), _ptr(out_grad), self._stream()))


class SPSA(object):
    """The score-based black-box attack: SPSA (Uesato et al. 2018) with Rademacher directions and the projected sign step of
    ``ProjectedGradientDescent`` and ``BPDA``, L-infinity.  It reads only the attacked model's logits, so it attacks the DEFENDED
    model (``add_rec_model``), whose gradient is identically zero (_REC_GRADIENT_NOTE), as well as a bare classifier, where the
    identity stands in for the projection.  Not in the reference.  With ``n = spsa_samples``, ``g`` an image's index in ``x``:

        x_0 = clip(x)
        for k < nb_iter:   u_i[e] = +-1 by bit (i & 31) of word (e & 3) of Philox4x32-10(key = seed, counter = (e >> 2, g,
                                    k ceil(n / 32) + (i >> 5), 0x53505341))                                            i < n
                           q_0 = x_k,  q+_i = clip(x_k + delta u_i),  q-_i = clip(x_k - delta u_i)     (2 n + 1 queries, clipped)
                           L(q) = max_{j != y} Z_j - Z_y  on the logits Z of the model (through the projection) at q
                           ghat = (1 / (2 delta n)) sum_i (L(q+_i) - L(q-_i)) u_i          (float32, ascending i; dg_spsa_step)
                           x_{k+1} = clip(x + clamp(x_k + eps_iter sign(ghat) - x, -eps, eps), clip_min, clip_max),  sign(0) = 0

    A label outside [0, classes) gives L = 0 and a zero step; a pair whose loss difference is not finite contributes 0.  Best
    tracking as BPDA's: iterate j = 1 .. nb_iter succeeds when the model's first arg-max on ITS query 0 is not ``y`` (iteration j's
    query 0 is x_j; iterate nb_iter is judged by one closing query per image); ``generate`` returns per image the first successful
    iterate, or else the last one.  ``return_info=True`` adds ``first_success`` [n] int32 (1 .. nb_iter, or -1) and ``queries``,
    the queries spent per image: ``nb_iter * (2 n + 1) + 1``.

    Defended model: iteration k projects with latent seed ``seed + k``, the closing pass with ``seed + nb_iter``; the latents of
    query c of image g are rows ``(g (2 n + 1) + c) rec_rr + r`` of that stream.  ``batch_size`` (default: the reconstruction
    layer's, else all) bounds the images whose queries are alive at once, and their flat query range is cut into engine calls by
    ``gan_defense.engine_step``; every row of the engine and every element of the two kernels is computed independently of its
    batch, so the result depends on neither, bit for bit.  On a bare model no latent seeds are used.

    ``x`` NumPy or a device tensor [n, H, W, C] (NumPy in gives NumPy out; a tensor gives tensors on the caller's current stream,
    not waited for); ``y`` class indices or one-hot rows, required.  ``seed`` defaults to BPDA_DEFAULT_SEED.  No host read is made
    inside the attack.  A reconstruction layer with a fixed ``z_init`` is a ValueError (every projection draws fresh latents); a
    USE_BN generator a NotImplementedError (its batch statistics would couple an image's queries to the cut)."""

    def __init__(self, model: MLP, back="tf", sess=None, ops=None):
        self.model = model
        self._ops = ops

    def generate(self, x, y, eps=0.3, eps_iter=0.05, nb_iter=10, spsa_samples=32, delta=0.01, clip_min=None, clip_max=None, seed=None,
                 batch_size=None, return_info=False):
        import torch
        from . import gan_defense
        m = self.model
        rl = m.rec_layer
        gan = rl.rec_model if rl is not None else None
        if rl is not None and rl.z_init is not None:
            raise ValueError("SPSA draws fresh latents for every projection; the reconstruction layer has a fixed z_init")
        if gan is not None and bool(getattr(gan, "use_bn", False)):
            raise NotImplementedError("SPSA on a USE_BN generator: its batch statistics would couple an image's queries to how the "
                                      "engine calls are cut")
        nb_iter, ns = int(nb_iter), int(spsa_samples)
        if ns < 1:
            raise ValueError("spsa_samples must be >= 1, got %d" % ns)
        if not float(delta) > 0:
            raise ValueError("delta must be > 0")
        _check_iterative(nb_iter, eps, eps_iter, batch_size)
        lo, hi = _clip_bounds(clip_min, clip_max)
        seed = BPDA_DEFAULT_SEED if seed is None else int(seed)
        ops = self._ops if self._ops is not None else SpsaDeviceOps(m)
        dev = ops.device
        t, was_numpy = nb._images(m, x, dev, batch="n", nonempty=True)
        n = int(t.shape[0])
        lab = _labels(y, n, dev)
        Q = 2 * ns + 1                                             # queries per image and iteration
        R = int(gan.rec_rr) if gan is not None else 1
        bs = min(n, int(batch_size or (rl.batch_size if rl is not None else None) or n))
        chunks = _chunks(n, bs)

        def cuts(count):
            """An engine call's share [c0, c1) of ``count`` consecutive rows; a bare model takes them in one."""
            return _chunks(count, gan_defense.engine_step(gan.reconstruct, 1, R, count) if gan is not None else count)

        x_cur = torch.clamp(t, lo, hi)
        x_next, x_best = torch.empty_like(x_cur), torch.empty_like(x_cur)
        first_success = torch.full((n,), -1, dtype=torch.int32, device=dev)
        q = torch.empty((bs * Q,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        for k in range(nb_iter):
            for a, b in chunks:
                nq = (b - a) * Q
                ops.queries(x_cur[a:b], ns, delta, seed, a, k, lo, hi, q[:nq])
                Z, rec0 = [], []
                for c0, c1 in cuts(nq):
                    rec = ops.project(q[c0:c1], (seed + k) if gan is not None else None, (a * Q + c0) * R)
                    Z.append(ops.logits(rec))
                    if k > 0 and -c0 % Q < c1 - c0:                # the cut holds query 0 of an image: the defended view of iterate k
                        rec0.append(rec[-c0 % Q::Q])
                if k > 0:
                    ops.track(ops.predict(rec0[0] if len(rec0) == 1 else torch.cat(rec0)), lab[a:b], k, x_cur[a:b], x_best[a:b],
                              first_success[a:b])
                ops.step(Z[0] if len(Z) == 1 else torch.cat(Z), lab[a:b], ns, delta, seed, a, k, x_cur[a:b], t[a:b], eps, eps_iter, lo, hi,
                         x_next[a:b])
            x_cur, x_next = x_next, x_cur
        for a, b in chunks:                                        # the closing query of every image judges iterate nb_iter
            preds = [ops.predict(ops.project(x_cur[a + c0:a + c1], (seed + nb_iter) if gan is not None else None, (a + c0) * Q * R, Q * R))
                     for c0, c1 in cuts(b - a)]
            ops.track(preds[0] if len(preds) == 1 else torch.cat(preds), lab[a:b], nb_iter, x_cur[a:b], x_best[a:b], first_success[a:b])
        return _pack(was_numpy, return_info, x_best, first_success, nb_iter * Q + 1)


def rand_fgsm_prestep(test_images, eps: float, alpha: float, min_val: float = 0.0, max_val: float = 1.0, rng=None):
    """The ``rand`` half of ``--attack_type rand+fgsm`` (/root/reference/whitebox.py:191-195): one random sign step of size
    ``alpha`` before the FGSM step, whose budget shrinks by it:

        x' = clip(x + alpha * sign(N(0, 1)), min_val, 1),   eps' = eps - alpha

    Returns ``(x', eps')``; feed both to ``FastGradientMethod.generate``.  ``rng``: a ``numpy.random.RandomState`` (the reference
    draws from the global NumPy generator it seeded with [11, 24, 1990], whitebox.py:143-144)."""
    rng = np.random if rng is None else rng
    x = np.asarray(test_images, np.float32)
    out = np.clip(x + np.float32(alpha) * np.sign(rng.randn(*x.shape)).astype(np.float32), min_val, max_val).astype(np.float32)
    return out, float(eps) - float(alpha)


LATENT_DEFAULT_SEED = 11241990


class LatentAttack(object):
    """The latent-space attack (Athalye, Carlini, Wagner 2018, section 5), the attack that breaks Defense-GAN: search the generator's
    range for ``z`` such that ``G(z)`` is misclassified and close to ``x``.  ``G(z)`` lies on the manifold, so the projection returns
    it almost unchanged and the defence does not help.  One asynchronous device call per ``batch_size`` images (``dg_latent_attack``,
    defensegan_amd/csrc/dg_latent.hip; DESIGN.md section 7 gives the definition): ``rec_rr`` restarts per image, TF's Adam
    (0.9, 0.999, 1e-8) on ``z`` for ``nb_iter`` steps of the loss

        mean_pixels (G(z) - x)^2 + c max(logits[y] - max_{k != y} logits[k] + confidence, 0)

    and per image the successful iterate (margin < -confidence) of the smallest distance, or -- with no success -- the final iterate
    of the smallest margin.

    ``model``: an MLP whose output before Softmax is the logits, without Dropout.  A model with the reconstruction layer attached
    (``add_rec_model``) is accepted: the attack uses its BARE classifier and, when ``gan`` is None, the layer's generator.  ``gan``:
    a DefenseGANBase of the MNIST / F-MNIST architecture with ``USE_BN: False``; a CelebA or Batchnorm generator raises
    NotImplementedError with the library's words.

    ``generate`` returns ``x_adv`` (NumPy in, NumPy out; a device tensor in, a device tensor out on the caller's current stream, not
    waited for); ``return_info=True`` adds a dict of best_dist, best_margin [n], best_iter, best_row [n] int32 (best_iter = -1: no
    success) and z [n rec_rr, latent].  ``y``: class indices or one-hot rows, required, checked on the host against the class count.
    ``z_init`` [n rec_rr, latent] or None: the rows are then drawn as ``init_latents(seed)`` draws them, keyed by the GLOBAL row
    (image index x rec_rr + restart), so the result does not depend on ``batch_size``, which only bounds the images per call."""

    def __init__(self, model: MLP, gan=None, back="tf", sess=None):
        self.model = model
        if gan is None and model.rec_layer is not None:
            gan = model.rec_layer.rec_model
        if gan is None:
            raise ValueError("LatentAttack needs the generator: pass gan, or a model with the reconstruction layer attached")
        self.gan = gan

    def _check_gan(self):
        from . import archs
        g = self.gan
        if g._arch.arch_id == archs.ARCH_CELEBA:
            raise NotImplementedError("dg_latent_attack: not implemented for the CelebA generator (only the MNIST / F-MNIST one)")
        if g.use_bn:
            raise NotImplementedError("dg_latent_attack: not implemented for use_bn (a Batchnorm generator)")

    def call(self, x, labels, R, nb_iter, learning_rate=0.05, c=1.0, confidence=0.0, z0=None, seed=0, first_row=0, beta1=0.9, beta2=0.999,
             m=None, v=None, t_start=0, keep_state=False, state=None, traces=False, want_dz=False):
        """One ``dg_latent_attack`` call on device tensors: ``x`` [B,28,28,1] float32, ``labels`` [B] int32.  ``state``: the dict a
        call before returned, whose x_adv / best_* buffers this call continues (``t_start`` > 0).  Returns a dict of device tensors:
        x_adv, best_dist, best_margin, best_iter, best_row, z, and with ``traces`` margin and dist [nb_iter + 1, B R], with
        ``want_dz`` dz [B R, latent].  Nothing is waited for."""
        import torch
        g, mdl = self.gan, self.model
        self._check_gan()
        g._ensure_handle()
        if not g.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        mdl._ensure()
        dev = x.device
        B, N, latent = int(x.shape[0]), int(x.shape[0]) * int(R), int(g.latent_dim)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out = dict(state) if state is not None else {
            "x_adv": torch.empty_like(x), "best_dist": f32(B), "best_margin": f32(B),
            "best_iter": torch.empty(B, dtype=torch.int32, device=dev), "best_row": torch.empty(B, dtype=torch.int32, device=dev)}
        out["z"] = f32(N, latent)
        if traces:
            out["margin"], out["dist"] = f32(int(nb_iter) + 1, N), f32(int(nb_iter) + 1, N)
        if want_dz:
            out["dz"] = f32(N, latent)
        with torch.cuda.device(dev):
            _native.check(g._lib().dg_latent_attack(
                g._handle, mdl._handle, x.data_ptr(), labels.data_ptr(), B, int(R), _ptr(z0), int(seed), int(first_row), int(nb_iter),
                float(learning_rate), float(beta1), float(beta2), float(c), float(confidence), _ptr(m), _ptr(v), int(t_start),
                1 if keep_state else 0, out["x_adv"].data_ptr(), out["best_dist"].data_ptr(), out["best_margin"].data_ptr(),
                out["best_iter"].data_ptr(), out["best_row"].data_ptr(), out["z"].data_ptr(), _ptr(out.get("margin")), _ptr(out.get("dist")),
                _ptr(out.get("dz")), torch.cuda.current_stream(dev).cuda_stream), g._lib())
        return out

    def generate(self, x, y, rec_rr=None, nb_iter=100, learning_rate=0.05, c=1.0, confidence=0.0, z_init=None, seed=None, batch_size=None,
                 return_info=False):
        import torch
        self._check_gan()
        mdl, g = self.model, self.gan
        R = int(g.rec_rr if rec_rr is None else rec_rr)
        nb_iter = int(nb_iter)
        if R < 1 or nb_iter < 0:
            raise ValueError("rec_rr must be >= 1 and nb_iter >= 0")
        if not (float(confidence) >= 0 and float(c) >= 0):
            raise ValueError("confidence and c must be >= 0")
        _check_iterative(batch_size=batch_size)
        seed = LATENT_DEFAULT_SEED if seed is None else int(seed)
        dev = nb._ready(mdl)
        g._ensure_handle()
        t, was_numpy = nb._images(mdl, x, dev, batch="n", nonempty=True)
        n = int(t.shape[0])
        lab = _labels(y, n, dev, range_words="latent", nb_classes=mdl.nb_classes)
        z0 = None
        if z_init is not None:
            z0 = nb._to_device(z_init, dev)
            if tuple(z0.shape) != (n * R, int(g.latent_dim)):
                raise ValueError("z_init must be [%d, %d], got %s" % (n * R, int(g.latent_dim), tuple(z0.shape)))
        parts = [self.call(t[a:b], lab[a:b], R, nb_iter, learning_rate, c, confidence, None if z0 is None else z0[a * R:b * R], seed, a * R)
                 for a, b in _chunks(n, batch_size)]
        info = {k: torch.cat([p[k] for p in parts]) for k in ("x_adv", "best_dist", "best_margin", "best_iter", "best_row", "z")}
        x_adv = info.pop("x_adv")
        return _pack(was_numpy, return_info, x_adv, info)


# ---------------------------------------------------------------------- the minimal-perturbation attack: DeepFool
_DEEPFOOL_REC_NOTE = (
    "DeepFool on a model with the Defense-GAN reconstruction layer attached (add_rec_model) is not implemented, for CarliniWagnerL2's "
    "reason: in the reference the gradient through ReconstructionLayer is identically zero (network_builder.py:266-271), so every "
    "w_j is zero and no step exists; DeepFool through the projection would need BPDA.  Build the attack before add_rec_model, or "
    "on a model without it.")
DEEPFOOL_CALL_IMAGES = 1000                   # images per dg_deepfool call when batch_size is None: bounds the workspace, not the result


class DeepFool(object):
    """DeepFool (Moosavi-Dezfooli, Fawzi, Frossard 2016; cleverhans' ``DeepFool``), the minimal-L2 attack: no budget, no labels, one
    asynchronous device call per ``batch_size`` images (``dg_deepfool``, defensegan_amd/csrc/dg_deepfool.hip; DESIGN.md section 7,
    "DeepFool", gives the definition).  On the model's LOGITS, before any Softmax:

        orig = first argmax at x;  cand[0 .. nb_candidate) = the classes of the largest logits at x, descending (fixed);  r = 0, adv = x
        while the first argmax over all classes at adv is orig (at most max_iter times):
            f_j = Z[cand_j] - Z[cand_0],  w_j = grad Z[cand_j] - grad Z[cand_0]  at adv;   pert_j = (|f_j| + 1e-5) / ||w_j||_2
            j* = the first index of the smallest pert_j;   r += pert_j* w_j* / ||w_j*||_2;   adv = clip(x + r, clip_min, clip_max)
        x_adv = clip(x + (1 + overshoot) r, clip_min, clip_max)

    ``||w_j|| == 0`` gives ``pert_j = +inf``, which is never chosen; an image with nothing to choose stops and keeps its r.  An image
    whose logits hold a NaN stops and returns ``clip(x + (1 + overshoot) r)`` from the last finite state.

    ``generate`` returns ``x_adv`` (NumPy in gives NumPy out; a device tensor in gives a device tensor out on the caller's current
    stream); ``return_info=True`` adds ``(r_norm, iters, final_class)``: ``||x_adv - x||_2`` [n] float32, the iterations the image
    was active and the first argmax at ``x_adv`` [n] int32.  ``batch_size`` only bounds the images per device call (default
    DEEPFOOL_CALL_IMAGES): every reduction is per image and in a fixed order, so the result does not depend on it, bit for bit.
    ``sess`` / ``back`` are accepted for signature compatibility and ignored.

    A model with the reconstruction layer attached raises NotImplementedError (see _DEEPFOOL_REC_NOTE); an unknown keyword is a
    ValueError."""

    DEFAULTS = dict(nb_candidate=10, overshoot=0.02, max_iter=50, clip_min=0.0, clip_max=1.0, batch_size=None, return_info=False)

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    @classmethod
    def parse_params(cls, params):
        """DEFAULTS overlaid with ``params``, checked on the host: what ``generate`` and ``robustness`` accept."""
        unknown = set(params) - set(cls.DEFAULTS)
        if unknown:
            raise ValueError("unknown DeepFool parameters: %s" % sorted(unknown))
        p = dict(cls.DEFAULTS, **params)
        if int(p["nb_candidate"]) < 2:
            raise ValueError("nb_candidate must be >= 2, got %d" % int(p["nb_candidate"]))
        if int(p["max_iter"]) < 0:
            raise ValueError("max_iter must be >= 0, got %d" % int(p["max_iter"]))
        _check_iterative(batch_size=p["batch_size"])
        p["clip_min"], p["clip_max"] = _clip_bounds(p["clip_min"], p["clip_max"])
        return p

    def generate(self, x, **params):
        import torch
        p = self.parse_params(params)
        m = self.model
        if m.rec_layer is not None:
            raise NotImplementedError(_DEEPFOOL_REC_NOTE)
        dev = nb._ready(m)
        if int(p["nb_candidate"]) > m.nb_classes:
            raise ValueError("nb_candidate must not exceed the model's %d classes, got %d" % (m.nb_classes, int(p["nb_candidate"])))
        t, was_numpy = nb._images(m, x, dev, batch="n", nonempty=True)
        n = int(t.shape[0])
        x_adv = torch.empty_like(t)
        r_norm = torch.empty(n, dtype=torch.float32, device=dev)
        iters = torch.empty(n, dtype=torch.int32, device=dev)
        final_class = torch.empty(n, dtype=torch.int32, device=dev)
        info = bool(p["return_info"])
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            for a, b in _chunks(n, p["batch_size"] or DEEPFOOL_CALL_IMAGES):
                _native.check(_native.load().dg_deepfool(
                    m._handle, t[a:b].data_ptr(), b - a, int(p["nb_candidate"]), float(p["overshoot"]), int(p["max_iter"]), p["clip_min"],
                    p["clip_max"], x_adv[a:b].data_ptr(), r_norm[a:b].data_ptr() if info else None, iters[a:b].data_ptr() if info else None,
                    final_class[a:b].data_ptr() if info else None, stream))
        return _pack(was_numpy, info, x_adv, r_norm, iters, final_class)


def robustness(model: MLP, x, **deepfool_params):
    """The DeepFool robustness of ``model`` on the images ``x`` (Moosavi-Dezfooli et al. 2016, eq. 15), a dict of floats:

        rho         the mean of ||x_adv - x||_2 / ||x||_2 over the images with ||x||_2 > 0
        mean_l2     the mean of ||x_adv - x||_2
        fooled      the share of images whose first argmax at x_adv is not the one at x
        mean_iters  the mean number of iterations an image was active

    ``deepfool_params``: ``DeepFool.generate``'s, without return_info.  Norms on the device (``dg_deepfool``'s r_norm, ``dg_row_norms``),
    means in float64 on the host; a NaN image makes rho and mean_l2 NaN."""
    import torch
    if "return_info" in deepfool_params:
        raise ValueError("robustness: return_info is not a parameter here")
    DeepFool.parse_params(deepfool_params)                        # refusals before the device is touched
    if model.rec_layer is not None:
        raise NotImplementedError(_DEEPFOOL_REC_NOTE)
    dev = nb._ready(model)
    t, _ = nb._images(model, x, dev, batch="n", nonempty=True)
    _, r_norm, iters, final_class = DeepFool(model).generate(t, return_info=True, **deepfool_params)
    orig = torch.cat([model.eval_batch(t[a:b], None, None, sync=False)[1] for a, b in _chunks(int(t.shape[0]), DEEPFOOL_CALL_IMAGES)])
    return robustness_summary(r_norm.cpu().numpy(), _row_norms(t, None, 2).cpu().numpy(), iters.cpu().numpy(), final_class.cpu().numpy(),
                              orig.cpu().numpy())


def robustness_summary(r_norm, x_norm, iters, final_class, orig):
    """``robustness``'s dict from its per-image arrays (host, float64 means)."""
    r, xn = np.asarray(r_norm, np.float64), np.asarray(x_norm, np.float64)
    nz = xn > 0
    return {"rho": float((r[nz] / xn[nz]).mean()) if nz.any() else float("nan"), "mean_l2": float(r.mean()),
            "fooled": float((np.asarray(final_class) != np.asarray(orig)).mean()), "mean_iters": float(np.asarray(iters, np.float64).mean())}


# ---------------------------------------------------------------------- the L0 attack: the Jacobian saliency map
_JSMA_REC_NOTE = (
    "SaliencyMapMethod on a model with the Defense-GAN reconstruction layer attached (add_rec_model) is not implemented, for "
    "CarliniWagnerL2's reason: in the reference the gradient through ReconstructionLayer is identically zero "
    "(network_builder.py:266-271), so no pair of features is admissible and no step exists.  Build the attack before add_rec_model, "
    "or on a model without it.")
JSMA_CALL_IMAGES = 1000                       # images per dg_jsma call when batch_size is None: bounds the workspace, not the result


class SaliencyMapMethod(object):
    """The Jacobian saliency-map attack (Papernot et al. 2016; cleverhans' ``SaliencyMapMethod``), the suite's L0 attack: targeted, two
    features moved by ``theta`` per iteration, at most ``floor(F * gamma / 2)`` iterations (F = H W C), one device call per
    ``batch_size`` images (``dg_jsma``, defensegan_amd/csrc/dg_jsma.hip; DESIGN.md section 7, "Saliency map", gives the definition):

        adv = x;  dom = the features with x < clip_max (theta > 0) or x > clip_min (theta < 0)
        while the first argmax of O(adv) is not the target and 2 features are left in dom (at most max_iters times):
            a = grad O[t],  b = grad sum_{j != t} O[j]  at adv
            (p, q) = the pair p < q in dom with a_p + a_q > 0 and b_p + b_q < 0 (theta < 0: both signs turned) of the largest
                     -(a_p + a_q)(b_p + b_q), ties to the smallest p, then q;  none of score > 0: the image stops where it is
            adv[p] = clip(adv[p] + theta), adv[q] likewise;  p and q leave dom

    ``of_probs=True`` (cleverhans' ``get_probs``, the default) takes O = softmax(logits): the outputs sum to one, so ``b = -a`` up to
    rounding and the score is ``(a_p + a_q)^2`` -- cleverhans' behaviour; ``of_probs=False`` takes the logits, where the two
    gradients are independent.  An image whose outputs hold a NaN stops and is returned as it is.

    ``generate(x, y_target=..., **params)`` returns ``x_adv`` (NumPy in gives NumPy out; a device tensor in gives a device tensor out
    on the caller's current stream); ``y_target``, required, is class indices or one-hot rows.  ``return_info=True`` adds ``(iters,
    final_class, n_changed)`` [n] int32: the pairs moved, the first argmax of the logits at ``x_adv`` and the number of elements with
    ``x_adv != x``.  ``batch_size`` only bounds the images per device call (default JSMA_CALL_IMAGES): an image's pairs are found
    by its own workgroup, so the result does not depend on it, bit for bit.  ``sess`` / ``back`` are accepted for signature
    compatibility and ignored.

    A model with the reconstruction layer attached raises NotImplementedError (see _JSMA_REC_NOTE); an unknown keyword is a
    ValueError."""

    DEFAULTS = dict(theta=1.0, gamma=1.0, clip_min=0.0, clip_max=1.0, of_probs=True, batch_size=None, return_info=False)

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    @classmethod
    def parse_params(cls, params):
        """DEFAULTS overlaid with ``params``, checked on the host: what ``generate`` accepts besides ``y_target``."""
        unknown = set(params) - set(cls.DEFAULTS)
        if unknown:
            raise ValueError("unknown SaliencyMapMethod parameters: %s" % sorted(unknown))
        p = dict(cls.DEFAULTS, **params)
        p["theta"], p["gamma"] = float(p["theta"]), float(p["gamma"])
        if not np.isfinite(p["theta"]) or p["theta"] == 0.0:
            raise ValueError("theta must be finite and not zero, got %r" % p["theta"])
        if not (np.isfinite(p["gamma"]) and p["gamma"] >= 0.0):
            raise ValueError("gamma must be finite and >= 0, got %r" % p["gamma"])
        _check_iterative(batch_size=p["batch_size"])
        p["clip_min"], p["clip_max"] = _clip_bounds(p["clip_min"], p["clip_max"])
        return p

    @staticmethod
    def max_iters(features, gamma):
        """floor(F * gamma / 2): every iteration moves two features."""
        return int(np.floor(int(features) * float(gamma) / 2))

    def generate(self, x, y_target=None, **params):
        import torch
        p = self.parse_params(params)
        if y_target is None:
            raise ValueError("SaliencyMapMethod is a targeted attack: y_target is required")
        m = self.model
        if m.rec_layer is not None:
            raise NotImplementedError(_JSMA_REC_NOTE)
        dev = nb._ready(m)
        t, was_numpy = nb._images(m, x, dev, batch="n", nonempty=True)
        n = int(t.shape[0])
        lab = _labels(y_target, n, dev, range_words="jsma", nb_classes=m.nb_classes)
        iters_max = self.max_iters(t[0].numel(), p["gamma"])
        x_adv = torch.empty_like(t)
        iters = torch.empty(n, dtype=torch.int32, device=dev)
        final_class = torch.empty(n, dtype=torch.int32, device=dev)
        n_changed = torch.empty(n, dtype=torch.int32, device=dev)
        info = bool(p["return_info"])
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            for a, b in _chunks(n, p["batch_size"] or JSMA_CALL_IMAGES):
                _native.check(_native.load().dg_jsma(
                    m._handle, t[a:b].data_ptr(), lab[a:b].data_ptr(), b - a, p["theta"], iters_max, p["clip_min"], p["clip_max"],
                    1 if p["of_probs"] else 0, x_adv[a:b].data_ptr(), iters[a:b].data_ptr() if info else None,
                    final_class[a:b].data_ptr() if info else None, n_changed[a:b].data_ptr() if info else None, stream))
        return _pack(was_numpy, info, x_adv, iters, final_class, n_changed)
