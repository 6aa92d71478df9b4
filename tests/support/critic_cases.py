"""The critic's value-check cases beyond the MNIST layout, and the helpers the CPU and GPU critic tests share (importable without a
GPU: nothing here touches the device until a critic's weights are installed).

    c, params = critic_of(CASES["mixed"])            # the device critic with the case's weights installed (needs the GPU)
    layers, params = reference_of(CASES["mixed"])    # the same weights for the float64 reference alone (no GPU)
    batch = case_batch(CASES["mixed"], B)            # the recorded draw: no search

Weights are Critic.tflib_init(seed) with biases uniform in +-0.1 (``weights_of``), then the case's ``change_params``.  A case's batch
is draw number ATTEMPT[B] of ``_draw`` (seed, seed + 1000, ...) passed through the case's ``change``: the first draw the float64
reference alone accepts (every activation input at least 1e-6 from zero, conditioning <= 10 under each of the case's axes).  The
attempt numbers were searched on the CPU (tests/test_critic_cases_cpu.py repeats the search and asserts them); the GPU tests use
the recorded draw and search nothing.

    name          input     layers                                                                       B      reaches
    relu_fused    9x6x2     Conv(4,5x5,s2,SAME) ReLU Conv(6,5x5,s2,SAME) ReLU Flatten Linear(1)          5      fused mask (low 0), both weight-gradient calls masked
    relu_unfused  7x5x2     Conv(4,3x3,s1,SAME) LeakyReLU ReLU Flatten Linear(1)                         4      the unfused low = 0 arm
    mixed         8x8x1     Conv(5,3x3,s2,VALID) ReLU Conv(3,1x1,s1,VALID) LeakyReLU Flatten Linear(7)   6      VALID, 1x1, a ReLU fused into a Linear, the hidden
                            ReLU Linear(1)                                                                       Linear's tangent map
    mlp           4x3x2     Flatten Linear(9) LeakyReLU Linear(5) LeakyReLU Linear(1)                    1, 7   Flatten first, the Linear tangent map twice
    nonsquare     11x6x3    Conv(4,(5,2),(3,1),SAME) LeakyReLU Conv(2,(2,3),(1,2),VALID) LeakyReLU       3      kernels and strides that differ per axis, odd SAME
                            Flatten Linear(1)                                                                    padding (1 above, 2 below; 0 left, 1 right)
    wide          3x65x4    Conv(3,3x3,s1,SAME) LeakyReLU Flatten Linear(1)                              3      W C = 260: the column loop's second trip
    flat_h1       1x7x3     Conv(4,(1,3),s1,SAME) LeakyReLU Flatten Linear(1)                            4      H = 1: s = |g|
    zero_columns  9x6x2     the small LeakyReLU critic, first filter's K[:, :, 1, :] = 0                 5      axes 0: s exactly 0 in every (w, c = 1) column
    dead_image    9x6x2     relu_fused, first-layer biases in [-0.1, -0.05], real[2] = fake[2] = 0       5      axes 1: s_2 exactly 0; axes 0: an image of zero columns
    many_images   2x2x1     Flatten Linear(3) LeakyReLU Linear(1)                                        65537  the norm kernels' grid loop; 256-slot plans

No row had to change shape: network_builder.MLP and the handle accept every layer list as written.

float32 headroom (tests/test_critic_cases_cpu.py::test_float32_headroom, measured against the float64 reference, never against the
device): the worst error of param_gradient(dtype=float32) over a case's gradient tensors, as a fraction of the 1e-4 bound -- see
HEADROOM below, asserted to stay under a quarter.  The small cases use under a tenth of the bound (nonsquare 0.072, the others at most
0.005).  many_images is the one that matters: its gradients sum 131074 and 65537 float32 terms.  Drawn from seed 40 its restatement
used 0.374 of the bound, from 41 to 44 it used 0.851, 0.297, 0.493 and 0.736 (the output layer's weight gradient each time, a sum
that cancels); seed 45 is the first under a quarter, 0.101, and is the case's seed.  It keeps the project's bounds unchanged.

mixed: its 3x3 stride-2 VALID convolution never reads input column 7 of 8, so that column's norm is exactly 0 under axes 0 as well
(a second, geometric source of zero norms next to zero_columns and dead_image).
"""
import numpy as np

from defensegan_amd import critic as K
from defensegan_amd import network_builder as nb
from tests.support import critic_reference as R


# ---------------------------------------------------------------------- the helpers of tests/test_gpu_critic.py
SMALL_NAMES = [("D.1.Filters", "D.1.Biases"), ("D.2.Filters", "D.2.Biases"), ("D.Output.W", "D.Output.b")]


def _small_layers():
    return [nb.Conv2D(4, (5, 5), (2, 2), "SAME"), nb.LeakyReLU(), nb.Conv2D(6, (5, 5), (2, 2), "SAME"), nb.LeakyReLU(),
            nb.Flatten(), nb.Linear(1)]


def weights_of(c, seed):
    """tflib's initial values with non-zero biases (the bias gradients and the bias-free tangent pass both show); no device."""
    w = c.tflib_init(seed)
    rs = np.random.RandomState(seed + 1)
    for _, bn in c.param_names:
        w[bn] = rs.uniform(-0.1, 0.1, w[bn].shape).astype(np.float32)
    return w


def _critic(net_dim=8, seed=0, small=False):
    """mnist_discriminator, or (small) a two-convolution critic on 9 x 6 x 2 inputs: 9x6 -> 5x3 -> 3x2, odd sizes on both axes."""
    if small:
        c = K.Critic(_small_layers(), (None, 9, 6, 2), SMALL_NAMES)
    else:
        c = K.mnist_discriminator(net_dim=net_dim)
    w = weights_of(c, seed)
    c.set_named_weights(w)
    return c, [(w[a], w[b]) for a, b in c.param_names]


def _draw(shape, B, seed):
    """real: dark images (uniform cubed, mean 1/4); fake: uniform noise (mean 1/2).  Two batches of ONE distribution would make
    w = mean D(fake) - mean D(real) almost pure cancellation, and a relative bound on it a bound on nothing (_check_terms)."""
    rs = np.random.RandomState(seed)
    real = (rs.uniform(0, 1, (B,) + shape) ** 3).astype(np.float32)
    fake = rs.uniform(0, 1, (B,) + shape).astype(np.float32)
    return real, fake, rs.uniform(0, 1, B).astype(np.float32)


def _safe_attempt(layers, shape, params, B, seed, lam=10.0, axes=(0, 1), change=lambda batch: batch, min_margin=1e-6):
    """(batch, attempt) of _safe, from the reference's layer tuples: no critic object and no device."""
    return R.safe_batch(layers, params, lambda a: change(_draw(tuple(shape), B, seed + 1000 * a)), min_margin=min_margin, max_condition=10.0,
                        lam=lam, axes=axes)


def _safe(c, params, B, seed, lam=10.0, axes=(0, 1), change=lambda batch: batch):
    """The first of the draws seed, seed + 1000, ... (each passed through ``change``) that the float64 reference alone calls well
    posed: every LeakyReLU input 1e-6 from zero, and neither w nor the cost more than nine tenths cancellation (conditioning <= 10),
    so that the relative bounds on them bound the arithmetic and not the luck of the draw."""
    return _safe_attempt(R.describe(c), c.input_shape[1:], params, B, seed, lam, axes, change)[0]


def _check_grads(dev, ref, B, bound=1e-4, what="", bias_scales=None):
    """tests/test_gpu_train.py's form.  One tensor is identically zero in exact arithmetic, the output layer's bias gradient
    sum_b (+1/B) + sum_b (-1/B): a bound relative to its largest entry says nothing there, so it gets the rounding of a float32 sum
    of 2 B terms whose partial sums stay within 1, 2 B 2^-24.  ``bias_scales``: where real == fake EVERY bias gradient is the sum
    of two halves that cancel exactly; each is then bounded relative to the largest entry of one half (given here), which is what
    the bound means for the two sums the device adds."""
    for i, ((dW, db), (rW, rb)) in enumerate(zip(dev, ref)):
        for name, d, r in (("W", dW, rW), ("b", db, rb)):
            scale, err = np.abs(r).max(), np.abs(d - r).max()
            if bias_scales is not None and name == "b":
                scale = bias_scales[i]
            floor = 2 * B * 2.0 ** -24 if (i == len(dev) - 1 and name == "b") else 1e-12
            print("%s layer %d d%s: max|dev - ref| = %.3g, max|ref| = %.3g" % (what, i, name, err, scale))
            assert err <= bound * scale + floor, "%s layer %d d%s: max|dev - ref| = %g, max|ref| = %g" % (what, i, name, err, scale)


def _check_terms(dev, ref, what=""):
    """1e-5 relative on each term (tests/test_gpu_train.py's bound on a loss); the inputs come from _safe, which keeps w and the
    cost from being mostly cancellation."""
    for name, d, r in zip(("cost", "w", "P"), dev, ref):
        print("%s %s: dev %.9g ref %.9g" % (what, name, d, r))
        assert abs(d - r) <= 1e-5 * abs(r), (what, name, d, r)


def _check_all(c, params, batch, lam=10.0, axes=0, what="", bias_scales=None):
    cost, grads, slopes = c.gradient(*batch, gp_lambda=lam, penalty_axes=axes)
    terms, rg, rs = R.param_gradient(R.describe(c), params, *batch, lam=lam, axes=axes)
    assert slopes.shape == rs.shape
    print("%s slopes: max|dev - ref| = %.3g, max|ref| = %.3g" % (what, np.abs(slopes - rs).max(), np.abs(rs).max()))
    assert np.abs(slopes - rs).max() <= 1e-4 * np.abs(rs).max()
    _check_terms(cost, terms, what)
    _check_grads(grads, rg, len(batch[2]), what=what, bias_scales=bias_scales)
    return cost, grads, slopes


# ---------------------------------------------------------------------- the case table
def _output(names):
    return [("D.%d.W" % (i + 1), "D.%d.b" % (i + 1)) for i in range(names - 1)] + [("D.Output.W", "D.Output.b")]


def _relu_fused_layers():
    return [nb.Conv2D(4, (5, 5), (2, 2), "SAME"), nb.ReLU(), nb.Conv2D(6, (5, 5), (2, 2), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(1)]


def _zero_channel_one(params):
    """The first filter ignores input channel 1: g's channel 1 and every (w, c = 1) column norm are exactly 0."""
    W = params[0][0].copy()
    W[:, :, 1, :] = 0.0
    return [(W, params[0][1])] + list(params[1:])


def _negative_first_biases(params):
    """First-layer biases in [-0.1, -0.05]: a zero image leaves every first-layer ReLU input negative."""
    b = np.random.RandomState(4242).uniform(-0.1, -0.05, params[0][1].shape).astype(np.float32)
    return [(params[0][0], b)] + list(params[1:])


DEAD = 2            # dead_image: the image of real and fake that is zero


def _kill_image(batch):
    real, fake, alpha = batch
    real[DEAD] = 0.0
    fake[DEAD] = 0.0
    return real, fake, alpha


class Case(object):
    def __init__(self, name, shape, layers, names, seed, Bs, axes=(0, 1), change=None, change_params=None, attempts=None):
        self.name, self.shape, self.layers, self.names, self.seed, self.Bs, self.axes = name, tuple(shape), layers, names, seed, tuple(Bs), tuple(axes)
        self.change = change or (lambda batch: batch)
        self.change_params = change_params or (lambda params: params)
        self.attempts = attempts or {}

    def critic(self):
        """The host-side container (no device call until weights are installed)."""
        return K.Critic(self.layers(), (None,) + self.shape, self.names)


_C, _L = nb.Conv2D, nb.Linear
CASES = {c.name: c for c in [
    Case("relu_fused", (9, 6, 2), _relu_fused_layers, SMALL_NAMES, seed=31, Bs=(5,), attempts={5: 0}),
    Case("relu_unfused", (7, 5, 2), lambda: [_C(4, (3, 3), (1, 1), "SAME"), nb.LeakyReLU(), nb.ReLU(), nb.Flatten(), _L(1)], _output(2),
         seed=32, Bs=(4,), attempts={4: 0}),
    Case("mixed", (8, 8, 1), lambda: [_C(5, (3, 3), (2, 2), "VALID"), nb.ReLU(), _C(3, (1, 1), (1, 1), "VALID"), nb.LeakyReLU(), nb.Flatten(),
                                      _L(7), nb.ReLU(), _L(1)], _output(4), seed=33, Bs=(6,), attempts={6: 1}),
    Case("mlp", (4, 3, 2), lambda: [nb.Flatten(), _L(9), nb.LeakyReLU(), _L(5), nb.LeakyReLU(), _L(1)], _output(3), seed=34, Bs=(1, 7),
         attempts={1: 0, 7: 0}),
    Case("nonsquare", (11, 6, 3), lambda: [_C(4, (5, 2), (3, 1), "SAME"), nb.LeakyReLU(), _C(2, (2, 3), (1, 2), "VALID"), nb.LeakyReLU(),
                                           nb.Flatten(), _L(1)], _output(3), seed=35, Bs=(3,), attempts={3: 0}),
    Case("wide", (3, 65, 4), lambda: [_C(3, (3, 3), (1, 1), "SAME"), nb.LeakyReLU(), nb.Flatten(), _L(1)], _output(2), seed=36, Bs=(3,),
         attempts={3: 0}),
    Case("flat_h1", (1, 7, 3), lambda: [_C(4, (1, 3), (1, 1), "SAME"), nb.LeakyReLU(), nb.Flatten(), _L(1)], _output(2), seed=37, Bs=(4,),
         attempts={4: 0}),
    Case("zero_columns", (9, 6, 2), _small_layers, SMALL_NAMES, seed=38, Bs=(5,), change_params=_zero_channel_one, attempts={5: 0}),
    Case("dead_image", (9, 6, 2), _relu_fused_layers, SMALL_NAMES, seed=39, Bs=(5,), change=_kill_image, change_params=_negative_first_biases,
         attempts={5: 0}),
    Case("many_images", (2, 2, 1), lambda: [nb.Flatten(), _L(3), nb.LeakyReLU(), _L(1)], _output(2), seed=45, Bs=(65537,), attempts={65537: 1}),
]}

# worst float32-restatement error of a case's gradient tensors as a fraction of the 1e-4 bound (test_float32_headroom prints and
# bounds them; recorded from its output)
HEADROOM = {"relu_fused": 0.0015, "relu_unfused": 0.0023, "mixed": 0.0023, "mlp": 0.0040, "nonsquare": 0.072, "wide": 0.0053, "flat_h1": 0.0018,
            "zero_columns": 0.0040, "dead_image": 0.0029, "many_images": 0.101}


def reference_of(case):
    """(layer tuples, [(W, b)] float32 arrays) of a case, for the float64 reference alone: no device."""
    c = case.critic()
    w = weights_of(c, case.seed)
    return R.describe(c), case.change_params([(w[a], w[b]) for a, b in c.param_names])


def critic_of(case):
    """(critic with the case's weights on the device, params)."""
    c = case.critic()
    w = weights_of(c, case.seed)
    params = case.change_params([(w[a], w[b]) for a, b in c.param_names])
    c.set_weights(params)
    return c, params


def draw_case(case, B, attempt):
    return case.change(_draw(case.shape, B, case.seed + 100 + 1000 * attempt))


def case_batch(case, B):
    """The recorded draw of (case, B): no search."""
    return draw_case(case, B, case.attempts[B])


def search_batch(case, B, min_margin=1e-6):
    """(batch, attempt): the search that ATTEMPT records, on the float64 reference alone."""
    layers, params = reference_of(case)
    return R.safe_batch(layers, params, lambda a: draw_case(case, B, a), min_margin=min_margin, max_condition=10.0, lam=10.0, axes=case.axes)


# the layouts tests/test_gpu_critic.py already runs, as (layer tuples, input shape, batch sizes): for the regime table
def existing_layouts():
    out = []
    for net_dim, Bs in ((8, (1, 3, 6, 8, 16, 50)), (128, (4,)), (4, (3, 16)), (2, (2,))):
        out.append((R.describe(K.mnist_discriminator(net_dim=net_dim)), (28, 28, 1), Bs))
    out.append((R.describe(K.Critic(_small_layers(), (None, 9, 6, 2), SMALL_NAMES)), (9, 6, 2), (5,)))
    return out


# ---------------------------------------------------------------------- LeakyReLU outside the critic: a small classifier
LEAKY_SEED, LEAKY_ATTEMPT = 17, 0            # the first draw whose float64 activation inputs all stay 1e-6 from zero (searched on the CPU)


def leaky_classifier():
    """(model, params, layer tuples): Conv(4,3x3,s2,SAME) LeakyReLU Flatten Linear(6) LeakyReLU Linear(3) Softmax on 8x8x1; no device."""
    from tests.support import bpda_reference, train_reference
    m = nb.MLP([nb.Conv2D(4, (3, 3), (2, 2), "SAME"), nb.LeakyReLU(), nb.Flatten(), nb.Linear(6), nb.LeakyReLU(), nb.Linear(3), nb.Softmax()],
               input_shape=(None, 8, 8, 1))
    return m, bpda_reference.init_params(m, LEAKY_SEED), train_reference.describe(m)


def leaky_inputs(attempt):
    """(x [5,8,8,1] float32 in [0, 1], y [5] int32) of draw ``attempt``."""
    rs = np.random.RandomState(50 + attempt)
    return rs.uniform(0, 1, (5, 8, 8, 1)).astype(np.float32), rs.randint(0, 3, 5).astype(np.int32)
