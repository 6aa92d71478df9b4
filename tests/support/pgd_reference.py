"""CPU restatement of projected gradient descent on a bare classifier ("Whitebox driver and PGD"): the BPDA
restatement of tests/support/bpda_reference.py driven with the identity as the projection and one EOT sample, float64 NumPy, written
independently of the device code (defensegan_amd/csrc/dg_pgd.hip, network_builder.ProjectedGradientDescent).  The classifier's
gradient and predictions are the oracle's (oracle/classifier_oracle.py).

    out = pgd(classifier_ops(layers, clf_params, y), x, y, eps, eps_iter, nb_iter, lo, hi)     # x_adv, first_success, iterates, grads
"""
import numpy as np

from tests.support import bpda_reference as R


class _Identity(object):
    """``ops`` of R.bpda whose projection returns its input: gradient and predict are the wrapped object's."""

    def __init__(self, inner):
        self.gradient, self.predict = inner.gradient, inner.predict

    def project(self, x_k, seed):
        return x_k


def pgd(ops, x, y, eps, eps_iter, nb_iter, lo, hi, x_init=None, noise=None):
    """ops.gradient(x_k) -> d CE / dx, ops.predict(x_k) -> [n] classes.  The dict R.bpda returns."""
    return R.bpda(_Identity(ops), x, y, eps, eps_iter, nb_iter, 1, lo, hi, 0, x_init=x_init, noise=noise)


class classifier_ops(object):
    """gradient = the oracle's cross-entropy input gradient for the labels y, predict = first argmax of the oracle's logits."""

    def __init__(self, layers, clf_params, y):
        self.layers, self.y = layers, np.asarray(y)
        self.cp = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in clf_params]

    def gradient(self, x_k):
        from oracle import classifier_oracle as CO
        return CO.input_gradient(self.layers, self.cp, x_k, self.y)

    def predict(self, x_k):
        from oracle import classifier_oracle as CO
        return CO.forward(self.layers, self.cp, x_k)[0].argmax(axis=1)


# The teacher-forced GPU cases, fixed on the CPU (tests/test_whitebox_cpu.py asserts what the choice of seeds promises: at most 1 % of
# the pixels undecided at every teacher-forced iterate): model F at 7 x 28 x 28 x 1; a Conv + Linear model at 3 x 5 x 5 x 1, whose
# 25-element rows take the scalar form of the step kernel; a two-class model at 3 x 64 x 64 x 3 with clip_min = -1.
CASES = {
    "F": dict(B=7, shape=(28, 28, 1), classes=10, clf_seed=70, x_seed=31, eps=0.3, eps_iter=0.05, lo=0.0, hi=1.0),
    "convlin5": dict(B=3, shape=(5, 5, 1), classes=10, clf_seed=5, x_seed=3, eps=0.3, eps_iter=0.05, lo=0.0, hi=1.0),
    "two64": dict(B=3, shape=(64, 64, 3), classes=2, clf_seed=7, x_seed=11, eps=0.3, eps_iter=0.05, lo=-1.0, hi=1.0),
}


def case_model(name):
    """The case's model (no device touched)."""
    from defensegan_amd import network_builder as nb
    c = CASES[name]
    shape = (None,) + c["shape"]
    if name == "F":
        return nb.model_f(input_shape=shape)
    if name == "convlin5":
        return nb.MLP([nb.Conv2D(4, (3, 3), (1, 1), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(c["classes"]), nb.Softmax()], input_shape=shape)
    return nb.MLP([nb.Conv2D(8, (5, 5), (2, 2), "SAME"), nb.ReLU(), nb.Conv2D(8, (3, 3), (2, 2), "VALID"), nb.ReLU(), nb.Flatten(),
                   nb.Linear(c["classes"]), nb.Softmax()], input_shape=shape)


def case_inputs(name):
    """(x [B,H,W,C] float32 in [lo, hi], y [B] int32, model, clf_params)."""
    c = CASES[name]
    model = case_model(name)
    rs = np.random.RandomState(c["x_seed"])
    x = rs.uniform(c["lo"], c["hi"], (c["B"],) + c["shape"]).astype(np.float32)
    y = rs.randint(0, c["classes"], c["B"]).astype(np.int32)
    return x, y, model, R.init_params(model, c["clf_seed"])


_REFS = {}


def case_reference(name, nb_iter=3):
    """The float64 run of the case, computed once and shared (never modified)."""
    if (name, nb_iter) not in _REFS:
        c = CASES[name]
        x, y, model, cp = case_inputs(name)
        _REFS[(name, nb_iter)] = pgd(classifier_ops(R.layers_of(model), cp, y), x, y, c["eps"], c["eps_iter"], nb_iter, c["lo"], c["hi"])
    return _REFS[(name, nb_iter)]
