"""-m "not gpu": what tests/test_gpu_strided.py compares the device with, pinned on its own, and what the choice of its cases
(tests/support/strided_cases.py) promises: the softmax seed at wide class counts against torch autograd, the float32 restatement of
the class gradient against float64, best tracking at a batch longer than a grid against a per-image loop, the grid caps against
the launchers' source text, and the cases' margins."""
import os

import numpy as np
import pytest

from oracle import classifier_oracle as CO
from tests.support import blackbox_reference as BR
from tests.support import bpda_reference as R
from tests.support import cw_cases as K
from tests.support import cw_reference as CW
from tests.support import pgd_reference as P
from tests.support import strided_cases as S
from tests.support import train_reference as TR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "defensegan_amd", "csrc")


# ---------------------------------------------------------------------- the references, pinned
@pytest.mark.parametrize("n", S.WIDTHS)
def test_softmax_seed_matches_autograd_at_wide_class_counts(n):
    """blackbox_reference.softmax_seed, TF's (delta_kc - p_c) * p_k, is d softmax(z)[c] / dz by torch autograd, on near-uniform
    logits and on logits spread over 30, with the class in every position a 64-lane stride distinguishes."""
    import torch
    rs = np.random.RandomState(n)
    for width in (0.3, 30.0):
        z = rs.uniform(-width / 2, width / 2, (6, n))
        classes = np.array([0, n - 1, n // 2, min(63, n - 1), min(64, n - 1), rs.randint(0, n)])
        zt = torch.tensor(z, requires_grad=True)
        p = torch.softmax(zt, dim=1)[torch.arange(6), torch.as_tensor(classes)]
        (want,) = torch.autograd.grad(p.sum(), zt)
        got = BR.softmax_seed(z, classes)
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-12, atol=1e-16)
        np.testing.assert_allclose(got.sum(axis=1), 0, atol=1e-15)           # the probabilities sum to 1


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("n", S.WIDTHS)
def test_float32_restatement_of_the_class_gradient_is_float64_to_rounding(kind, n):
    """strided_cases.class_gradient32 (every sum in the kernels' documented order, the butterfly included) against
    blackbox_reference.class_gradient: the same function, to float32 rounding, on the plain and on the spread case; a class outside
    the range gives a zero row."""
    for spread in (False, True):
        c = S.case(kind, n, spread)
        classes = S.spread_classes(c["z"]) if spread else c["y"]
        ref = BR.class_gradient(c["layers"], c["p64"], c["x"], classes)
        g32 = S.class_gradient32(kind, c["params"], c["x"], classes)
        err = np.abs(g32 - ref).max() / np.abs(ref).max()
        rows = np.abs(g32 - ref).reshape(len(ref), -1).max(axis=1) / np.abs(ref).reshape(len(ref), -1).max(axis=1)
        print("%s n %d spread %d: float32 restatement within %.3g of max|f64|; per image at worst %.3g of its own largest element"
              % (kind, n, spread, err, rows.max()))
        assert g32.dtype == np.float32 and err <= 1e-5
    bad = np.array(classes)
    bad[0], bad[1] = n, -1
    g = S.class_gradient32(kind, c["params"], c["x"], bad)
    assert (g[:2] == 0).all() and g[2:].tobytes() == g32[2:].tobytes()


def test_butterfly_sum_is_the_sum():
    rs = np.random.RandomState(0)
    lanes = rs.uniform(0, 1, (5, 64)).astype(np.float32)
    np.testing.assert_allclose(S._butterfly_sum32(lanes), lanes.astype(np.float64).sum(axis=1), rtol=1e-6)


# ---------------------------------------------------------------------- the cases
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("n", S.WIDTHS)
def test_cases_are_decided_and_spread(kind, n):
    for spread in (False, True):
        c = S.case(kind, n, spread)
        z = c["z"]
        assert c["x"].shape[0] == max(S.BATCHES) == 67 and c["x"].dtype == np.float32 and c["x"].min() >= 0 and c["x"].max() <= 1
        assert TR.relu_margins(c["layers"], c["p64"], c["x"]).min() >= S.MARGIN and S.top_gap(z).min() >= S.GAP
        np.testing.assert_allclose(z, CO.forward(c["layers"], c["p64"], c["x"].astype(np.float64))[0], rtol=1e-12, atol=1e-12)
        rng = z.max(axis=1) - z.min(axis=1)
        if not spread:
            assert rng.max() < 0.2 * S.SPREAD                                 # as drawn, no row is concentrated
            continue
        target = S.SPREAD if n > 2 else S.SPREAD_TWO
        assert abs(np.median(rng) - target) < 0.1 * target
        p = BR.softmax(z)
        classes = S.spread_classes(z)
        pc = p[np.arange(len(z)), classes]
        # concentrated, yet p_c has not rounded to 1 in float32 (1 - p_c well above 2^-24) on the images of B = 1 and 5 and on nine
        # in ten of all 67 (with two classes a few rows' only gap is wide enough to saturate), and some p_c carry real mass
        assert p.max(axis=1).min() > (0.5 if n == 2 else 2.0 / n) and (1 - pc[:5]).min() > 1e-5 and (1 - pc > 1e-5).mean() >= 0.9
        assert (pc > 0.1).sum() >= 3
        if n > 64:
            assert (classes >= 64).all() and z[0].argmax() == 64 and classes[0] == 64 and pc[0] > 0.1
        assert all((classes[:B] < n).all() for B in S.BATCHES)


def test_grid_caps_are_the_launchers():
    """The caps the long-batch tests are sized by, as the launchers state them."""
    for name, text in S.CAP_SOURCES:
        with open(os.path.join(CSRC, name)) as fh:
            assert text in fh.read(), (name, text)
    assert (S.BPDA_TRACK_CAP, S.PGD_TRACK_CAP, S.BALL_CAP) == (1024, 4096 * 4, 65536)


# ---------------------------------------------------------------------- tracking at a long batch
@pytest.mark.parametrize("row_elems", [5, 300])
def test_track_at_a_long_batch_is_the_per_image_rule(row_elems):
    B = 2 * S.BPDA_TRACK_CAP + 3
    labels, preds, iterates, want_first = S.track_case(B, row_elems)
    adv, first = R.track(preds, labels, iterates)
    for b in list(range(10)) + list(range(S.BPDA_TRACK_CAP - 3, S.BPDA_TRACK_CAP + 7)) + list(range(B - 8, B)):
        hit = [k for k in (1, 2, 3) if preds[k][b] != labels[b]]
        assert first[b] == (hit[0] if hit else -1) == want_first[b]
        assert adv[b].tobytes() == iterates[hit[0] if hit else 3][b].tobytes()
    assert first.tolist() == want_first.tolist()
    pat = np.arange(B) % 5
    assert ((preds[2] == labels) & (preds[3] == labels))[pat == 3].all() and (preds[3] == labels)[pat == 4].all()      # undone later
    for lo, hi in ((0, S.BPDA_TRACK_CAP), (S.BPDA_TRACK_CAP, 2 * S.BPDA_TRACK_CAP)):
        assert set(want_first[lo:hi].tolist()) == {-1, 1, 2, 3} and set(pat[lo:hi].tolist()) == set(range(5))
    assert pat[B - 3:].tolist() == [3, 4, 0]


# ---------------------------------------------------------------------- what the 130-class attack cases promise
def test_pgd_case_at_130_classes_spreads_its_successes():
    c = S.case("mlp", 130)
    x = c["x"]
    own = c["z"].argmax(axis=1)
    g = CO.input_gradient(c["layers"], c["p64"], x.astype(np.float64), own)
    for B in S.BATCHES:
        assert (np.abs(g[:B]) <= 1e-4 * np.abs(g[:B]).max()).mean() <= 0.005
    y = own.copy()
    y[0] = (y[0] + 1) % 130
    out = P.pgd(P.classifier_ops(c["layers"], c["p64"], y), x, y, 0.3, 0.01, 4, 0.0, 1.0)
    first = out["first_success"]
    print("float64 PGD at 130 classes: first_success %s" % first.tolist())
    assert first[0] == 1 and len(set(first.tolist())) >= 4 and (first == -1).sum() >= 5
    assert max(int(p.max()) for p in out["preds"].values()) >= 64


def test_carlini_wagner_case_at_130_classes_is_decidable():
    c = S.case("mlp", 130, True)
    for B in S.BATCHES:
        x = c["x"][:B]
        labels = c["z"][:B].argmax(axis=1)
        labels[1::2] = np.argsort(c["z"][:B], axis=1)[1::2, -2]
        for name in ("b-i1", "b-i2"):
            ref = CW.cw_l2(c["layers"], c["p64"], x.astype(np.float64), labels=labels, targeted=False, trace=True, **K.case(name)["kw"])
            keep, chunks_ok = K.decidable(ref)
            assert chunks_ok and keep.all()
            assert (ref["best_class"][1::2] != -1).all() and (ref["best_l2"][1::2] == 0).all()
    assert K.case("b-i1")["kw"]["max_iterations"] == 1 == min(K.case(nm)["kw"]["max_iterations"] for nm in K.NAMES)
