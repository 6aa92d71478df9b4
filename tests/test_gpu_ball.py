"""-m gpu: the L1 / L2 attacks on the device (defensegan_amd/csrc/dg_ball.hip: dg_row_norms, dg_fgm, dg_pgd_ball, dg_bpda_step_ball;
network_builder's ``ord``) against the float64 restatement in tests/support/ball_reference.py, and their bitwise identities.

Row lengths: model E on 28 x 28 x 1 (P = 784: the register path, float4), case G1 of tests/support/geometry_cases.py (P = 378, no
multiple of 4: the scalar path, in registers), the 64 x 64 x 3 two-class model of the training tests (P = 12 288: the re-read path,
48 full rounds of 256 float4) and a small model on 13 x 20 x 4 (P = 1040: the re-read path with a ragged last round, 260 float4 or
1040 floats).  Views offset by one float put the two long rows, and every row length of dg_row_norms, on the scalar instantiations.
Batch sizes 1, 5 and 11: every image is its own workgroup's work, so rows [:B] of the B = 11 reference are the reference of batch
size B; each case's float64 run is computed once and shared.  Each test prints the figure it is about to assert (pytest -s shows them).

Bounds, with u = 2^-24:
  norm(P) = (ceil(P / 256) + 10) u, relative: a thread adds at most ceil(P / 256) + 3 non-negative terms in order (float4: four per
      vector), the butterfly adds 6 roundings, the wave partials 3, the difference v - w one, the root halves the sum's relative
      error and adds half an ulp.
  teacher-forced (the device's own float32 gradient fed to float64): (norm(P) + 4 u) of the largest element of the step's result.
      adv = fl(x + s g_i), s = fl(eps / n): s carries the norm's error and half an ulp of the division, the fused multiply-add
      rounds once at the result's magnitude (one u of it); the L2 step adds the rounding of x_k + a t (one u at the iterate's
      magnitude), of the subtraction of x, and a second norm, of d.  Each root halves its sum's error, so the two norms together stay
      within norm(P); the remaining roundings are the 4 u.  The scale is the result, not the perturbation: the final addition rounds
      at the magnitude of x + d whatever the size of d.
  end to end (the gradient is the device's, the reference's is float64): dg_clf_backward's bound (tests/test_gpu_geometry.py) says
      that the device's gradient is g + e with |e_bi| <= E = 2e-5 max|g| over the batch.  The perturbation of image b is
      p = eps g_b / n_b with n_b the ord-norm, and |n(g_b + e_b) - n_b| <= n(e_b) <= c E, c = sqrt(P) for ord 2 and P for ord 1.  So
          |p'_i - p_i| <= eps |e_i| / n' + eps |g_i| |1 / n' - 1 / n| <= eps E (1 + c max|g_b| / n_b) / (n_b - c E)       (grad_term)
      per image, nothing dropped.  The clip is 1-Lipschitz, so the same holds for adv; the kernel's own roundings add the
      teacher-forced bound.  The first L2 step from x_0 = x stays inside the ball (eps_iter < eps), so it is the ord-2 formula with
      eps_iter.  With m EOT samples E is the sum of the samples' 2e-5 max|g_s|.  The factor (1 + c max|g_b| / n_b) is 5 to 12 on
      these cases: an elementwise gradient error may move the norm by sqrt(P) times as much, which no tighter figure can exclude.
Measured on an MI355X, the worst case over every case and batch size: dg_row_norms 2.4 u relative (bounds 12 to 58 u); teacher-forced
FGM 6.5 % of its bound, teacher-forced L2 steps 6.1 %, the offset views 5.2 %; end to end 0.5 % (FGM), 0.6 % (first L2 step) and
0.6 % (BPDA) of theirs: the end-to-end check is as loose as dg_clf_backward's own figure, the teacher-forced one is the sharp one.

Throw-away mutations of dg_ball.hip, each built into a scratch copy of the library and run against this file on an MI355X (48 tests;
"all" = every case of the parametrised test):
  ball_block_sum drops the fourth wave partial        45 fail: row_norms (all), teacher_forced (all), long_rows_on_views (both),
                                                      end_to_end (all), full_pgd_l2_runs (all), both bpda_l2 step cases, bpda batch_size
  ball_step_kernel projects with ||t|| for ||d||      20 fail: teacher_forced (all, at the projected step k = 2), long_rows_on_views
                                                      (both), full_pgd_l2_runs (all), bpda batch_size, whitebox
  ball_step_kernel without min(1, .)                  30 fail: teacher_forced (all), end_to_end (all: the first step is scaled up to
                                                      eps), full_pgd_l2_runs (all), both bpda_l2 step cases
  the step kernels' re-read loops stop at the last    8 fail, the T1040 cases alone: teacher_forced (3), long_rows_on_views, end_to_end (3),
  full round of 256 vectors                           full_pgd_l2_runs; A16c's 3072 float4 and 12 288 floats have no tail and pass
"""
import functools
import math
import os

import numpy as np
import pytest

from defensegan_amd import _native, gan_defense, network_builder as nb, whitebox as wb
from tests.helpers import make_gan
from tests.support import ball_reference as BR
from tests.support import bpda_reference as R
from tests.support import geometry_cases as G
from tests.support import pgd_reference as P
from tests.support import train_reference as TR

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MARGIN = 1e-6                                     # tests/test_gpu_train_shapes.py: every float64 ReLU input this far from zero
BATCH_SIZES = (1, 5, 11)
NB_ITER = 4
# eps_iter < eps < NB_ITER eps_iter: the first step lands inside the ball, later ones are projected.  All exact in float32.
CASES = {
    "E": dict(shape=(28, 28, 1), lo=0.0, hi=1.0, eps=2.0, eps_iter=0.75, eps_l1=49.0),
    "G1": dict(shape=G.input_shape("G1"), lo=-1.0, hi=1.0, eps=1.0, eps_iter=0.375, eps_l1=23.625),
    "A16c": dict(shape=(64, 64, 3), lo=-1.0, hi=1.0, eps=4.0, eps_iter=1.5, eps_l1=768.0),
    "T1040": dict(shape=(13, 20, 4), lo=-1.0, hi=1.0, eps=1.5, eps_iter=0.5625, eps_l1=48.0),
}
LONG = ("A16c", "T1040")                          # P > 1024: the re-read path
BETA = 2e-5                                       # dg_clf_backward's bound: of the largest element of the reference gradient


def norm_bound(row_elems):
    return (math.ceil(row_elems / 256.0) + 10) * U


def step_bound(row_elems):
    return norm_bound(row_elems) + 4 * U


def _ragged_model():
    """13 x 20 x 4 -> a (3,3)/(2,2) SAME convolution with 4 filters, ReLU, Linear 3, Softmax; weights as geometry_cases.params draws them."""
    m = nb.MLP([nb.Conv2D(4, (3, 3), (2, 2), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(3), nb.Softmax()], (None, 13, 20, 4))
    probe = nb.MLP([nb.Conv2D(4, (3, 3), (2, 2), "SAME"), nb.ReLU(), nb.Flatten(), nb.Linear(3), nb.Softmax()], (None, 13, 20, 4))
    probe.set_weights = lambda p: None
    rs = np.random.RandomState(1041)
    return m, [(W, rs.uniform(-G.BIAS_WIDTH, G.BIAS_WIDTH, size=b.shape).astype(np.float32)) for W, b in probe.init_like_reference(seed=1040)]


def _model(name):
    if name == "T1040":
        return _ragged_model()
    if name == "E":
        m = nb.model_e()
        return m, R.init_params(m, 70)
    if name == "G1":
        return G.model(name), G.params(name)
    m = TR.shape_model("A16c")
    return m, R.init_params(m, 7)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x [11, ...] float32 in [lo, hi] with every float64 ReLU input MARGIN from zero, y [11] int32, layers, float64 parameters)."""
    c = CASES[name]
    m, cp = _model(name)
    layers = TR.describe(m)
    p64 = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in cp]
    rs = np.random.RandomState(sum(map(ord, name)))
    draw = lambda n: rs.uniform(c["lo"], c["hi"], (n,) + c["shape"]).astype(np.float32)
    x = draw(max(BATCH_SIZES))
    for _ in range(40):
        bad = TR.relu_margins(layers, p64, x) < MARGIN
        if not bad.any():
            break
        x[bad] = draw(int(bad.sum()))
    else:
        raise AssertionError("no batch with every ReLU input %g from zero" % MARGIN)
    classes = p64[-1][1].size
    return x, rs.randint(0, classes, len(x)).astype(np.int32), layers, p64


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case's float64 PGD-L2 run at B = 11, computed once and never modified."""
    c = CASES[name]
    x, y, layers, p64 = _case(name)
    return BR.pgd_l2(P.classifier_ops(layers, p64, y), x, y, c["eps"], c["eps_iter"], NB_ITER, c["lo"], c["hi"])


@functools.lru_cache(maxsize=None)
def _oracle_gradient(name, own):
    """The float64 input gradient at the case's x for its labels, or (own) the model's own arg-max: once, at B = 11."""
    from oracle import classifier_oracle as CO
    x, y, layers, p64 = _case(name)
    return CO.input_gradient(layers, p64, x.astype(np.float64), None if own else y)


@pytest.fixture(scope="module")
def models():
    import torch
    out = {}
    for name in CASES:
        m, cp = _model(name)
        m.set_weights(list(cp))
        out[name] = m
    yield out
    torch.cuda.synchronize()
    for m in out.values():
        m.close()


def _kw(c):
    return dict(eps=c["eps"], eps_iter=c["eps_iter"], clip_min=c["lo"], clip_max=c["hi"], ord=2)


def _within(what, got, ref, bound, scale):
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    print("%s: max|dev - f64| = %.3g = %.3g of the bound %.3g (scale %.3g)" % (what, err, err / (bound * scale), bound * scale, scale))
    assert np.isfinite(got).all() and err <= bound * scale, (what, err, bound * scale)
    return err / (bound * scale)


def grad_term(g, eps, ord, E):
    """[n]: the module docstring's end-to-end bound on |p' - p| per image, for the float64 gradient g [n, ...] whose device
    counterpart is within E of it element by element."""
    g = np.asarray(g, np.float64).reshape(len(g), -1)
    c = g.shape[1] if ord == 1 else math.sqrt(g.shape[1])
    n = BR.row_norms(g, ord)
    assert (n > 2 * c * E).all(), "a gradient too small for its norm to be known"
    return eps * E * (1 + c * np.abs(g).max(axis=1) / n) / (n - c * E)


def _within_rows(what, got, ref, bound_rows):
    """max over each image of |got - ref| against that image's bound."""
    err = np.abs(np.asarray(got, np.float64) - ref).reshape(len(ref), -1).max(axis=1)
    worst = float((err / bound_rows).max())
    print("%s: max|dev - f64| = %.3g, at worst %.3g of the image's bound (bounds %.3g .. %.3g)" % (what, err.max(), worst, bound_rows.min(), bound_rows.max()))
    assert np.isfinite(got).all() and (err <= bound_rows).all(), (what, err, bound_rows)
    return worst


# ---------------------------------------------------------------------- 1. dg_row_norms
@pytest.mark.parametrize("row_elems", [784, 378, 12288, 1040])
@pytest.mark.parametrize("B", BATCH_SIZES)
def test_row_norms_against_float64(row_elems, B):
    """ord 1 and 2, of v and of v - w, aligned and on a view offset by one float; a row whose only non-zero element is its last, and
    a row of zeros.  Relative bound norm(P); the row of zeros gives exactly 0."""
    import torch
    rs = np.random.RandomState(row_elems + B)
    v = rs.standard_normal((B, row_elems)).astype(np.float32)
    w = rs.standard_normal((B, row_elems)).astype(np.float32)
    if B >= 3:
        v[1] = 0
        v[1, -1] = -1.7
        v[2] = 0
    flat = torch.empty(2 * B * row_elems + 1, device="cuda")
    for off in (0, 1):
        tv = flat[off:off + B * row_elems].view(B, row_elems)
        tw = torch.from_numpy(w).cuda()
        tv.copy_(torch.from_numpy(v))
        assert (tv.data_ptr() % 16 == 0) == (off == 0)
        for ord in (1, 2):
            for with_w in (False, True):
                got = nb._row_norms(tv, tw if with_w else None, ord).cpu().numpy()
                want = BR.row_norms(v, ord, w if with_w else None)
                rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
                print("P %d B %d offset %d ord %d w %d: max relative error %.3g u (bound %.1f u)" %
                      (row_elems, B, off, ord, with_w, rel.max() / U, norm_bound(row_elems) / U))
                assert got.dtype == np.float32 and np.isfinite(got).all() and rel.max() <= norm_bound(row_elems)
                if B >= 3 and not with_w:
                    assert got[2] == 0.0 and got[1] == np.float32(1.7)


# ---------------------------------------------------------------------- 2. the new kernels, teacher-forced
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("B", BATCH_SIZES)
def test_fgm_and_l2_step_teacher_forced(models, name, B):
    """The device's own float32 gradient (input_gradient) fed to the float64 restatement: FGM ord 1 and 2 at x, and one L2 step from
    the reference's x_k, k = 0, 1, 2.  Bound: the module docstring's teacher-forced one."""
    c, m = CASES[name], models[name]
    x, y = _case(name)[0][:B], _case(name)[1][:B]
    row = x[0].size
    g = m.input_gradient(x, labels=y)
    assert np.abs(g).reshape(B, -1).max(axis=1).min() > 0
    for ord, eps in ((1, c["eps_l1"]), (2, c["eps"])):
        for lo, hi in ((c["lo"], c["hi"]), (None, None)):
            adv = nb.FastGradientMethod(m).generate(x, eps=eps, ord=ord, y=y, clip_min=lo, clip_max=hi)
            ref = BR.fgm(x, g, eps, ord, -np.inf if lo is None else lo, np.inf if hi is None else hi)
            _within("%s B %d FGM ord %d clip %s" % (name, B, ord, lo is not None), adv, ref, step_bound(row), np.abs(ref).max())
            assert np.abs(adv - x).max() > 0.01
    ref_run = _reference(name)
    atk = nb.ProjectedGradientDescent(m)
    for k in range(3):
        xk = ref_run["iterates"][k][:B].astype(np.float32)
        gk = m.input_gradient(xk, labels=y)
        nxt = atk.generate(x, y, nb_iter=1, x_init=xk, **_kw(c))
        info = {}
        ref = BR.l2_step(x, xk, gk, c["eps"], c["eps_iter"], c["lo"], c["hi"], info=info)
        _within("%s B %d L2 step k %d (projected: %d of %d)" % (name, B, k, int(info["projected"].sum()), B), nxt, ref, step_bound(row),
                np.abs(ref).max())
        # k = 0 and 1 stay inside the ball (2 eps_iter < eps); k = 2 is the projected step: image 0, so that every B has one
        assert info["projected"][0] == (k == 2) and not (k < 2 and info["projected"].any())


@pytest.mark.parametrize("name", LONG)
def test_long_rows_on_views_offset_by_one_float(models, name):
    """The scalar instantiations of the re-read path (fgm_norm_step_kernel<1, false>, ball_step_kernel<1, false>): x and x_init are
    device views one float past a 16-byte boundary, as a caller's slice may be.  FGM ord 1 and 2 and the projected L2 step from the
    reference's x_2, teacher-forced as above and to the same bound."""
    import torch
    c, m, B = CASES[name], models[name], 5
    x, y = _case(name)[0][:B], _case(name)[1][:B]
    row = x[0].size
    x2 = _reference(name)["iterates"][2][:B].astype(np.float32)
    flat = torch.empty(2 * (B * row + 4), device="cuda")
    tx = flat[1:1 + B * row].view(x.shape)
    t2 = flat[B * row + 5:2 * B * row + 5].view(x.shape)
    tx.copy_(torch.from_numpy(x))
    t2.copy_(torch.from_numpy(x2))
    assert tx.data_ptr() % 16 == 4 and t2.data_ptr() % 16 == 4 and tx.is_contiguous() and t2.is_contiguous()
    g = m.input_gradient(x, labels=y)
    for ord, eps in ((1, c["eps_l1"]), (2, c["eps"])):
        adv = nb.FastGradientMethod(m).generate(tx, eps=eps, ord=ord, y=y, clip_min=c["lo"], clip_max=c["hi"]).cpu().numpy()
        ref = BR.fgm(x, g, eps, ord, c["lo"], c["hi"])
        _within("%s offset FGM ord %d" % (name, ord), adv, ref, step_bound(row), np.abs(ref).max())
        assert np.abs(adv - x).max() > 0.01
    info = {}
    ref = BR.l2_step(x, x2, m.input_gradient(x2, labels=y), c["eps"], c["eps_iter"], c["lo"], c["hi"], info=info)
    nxt = nb.ProjectedGradientDescent(m).generate(tx, y, nb_iter=1, x_init=t2, **_kw(c)).cpu().numpy()
    assert info["projected"].all()
    _within("%s offset L2 step k 2" % name, nxt, ref, step_bound(row), np.abs(ref).max())
    assert np.array_equal(tx.cpu().numpy(), x) and np.array_equal(t2.cpu().numpy(), x2)


# ---------------------------------------------------------------------- 3. end to end against float64
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("B", BATCH_SIZES)
def test_fgm_and_first_step_end_to_end_against_float64(models, name, B):
    """The gradient is the oracle's here (float64, labels given and the model's own arg-max): the module docstring's end-to-end bound."""
    c, m = CASES[name], models[name]
    x, y, layers, p64 = _case(name)
    x, y = x[:B], y[:B]
    row = x[0].size
    for labels in (y, None):
        g = _oracle_gradient(name, labels is None)[:B]
        for ord, eps in ((1, c["eps_l1"]), (2, c["eps"])):
            adv = nb.FastGradientMethod(m).generate(x, eps=eps, ord=ord, y=labels)
            ref = BR.fgm(x, g, eps, ord, -np.inf, np.inf)
            _within_rows("%s B %d FGM ord %d labels %d" % (name, B, ord, labels is not None), adv, ref,
                         grad_term(g, eps, ord, BETA * np.abs(g).max()) + step_bound(row) * np.abs(ref).max())
    ref_run = _reference(name)
    nxt = nb.ProjectedGradientDescent(m).generate(x, y, nb_iter=1, **_kw(c))
    ref = ref_run["iterates"][1][:B]
    g = ref_run["grads"][0][:B]
    assert not ref_run["projected"][0].any() and np.array_equal(ref_run["iterates"][0][:B], x)
    _within_rows("%s B %d first L2 step" % (name, B), nxt, ref, grad_term(g, c["eps_iter"], 2, BETA * np.abs(g).max()) + step_bound(row) * np.abs(ref).max())


# ---------------------------------------------------------------------- 4. full PGD-L2 runs
@pytest.mark.parametrize("name", sorted(CASES))
def test_full_pgd_l2_runs(models, name):
    c, m = CASES[name], models[name]
    x, y, _, _ = _case(name)
    ref = _reference(name)
    assert c["eps_iter"] < c["eps"] < NB_ITER * c["eps_iter"]
    assert not ref["projected"][0].any() and ref["projected"][-1].all()             # inside the ball first, projected later
    atk = nb.ProjectedGradientDescent(m)
    own = m.get_probs(x).argmax(axis=1).astype(np.int32)
    labels = own.copy()
    labels[0] = (labels[0] + 1) % int(m.nb_classes)                                 # misclassified from the start
    adv, first, dist = atk.generate(x, labels, nb_iter=NB_ITER, return_info=True, **_kw(c))
    bound = step_bound(x[0].size)
    true = BR.row_norms(adv, 2, x)
    print("%s: dist %s, eps %.3g, largest dist / eps - 1 = %.3g (bound %.3g); first_success %s" %
          (name, np.round(dist, 4).tolist(), c["eps"], dist.max() / c["eps"] - 1, bound, first.tolist()))
    assert np.isfinite(adv).all() and dist.dtype == np.float32 and dist.max() <= c["eps"] * (1 + bound)
    assert np.abs(dist - true).max() <= norm_bound(x[0].size) * true.max() and dist.min() > 0
    assert adv.min() >= c["lo"] and adv.max() <= c["hi"]
    # first_success by today's rule: the iterates rebuilt by chained one-iteration calls, judged by dg_eval_batch
    iterates, cur = [], None
    for _ in range(NB_ITER):
        cur = atk.generate(x, labels, nb_iter=1, x_init=cur, **_kw(c))
        iterates.append(cur)
    last = BR.row_norms(iterates[-1], 2, x)                 # the returned image may be an early iterate; the last one was projected
    print("%s: the last iterate's distance / eps - 1: %.3g .. %.3g" % (name, last.min() / c["eps"] - 1, last.max() / c["eps"] - 1))
    assert last.max() <= c["eps"] * (1 + bound) and last.min() > 0.8 * c["eps"]
    preds = {j + 1: m.eval_batch(it, None, labels)[1].cpu().numpy() for j, it in enumerate(iterates)}
    want_adv, want_first = R.track(preds, labels, [np.clip(x, c["lo"], c["hi"])] + iterates)
    assert first.tolist() == want_first.tolist() and first[0] == 1
    assert adv.tobytes() == want_adv.astype(np.float32).tobytes()
    # a label outside the class range: a zero gradient, a zero step, no NaN -- the image stays at x_0
    bad = own.copy()
    bad[1], bad[3] = int(m.nb_classes), -1
    adv_bad, first_bad, dist_bad = atk.generate(x, bad, nb_iter=NB_ITER, return_info=True, **_kw(c))
    assert np.isfinite(adv_bad).all()
    for i in (1, 3):
        assert adv_bad[i].tobytes() == x[i].tobytes() and dist_bad[i] == 0.0 and first_bad[i] == 1
    ok = np.ones(len(x), bool)
    ok[[1, 3]] = False
    assert adv_bad[ok].tobytes() == atk.generate(x[ok], own[ok], nb_iter=NB_ITER, **_kw(c)).tobytes()
    # independent of batch_size and repeatable, bit for bit, rand_init included
    kw = dict(_kw(c), nb_iter=NB_ITER, rand_init=True, seed=5, return_info=True)
    runs = [atk.generate(x, own, batch_size=bs, **kw) for bs in (2, 7, None, None)]
    for r in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0]))
    assert not np.array_equal(runs[0][0], atk.generate(x, own, nb_iter=NB_ITER, **_kw(c)))
    # the rand_init start lies in the L2 ball: with eps_iter = 0 the first iterate is x_0 (to the step's roundings)
    x0 = atk.generate(x, own, nb_iter=1, eps=c["eps"], eps_iter=0.0, clip_min=c["lo"], clip_max=c["hi"], ord=2, rand_init=True, seed=5)
    noise = BR.project_noise(R.rand_noise(len(x), x[0].size, c["eps"], 5), c["eps"]).reshape(x.shape)
    np.testing.assert_allclose(x0, np.clip(x + noise, c["lo"], c["hi"]), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------- 5. ord = inf is today's call
def test_ord_inf_returns_the_bits_of_a_call_without_ord(models):
    m, c = models["E"], CASES["E"]
    x, y, _, _ = _case("E")
    kw = dict(eps=0.3, eps_iter=0.05, nb_iter=3, clip_min=0.0, clip_max=1.0, rand_init=True, seed=3, return_info=True)
    a = nb.ProjectedGradientDescent(m).generate(x, y, **kw)
    b = nb.ProjectedGradientDescent(m).generate(x, y, ord=np.inf, **kw)
    assert len(a) == len(b) == 2 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    f = nb.FastGradientMethod(m)
    assert f.generate(x, eps=0.3, clip_min=0.0, clip_max=1.0).tobytes() == f.generate(x, eps=0.3, ord="inf", clip_min=0.0, clip_max=1.0).tobytes()
    l2 = nb.ProjectedGradientDescent(m).generate(x, y, ord=2, **kw)
    assert len(l2) == 3 and not np.array_equal(l2[0], a[0])


# ---------------------------------------------------------------------- 6. BPDA ord 2
C = R.CASE


@pytest.fixture(scope="module")
def defended():
    """tests/test_gpu_bpda.py's case: the synthetic MNIST generator at gain 2.0, rec_rr 2, rec_iters 5, classifier F (no USE_BN)."""
    import torch
    p, x, y, model, cp = R.case_inputs()
    gan, _ = make_gan(C["arch"], wseed=C["wseed"], gain=C["gain"], bias_range=C["bias_range"], rec_rr=C["R"], rec_iters=C["L"], rec_lr=C["lr"])
    model.set_weights(cp)
    model.add_rec_model(gan, None, 50)
    yield dict(x=x, y=y, model=model, gan=gan, layers=R.layers_of(model), p64=[(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in cp])
    torch.cuda.synchronize()
    model.close()
    gan.close()


BKW = dict(eps=2.0, eps_iter=0.75, clip_min=C["lo"], clip_max=C["hi"], ord=2)


@pytest.mark.parametrize("m_eot", [1, 3])
def test_bpda_l2_step_teacher_forced_on_the_device_reconstructions(defended, m_eot):
    """One iteration from x_0: the float64 gradients at the device's own reconstructions (seeds seed .. seed + m - 1), summed in
    order, through the float64 L2 step.  The end-to-end bound; with m = 3 the step goes through gsum."""
    from oracle import classifier_oracle as CO
    x, y, gan, model = defended["x"], defended["y"], defended["gan"], defended["model"]
    x0 = np.clip(x, C["lo"], C["hi"])
    recs = [gan.reconstruct(x0, seed=C["seed"] + s, first_row=0) for s in range(m_eot)]
    recs = [r if isinstance(r, np.ndarray) else r.cpu().numpy() for r in recs]
    grads = [CO.input_gradient(defended["layers"], defended["p64"], r.astype(np.float64), y) for r in recs]
    g = R.eot_sum(grads)
    info = {}
    ref = BR.l2_step(x, x0, g, BKW["eps"], BKW["eps_iter"], C["lo"], C["hi"], info=info)
    assert np.array_equal(x0, x) and not info["projected"].any()          # grad_term's case: the step from x itself, inside the ball
    adv, first, dist = nb.BPDA(model).generate(x, y, nb_iter=1, eot_samples=m_eot, seed=C["seed"], return_info=True, **BKW)
    E = BETA * sum(np.abs(gs).max() for gs in grads)
    _within_rows("BPDA ord 2, m %d" % m_eot, adv, ref, grad_term(g, BKW["eps_iter"], 2, E) + step_bound(784) * np.abs(ref).max())
    assert np.abs(adv - x0).max() > 0.01 and dist.max() <= BKW["eps_iter"] * (1 + step_bound(784)) and len(first) == len(x)
    # the device's own float32 gradients through the restatement: the teacher-forced bound
    g32 = [model.input_gradient(r, labels=y, no_rec=True) for r in recs]
    t = g32[0]
    for gi in g32[1:]:
        t = t + gi                                                                  # float32, dg_bpda_step's order
    ref32 = BR.l2_step(x, x0, t, BKW["eps"], BKW["eps_iter"], C["lo"], C["hi"])
    _within("BPDA ord 2, m %d, device gradients" % m_eot, adv, ref32, step_bound(784), np.abs(ref32).max())


def test_bpda_l2_is_independent_of_batch_size_and_ord_inf_is_todays_call(defended, monkeypatch):
    monkeypatch.setattr(gan_defense, "COALESCE_ROWS", 1)          # one caller batch per engine call: batch_size really cuts
    x, y, atk = defended["x"], defended["y"], nb.BPDA(defended["model"])
    kw = dict(BKW, nb_iter=2, eot_samples=2, seed=C["seed"], rand_init=True, return_info=True)
    runs = [atk.generate(x, y, batch_size=bs, **kw) for bs in (2, 7, 50, 7)]
    for r in runs[1:]:
        assert len(r) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0]))
    adv, _, dist = runs[0]
    assert adv.min() >= C["lo"] and adv.max() <= C["hi"] and dist.max() <= BKW["eps"] * (1 + step_bound(784)) and dist.min() > 0
    np.testing.assert_allclose(dist, BR.row_norms(adv, 2, x), rtol=norm_bound(784))
    kw = dict(eps=C["eps"], eps_iter=C["eps_iter"], clip_min=C["lo"], clip_max=C["hi"], nb_iter=2, seed=C["seed"], return_info=True)
    a, b = atk.generate(x, y, **kw), atk.generate(x, y, ord=np.inf, **kw)
    assert len(a) == len(b) == 2 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------------- 7. whitebox() and the C entries
def test_whitebox_pgd_with_attack_ord_2_at_toy_sizes(tmp_path):
    """whitebox(attack_type='pgd', attack_ord=2) on model E, one epoch on 512 images of a separable set: the accuracy it returns is
    that of ProjectedGradientDescent(ord=2) called by hand on the trained model, and the L2 attack is not the L-infinity one."""
    import argparse
    from tests.test_gpu_train import _synthetic
    xtr, ytr = _synthetic(512, seed=1)
    xte, yte = _synthetic(64, seed=2)
    model = nb.model_e()
    kw = dict(batch_size=64, nb_epochs=1, eps=2.0, attack_type="pgd", attack_params={"eps_iter": 0.75, "nb_iter": 4})
    acc, zero, roc = wb.whitebox(None, model, (xtr, ytr, xte, yte), attack_ord=2, **kw)
    adv, first, dist = nb.ProjectedGradientDescent(model).generate(xte, yte, eps=2.0, eps_iter=0.75, nb_iter=4, clip_min=0.0, clip_max=1.0,
                                                                   seed=wb.SEED, ord=2, return_info=True)
    correct, _, _ = model.eval_batch(adv, labels=yte)
    clean, _, _ = model.eval_batch(xte, labels=yte)
    print("model E: clean accuracy %.3f, under PGD-L2(eps 2) %.3f; largest dist %.4f" % (clean / 64.0, acc, dist.max()))
    assert zero == 0 and roc is None and acc == correct / 64.0
    assert dist.max() <= 2.0 * (1 + step_bound(784)) and dist.max() > 0.1
    inf = nb.ProjectedGradientDescent(model).generate(xte, yte, eps=2.0, eps_iter=0.75, nb_iter=4, clip_min=0.0, clip_max=1.0, seed=wb.SEED)
    assert not np.array_equal(inf, adv)
    flags = argparse.Namespace(defense_type="none", attack_type="pgd", attack_ord="2", dataset_name="mnist", rec_path=None, train_on_recs=False,
                               num_tests=-1, num_train=-1, model="E", fgsm_eps_tr=0.15)
    results_dir, fname = wb.get_results_dir_filename(flags, None)
    path = wb.result_path(os.path.join(str(tmp_path), results_dir), fname, "run")
    wb.write_results(path, (acc, zero, roc))
    assert os.path.basename(path) == "0_model=E_nodefense_attack=pgd_ord=2.txt" and open(path).read() == str(acc) + " 0 \n"
    model.close()


def test_entry_argument_errors(models):
    import torch
    lib, h = _native.load(), models["G1"]._handle
    buf, out = torch.zeros(3 * 378, device="cuda"), torch.zeros(3 * 378, device="cuda")
    lab = torch.zeros(3, dtype=torch.int32, device="cuda")
    p, q, l = buf.data_ptr(), out.data_ptr(), lab.data_ptr()
    for ord, text in ((1, b"needs a sort"), (0, b"ord must be 2")):
        assert lib.dg_pgd_ball(h, p, p, l, 3, 0.3, 0.05, 1, ord, 0.0, 1.0, q, l, None) == -1 and text in lib.dg_last_error()
        assert lib.dg_bpda_step_ball(h, p, l, 3, p, p, None, 0, 0.3, 0.05, ord, 0.0, 1.0, q, None) == -1 and text in lib.dg_last_error()
    for args, text in (((0.3, 0.05, 0, 0.0, 1.0, q), b"dg_pgd_ball: nb_iter"), ((-0.3, 0.05, 1, 0.0, 1.0, q), b"dg_pgd_ball: eps"),
                       ((0.3, 0.05, 1, 1.0, 0.0, q), b"clip_min"), ((0.3, 0.05, 1, 0.0, 1.0, p), b"x_adv must not be")):
        eps, eps_iter, nb_iter, lo, hi, dst = args
        assert lib.dg_pgd_ball(h, p, p, l, 3, eps, eps_iter, nb_iter, 2, lo, hi, dst, l, None) == -1 and text in lib.dg_last_error()
    assert lib.dg_bpda_step_ball(h, p, l, 3, None, None, None, 1, 0.3, 0.05, 2, 0.0, 1.0, None, None) == -1       # accumulate_only: no gsum
    assert lib.dg_bpda_step_ball(h, p, l, 3, p, p, None, 0, 0.3, 0.05, 2, 0.0, 1.0, None, None) == -1             # no x_next
    for ord in (0, 3):
        assert lib.dg_fgm(h, p, None, 3, 0.3, ord, 0.0, 1.0, q, None) == -1 and b"dg_fgm: ord" in lib.dg_last_error()
        assert lib.dg_row_norms(p, None, 3, 378, ord, q, None) == -1 and b"dg_row_norms: ord" in lib.dg_last_error()
    assert lib.dg_fgm(None, p, None, 3, 0.3, 2, 0.0, 1.0, q, None) == -1
    assert lib.dg_row_norms(p, None, 0, 378, 2, q, None) == -1 and lib.dg_row_norms(p, None, 3, 0, 2, q, None) == -1
    assert lib.dg_row_norms(None, None, 3, 378, 2, q, None) == -1
