"""-m gpu: the strided loops of the classifier's attack and evaluation kernels, where no other test takes them.

1. Wide class counts.  jac_seed_kernel (dg_jacobian.hip) and pgd_track_kernel (dg_pgd.hip) stride the classes over a wave's 64 lanes
   and reduce with a butterfly; clf_softmax_kernel, clf_ce_grad_kernel, clf_eval_kernel, tr_ce_kernel and cw_head_kernel loop over them
   in one thread.  n in {2, 63, 64, 65, 130} classes and B in {1, 5, 67} images (67: more than one 64-row block of the kernels with one
   thread per row), the two tiny models of tests/support/strided_cases.py, against float64 -- the oracle's forward and input
   gradient, blackbox_reference.class_gradient, pgd_reference, cw_reference, train_reference.
2. Batches longer than a grid cap, bit for bit.  dg_bpda_track caps its grid at 1024 workgroups, pgd_track_kernel at 4096 workgroups
   of 4 images, the row kernels of dg_ball.hip at 65536 (strided_cases.*_CAP, read from the launchers): B = 2 * 1024 + 3, 16384 + 5
   and 65536 + 5 take the loop-back, the first twice.
3. NaN logits.  pgd_track_kernel answers what clf_eval_kernel (dg_eval_batch) answers on the same row: a NaN is never the maximum
   unless it sits at class 0, where it always is.

Tolerances are the project's own: probabilities 2e-6 absolute (tests/test_classifier.py), input and class gradients rtol 1e-5 and
atol 1e-5 of the reference's largest element (tests/test_gpu_blackbox.py), PGD steps 1e-6 on the decided pixels (tests/test_gpu_pgd.py),
Carlini-Wagner the gates of tests/test_gpu_cw_edges.py, training 1e-5 relative on the loss and 1e-4 of a gradient tensor's largest
element (tests/test_gpu_train_shapes.py), the L1 / L2 steps the per-image bound tests/test_gpu_ball.py derives.  No tolerance here
was measured: the spread-logit check (1c) prints, next to the device's error, the error of the float32 restatement
strided_cases.class_gradient32 against the same float64 reference, and both stay inside the project's tolerance (see its docstring).
Each test prints the figure it is about to assert (pytest -s shows them).

Measured on an MI355X, the worst case over the file: probabilities 9.2e-8, input gradients 5.5e-7 and class gradients 4.6e-7 of the
reference's largest element (spread: 3.8e-6), the Jacobian's class sum 1.7e-6 of its largest element, the ball steps 0.4 % of their bound.

Throw-away mutations, each built into a scratch copy of the library and run on an MI355X against this file (108 tests) and the older
file of the kernel it touches, where nothing failed:
  jac_seed_kernel's sum loop makes one trip (break)    24 fail: class_gradient_and_jacobian and class_gradient_on_spread_logits at n = 65
                                                       and 130 (all); tests/test_gpu_blackbox.py passes
  bpda_track_kernel without its loop-back              2 fail: bpda_track_on_a_batch_of_two_grids_and_three (both); tests/test_gpu_bpda.py passes
  pgd_track_kernel as it was before the NaN rule       2 fail: nan_logits "n4 NaN at 1, maximum at 3" and "n70 NaN at 5, maximum at 69";
                                                       tests/test_gpu_pgd.py passes
"""
import numpy as np
import pytest

from defensegan_amd import _native
from defensegan_amd import network_builder as nb
from oracle import classifier_oracle as CO
from tests.support import ball_reference as BALL
from tests.support import blackbox_reference as BR
from tests.support import bpda_reference as R
from tests.support import cw_cases as K
from tests.support import cw_reference as CW
from tests.support import strided_cases as S
from tests.support import train_reference as TR

pytestmark = pytest.mark.gpu

WIDE = 130
SEED = 11241990


_OPEN = {}


def _model(kind, n, spread=False):
    """The case's model on the device, made once per module run and closed by the ``models`` fixture."""
    if (kind, n, spread) not in _OPEN:
        m = S.model(kind, n)
        m.set_weights(S.case(kind, n, spread)["params"])
        _OPEN[(kind, n, spread)] = m
    return _OPEN[(kind, n, spread)]


@pytest.fixture(scope="module", autouse=True)
def models():
    import torch
    yield
    torch.cuda.synchronize()
    for m in _OPEN.values():
        m.close()
    _OPEN.clear()


def _close_to(what, got, ref):
    """The project's gradient tolerance: rtol 1e-5, atol 1e-5 of the reference's largest element."""
    scale = float(np.abs(ref).max())
    assert scale > 0
    err = float(np.abs(got - ref).max())
    print("%s: max|dev - f64| = %.3g = %.3g of max|f64| (%.3g)" % (what, err, err / scale, scale))
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * scale, err_msg=what)
    return err


GRID = [(kind, n, B) for kind in S.KINDS for n in S.WIDTHS for B in S.BATCHES]


# ---------------------------------------------------------------------- 1a. forward, prediction, input gradient
@pytest.mark.parametrize("kind,n,B", GRID)
def test_forward_prediction_and_input_gradient_match_float64(kind, n, B):
    """clf_softmax_kernel, clf_eval_kernel and clf_ce_grad_kernel (labels given, and the model's own first arg-max) at n classes."""
    c, m = S.case(kind, n), _model(kind, n)
    x, y = c["x"][:B], c["y"][:B]
    z64, p64 = CO.forward(c["layers"], c["p64"], x.astype(np.float64))
    probs = m.get_probs(x)
    err = np.abs(probs - p64).max()
    print("%s n %d B %d: max|probs - f64| = %.3g (2e-6), |sum - 1| = %.3g" % (kind, n, B, err, np.abs(probs.sum(axis=1) - 1).max()))
    assert probs.shape == (B, n) and np.isfinite(probs).all()
    np.testing.assert_allclose(probs, p64, rtol=0, atol=2e-6)
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, atol=1e-6)
    want = z64.argmax(axis=1)
    correct, preds, _ = m.eval_batch(x, None, want)
    assert preds.cpu().numpy().tolist() == want.tolist() and correct == B
    assert m.eval_batch(x, None, y)[0] == int((want == y).sum())
    for labels in (y, None):
        g = m.input_gradient(x, labels=labels)
        ref = CO.input_gradient(c["layers"], c["p64"], x.astype(np.float64), labels)
        _close_to("%s n %d B %d input gradient, labels %s" % (kind, n, B, "given" if labels is not None else "own"), g, ref)


# ---------------------------------------------------------------------- 1b. class gradient and Jacobian
@pytest.mark.parametrize("kind,n,B", GRID)
def test_class_gradient_and_jacobian_match_float64(kind, n, B):
    """jac_seed_kernel at n classes: both seeds against blackbox_reference.class_gradient, every slice of the Jacobian bitwise the
    class gradient of its class, the probabilities' slices summing to zero within tests/test_gpu_blackbox.py's bound."""
    c, m = S.case(kind, n), _model(kind, n)
    x = c["x"][:B]
    classes = np.random.RandomState(n + B).randint(0, n, B)
    classes[0] = n - 1                                              # the last class: the last lane trip's last lane
    for of_probs in (True, False):
        g = m.class_gradient(x, classes, of_probs=of_probs)
        ref = BR.class_gradient(c["layers"], c["p64"], x, classes, of_probs=of_probs)
        _close_to("%s n %d B %d class gradient of_probs=%d" % (kind, n, B, of_probs), g, ref)
        jac = m.jacobian(x, of_probs=of_probs)
        assert jac.shape == (B, n) + x.shape[1:]
        for k in range(n):
            np.testing.assert_array_equal(jac[:, k], m.class_gradient(x, np.full(B, k), of_probs=of_probs), err_msg="class %d" % k)
        if of_probs:
            jp = jac.astype(np.float64)
            total = np.abs(jp.sum(axis=1)).max()
            print("%s n %d B %d: |sum over classes of the Jacobian| = %.3g of its largest element" % (kind, n, B, total / np.abs(jp).max()))
            assert total <= 1e-4 * np.abs(jp).max()


# ---------------------------------------------------------------------- 1c. spread logits
@pytest.mark.parametrize("kind,n,B", GRID)
def test_class_gradient_on_spread_logits(kind, n, B):
    """The last Linear layer scaled until a row's logits span about 30: the mass sits on a few classes, p_c has not rounded to 1, and
    the butterfly's maximum and sum decide the value (with the weights as drawn every probability is near 1 / n).  The class is in
    the second lane trip (c >= 64) for n = 65 and 130; image 0 of those has its largest logit at class 64.  The project's tolerance.
    Device classes outside [0, n) give exact zeros.

    Measured on an MI355X over the 30 cases: the device within 3.8e-6 of the reference's largest element at worst (lin, n = 2, B = 1,
    where 1 - p_c = 3e-3 is formed by cancellation), the float32 restatement (strided_cases.class_gradient32, every sum in the kernels'
    order) within 3.8e-6 as well: the project's 1e-5 holds and nothing wider was needed."""
    import torch
    c, m = S.case(kind, n, True), _model(kind, n, True)
    x, z = c["x"][:B], c["z"][:B]
    classes = S.spread_classes(c["z"])[:B]
    assert n <= 64 or (classes >= 64).all()
    g = m.class_gradient(x, classes, of_probs=True)
    ref = BR.class_gradient(c["layers"], c["p64"], x, classes, of_probs=True)
    g32 = S.class_gradient32(kind, c["params"], x, classes)
    scale = np.abs(ref).max()
    print("%s n %d B %d spread: logit range %.3g .. %.3g, largest p_c %.6f; float32 restatement within %.3g of max|f64|" %
          (kind, n, B, (z.max(axis=1) - z.min(axis=1)).min(), (z.max(axis=1) - z.min(axis=1)).max(),
           BR.softmax(z)[np.arange(B), classes].max(), np.abs(g32 - ref).max() / scale))
    assert np.abs(ref).reshape(B, -1).max(axis=1).min() > 0
    _close_to("%s n %d B %d spread class gradient" % (kind, n, B), g, ref)
    # the probabilities themselves, and the prediction, on the same spread logits
    np.testing.assert_allclose(m.get_probs(x), BR.softmax(z), rtol=0, atol=2e-6)
    assert m.eval_batch(x, None, None)[1].cpu().numpy().tolist() == z.argmax(axis=1).tolist()
    # a device class outside the range: an exactly zero gradient for that image, the others untouched
    bad = classes.copy()
    bad[0] = n
    if B > 1:
        bad[B - 1] = -1
    for of_probs in (True, False):
        full = m.class_gradient(x, classes, of_probs=of_probs)
        gb = m.class_gradient(torch.from_numpy(x).cuda(), torch.from_numpy(bad).cuda(), of_probs=of_probs).cpu().numpy()
        out = bad != classes
        assert (gb[out] == 0).all() and gb[~out].tobytes() == full[~out].tobytes()


# ---------------------------------------------------------------------- 1d. PGD and Carlini-Wagner at 130 classes
@pytest.mark.parametrize("B", S.BATCHES)
def test_pgd_step_and_first_success_at_130_classes(B):
    """pgd_track_kernel with three trips of its class loop.  One step teacher-forced from x_0 on the decided pixels
    (tests/test_gpu_pgd.py's rule and bound), then a four-iteration run whose first_success and result are those of dg_eval_batch on
    every iterate, rebuilt by chained one-iteration calls."""
    c, m = S.case("mlp", WIDE), _model("mlp", WIDE)
    x = c["x"][:B]
    own = c["z"][:B].argmax(axis=1).astype(np.int32)
    atk = nb.ProjectedGradientDescent(m)
    kw = dict(eps=0.3, eps_iter=0.05, clip_min=0.0, clip_max=1.0)
    g = CO.input_gradient(c["layers"], c["p64"], x.astype(np.float64), own)
    decided = np.abs(g) > 1e-4 * np.abs(g).max()
    adv = atk.generate(x, own, nb_iter=1, **kw)
    d = np.abs(adv.astype(np.float64) - R.step_rule(x.astype(np.float64), x.astype(np.float64), g, 0.3, 0.05, 0.0, 1.0))
    print("B %d: undecided %.5f, max |dx| on decided pixels %.3e" % (B, 1 - decided.mean(), d[decided].max()))
    assert 1 - decided.mean() <= 0.01
    assert d[decided].max() <= 1e-6
    y = own.copy()
    y[0] = (y[0] + 1) % WIDE                                        # misclassified from the start
    if B > 2:
        y[B - 1] = WIDE                                             # no prediction equals a label outside the classes
    nb_iter = 4
    kw = dict(kw, eps_iter=0.01)
    adv, first = atk.generate(x, y, nb_iter=nb_iter, return_info=True, **kw)
    iterates, cur = [], None
    for _ in range(nb_iter):
        cur = atk.generate(x, y, nb_iter=1, x_init=cur, **kw)
        iterates.append(cur)
    preds = {j + 1: m.eval_batch(it, None, y)[1].cpu().numpy() for j, it in enumerate(iterates)}
    want_adv, want_first = R.track(preds, y, [np.clip(x, 0.0, 1.0)] + iterates)
    print("B %d: first_success %s" % (B, first.tolist()))
    assert first.tolist() == want_first.tolist() and first[0] == 1
    assert adv.tobytes() == want_adv.astype(np.float32).tobytes()
    assert B < 67 or len(set(first.tolist())) >= 3                  # the successes spread over the iterates, and some never come
    assert B < 67 or (np.concatenate([p for p in preds.values()]) >= 64).any()


@pytest.mark.parametrize("B", S.BATCHES)
def test_carlini_wagner_at_130_classes(B):
    """cw_head_kernel and first_argmax at 130 classes on the smallest schedule of tests/support/cw_cases.py (case b-i1: one outer
    step, one iteration) and on the next (b-i2, whose second iteration sees the first one's seed), against cw_reference.cw_l2 and
    through the gates of tests/test_gpu_cw_edges.py.  Even images carry the model's own label, odd images the runner-up, which
    succeeds at once and records the first arg-max."""
    from tests.test_gpu_cw_edges import _gates
    c, m = S.case("mlp", WIDE, True), _model("mlp", WIDE, True)
    x = c["x"][:B]
    labels = c["z"][:B].argmax(axis=1)
    labels[1::2] = np.argsort(c["z"][:B], axis=1)[1::2, -2]
    for name in ("b-i1", "b-i2"):
        kw = K.case(name)["kw"]
        ref = CW.cw_l2(c["layers"], c["p64"], x.astype(np.float64), labels=labels, targeted=False, trace=True, **kw)
        got = nb.CarliniWagnerL2(m).generate(np.array(x), y=labels, return_info=True, return_search=True, **kw)
        _gates("n 130 B %d %s" % (B, name), got, ref)
        if B > 1:
            assert (got[2][1::2] == c["z"][:B].argmax(axis=1)[1::2]).all() and (got[1][1::2] == 0).all()


# ---------------------------------------------------------------------- 1e. one training step at 130 classes
@pytest.mark.parametrize("B", S.BATCHES)
def test_one_training_step_at_130_classes(B):
    """tr_ce_kernel at 130 classes: dg_clf_param_gradient's loss and weight gradients against train_reference.param_gradient, and one
    dg_clf_train step whose loss is that loss bit for bit and whose weights are TF Adam's first step on those gradients
    (tests/test_gpu_train_shapes.py's tolerances: 1e-5, 1e-4 of a tensor's largest element, 1e-6 on the step).  One label is outside the classes
    when there is room: it contributes nothing."""
    from tests.test_gpu_train_shapes import _check_grads, _check_loss, _device_gradient, _train
    c = S.case("mlp", WIDE)
    m = S.model("mlp", WIDE)
    m.set_weights(c["params"])
    x, y = c["x"][:B], c["y"][:B].copy()
    y[0] = WIDE - 1
    loss, grads, _ = _device_gradient(m, x, y, step=0)
    rl, rg, _ = TR.param_gradient(c["layers"], c["params"], x, y, SEED, 0)
    what = "mlp n 130 B %d" % B
    _check_loss(loss, rl, what)
    _check_grads(grads, rg, what)
    before = m.get_weights()
    _native.check(_native.load().dg_clf_adam_reset(m._handle))
    got = _train(m, x, y, np.arange(B, dtype=np.int32), 1, B, 0.001)
    assert got[0] == np.float32(loss)
    for i, ((W, b), (W0, b0)) in enumerate(zip(m.get_weights(), before)):
        for k, (p, p0) in enumerate(((W, W0), (b, b0))):
            want = TR.adam_update(p0, grads[i][k], np.zeros_like(p0), np.zeros_like(p0), 1, 0.001, dtype=np.float32)[0]
            np.testing.assert_allclose(p, want, rtol=1e-6, atol=1e-6 * np.abs(want).max(), err_msg="layer %d %s" % (i, "Wb"[k]))
            assert np.abs(p - p0).max() > 0
    if B > 1:
        y[1] = WIDE                                                 # outside the classes: the mean keeps its divisor B
        loss2, grads2, _ = _device_gradient(m, x, y, step=0)
        ylab = np.where(y >= WIDE, -1, y)
        rl2, rg2, _ = TR.param_gradient(c["layers"], m.get_weights(), x, ylab, SEED, 0)
        _check_loss(loss2, rl2, what + " with a label outside the classes")
        _check_grads(grads2, rg2, what + " with a label outside the classes")
    m.close()


# ---------------------------------------------------------------------- 2a. dg_bpda_track beyond its grid cap
@pytest.mark.parametrize("row_elems", [5, 300])
def test_bpda_track_on_a_batch_of_two_grids_and_three(row_elems):
    """B = 2 * 1024 + 3 through the C ABI: every workgroup takes its loop twice, three of them a third time, with the barrier and
    the ``continue`` of an image that has succeeded in between.  Rows of 5 and 300 elements (fewer and more than the workgroup's 256
    threads).  Three calls, k = 1, 2, 3, on prescribed predictions (strided_cases.track_case: every pattern below the cap, in the
    second pass and among the last three); x_best and first_success are bpda_reference.track's, as bytes."""
    import torch
    B = 2 * S.BPDA_TRACK_CAP + 3
    labels, preds, iterates, want_first = S.track_case(B, row_elems)
    want_adv, ref_first = R.track(preds, labels, iterates)
    assert ref_first.tolist() == want_first.tolist()
    lib = _native.load()
    dev = lambda a: torch.from_numpy(a).cuda()
    lab = dev(labels)
    x_best = torch.full((B, row_elems), float("nan"), device="cuda")
    first = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for k in (1, 2, 3):
        p, it = dev(preds[k]), dev(iterates[k])
        _native.check(lib.dg_bpda_track(p.data_ptr(), lab.data_ptr(), B, k, it.data_ptr(), x_best.data_ptr(), first.data_ptr(), row_elems, stream))
        torch.cuda.synchronize()
    got_first, got_best = first.cpu().numpy(), x_best.cpu().numpy()
    wrong = np.flatnonzero(got_first != want_first)
    print("row_elems %d: %d of %d first_success differ (first at %s); rows of x_best that differ: %d" %
          (row_elems, len(wrong), B, wrong[:3].tolist(), int((got_best != want_adv).any(axis=1).sum())))
    assert got_first.tobytes() == want_first.tobytes()
    assert got_best.tobytes() == want_adv.astype(np.float32).tobytes()
    for lo, hi in ((0, S.BPDA_TRACK_CAP), (S.BPDA_TRACK_CAP, 2 * S.BPDA_TRACK_CAP), (B - 3, B)):
        assert hi - lo == 3 or set(want_first[lo:hi].tolist()) == {-1, 1, 2, 3}
    assert set(want_first[B - 3:].tolist()) == {1, 2}               # patterns 3, 4, 0: undone, undone, kept


# ---------------------------------------------------------------------- 2b. dg_pgd beyond pgd_track_kernel's grid cap
def test_pgd_on_a_batch_longer_than_the_track_grid():
    """B = 4096 * 4 + 5 on a 2 x 2 x 1 input with Linear(3), two iterations: the call is bitwise the call in chunks of 4096 (the
    kernel file's batch independence), first_success is dg_eval_batch's verdict on every iterate, and successes (and images without
    one) fall into both passes of the grid loop."""
    B = S.PGD_TRACK_CAP + 5
    m = S.model("lin", 3, shape=(2, 2, 1))
    m.set_weights(R.init_params(m, 3))
    rs = np.random.RandomState(22)
    x = rs.uniform(0, 1, (B, 2, 2, 1)).astype(np.float32)
    own = m.eval_batch(x, None, None)[1].cpu().numpy()
    y = own.copy()
    y[::3] = (y[::3] + 1) % 3                                       # every third image is misclassified from the start
    y[B - 2] = own[B - 2]
    atk = nb.ProjectedGradientDescent(m)
    kw = dict(eps=0.3, eps_iter=0.02, clip_min=0.0, clip_max=1.0)   # small steps: most images with their own label never succeed
    adv, first = atk.generate(x, y, nb_iter=2, return_info=True, **kw)
    adv_c, first_c = atk.generate(x, y, nb_iter=2, batch_size=4096, return_info=True, **kw)
    assert adv.tobytes() == adv_c.tobytes() and first.tobytes() == first_c.tobytes()
    iterates, cur = [], None
    for _ in range(2):
        cur = atk.generate(x, y, nb_iter=1, x_init=cur, **kw)
        iterates.append(cur)
    preds = {j + 1: m.eval_batch(it, None, y)[1].cpu().numpy() for j, it in enumerate(iterates)}
    want_adv, want_first = R.track(preds, y, [np.clip(x, 0.0, 1.0)] + iterates)
    counts = [{v: int((first[a:b] == v).sum()) for v in (-1, 1, 2)} for a, b in ((0, S.PGD_TRACK_CAP), (S.PGD_TRACK_CAP, B))]
    print("B %d: first_success counts in the first pass %s, in the second %s" % (B, counts[0], counts[1]))
    assert first.tobytes() == want_first.tobytes()
    assert adv.tobytes() == want_adv.astype(np.float32).tobytes()
    assert all(cnt[1] > 0 and cnt[-1] + cnt[2] > 0 for cnt in counts) and counts[0][2] > 0 and counts[0][-1] > 0
    m.close()


# ---------------------------------------------------------------------- 2c. the row kernels of dg_ball.hip beyond their grid cap
def test_ball_kernels_on_a_batch_longer_than_their_grid():
    """B = 65536 + 5 rows of 12 elements: dg_fgm with ord 1 and 2 and one dg_pgd_ball step are bitwise the same call in chunks of
    16384, and five rows -- the first, one inside, the last of the first pass, the first of the second and the last -- match the
    float64 restatement of tests/support/ball_reference.py within the per-image end-to-end bound of tests/test_gpu_ball.py."""
    import torch
    from tests.test_gpu_ball import BETA, _within_rows, grad_term, step_bound
    B, chunk = S.BALL_CAP + 5, 16384
    m = S.model("lin", 3, shape=(3, 4, 1))
    params = R.init_params(m, 12)
    m.set_weights(params)
    layers, p64 = TR.describe(m), S.as64(params)
    rs = np.random.RandomState(12)
    x = rs.uniform(0, 1, (B, 3, 4, 1)).astype(np.float32)
    y = rs.randint(0, 3, B).astype(np.int32)
    rows = np.array([0, 30000, S.BALL_CAP - 1, S.BALL_CAP, B - 1])
    g = CO.input_gradient(layers, p64, x[rows].astype(np.float64), y[rows])
    E = BETA * np.abs(g).max()
    xt = torch.from_numpy(x).cuda()
    fgm = nb.FastGradientMethod(m)
    for ord, eps in ((1, 3.0), (2, 0.75)):
        whole = fgm.generate(xt, eps=eps, ord=ord, y=y).cpu().numpy()
        parts = [fgm.generate(xt[a:a + chunk], eps=eps, ord=ord, y=y[a:a + chunk]).cpu().numpy() for a in range(0, B, chunk)]
        assert whole.tobytes() == np.concatenate(parts).tobytes() and np.isfinite(whole).all()
        ref = BALL.fgm(x[rows], g, eps, ord, -np.inf, np.inf)
        _within_rows("B %d FGM ord %d, rows %s" % (B, ord, rows.tolist()), whole[rows], ref, grad_term(g, eps, ord, E) + step_bound(12) * np.abs(ref).max())
        assert np.abs(whole - x).reshape(B, -1).max(axis=1).min() > 0
    kw = dict(eps=0.75, eps_iter=0.25, clip_min=0.0, clip_max=1.0, ord=2)
    atk = nb.ProjectedGradientDescent(m)
    whole = atk.generate(x, y, nb_iter=1, **kw)
    assert whole.tobytes() == atk.generate(x, y, nb_iter=1, batch_size=chunk, **kw).tobytes()
    info = {}
    ref = BALL.l2_step(x[rows], x[rows], g, 0.75, 0.25, 0.0, 1.0, info=info)
    assert not info["projected"].any()                              # the first step from x stays inside the ball: grad_term's case
    _within_rows("B %d first L2 step, rows %s" % (B, rows.tolist()), whole[rows], ref, grad_term(g, 0.25, 2, E) + step_bound(12) * np.abs(ref).max())
    assert np.abs(whole - x).reshape(B, -1).max(axis=1).min() > 0
    m.close()


# ---------------------------------------------------------------------- 3. NaN logits: one arg-max rule
NAN_CASES = {
    "n4 NaN at 1, maximum at 3": (4, {0: 0.0, 1: np.nan, 2: 1.0, 3: 5.0}, 3),
    "n4 NaN at 0": (4, {0: np.nan, 1: 0.0, 2: 1.0, 3: 5.0}, 0),
    "n70 NaN at 5, maximum at 69": (70, {5: np.nan, 20: 0.5, 69: 1.0}, 69),
    "n70 NaN at 6, maximum at 7": (70, {6: np.nan, 20: 0.5, 7: 1.0}, 7),
    "n70 NaNs only": (70, {k: np.nan for k in range(70)}, 0),
}


@pytest.mark.parametrize("name", sorted(NAN_CASES))
def test_nan_logits_pgd_tracks_what_dg_eval_batch_predicts(name):
    """Flatten, Linear(n) with zero weights: the logits are the bias.  clf_eval_kernel's scan (best = 0; s[k] > s[best] moves it) never
    picks a NaN unless it is class 0, which then never yields.  dg_pgd's first_success, with a label equal to each candidate class in
    turn, is what dg_eval_batch says of every iterate.  (Before the fix of pgd_track_kernel a lane whose first class was a NaN kept
    it through the butterfly and lost its partners' values: "n4 NaN at 1" answered class 2, "n70 NaN at 5" class 20.)"""
    n, entries, want = NAN_CASES[name]
    m = nb.MLP([nb.Flatten(), nb.Linear(n)], input_shape=(None, 3, 3, 1))
    b = np.zeros(n, np.float32)
    for k, v in entries.items():
        b[k] = v
    m.set_weights([(np.zeros((9, n), np.float32), b)])
    labels = np.array(sorted(set(entries) | {0, want})[:8] + [want], np.int32)
    x = np.random.RandomState(0).uniform(0, 1, (len(labels), 3, 3, 1)).astype(np.float32)
    assert m.eval_batch(x, None, None)[1].cpu().numpy().tolist() == [want] * len(labels)
    atk = nb.ProjectedGradientDescent(m)
    kw = dict(eps=0.3, eps_iter=0.05, clip_min=0.0, clip_max=1.0)
    adv, first = atk.generate(x, labels, nb_iter=2, return_info=True, **kw)
    iterates, cur = [], None
    for _ in range(2):
        cur = atk.generate(x, labels, nb_iter=1, x_init=cur, **kw)
        iterates.append(cur)
    preds = {j + 1: m.eval_batch(it, None, labels)[1].cpu().numpy() for j, it in enumerate(iterates)}
    want_adv, want_first = R.track(preds, labels, [np.clip(x, 0.0, 1.0)] + iterates)
    print("%s: labels %s, dg_eval_batch predicts %s, first_success %s" % (name, labels.tolist(), preds[1].tolist(), first.tolist()))
    assert first.tolist() == want_first.tolist() == [-1 if l == want else 1 for l in labels]
    assert adv.tobytes() == want_adv.astype(np.float32).tobytes()
    m.close()
