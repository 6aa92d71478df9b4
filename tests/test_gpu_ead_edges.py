"""-m gpu: the parts of dg_ead.hip that tests/test_gpu_ead.py does not execute -- a nonzero confidence in both hinge kernels and in the
success rule (untargeted with labels 0 and not 0, targeted; with the abort check on, where alone the iterate's hinge counts), a
chunk of more than 256 images (ead_chunk_kernel's second trip), the abort check on every iteration, untargeted labels from the caller, labels outside the classes, no outer step at all, beta = 0 and a
two-class model.  The inputs are EDGE_CASES of tests/support/ead_reference.py, each through find_seed (tests/test_ead_cpu.py re-derives
the seeds, tests/test_ead_edges_cpu.py asserts what each case is named for).  The bounds are tests/test_gpu_ead.py's ``_check``, with
constants and stop iterations exact; every test prints how much of each bound it used."""
import numpy as np
import pytest

from defensegan_amd import _native, network_builder as nb
from tests.support import ead_reference as E
from tests.test_gpu_ead import DIST_RTOL, PIXEL_SHARE, PIXEL_TOL, _check, _reference

pytestmark = pytest.mark.gpu


def _model(name):
    m = E.case_mlp(E.CASES[name])
    m.set_weights(E.case_model(name)[1])
    return m


def _run(name, **more):
    """The case through the front end with return_search: (adv, dist, cls, const, stop)."""
    c = E.CASES[name]
    x, labels, _ = _reference(name)
    lab = {} if labels is None else ({"y_target": labels} if c.get("targeted") else {"y": labels})
    m = _model(name)
    out = nb.ElasticNetMethod(m).generate(x, return_info=True, return_search=True, **lab, **dict(c["kw"], **more))
    m.close()
    return out


def _stops(ref):
    return [[-1 if s is None else s for s in step] for step in ref["abort_iters"]]


@pytest.mark.parametrize("name", ["kappa_F", "kappa_targeted_F"])
def test_confidence(name):
    """kappa in the slack's hinge (the seed) and in the success rule Z'_t = Z_t +- kappa, on both sides of the rule's t == 0 branch: a
    wrong sign in either moves best_dist by far more than rtol 1e-3, as dropping kappa does on the reference
    (tests/test_ead_edges_cpu.py).  abort_early is off here, so kappa in the ITERATE's hinge (loss1_X) reaches nothing these two cases
    return: that use is test_confidence_reaches_the_abort_check's."""
    adv, dist, cls, const, _ = _run(name)
    ref = _check(name, adv, dist, cls)
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    if name == "kappa_F":
        assert (ref["labels"] == 0).any() and (ref["labels"] != 0).any()
    zero = _run(name, confidence=0.0)
    moved = np.abs(dist - zero[1]) / zero[1]
    print("%s: against confidence 0 on the device best_dist moves by up to %.3f relative" % (name, moved.max()))
    assert moved.max() > 1e-3                                       # and the device's own confidence 0 is another result


def test_confidence_reaches_the_abort_check():
    """kappa_abort_F: loss1_X = const max(0, real - oth + kappa) enters the chunk's L, and L decides where a chunk stops.  On the
    reference the stops move when kappa is dropped or negated there alone (tests/test_ead_edges_cpu.py); here they are held exact,
    then the rest to ``_check``."""
    name = "kappa_abort_F"
    adv, dist, cls, const, stop = _run(name)
    ref = _reference(name)[2]
    print("kappa_abort_F: stops %s (reference %s)" % (stop.tolist(), _stops(ref)))
    assert stop.tolist() == _stops(ref) and min(stop.tolist()[0]) >= 1
    _check(name, adv, dist, cls)
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    assert (cls == -1).any() and (cls != -1).any()


def test_a_chunk_of_more_than_256_images():
    name = "huge_chunk_tiny"
    adv, dist, cls, const, stop = _run(name)
    x, _, ref = _reference(name)
    assert stop.tolist() == _stops(ref)
    _check(name, adv, dist, cls)
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    assert (cls[256:272] != -1).any()                               # the images of the chunk kernel's second trip are tracked
    ok = cls != -1
    assert adv[~ok].tobytes() == np.clip(x[~ok], 0, 1).tobytes()


def test_the_abort_check_on_every_iteration():
    name = "abort_every_F"
    adv, dist, cls, const, stop = _run(name)
    ref = _reference(name)[2]
    print("abort_every_F: stops %s (reference %s)" % (stop.tolist(), _stops(ref)))
    assert stop.tolist() == _stops(ref) and max(stop.tolist()[0]) >= 1
    _check(name, adv, dist, cls)
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)


def test_untargeted_labels_from_the_caller():
    """An image whose given label is not the model's prediction succeeds on the first iterate without moving: its hinge is off, g = 0,
    X' = x0 and best_dist is exactly 0, on the reference and on the device.  ``_check`` divides by the reference's best_dist, so those
    images are held to the exact result here and the others to ``_check``'s bounds."""
    name = "given_y_F"
    x, labels, ref = _reference(name)
    adv, dist, cls, const, _ = _run(name)
    np.testing.assert_array_equal(cls, ref["best_class"])
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    zero = ref["best_dist"] == 0
    assert zero.mean() >= 0.25 and (~zero).mean() >= 0.25 and (ref["best_class"] != -1).all()
    assert (dist[zero] == 0).all() and adv[zero].tobytes() == np.clip(x[zero], 0, 1).tobytes()
    rel = np.abs(dist[~zero] - ref["best_dist"][~zero]) / ref["best_dist"][~zero]
    off = float((np.abs(adv - ref["x_adv"]) > PIXEL_TOL).mean())
    print("%s: %d images at distance 0 exactly; on the other %d best_dist uses %.4f of rtol %g; %.2e of the pixels differ by more than %g "
          "(%.3f of the %.0e allowed)" % (name, zero.sum(), (~zero).sum(), rel.max() / DIST_RTOL, DIST_RTOL, off, PIXEL_TOL,
                                          off / (1 - PIXEL_SHARE), 1 - PIXEL_SHARE))
    assert rel.max() <= DIST_RTOL and 1 - off >= PIXEL_SHARE
    m = _model(name)
    own = m.get_logits(x).argmax(axis=1)
    a2, d2, c2 = nb.ElasticNetMethod(m).generate(x, y=np.eye(10, dtype=np.float32)[labels], return_info=True, **E.CASES[name]["kw"])
    m.close()
    assert np.array_equal(own != labels, zero)                      # exactly the images the model already gets wrong
    assert a2.tobytes() == adv.tobytes() and d2.tobytes() == dist.tobytes() and c2.tobytes() == cls.tobytes()      # y one-hot: the same bits


def _c_call(m, x, labels, kw):
    """dg_ead through the C entry with int32 labels as given (the front end refuses labels outside the classes)."""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    B = len(x)
    lab = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).cuda()
    out, dist, cls = torch.empty_like(xt), torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    p = dict(nb.ElasticNetMethod.DEFAULTS, **kw)
    lib = _native.load()
    _native.check(lib.dg_ead(m._handle, xt.data_ptr(), lab.data_ptr(), B, 0, int(p["batch_size"]), float(p["confidence"]), float(p["beta"]),
                             0, 1 if p["fista"] else 0, float(p["learning_rate"]), int(p["binary_search_steps"]), int(p["max_iterations"]),
                             1 if p["abort_early"] else 0, float(p["initial_const"]), float(p["clip_min"]), float(p["clip_max"]),
                             out.data_ptr(), dist.data_ptr(), cls.data_ptr(), None, None, None), lib)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dist.cpu().numpy(), cls.cpu().numpy()


def test_labels_outside_the_classes_never_succeed_and_touch_nothing_else():
    """five_F (abort_early off) with its own labels, then with image 3's label -1 and image 7's label n.  Those two get a zero seed, so
    g = 2 (Y - x0) = 0 at X = Y = x0, S = x0, d = 0 and the shrinkage's middle branch returns x0: they stay at x0 with l1 = l2 = 0 and
    loss1 = 0, are never a success, and would add exactly 0 to the chunk's loss.  Nothing else couples the images of a chunk, so every
    other image is what the call with the valid labels returns, bit for bit."""
    name = "five_F"
    x, _, ref = _reference(name)
    kw = E.CASES[name]["kw"]
    assert not kw["abort_early"]
    m = _model(name)
    valid = ref["labels"].astype(np.int32)
    a0, d0, c0 = _c_call(m, x, valid, kw)
    _check(name, a0, d0, c0)                                        # labels given through the C entry: the case's own result
    bad = valid.copy()
    bad[3], bad[7] = -1, m.nb_classes
    a1, d1, c1 = _c_call(m, x, bad, kw)
    m.close()
    out = np.zeros(len(x), bool)
    out[[3, 7]] = True
    assert (c1[out] == -1).all() and (d1[out] == np.float32(1e10)).all()
    assert a1[out].tobytes() == np.clip(x[out], 0, 1).tobytes()
    assert (c0[out] != -1).all()                                    # with their valid labels the two images do succeed
    assert a1[~out].tobytes() == a0[~out].tobytes() and d1[~out].tobytes() == d0[~out].tobytes() and c1[~out].tobytes() == c0[~out].tobytes()


def test_no_outer_step_at_all():
    name = "five_F"
    x = _reference(name)[0].copy()
    x[0, :2] = -0.25                                                # something for the clip to do
    x[1, :2] = 1.5
    m = _model(name)
    adv, dist, cls, const, stop = nb.ElasticNetMethod(m).generate(x, return_info=True, return_search=True,
                                                                  **dict(E.CASES[name]["kw"], binary_search_steps=0, initial_const=7.5))
    m.close()
    assert adv.tobytes() == np.clip(x, 0, 1).tobytes()
    assert (dist == np.float32(1e10)).all() and (cls == -1).all()
    assert const.dtype == np.float64 and (const == 7.5).all()       # final_const is initial_const: no update without a step
    assert stop.shape == (0, 1)


def test_beta_zero():
    name = "beta0_F"
    adv, dist, cls, const, _ = _run(name)
    x, _, ref = _reference(name)
    _check(name, adv, dist, cls)
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    kept = (adv == np.clip(x, 0, 1)).reshape(len(x), -1)[cls != -1]
    print("beta0_F: %.5f of the successful images' pixels are still x0 (reference %.5f)" % (kept.mean(), ref["kept"][ref["best_class"] != -1].mean()))
    assert kept.mean() < 0.1                                        # the middle branch is d == 0 alone


def test_two_classes():
    name = "two_class_tiny"
    adv, dist, cls, const, _ = _run(name)
    ref = _check(name, adv, dist, cls)
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    assert set(cls.tolist()) <= {-1, 0, 1}
