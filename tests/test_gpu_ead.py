"""-m gpu: the elastic-net attack on the device (dg_ead, attacks.ElasticNetMethod, whitebox --attack_type ead) against the float64
restatement in tests/support/ead_reference.py, on the inputs its seed search recorded (tests/test_ead_cpu.py re-derives the seeds and
shows on the CPU that each case has the property it is named for).

The bounds are tests/test_gpu_cw.py's: best_class equal, best_dist rtol 1e-3, |x_adv - ref| <= 1e-4 on >= 0.999 of the pixels, constants
rtol 1e-12, stop iterations equal.  Every test prints how much of each bound it used."""
import functools
import os

import numpy as np
import pytest

from defensegan_amd import _native, network_builder as nb, whitebox as wb
from tests.support import ead_reference as E

pytestmark = pytest.mark.gpu

DIST_RTOL, PIXEL_TOL, PIXEL_SHARE = 1e-3, 1e-4, 0.999


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(x, labels or None, the float64 reference's result) of the recorded draw: computed once, shared, never written to."""
    layers, params = E.case_model(name)
    x, labels, ref = E.run_case(E.CASES[name], E.SEEDS[name], layers, params)
    return x, labels, ref


def _model(name):
    c = E.CASES[name]
    m = nb.MODELS[c["model"]](input_shape=(None,) + tuple(c.get("shape", (28, 28, 1))))
    m.set_weights(E.case_model(name)[1])
    return m


def _generate(name, m=None, x=None, **more):
    c = E.CASES[name]
    x0, labels, _ = _reference(name)
    own = m is None
    m = _model(name) if own else m
    lab = {"y_target": labels} if c.get("targeted") else {}
    out = nb.ElasticNetMethod(m).generate(x0 if x is None else x, return_info=True, **lab, **dict(c["kw"], **more))
    if own:
        m.close()
    return out


def _check(name, adv, dist, cls, pixels=True):
    """The family's bounds against the case's reference; prints the share of each bound used."""
    ref = _reference(name)[2]
    np.testing.assert_array_equal(cls, ref["best_class"])
    ok = ref["best_class"] != -1
    assert ok.mean() >= 0.25
    rel = np.abs(dist[ok] - ref["best_dist"][ok]) / ref["best_dist"][ok]
    assert (dist[~ok] == np.float32(1e10)).all()
    off = float((np.abs(adv - ref["x_adv"]) > PIXEL_TOL).mean())
    print("%s: %d/%d succeeded; best_dist uses %.4f of rtol %g; %.2e of the pixels differ by more than %g (%.3f of the %.0e allowed); "
          "largest pixel difference %.2e" % (name, ok.sum(), len(ok), rel.max() / DIST_RTOL, DIST_RTOL, off, PIXEL_TOL,
                                             off / (1 - PIXEL_SHARE), 1 - PIXEL_SHARE, np.abs(adv - ref["x_adv"]).max()))
    assert rel.max() <= DIST_RTOL
    if pixels:
        assert 1 - off >= PIXEL_SHARE
    return ref


@pytest.mark.parametrize("name", ["one_A", "one_F", "two_A", "two_F"])
def test_one_and_two_iterations(name):
    adv, dist, cls = _generate(name)
    _check(name, adv, dist, cls)


@pytest.mark.parametrize("model", ["A", "F"])
def test_five_iterations_with_and_without_fista(model):
    on, off = _generate("five_" + model), _generate("five_ista_" + model)
    _check("five_" + model, *on)
    _check("five_ista_" + model, *off)
    assert not np.array_equal(_reference("five_" + model)[2]["x_adv"], _reference("five_ista_" + model)[2]["x_adv"])
    assert not np.array_equal(on[0], off[0])


def test_sparsity_the_untouched_pixels_are_the_bits_of_clip_x():
    adv, dist, cls = _generate("sparse_F")
    x, _, ref = _reference("sparse_F")
    _check("sparse_F", adv, dist, cls)
    kept_dev = (adv == np.clip(x, 0, 1)).reshape(len(x), -1)          # bit-equal float32
    share = float((kept_dev == ref["kept"]).mean())
    print("sparse_F: reference keeps %.3f of the pixels at x0, device %.3f; the two sets agree on %.5f" % (ref["kept"].mean(), kept_dev.mean(), share))
    assert 0.05 < ref["kept"].mean() < 0.95 and 0.05 < kept_dev.mean() < 0.95
    assert share >= 0.999


def test_clip_branches():
    x, _, ref = _reference("clip_F")
    assert (x == 0).mean() > 0.2 and (x == 1).mean() > 0.2
    assert min(ref["clamped"]) > 100, ref["clamped"]                  # the reference clamps at both bounds
    adv, dist, cls = _generate("clip_F")
    _check("clip_F", adv, dist, cls)
    assert adv.min() >= 0.0 and adv.max() <= 1.0
    # the pixels that sit exactly on a bound are the reference's (most of the clamped ones started there: the clamp holds them)
    for bound in (0.0, 1.0):
        share = float(((adv == bound) == (ref["x_adv"] == bound)).mean())
        print("clip_F: the pixels at exactly %g agree with the reference on %.5f" % (bound, share))
        assert share >= 0.999 and (adv == bound).any()


def test_decision_rule():
    en, l1 = _reference("rule_en_F")[2], _reference("rule_l1_F")[2]
    assert np.array_equal(_reference("rule_en_F")[0], _reference("rule_l1_F")[0])
    differ = np.abs(en["x_adv"] - l1["x_adv"]).reshape(16, -1).max(axis=1) > 1e-3
    assert differ.any()                                               # the reference returns different images under the two rules
    m = _model("rule_en_F")
    a_en, a_l1 = _generate("rule_en_F", m), _generate("rule_l1_F", m)
    m.close()
    _check("rule_en_F", *a_en)
    _check("rule_l1_F", *a_l1)
    assert (np.abs(a_en[0] - a_l1[0]).reshape(16, -1).max(axis=1) > 1e-3).tolist() == differ.tolist()


def test_abort_chunks_and_repeatability():
    name = "abort_F"
    x, _, ref = _reference(name)
    stops = ref["abort_iters"][0]
    assert None not in stops and len(set(stops)) >= 2, stops          # the chunks stop at different checks
    m = _model(name)
    ead = nb.ElasticNetMethod(m)
    kw = E.CASES[name]["kw"]
    adv, dist, cls, _, stop = ead.generate(x, return_info=True, return_search=True, **kw)
    assert stop.tolist() == [stops]
    _check(name, adv, dist, cls)
    adv2, dist2, cls2 = ead.generate(x, return_info=True, **kw)       # a repeated call: the same bits
    assert adv.tobytes() == adv2.tobytes() and dist.tobytes() == dist2.tobytes() and cls.tobytes() == cls2.tobytes()
    a1, d1, c1 = ead.generate(x[16:32], return_info=True, **kw)       # chunk 1 alone: chunk 1's bits
    assert a1.tobytes() == adv[16:32].tobytes() and d1.tobytes() == dist[16:32].tobytes() and c1.tobytes() == cls[16:32].tobytes()
    m.close()


def test_chunks_wider_than_a_wave_and_a_trailing_partial_chunk():
    name = "wide_F"
    x, _, ref = _reference(name)
    assert None not in ref["abort_iters"][0]
    m = _model(name)
    adv, dist, cls, _, stop = nb.ElasticNetMethod(m).generate(x, return_info=True, return_search=True, **E.CASES[name]["kw"])
    m.close()
    assert stop.tolist() == ref["abort_iters"]
    _check(name, adv, dist, cls)
    ok = cls != -1
    assert adv[~ok].tobytes() == np.clip(x[~ok], 0, 1).tobytes()


def test_binary_search():
    name = "search_F"
    x, _, ref = _reference(name)
    assert (ref["const"] < 6.0).any() and (ref["const"] > 6.0).any()  # the search moved the constants both ways
    m = _model(name)
    adv, dist, cls, const, _ = nb.ElasticNetMethod(m).generate(x, return_info=True, return_search=True, **E.CASES[name]["kw"])
    m.close()
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    _check(name, adv, dist, cls)


def test_repeat_runs_the_last_step_at_the_upper_bound():
    name = "repeat_F"
    x, _, ref = _reference(name)
    m = _model(name)
    adv, dist, cls, const, _ = nb.ElasticNetMethod(m).generate(x, return_info=True, return_search=True, **E.CASES[name]["kw"])
    m.close()
    np.testing.assert_allclose(const, ref["const"], rtol=1e-12)
    _check(name, adv, dist, cls)


def test_targeted_large_images_and_torch_stream():
    import torch
    name = "targeted_F"
    x, yt, ref = _reference(name)
    assert x.shape[1:] == (64, 64, 3) and x.min() < -0.9
    m = _model(name)
    ead = nb.ElasticNetMethod(m)
    kw = E.CASES[name]["kw"]
    adv, dist, cls = ead.generate(x, y_target=np.eye(10, dtype=np.float32)[yt], return_info=True, **kw)
    _check(name, adv, dist, cls)
    assert ((cls == -1) | (cls == yt)).all()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xt = torch.from_numpy(x).cuda()
        at, dt, ct = ead.generate(xt, y_target=torch.from_numpy(yt), return_info=True, **kw)
    s.synchronize()
    assert at.cpu().numpy().tobytes() == adv.tobytes() and dt.cpu().numpy().tobytes() == dist.tobytes()
    assert ct.cpu().numpy().tobytes() == cls.tobytes()
    m.close()


@pytest.mark.parametrize("rule", ["EN", "L1"])
def test_self_consistency(rule):
    name = "mixed_F"
    x, _, ref = _reference(name)
    m = _model(name)
    beta = np.float32(E.CASES[name]["kw"]["beta"])
    adv, dist, cls = _generate(name, m, decision_rule=rule)
    if rule == "EN":
        _check(name, adv, dist, cls)
    ok = cls != -1
    assert ok.any() and (~ok).any()
    own = m.get_logits(x).argmax(axis=1)
    pred = m.get_logits(adv).argmax(axis=1)
    m.close()
    assert (pred[ok] != own[ok]).all() and (pred[ok] == cls[ok]).all()
    d = (adv.astype(np.float64) - np.clip(x, 0, 1).astype(np.float64)).reshape(len(x), -1)
    l1, l2 = np.abs(d).sum(axis=1), (d * d).sum(axis=1)
    crit = l2 + float(beta) * l1 if rule == "EN" else l1
    rel = np.abs(crit[ok] - dist[ok]) / crit[ok]
    print("mixed_F %s: %d/%d succeeded; the criterion recomputed from x_adv uses %.4f of rtol 1e-5" % (rule, ok.sum(), len(ok), rel.max() / 1e-5))
    assert rel.max() <= 1e-5
    assert adv[~ok].tobytes() == np.clip(x[~ok], 0, 1).tobytes()
    assert (dist[~ok] == np.float32(1e10)).all() and (cls[~ok] == -1).all()


def test_refusals():
    import ctypes as C
    import torch
    m = _model("one_F")
    ead = nb.ElasticNetMethod(m)
    x = _reference("one_F")[0]
    with pytest.raises(ValueError, match="x must be"):
        ead.generate(np.zeros((2, 28, 27, 1), np.float32))
    with pytest.raises(ValueError, match="decision_rule"):
        ead.generate(x, decision_rule="l1")
    with pytest.raises(ValueError, match="beta"):
        ead.generate(x, beta=-1.0)
    with pytest.raises(ValueError, match="labels must be"):
        ead.generate(x, y=np.full(16, 10))
    # through the C entry: errors, not faults
    lib, h = _native.load(), m._handle
    xt = torch.from_numpy(x).cuda()
    out, dist = torch.empty_like(xt), torch.empty(16, device="cuda")
    cls = torch.empty(16, dtype=torch.int32, device="cuda")
    p, q, d, c = xt.data_ptr(), out.data_ptr(), dist.data_ptr(), cls.data_ptr()

    def call(h=h, x=p, B=16, beta=1e-2, rule=0, iters=2, lo=0.0, hi=1.0, x_adv=q, best_dist=d, best_class=c):
        return lib.dg_ead(h, x, None, B, 0, 16, 0.0, beta, rule, 1, 0.1, 1, iters, 0, 1.0, lo, hi, x_adv, best_dist, best_class, None, None, None)
    for kw, text in ((dict(h=None), b"null"), (dict(x=None), b"null"), (dict(x_adv=None), b"null"), (dict(best_dist=None), b"null"),
                     (dict(best_class=None), b"null"), (dict(B=0), b"B must be"), (dict(B=-3), b"B must be"), (dict(beta=-1e-3), b"beta"),
                     (dict(lo=1.0, hi=1.0), b"clip_min"), (dict(lo=1.0, hi=0.0), b"clip_min"), (dict(iters=0), b"max_iterations"),
                     (dict(rule=2), b"decision_rule"), (dict(rule=-1), b"decision_rule")):
        assert call(**kw) == -1 and text in lib.dg_last_error(), kw
    assert call() == 0                                                # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    gan_like = object()
    m.rec_layer = gan_like
    with pytest.raises(NotImplementedError, match="reconstruction layer"):
        ead.generate(x)
    m.rec_layer = None
    m.close()


@pytest.mark.parametrize("defense_type", ["none", "adv_tr"])
def test_whitebox_driver(defense_type, tmp_path):
    """whitebox(attack_type='ead') on a tiny separable split: the accuracy is that of the attack called by hand on the trained model, and
    the result line carries the two norms."""
    import argparse
    from tests.test_gpu_train import _synthetic
    xtr, ytr = _synthetic(512, seed=1)
    xte, yte = _synthetic(64, seed=2)
    model = nb.model_e()
    norms = {}
    params = {"binary_search_steps": 2, "max_iterations": 20, "learning_rate": 0.1, "initial_const": 10.0, "ead_beta": 1e-2, "ead_rule": "L1"}
    acc, zero, roc = wb.whitebox(None, model, (xtr, ytr, xte, yte), batch_size=64, nb_epochs=1, attack_type="ead", defense_type=defense_type,
                                 attack_params=params, norms=norms)
    hand = dict(wb.EAD_PARAMS, batch_size=64, binary_search_steps=2, max_iterations=20, learning_rate=0.1, initial_const=10.0, beta=1e-2,
                decision_rule="L1")
    adv, dist, cls = nb.ElasticNetMethod(model).generate(xte, return_info=True, **hand)
    correct, _, _ = model.eval_batch(adv, labels=yte)
    assert zero == 0 and roc is None and acc == correct / 64.0
    ok = cls != -1
    assert norms["successes"] == int(ok.sum()) and ok.any()
    d = (adv.astype(np.float64) - xte.astype(np.float64)).reshape(64, -1)
    np.testing.assert_allclose(norms["l1"], np.abs(d).sum(axis=1)[ok].mean(), rtol=1e-5)
    np.testing.assert_allclose(norms["l2"], np.sqrt((d * d).sum(axis=1))[ok].mean(), rtol=1e-5)
    print("model E, %s: accuracy under ead %.3f, %d/64 succeeded, mean L1 %.4f, mean L2 %.4f" % (defense_type, acc, ok.sum(), norms["l1"], norms["l2"]))
    flags = argparse.Namespace(defense_type=defense_type, attack_type="ead", attack_ord="inf", dataset_name="mnist", rec_path=None,
                               train_on_recs=False, num_tests=-1, num_train=-1, model="E", fgsm_eps_tr=0.15)
    results_dir, fname = wb.get_results_dir_filename(flags, None)
    path = wb.result_path(os.path.join(str(tmp_path), results_dir), fname, "run")
    wb.write_results(path, (acc, zero, roc), norms)
    assert os.path.basename(path).endswith("attack=ead.txt")
    assert open(path).read() == "%s 0 l1=%s l2=%s \n" % (acc, norms["l1"], norms["l2"])
    model.close()
