"""-m gpu: Carlini-Wagner L2 on the device (dg_cw) against the float64 restatement (tests/support/cw_reference.py) off the corridor
tests/test_gpu_cw.py walks: confidence != 0, ties at the maximum, inputs outside and on the clip bounds, abort inside a binary
search, the degenerate schedules, labels outside the classes (C ABI), and independence of the chunking with abort off.  The
inputs are tests/support/cw_cases.py's; tests/test_cw_cpu.py asserts on the reference alone that they are decidable and that a
reference with the rule in question broken misses the gates below by more than ten times on a quarter of the images.

The gates are those of tests/test_gpu_cw.py: best_class equal, best_l2 at rtol 1e-3, |x_adv - ref| <= 1e-4 on 99.9 % of the
pixels, final_const at rtol 1e-12, chunk_stop equal; on the images the reference calls decidable (cw_cases.decidable).

What the tie cases can and cannot tell.  The ties come from equal columns of the last layer, so the input gradient sees only the
SUM of the shares inside a tied group: a share that is not split (2c, 3c) or partly lost to the label shows, an even split
against the whole share going to the first maximiser does not.  The -c/2, -c/3 distribution itself is pinned on the CPU
reference only (tests/test_cw_cpu.py).  Of the tie runs only b-i6, b-own and b-own-k0 are shown sensitive to a broken rule; b-i1
to b-i3 (and the good rows of case f) are shown sensitive on the reference only through the first argmax of the recorded class."""
import ctypes as C

import numpy as np
import pytest

from defensegan_amd import _native
from defensegan_amd import network_builder as nb
from tests.support import cw_cases as K

pytestmark = pytest.mark.gpu


def _device_model(name):
    m = K.model(name)
    m.set_weights(K.params(name))
    return m


def _generate(m, case, **override):
    c = case
    kw = dict(c["kw"], **override)
    lab = {} if c["labels"] is None else {"y_target" if c["targeted"] else "y": c["labels"]}
    return nb.CarliniWagnerL2(m).generate(np.array(c["x"]), return_info=True, return_search=True, **dict(kw, **lab))


def _gates(name, got, ref, exact=None):
    """``exact``: images compared although their margins are 0, because the tie behind them is exact on both sides."""
    adv, l2, cls, const, stop = got
    keep, chunks_ok = K.decidable(ref)
    if exact is not None:
        keep = keep | exact
    assert chunks_ok and (~keep).sum() <= len(keep) // 8
    d = np.abs(adv.astype(np.float64) - ref["x_adv"])[keep]
    ok = ref["best_class"][keep] != -1
    rel = np.abs(l2[keep][ok] - ref["best_l2"][keep][ok]) / np.maximum(ref["best_l2"][keep][ok], 1e-300)
    print("%s: left out %d, classes differ %d, best_l2 rel %.3g, pixels beyond 1e-4 %.3g (max %.3g), const rel %.3g" % (
        name, int((~keep).sum()), int((cls[keep] != ref["best_class"][keep]).sum()), rel.max() if rel.size else 0.0,
        (d > K.PIXEL_ATOL).mean(), d.max(), (np.abs(const - ref["const"]) / ref["const"]).max()))
    assert stop.tolist() == K.stops(ref)
    np.testing.assert_array_equal(cls[keep], ref["best_class"][keep])
    np.testing.assert_allclose(l2[keep], ref["best_l2"][keep], rtol=K.L2_RTOL)
    assert (d <= K.PIXEL_ATOL).mean() >= K.PIXEL_SHARE
    np.testing.assert_allclose(const[keep], ref["const"][keep], rtol=K.CONST_RTOL)
    return keep


def _bytes(outs):
    return [o.tobytes() for o in outs]


# ---------------------------------------------------------------------- a. confidence
@pytest.mark.parametrize("name", K.A_NAMES)
def test_confidence(name):
    m = _device_model("F")
    ref = K.reference(name)
    _gates(name, _generate(m, K.case(name)), ref)
    m.close()


# ---------------------------------------------------------------------- b. ties at the maximum
def _assert_tied_logits(m, x):
    Z = m.get_logits(np.array(x))
    for g in K.TIE_GROUPS:
        for k in g[1:]:
            assert Z[:, k].tobytes() == Z[:, g[0]].tobytes()      # equal columns, the same fma chain: equal bit for bit
    return Z


@pytest.mark.parametrize("name", K.B_NAMES)
def test_ties_with_the_label_outside_the_tied_groups(name):
    m = _device_model("T")
    c = K.case(name)
    _assert_tied_logits(m, c["x"])
    ref = K.reference(name)
    adv, l2, cls, const, stop = got = _generate(m, c)
    _gates(name, got, ref)
    assert set(cls.tolist()) <= {-1, 1, 3}                         # a success records the lowest index of the tied maximum
    Zadv = m.get_logits(adv)
    ok = cls != -1
    assert (Zadv.argmax(axis=1)[ok] == cls[ok]).all() and (Zadv.max(axis=1)[ok] == Zadv[ok, cls[ok]]).all()
    m.close()


def test_ties_with_the_models_own_label_inside_a_tied_group():
    """y=None, kappa = 0: an image whose top two logits tie is labelled with the first of them.  Its twin then keeps arg = 0 and
    the first argmax stays the label: the image never succeeds and never moves.  Labelled with any later member of the tie, it
    would succeed at iteration 0 at l2 = 0 (the first argmax is not that label).  The logits tie bit for bit, so the decision is
    exact on the device and these images are compared at margin 0."""
    m = _device_model("U")
    c = K.case(K.OWN_K0)
    Z = _assert_tied_logits(m, c["x"])
    ref = K.reference(K.OWN_K0)
    tied = K.tied_own(ref)
    assert tied.sum() >= 4 and (np.sort(Z, axis=1)[tied, -1] == np.sort(Z, axis=1)[tied, -2]).all()
    adv, l2, cls, const, stop = got = _generate(m, c)
    assert (cls[tied] == -1).all() and (l2[tied] == np.float32(1e10)).all()
    assert adv[tied].tobytes() == np.clip(c["x"], 0, 1)[tied].tobytes()
    _gates(K.OWN_K0, got, ref, exact=tied)
    ok = cls != -1
    assert ok.any() and (cls[ok] != ref["labels"][ok]).all()
    m.close()


def test_ties_with_the_label_inside_a_tied_group_and_a_confidence():
    """y=None at kappa = 0.5: the label's tied twin holds arg at kappa exactly, so the loss of such an image has no gradient
    while a wrong count of the maximisers (the label's own entry among them) gives it one.  This run does not depend on WHICH
    member of the tie becomes the label; the test above does."""
    m = _device_model("U")
    c = K.case("b-own")
    _assert_tied_logits(m, c["x"])
    ref = K.reference("b-own")
    assert K.tied_own(ref).sum() >= 4
    adv, l2, cls, const, stop = got = _generate(m, c)
    _gates("b-own", got, ref)
    ok = cls != -1
    assert (cls[ok] != ref["labels"][ok]).all()
    m.close()


# ---------------------------------------------------------------------- c. clip edges and the degenerate schedules
@pytest.mark.parametrize("name", K.C_NAMES)
def test_clip_edges(name):
    c = K.case(name)
    m = _device_model(c["model"])
    lo, hi = np.float32(c["kw"]["clip_min"]), np.float32(c["kw"]["clip_max"])
    ref = K.reference(name)
    adv, l2, cls, const, stop = got = _generate(m, c)
    _gates(name, got, ref)
    never = cls == -1
    assert 0 < never.sum() < len(cls)
    assert adv[never].tobytes() == np.clip(c["x"], lo, hi)[never].tobytes()
    assert adv.min() >= lo and adv.max() <= hi and np.isfinite(adv).all()
    assert (l2[never] == np.float32(1e10)).all()
    m.close()


@pytest.mark.parametrize("name", K.C_NAMES)
@pytest.mark.parametrize("schedule", [dict(max_iterations=0, binary_search_steps=2), dict(binary_search_steps=0)], ids=["no-iterations", "no-steps"])
def test_degenerate_schedules(name, schedule):
    c = K.case(name)
    m = _device_model(c["model"])
    lo, hi = np.float32(c["kw"]["clip_min"]), np.float32(c["kw"]["clip_max"])
    ref = K.run(name, **schedule)
    adv, l2, cls, const, stop = _generate(m, c, **schedule)
    assert adv.tobytes() == np.clip(c["x"], lo, hi).tobytes()
    assert (l2 == np.float32(1e10)).all() and (cls == -1).all()
    np.testing.assert_allclose(const, ref["const"], rtol=K.CONST_RTOL)
    c0 = c["kw"]["initial_const"]
    assert (ref["const"] == (c0 if schedule["binary_search_steps"] == 0 else c0 * 100)).all()
    assert stop.shape == (schedule["binary_search_steps"], 1) and (stop == -1).all()
    m.close()


# ---------------------------------------------------------------------- d. abort inside the binary search
@pytest.mark.parametrize("name", K.D_NAMES)
def test_abort_inside_the_binary_search(name):
    m = _device_model("F")
    c = K.case(name)
    ref = K.reference(name)
    stop_ref = np.array(K.stops(ref))
    assert stop_ref.shape == (3, 3) and (stop_ref == -1).any() and (stop_ref >= 0).any()
    got = _generate(m, c)
    _gates(name, got, ref)
    assert _bytes(_generate(m, c)) == _bytes(got)                  # the same handle, the same bytes
    m.close()


# ---------------------------------------------------------------------- e. chunking with abort off
@pytest.mark.parametrize("name", K.A_NAMES)
def test_chunking_does_not_couple_images_with_abort_off(name):
    m = _device_model("F")
    c = K.case(name)
    assert not c["kw"]["abort_early"]
    base = _generate(m, c, batch_size=16)
    for bs in (5, 64):
        got = _generate(m, c, batch_size=bs)
        assert _bytes(got[:4]) == _bytes(base[:4])
        assert got[4].shape == (1, -(-16 // bs)) and (got[4] == -1).all() and (base[4] == -1).all()
    tail = dict(c, x=c["x"][-3:], labels=c["labels"][-3:])
    alone = _generate(m, tail, batch_size=16)
    assert _bytes(alone[:4]) == _bytes([o[-3:] for o in base[:4]])
    m.close()


# ---------------------------------------------------------------------- f. labels outside the classes, through the C ABI
def _cw_native(m, x, labels, kw):
    import torch
    dev = torch.device("cuda", m._device)
    B, chunks = len(x), -(-len(x) // kw["batch_size"])
    xt = torch.from_numpy(np.array(x, np.float32)).to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(dev)
    adv = torch.empty_like(xt)
    l2 = torch.empty(B, dtype=torch.float32, device=dev)
    cls = torch.empty(B, dtype=torch.int32, device=dev)
    const = torch.empty(B, dtype=torch.float64, device=dev)
    stop = torch.empty(kw["binary_search_steps"], chunks, dtype=torch.int32, device=dev)
    _native.check(_native.load().dg_cw(
        m._handle, xt.data_ptr(), lab.data_ptr(), B, 0, int(kw["batch_size"]), float(kw.get("confidence", 0.0)), float(kw["learning_rate"]),
        int(kw["binary_search_steps"]), int(kw["max_iterations"]), 1 if kw["abort_early"] else 0, float(kw["initial_const"]), 0.0, 1.0,
        adv.data_ptr(), l2.data_ptr(), cls.data_ptr(), const.data_ptr(), stop.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return tuple(t.cpu().numpy() for t in (adv, l2, cls, const, stop))


def test_labels_outside_the_classes_through_the_c_abi():
    """cw_head_kernel's t < 0 || t >= n branch: such a row never succeeds, gets no gradient and leaves the others alone."""
    from tests.support import cw_reference as R
    m = _device_model("F")
    c = K.bad_label_case()
    m._ensure()
    kw, good, bad = c["kw"], c["good"], c["bad"]
    assert kw["batch_size"] == 1 and not kw["abort_early"]
    adv, l2, cls, const, stop = _cw_native(m, c["x"], c["labels"], kw)
    assert adv[bad].tobytes() == np.clip(c["x"][bad], 0, 1).tobytes()
    assert (l2[bad] == np.float32(1e10)).all() and (cls[bad] == -1).all() and (stop == -1).all()
    want, lower, upper = np.full(3, kw["initial_const"]), np.zeros(3), np.full(3, 1e10)
    for _ in range(kw["binary_search_steps"]):
        want, lower, upper = R.const_update(np.full(3, -1), c["labels"][bad], want, lower, upper, False)
    np.testing.assert_allclose(const[bad], want, rtol=K.CONST_RTOL)
    alone = _cw_native(m, c["x"][good], c["labels"][good], kw)
    assert _bytes(alone[:4]) == _bytes([adv[good], l2[good], cls[good], const[good]])
    ref = K.reference("f-good")
    # the good rows carry their own classes: one succeeds only after some Adam steps, the other never, so that every one of the
    # 2 x 5 iterations next to the bad rows shows in x_adv, best_l2 or final_const
    assert (ref["best_class"] != -1).sum() == 1 and (ref["best_l2"] > 0).all() and ref["const"][0] != ref["const"][1]
    _gates("f-good", alone, ref)
    m.close()
