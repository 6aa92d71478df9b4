"""-m gpu: the generator's training step (defensegan_amd/csrc/dg_gen_train.hip) where tests/test_gpu_gen_train.py does not go: batches
past 50 rows, where every reduction changes its chunking; one handle called with many row counts; options changed after a training
step; Adam away from its default.

Bounds are the project's, unchanged (test_gpu_gen_train.check_grads: every gradient tensor within 1e-4 of its reference's largest
entry, a bias of the sum of its absolute terms; dz within 1e-4 of its largest entry; rtol 1e-6 / atol 1e-6 max on an Adam step from
the device's own state).  Large batches come from generator_reference.draw_rows: rows none of whose ReLU gates float32 can flip
(tests/test_gen_train_regimes_cpu.py shows each case is served and costs float32 itself at most 0.033 of the bound).

THE SPLIT RULE, restated from the kernel file's description and not imported from it (``split`` below): a reduction axis of `total`
terms is cut into chunks of `least` terms; were that more than `most` chunks, the length becomes ceil(total / most); the length is
rounded up to a multiple of `multiple`; the chunks are ceil(total / length).  The MFMA weight gradients use (most 16, least 256,
multiple 2) on N h_in^2 terms (h_in = 7 for Generator.3, 4 for Generator.2, 1 for the Linear layer); dF5 and the bias sums use
(most 256, least 1, multiple 1) on their rows (dF5: the N batch rows; a bias: rows times positions)."""
import functools

import numpy as np
import pytest

from tests.support import generator_reference as GR
from tests.test_gpu_gen_train import GRAD_TOL, check_grads, make

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------- the rule, restated
def split(total, most, least, multiple):
    length = least
    if -(-total // length) > most:
        length = -(-total // most)
    length = -(-length // multiple) * multiple
    return max(1, -(-total // length)), length


def regimes(N):
    """(chunks, length) of every reduction of an N-row call."""
    return {"G3": split(49 * N, 16, 256, 2), "G2": split(16 * N, 16, 256, 2), "lin": split(N, 16, 256, 2),
            "tail": split(N, 256, 1, 1), "bias1": split(N, 256, 1, 1)}


def test_every_case_is_in_the_regime_it_is_named_for():
    """Needs no device, but belongs to the GPU cases it guards: a later change of the chunk length or of the cap (and of this
    restatement with it) cannot leave the cases below outside what they are there for."""
    assert regimes(50)["G3"] == (10, 256) and regimes(83)["G3"] == (16, 256)      # up to 83 rows: chunks of 256, what ran so far
    # 84, 85: Generator.3 at the cap with a recomputed length -- 84 gives an even one, 85 an odd one that is rounded up
    assert regimes(84)["G3"] == (16, 258) and -(-49 * 84 // 16) == 258
    assert regimes(85)["G3"] == (16, 262) and -(-49 * 85 // 16) == 261
    for N in (84, 85):
        r = regimes(N)
        assert r["G2"][1] == 256 and r["lin"] == (1, 256) and r["tail"] == (N, 1)
        assert 49 * N - 15 * r["G3"][1] < r["G3"][1]                              # a shorter last chunk
        assert any((c * r["G3"][1]) % 49 for c in range(1, 16))                   # chunks that start in the middle of a row
    # 257: Generator.2 capped as well, the Linear layer in two splits (the second of one term), two rows per dF5 chunk with a last
    # chunk of one row, and the Linear bias sum capped in the same way
    assert regimes(256)["G2"] == (16, 256) and regimes(256)["lin"] == (1, 256) and regimes(256)["tail"] == (256, 1)
    r = regimes(257)
    assert r["G2"] == (16, 258) and r["G3"] == (16, 788) and r["lin"] == (2, 256) and r["tail"] == (129, 2) and r["bias1"] == (129, 2)
    assert 257 - 128 * 2 == 1 and 257 - 256 == 1
    # NET_DIM 128 at 33 rows: 7 and 3 K splits where only one ran so far (3 rows: one split per layer)
    assert regimes(3)["G3"][0] == 1 and regimes(3)["G2"][0] == 1
    assert regimes(33)["G3"] == (7, 256) and regimes(33)["G2"] == (3, 256)


# ---------------------------------------------------------------------- shared inputs and references (computed once, never written)
@functools.lru_cache(maxsize=None)
def case(latent, nd, N):
    """(weights, z, dy, float64 gradient, bias scales) of a large-batch case."""
    p = GR.weights(latent, nd)
    z, dy, info = GR.draw_rows(latent, nd, N)
    print("draw_rows(%d, %d, %d): pool %d, kept %.3f, margins %s" % (latent, nd, N, info["pool"], info["kept"], info["margins"]))
    return p, z, dy, GR.gradient(p, z, dy), GR.bias_scales(p, z, dy)


def small(N):
    z, dy = GR.draw(GR.SEEDS[(128, 64, N)], N, 128)
    return z, dy


def check_dz(dz, ref_dz, what):
    used = float(np.abs(dz - ref_dz).max()) / (GRAD_TOL * float(np.abs(ref_dz).max()))
    print("%s dz uses %.3f of the bound" % (what, used))
    assert used <= 1.0, (what, used)
    return used


def raw_gradient(g, z, dy):
    """dg_gen_param_gradient with out_y and out_dz: (flat gradient, dz, y) as arrays."""
    import torch
    h = g._ensure_handle()
    zz, dd = g._to_device(z), g._to_device(dy)
    N = int(zz.shape[0])
    flat = torch.empty(g.n_params(), dtype=torch.float32, device=zz.device)
    y = torch.empty(N, 28, 28, 1, dtype=torch.float32, device=zz.device)
    dz = torch.empty_like(zz)
    with torch.cuda.device(zz.device):
        g._check(g._lib().dg_gen_param_gradient(h, zz.data_ptr(), dd.data_ptr(), N, flat.data_ptr(), y.data_ptr(), dz.data_ptr(),
                                                torch.cuda.current_stream(zz.device).cuda_stream))
    return flat.cpu().numpy(), dz.cpu().numpy(), y.cpu().numpy()


# ---------------------------------------------------------------------- B. every split regime
@pytest.mark.parametrize("latent,nd,N", GR.ROW_CASES)
def test_gradients_in_every_split_regime(latent, nd, N):
    """generator_gradient on draw_rows inputs against float64, the eight tensors and dz, at the smallest N of every chunking regime
    (see test_every_case_is_in_the_regime_it_is_named_for); a second call returns the same bits.  Measured (one MI355X, one run): the
    worst tensor of the five cases uses 0.014 of the 1e-4 bound
    (Generator.5.Filters at 128 / 64 / 257), dz at most 0.011; every use is printed."""
    p, z, dy, ref, scales = case(latent, nd, N)
    g, _ = make(latent, nd)
    _, grads, dz = g.generator_gradient(z, dy)
    worst = check_grads(grads, ref["grads"], scales, "%d/%d N=%d" % (latent, nd, N))
    check_dz(dz, ref["dz"], "%d/%d N=%d" % (latent, nd, N))
    print("worst tensor uses %.3f of the bound" % worst)
    _, again, dz2 = g.generator_gradient(z, dy)
    for n in GR.NAMES:
        assert np.array_equal(grads[n], again[n]), n
    assert np.array_equal(dz, dz2)
    g.close()


@pytest.mark.parametrize("latent", [128, 64])
def test_the_last_row_of_257_alone(latent):
    """N = 257 with a dy that is zero except in row 256: every gradient is the float64 gradient of that row alone, dz[:256] is exactly
    zero.  Row 256 is the whole last chunk of the Linear K split, of the dF5 rows and of the Linear bias sum, and the end of the
    short last chunk of Generator.2's and Generator.3's axes: dropped or doubled, the gradient is off by its whole size.  Measured
    (one MI355X, one run): the worst tensor uses 0.014 of the 1e-4 bound (Generator.Input.W at LATENT_DIM 128), dz 0.010."""
    p, z, dy, _, _ = case(latent, 64, 257)
    dy = dy.copy()
    dy[:256] = 0
    ref = GR.gradient(p, z[256:], dy[256:])
    g, _ = make(latent, 64)
    _, grads, dz = g.generator_gradient(z, dy)
    worst = check_grads(grads, ref["grads"], GR.bias_scales(p, z[256:], dy[256:]), "last row, latent %d" % latent)
    print("worst tensor uses %.3f of the bound" % worst)
    assert not dz[:256].any()
    check_dz(dz[256:], ref["dz"], "last row, latent %d" % latent)
    g.close()


# ---------------------------------------------------------------------- C. one handle, many row counts
REUSE_ORDER = (3, 257, 3, 85, 1)


@functools.lru_cache(maxsize=None)
def reuse_inputs(N):
    if N in (257, 85):
        p, z, dy, ref, scales = case(128, 64, N)
        return z, dy, ref, scales
    z, dy = small(N)
    p = GR.weights()
    return z, dy, GR.gradient(p, z, dy), GR.bias_scales(p, z, dy)


def test_one_handle_called_with_many_row_counts():
    """One handle called with N = 3, 257, 3, 85, 1: the workspace grows (dpre5 and the chunk sums are freed and allocated again),
    then serves smaller calls whose buffers still hold the larger call's rows beyond N.  Every result -- flat gradient, dz, and y
    through out_y -- is bit-identical to a FRESH handle's for that N alone and within the float64 bounds.  Measured (one MI355X, one
    run): at most 0.014 of the 1e-4 bound on a tensor and 0.011 on dz."""
    g, p = make()
    for N in REUSE_ORDER:
        z, dy, ref, scales = reuse_inputs(N)
        flat, dz, y = raw_gradient(g, z, dy)
        fresh, _ = make()
        flat_f, dz_f, y_f = raw_gradient(fresh, z, dy)
        fresh.close()
        assert np.array_equal(flat, flat_f) and np.array_equal(dz, dz_f) and np.array_equal(y, y_f), N
        check_grads(g.split_grads(flat), ref["grads"], scales, "reused handle N=%d" % N)
        check_dz(dz, ref["dz"], "reused handle N=%d" % N)
        assert np.abs(y - ref["y"]).max() <= 1e-5
    g.close()


def adam_check(w0, m0, v0, grads, t, w1, m1, v1, lr, b1, b2, what):
    """The device's step against generator_reference.adam_f32 from the device's own state: rtol 1e-6, atol 1e-6 max."""
    worst = 0.0
    for n in GR.NAMES:
        pw, pm, pv = GR.adam_f32(w0[n], grads[n], m0[n], v0[n], t, lr, b1, b2)
        for got, want, kind in ((w1[n], pw, "w"), (m1[n], pm, "m"), (v1[n], pv, "v")):
            bound = 1e-6 * float(np.abs(want).max()) + 1e-6 * np.abs(want)
            if float(np.abs(want).max()) > 0:
                worst = max(worst, float((np.abs(got - want) / bound).max()))
            assert np.allclose(got, want, rtol=1e-6, atol=1e-6 * float(np.abs(want).max())), (what, n, kind)
    print("%s: worst use of the rtol 1e-6 / atol 1e-6 max bound %.4f" % (what, worst))
    return worst


def step_and_check(g, z, dy, lr, b1, b2, what, latent=128, nd=64):
    """One generator_step on ``g``; the gradient from a twin handle holding g's weights; Adam restated from g's own state."""
    w0 = g.get_weights()
    m0, v0, t0 = g.generator_adam_state()
    twin, _ = make(latent, nd, weights=w0)
    _, grads, _ = twin.generator_gradient(z, dy)
    twin.close()
    assert g.generator_step(z, dy, learning_rate=lr, beta1=b1, beta2=b2) is None
    w1 = g.get_weights()
    m1, v1, t1 = g.generator_adam_state()
    assert t1 == t0 + 1
    adam_check(w0, m0, v0, grads, t1, w1, m1, v1, lr, b1, b2, what)
    return w0, w1


def test_steps_on_a_reused_handle():
    """After the five gradient calls of the test above (the last with N = 1), generator_step at N = 85 and then N = 3 on the same
    handle: weights and moments match adam_f32 from the device's own state with a twin handle's gradient.  Measured (one MI355X,
    one run): under 0.0001 of the rtol 1e-6 / atol 1e-6 max bound (the restatement gives the device's bits)."""
    g, p = make()
    for N in REUSE_ORDER:
        z, dy, _, _ = reuse_inputs(N)
        g.generator_gradient(z, dy)
    for N in (85, 3):
        z, dy, _, _ = reuse_inputs(N)
        w0, w1 = step_and_check(g, z, dy, 1e-4, 0.5, 0.9, "reused handle, step at N=%d" % N)
        assert all(not np.array_equal(w0[n], w1[n]) for n in GR.NAMES)
    g.close()


# ---------------------------------------------------------------------- D. handle state changed after training
def same_as_fresh(g, options, zs, x, latent=128, nd=64):
    """generate and reconstruct of ``g`` are the bits of a fresh handle given g's weights and the same options."""
    fresh, _ = make(latent, nd, weights=g.get_weights())
    for o in options:
        fresh.set_option(*o)
    assert np.array_equal(g.generate(zs), fresh.generate(zs))
    a = g.reconstruct(x, seed=5, return_details=True)
    b = fresh.reconstruct(x, seed=5, return_details=True)
    for k in ("rec", "loss", "z", "idx"):
        assert np.array_equal(a[k], b[k]), k
    fresh.close()


def nsplit_gradient_check(g, what):
    """generator_gradient of a handle with a non-default nsplit at its own (trained) weights: within the float64 bounds, the
    gradients the bits of a default (nsplit 16) handle's, which do not depend on it; dz is a different sum and only bounded."""
    w = g.get_weights()
    z, dy, info = GR.draw_rows(128, 64, 4, seed=11, params=w)
    ref = GR.gradient(w, z, dy)
    _, grads, dz = g.generator_gradient(z, dy)
    used = check_grads(grads, ref["grads"], GR.bias_scales(w, z, dy), what)
    used_dz = check_dz(dz, ref["dz"], what)
    base, _ = make(weights=w)
    _, grads16, dz16 = base.generator_gradient(z, dy)
    base.close()
    for n in GR.NAMES:
        assert np.array_equal(grads[n], grads16[n]), n
    check_dz(dz16, ref["dz"], what + " (nsplit 16)")
    return max(used, used_dz)


@pytest.mark.parametrize("options", [(("nsplit", 8),), (("frag_path", 1),), (("latent_turn", 0),), (("nsplit", 8), ("frag_path", 1))],
                         ids=["nsplit8", "frag_path", "latent_turn0", "nsplit8+frag_path"])
def test_options_changed_after_a_training_step(options):
    """Two steps at N = 4, then the option(s), then two more steps.  After the option call and again after the further steps:
    generate and reconstruct (B 3, R 2, L 3) are the bits of a fresh handle given get_weights() and the same options; the option call
    itself leaves get_weights() unchanged; with nsplit = 8 the gradients and dz are within the float64 bounds and the gradients are
    the bits of an nsplit 16 handle's.  nsplit repacks the Linear weights from the TRAINED device copy and frees both packs, so the
    next step has to rebuild its gather maps.  Measured (one MI355X, one run): the nsplit gradients use at most 0.081 of the 1e-4
    bound (Generator.5.Filters at the weights of two lr 1e-2 steps), dz at most 0.066."""
    g, p = make()
    zs = GR.draw(7, 6, 128)[0]
    x = g.generate(zs[:3])
    before = g.generate(zs)
    for t in range(2):
        z, dy = GR.draw(200 + t, 4, 128)
        g.generator_step(z, dy, learning_rate=1e-2)
    w = g.get_weights()
    trained = g.generate(zs)
    assert not np.array_equal(trained, before)
    for o in options:
        g.set_option(*o)
    w2 = g.get_weights()
    for n in GR.NAMES:
        assert np.array_equal(w[n], w2[n]), n
    same_as_fresh(g, options, zs, x)
    has_nsplit = any(k == "nsplit" for k, _ in options)
    if has_nsplit:
        nsplit_gradient_check(g, "after the option")
    for t in range(2, 4):
        z, dy = GR.draw(200 + t, 4, 128)
        g.generator_step(z, dy, learning_rate=1e-2)
    assert not np.array_equal(g.generate(zs), trained)
    assert g.generator_adam_state()[2] == 4
    same_as_fresh(g, options, zs, x)
    if has_nsplit:
        nsplit_gradient_check(g, "after two more steps")
    g.close()


@pytest.mark.parametrize("option", [None, ("frag_path", 1)], ids=["default", "frag_path"])
@pytest.mark.parametrize("latent,nd", [(64, 64), (128, 128)])
def test_the_refresh_at_other_widths(latent, nd, option):
    """test_gpu_gen_train's refresh check (three steps, then generate and reconstruct the bits of a fresh handle given get_weights())
    at LATENT_DIM 64, which has no backward pack of the Linear weights and therefore another set of gather maps, and at NET_DIM 128."""
    options = (option,) if option else ()
    g, p = make(latent, nd)
    for o in options:
        g.set_option(*o)
    zs = GR.draw(7, 6, latent)[0]
    x = g.generate(zs[:3])
    before = g.generate(zs)
    for t in range(3):
        z, dy = GR.draw(200 + t, 4, latent)
        g.generator_step(z, dy, learning_rate=1e-2)
    assert not np.array_equal(g.generate(zs), before)
    same_as_fresh(g, options, zs, x, latent, nd)
    g.close()


# ---------------------------------------------------------------------- E. Adam off the default
def test_adam_with_beta1_zero():
    """Three steps at (lr 2e-4, beta1 0, beta2 0.999) against adam_f32 from the device's own state.  Measured (one MI355X, one run):
    under 0.0001 of the rtol 1e-6 / atol 1e-6 max bound."""
    g, p = make()
    for t in range(3):
        z, dy = GR.draw(100 + t, 4, 128)
        step_and_check(g, z, dy, 2e-4, 0.0, 0.999, "beta1 = 0, step %d" % (t + 1))
    g.close()


def test_adam_with_a_long_running_counter():
    """Two steps, then the counter set to 99 999 with the moments kept (_set_generator_adam), then the step with t = 100 000: lr_t
    from a large t.  Measured (one MI355X, one run): under 0.0001 of the bound."""
    g, p = make()
    for t in range(2):
        z, dy = GR.draw(100 + t, 4, 128)
        g.generator_step(z, dy)
    m, v, t = g.generator_adam_state()
    assert t == 2
    g._set_generator_adam(m, v, 99999)
    m2, v2, t2 = g.generator_adam_state()
    assert t2 == 99999 and all(np.array_equal(m[n], m2[n]) and np.array_equal(v[n], v2[n]) for n in GR.NAMES)
    z, dy = GR.draw(102, 4, 128)
    step_and_check(g, z, dy, 1e-4, 0.5, 0.9, "t = 100 000")
    assert g.generator_adam_state()[2] == 100000
    g.close()


def test_adam_on_a_zero_gradient():
    """dy = 0 on a fresh optimiser: the weights keep their bits, m and v are exactly zero, t = 1.  dy = 0 after two real steps: the
    weights move by the momentum alone and match adam_f32 (every element's gradient is exactly zero).  Measured (one MI355X, one
    run): under 0.0001 of the bound."""
    g, p = make()
    z, _ = GR.draw(100, 4, 128)
    zero = np.zeros((4, 28, 28, 1), np.float32)
    w0 = g.get_weights()
    g.generator_step(z, zero)
    w1 = g.get_weights()
    m, v, t = g.generator_adam_state()
    assert t == 1
    for n in GR.NAMES:
        assert np.array_equal(w0[n], w1[n]) and not m[n].any() and not v[n].any(), n
    g.generator_adam_reset()
    for k in range(2):
        zk, dyk = GR.draw(100 + k, 4, 128)
        g.generator_step(zk, dyk)
    w0, w1 = step_and_check(g, z, zero, 1e-4, 0.5, 0.9, "zero gradient after two steps")
    assert all(not np.array_equal(w0[n], w1[n]) for n in GR.NAMES)
    g.close()


def test_refused_betas_and_widths():
    """beta = 1.0 and a negative beta are refused with -1 and change neither the counter nor the weights; LATENT_DIM 96 (no multiple
    of 32 for the weight-gradient tiles) never reaches dg_gen_param_gradient: dg_create refuses it first, with an error code."""
    import ctypes as C
    import torch
    from defensegan_amd import _native
    lib = _native.load()
    g, p = make()
    z, dy = GR.draw(100, 4, 128)
    g.generator_step(z, dy)
    w0 = g.get_weights()
    zz, dd = g._to_device(z), g._to_device(dy)
    s = torch.cuda.current_stream(zz.device).cuda_stream
    for b1, b2 in ((1.0, 0.9), (0.5, 1.0), (-0.1, 0.9), (0.5, -0.5), (float("nan"), 0.9)):
        assert lib.dg_gen_step(g._handle, zz.data_ptr(), dd.data_ptr(), 4, 1e-4, b1, b2, s) == -1
        assert b"outside [0, 1)" in lib.dg_last_error()
    assert g.generator_adam_state()[2] == 1
    w1 = g.get_weights()
    assert all(np.array_equal(w0[n], w1[n]) for n in GR.NAMES)
    g.close()
    h = C.c_void_p()
    assert lib.dg_create(0, 96, 64, 0, 0, C.byref(h)) == -1
    assert b"multiple of 64" in lib.dg_last_error() and not h.value
