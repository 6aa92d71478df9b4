"""-m "not gpu": the case table of tests/support/critic_cases.py, decided on the float64 reference alone -- the reference agrees with
central differences and the closed form with autograd's double backward on every layout of the table (ReLU, hidden Linear, Flatten
first, zero norms); every case reaches what its row claims; the recorded draws are the first the reference accepts; the weight-
gradient regimes the critic's two calls per layer reach; and what float32 alone costs each case against the project's 1e-4 bound."""
import numpy as np
import pytest

from tests.support import critic_cases as T
from tests.support import critic_reference as R
from tests.support import train_reference as TR

NAMES = list(T.CASES)
CPU_B = {"many_images": 33}                  # the reference's own checks need no 65537 images


def _cpu_batches(name):
    """[(B, layers, params, batch)]: the recorded draw of every batch size (many_images: the first accepted draw at B = 33)."""
    case = T.CASES[name]
    layers, params = T.reference_of(case)
    if name in CPU_B:
        return [(CPU_B[name], layers, params, T.search_batch(case, CPU_B[name])[0])]
    return [(B, layers, params, T.case_batch(case, B)) for B in case.Bs]


def _wide_margin_batch(name):
    """A draw of the case whose activation inputs stay 1e-4 from zero, as the central-difference steps need (they cross no kink)."""
    case = T.CASES[name]
    B = CPU_B.get(name, case.Bs[-1])
    layers, params = T.reference_of(case)
    batch, _ = T.search_batch(case, B, min_margin=1e-4)
    return case, layers, [(W.astype(np.float64), b.astype(np.float64)) for W, b in params], batch


@pytest.mark.parametrize("name", NAMES)
def test_reference_gradient_against_central_differences(name):
    """tests/test_critic_cpu.py's form and bound, on every layout.  At a zero norm the cost has a kink in the zeroed weights (s = c |h|);
    the central difference sees its even part, slope 0, which is the value the project defines there."""
    case, layers, params, batch = _wide_margin_batch(name)
    assert R.margin(layers, params, *batch) > 1e-4
    for axes in case.axes:
        _, grads, _ = R.param_gradient(layers, params, *batch, lam=10.0, axes=axes)
        rs, h = np.random.RandomState(5), 1e-6
        for i, (pair, gpair) in enumerate(zip(params, grads)):
            for k in range(2):
                for _ in range(4):
                    idx = tuple(rs.randint(0, n) for n in pair[k].shape)
                    vals = []
                    for sgn in (1, -1):
                        q = [[W.copy(), b.copy()] for W, b in params]
                        q[i][k][idx] += sgn * h
                        vals.append(R.cost_of(layers, [tuple(t) for t in q], *batch, lam=10.0, axes=axes))
                    fd = (vals[0] - vals[1]) / (2 * h)
                    assert abs(fd - gpair[k][idx]) <= 1e-6 * max(1.0, np.abs(gpair[k]).max()), (name, axes, i, k, idx, fd, gpair[k][idx])


@pytest.mark.parametrize("name", NAMES)
def test_the_derivation_equals_autograd(name):
    """The closed form the device uses (frozen slopes, bias-free tangent pass, wgrad(u_{j-1}, a_j)) against the double backward, with
    ReLU slopes 1 / 0, through hidden Linear layers, and with v = 0 at a zero norm."""
    for B, layers, params, batch in _cpu_batches(name):
        for axes in T.CASES[name].axes:
            _, full, _ = R.param_gradient(layers, params, *batch, lam=10.0, axes=axes)
            _, wass, _ = R.param_gradient(layers, params, *batch, lam=0.0, axes=axes)
            derived = R.derived_gradient(layers, params, *batch, lam=10.0, axes=axes)
            for (fW, fb), (wW, wb), (dW, db) in zip(full, wass, derived):
                assert np.abs(fW - wW - dW).max() <= 1e-12 * max(1.0, np.abs(fW).max()), (name, B, axes)
                assert np.abs(fb - wb).max() == 0.0 and not db.any()


@pytest.mark.parametrize("name", NAMES)
def test_recorded_draw_is_the_first_the_reference_accepts(name):
    case = T.CASES[name]
    layers, params = T.reference_of(case)
    for B in case.Bs:
        batch, attempt = T.search_batch(case, B)
        assert attempt == case.attempts[B], "%s B=%d: the first accepted draw is attempt %d" % (name, B, attempt)
        for a, b in zip(batch, T.case_batch(case, B)):
            np.testing.assert_array_equal(a, b)
        m = R.margin(layers, params, *batch)
        conds = [max(R.conditioning(layers, params, *batch, lam=10.0, axes=a)) for a in case.axes]
        print("%s B=%d: attempt %d, margin %.3g, conditioning %s" % (name, B, attempt, m, ", ".join("%.3g" % v for v in conds)))
        assert m >= 1e-6 and max(conds) <= 10.0


def _first_layer_pre(layers, params, x):
    import torch
    pre = []
    R.forward(layers, R.as_params(params), torch.as_tensor(np.asarray(x, np.float64)), pre=pre)
    return pre[0].numpy()


def test_zero_columns_has_exact_zero_slopes_and_no_penalty_gradient_there():
    case = T.CASES["zero_columns"]
    (B, layers, params, batch), = _cpu_batches("zero_columns")
    assert not params[0][0][:, :, 1, :].any() and params[0][0][:, :, 0, :].all()
    terms, grads, s = R.param_gradient(layers, params, *batch, axes=0)
    assert s.shape == (B, 6, 2) and (s[:, :, 1] == 0.0).all() and s[:, :, 0].min() > 1e-3
    _, _, s1 = R.param_gradient(layers, params, *batch, axes=1)
    assert s1.min() > 1e-3
    assert all(np.isfinite(g).all() for pair in grads for g in pair) and np.isfinite(terms).all()
    # the zeroed slice's rows: the PENALTY's gradient there is exactly 0 (its input v is 0 in channel 1).  The Wasserstein term's is
    # not -- d w / dK[:, :, 1, :] is a sum of inputs times a_1, whatever K holds -- so the cost's rows equal the lambda = 0 rows, bit
    # for bit, and are no zeros themselves.
    derived = R.derived_gradient(layers, params, *batch, axes=0)
    assert not derived[0][0][:, :, 1, :].any() and derived[0][0][:, :, 0, :].any()
    _, wass, _ = R.param_gradient(layers, params, *batch, lam=0.0, axes=0)
    np.testing.assert_array_equal(grads[0][0][:, :, 1, :], wass[0][0][:, :, 1, :])
    assert np.abs(grads[0][0][:, :, 0, :] - wass[0][0][:, :, 0, :]).max() > 1e-3


def test_dead_image_has_one_exact_zero_norm_and_live_neighbours():
    (B, layers, params, batch), = _cpu_batches("dead_image")
    assert (params[0][1] <= -0.05).all() and (params[0][1] >= -0.1).all()
    assert not batch[0][T.DEAD].any() and not batch[1][T.DEAD].any()
    others = [b for b in range(B) if b != T.DEAD]
    for axes in (0, 1):
        terms, grads, s = R.param_gradient(layers, params, *batch, axes=axes)
        assert (s[T.DEAD] == 0.0).all() and s[others].min() > 1e-3, (axes, s[others].min())
        assert all(np.isfinite(g).all() for pair in grads for g in pair) and np.isfinite(terms).all()
    xhat = batch[0] + batch[2].reshape(-1, 1, 1, 1) * (batch[1] - batch[0])
    pre = _first_layer_pre(layers, params, xhat)
    assert (pre[T.DEAD] < 0).all()
    active = float((pre[others] > 0).mean())
    print("dead_image: %.3f of the other images' first-layer units are active" % active)
    assert active >= 1.0 / 3.0


def test_wide_has_more_than_256_columns_and_h1_has_one_row():
    assert T.CASES["wide"].shape[1] * T.CASES["wide"].shape[2] == 260 > 256
    assert T.CASES["flat_h1"].shape[0] == 1
    (B, layers, params, batch), = _cpu_batches("flat_h1")
    import torch
    xhat = torch.tensor((batch[0] + batch[2].reshape(-1, 1, 1, 1) * (batch[1] - batch[0])).astype(np.float64), requires_grad=True)
    (g,) = torch.autograd.grad(R.forward(layers, R.as_params(params), xhat).sum(), xhat)
    _, _, s = R.param_gradient(layers, params, *batch, axes=0)
    np.testing.assert_array_equal(s, np.abs(g.numpy()[:, 0]))                     # H = 1: s = |g|
    assert T.CASES["many_images"].Bs == (65537,) and 65537 > 65536                  # one image past the norm kernels' grid cap


# ---------------------------------------------------------------------- the weight-gradient regimes of the critic's two calls
# What the table (with tests/test_gpu_critic.py's layouts) does not reach, and why:
UNREACHED = {
    # a layer of more than 64 outputs that is no multiple of 64: the table's widest layer has 9, the MNIST critic's widths are
    # multiples of 64 where they pass it; tests/test_gpu_train_shapes.py covers the regime for the same kernel
    "ragged last N-tile",
}
NAMED = ("256-slot cap", "K < 16", "N < 4", "slot start off a chunk boundary", "linear layer with >= 2 slots of >= 2 chunks")


def _reached(layers, shape, Bs, table):
    for B in Bs:
        for j, (kind, M, N, pos) in enumerate(TR.wgrad_shapes(layers, shape)):
            for which, n in (("w", 2 * B), ("t", B)):
                table.setdefault((j, which, B), set()).update(TR.regimes(kind, M, N, pos, n))


def test_regime_table():
    union, new = set(), set()
    for name, case in T.CASES.items():
        layers, _ = T.reference_of(case)
        table = {}
        _reached(layers, case.shape, case.Bs, table)
        for (j, which, B), hit in sorted(table.items()):
            print("%s B=%d layer %d %s: %s" % (name, B, j, "Wasserstein (2B)" if which == "w" else "penalty (B)", ", ".join(sorted(hit)) or "-"))
            new |= hit
    union |= new
    for layers, shape, Bs in T.existing_layouts():
        table = {}
        _reached(layers, shape, Bs, table)
        for hit in table.values():
            union |= hit
    assert set(NAMED) <= union
    assert set(TR.REGIMES) - union == UNREACHED, (set(TR.REGIMES) - union, UNREACHED)
    layers, _ = T.reference_of(T.CASES["many_images"])
    table = {}
    _reached(layers, (2, 2, 1), (65537,), table)
    assert all("256-slot cap" in table[(j, which, 65537)] for j in (0, 1) for which in "wt")


# ---------------------------------------------------------------------- what the number format alone costs
@pytest.mark.parametrize("name", NAMES)
def test_float32_headroom(name):
    """param_gradient in float32 against float64 at the GPU tests' own batch (many_images: all 65537 images, where each slot sums
    about 512 float32 terms).  The worst gradient-tensor error as a fraction of the 1e-4 bound stays under a quarter, so three
    quarters of every bound are left to the device's order of summation."""
    case = T.CASES[name]
    layers, params = T.reference_of(case)
    worst = 0.0
    for B in case.Bs:
        batch = T.case_batch(case, B)
        for axes in case.axes:
            t64, g64, s64 = R.param_gradient(layers, params, *batch, axes=axes)
            t32, g32, s32 = R.param_gradient(layers, params, *batch, axes=axes, dtype=np.float32)
            fr = [np.abs(a - b).max() / (1e-4 * np.abs(b).max()) for i, (p32, p64) in enumerate(zip(g32, g64))
                  for k, (a, b) in enumerate(zip(p32, p64)) if not (i == len(g64) - 1 and k == 1)]
            fs = np.abs(s32 - s64).max() / (1e-4 * np.abs(s64).max())
            ft = max(abs(a - b) / (1e-5 * abs(b)) for a, b in zip(t32, t64))
            print("%s B=%d axes %d: float32 uses %.3f of the gradient bound, %.3f of the slope bound, %.3f of the cost-term bound"
                  % (name, B, axes, max(fr), fs, ft))
            worst = max(worst, max(fr))
    print("%s: float32 headroom %.3f of the 1e-4 gradient bound (recorded: %.3f)" % (name, worst, T.HEADROOM[name]))
    assert worst <= 0.25 and T.HEADROOM[name] <= 0.25


# ---------------------------------------------------------------------- the LeakyReLU classifier of tests/test_gpu_critic_shapes.py
def test_leakyrelu_classifier_references_agree_and_its_inputs_are_the_first_safe_draw():
    """The leakyrelu branches added to the float64 references: the oracle's hand-written input gradient equals autograd through
    train_reference.logits; a tie at 0 takes the slope 0.2 in both; the recorded inputs are the first draw 1e-6 from every kink, and
    the teacher-forced PGD run leaves at most 1 % of the pixels undecided at every iterate."""
    import torch
    from oracle import classifier_oracle as CO
    from tests.support import bpda_reference as B
    from tests.support import pgd_reference as P
    m, params, layers = T.leaky_classifier()
    first = next(a for a in range(20) if TR.relu_margins(layers, params, T.leaky_inputs(a)[0]).min() >= 1e-6)
    assert first == T.LEAKY_ATTEMPT
    x, y = T.leaky_inputs(first)
    pre = []
    TR.logits(layers, TR.as_params(params), torch.as_tensor(x.astype(np.float64)), pre=pre)
    assert len(pre) == 2 and all(0.2 < float((h < 0).double().mean()) < 0.8 for h in pre)         # both slopes are in play
    cp = [(W.astype(np.float64), b.astype(np.float64)) for W, b in params]
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    z = TR.logits(layers, TR.as_params(params), xt)
    (g,) = torch.autograd.grad(torch.nn.functional.cross_entropy(z, torch.as_tensor(y, dtype=torch.long), reduction="sum"), xt)
    np.testing.assert_allclose(CO.forward(B.layers_of(m), cp, x.astype(np.float64))[0], z.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(CO.input_gradient(B.layers_of(m), cp, x.astype(np.float64), y), g.numpy(), rtol=1e-10, atol=1e-14)
    # the tie: a zero image under zero biases gives pre-activations of exactly 0, whose slope is 0.2 on both references
    zp = [(W.astype(np.float64), np.zeros_like(b, np.float64)) for W, b in params]
    x0 = torch.zeros(1, 8, 8, 1, dtype=torch.float64, requires_grad=True)
    (g0,) = torch.autograd.grad(TR.logits(layers, TR.as_params(zp), x0)[0, 1], x0)
    assert np.abs(g0.numpy()).max() > 0                   # 0.2 * 0.2 of the linear map, not 0
    g1 = CO.input_gradient(B.layers_of(m), zp, np.zeros((1, 8, 8, 1)), np.array([1]))
    xs = torch.zeros(1, 8, 8, 1, dtype=torch.float64, requires_grad=True)
    (gs,) = torch.autograd.grad(torch.nn.functional.cross_entropy(TR.logits(layers, TR.as_params(zp), xs), torch.tensor([1]), reduction="sum"), xs)
    np.testing.assert_allclose(g1, gs.numpy(), rtol=1e-10, atol=1e-14)
    ref = P.pgd(P.classifier_ops(B.layers_of(m), params, y), x, y, 0.3, 0.05, 3, 0.0, 1.0)
    for k in range(3):
        gk = ref["grads"][k]
        assert (np.abs(gk) > 1e-4 * np.abs(gk).max()).mean() >= 0.99
