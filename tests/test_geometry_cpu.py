"""The table of tests/support/geometry_cases.py keeps the properties its cases were chosen for, and the two float64 references
that tests/test_gpu_geometry.py compares the device with (oracle/classifier_oracle.py, written with NumPy loops, and
tests/support/train_reference.py, torch autograd) agree on every case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from defensegan_amd import network_builder as nb
from oracle import classifier_oracle as CO
from tests.support import geometry_cases as G
from tests.support import train_reference as R

# per convolution, worked by hand: (output H, W, C), (pad top, bottom), (pad left, right)
CONVS = {
    "G1": [((5, 5, 5), (1, 1), (1, 2)), ((4, 3, 6), (0, 0), (0, 0))],
    "G2": [((4, 3, 4), (0, 0), (0, 0))],
    "G3": [((5, 3, 3), (3, 3), (0, 1))],
    "G4": [((3, 10, 66), (0, 0), (1, 2)), ((1, 4, 2), (0, 0), (0, 0))],
}
FLAT = {"G1": 72, "G2": 48, "G3": 45, "G4": 8}
CLASSES = {"G1": 3, "G2": 5, "G3": 4, "G4": 6}
# per Conv2D / Linear layer: (kind, M, N, output positions) of the weight gradient's GEMM
WGRAD = {
    "G1": [("conv", 45, 5, 25), ("conv", 10, 6, 12), ("linear", 72, 7, 1), ("linear", 7, 3, 1)],
    "G2": [("conv", 12, 4, 12), ("linear", 48, 5, 1)],
    "G3": [("conv", 14, 3, 15), ("linear", 45, 4, 1)],
    "G4": [("conv", 8, 66, 30), ("conv", 594, 2, 4), ("linear", 8, 65, 1), ("linear", 65, 6, 1)],
}


def test_the_table_is_what_the_builders_describe():
    assert G.NAMES == ("G1", "G2", "G3", "G4") and G.BATCH_SIZES == (1, 5, 11)
    for name in G.NAMES:
        m = G.model(name)
        assert R.describe(m) == G.layers(name)
        assert tuple(m.input_shape[1:]) == G.input_shape(name)
        shapes = [(W.shape, b.shape) for W, b in G.params(name)]
        assert shapes == m.param_shapes()
        assert all(W.dtype == np.float32 and b.dtype == np.float32 and np.abs(b).max() <= G.BIAS_WIDTH and b.any() for W, b in G.params(name))


def test_output_shapes_and_pads_worked_by_hand():
    for name in G.NAMES:
        shape, convs = G.input_shape(name), []
        for L in G.layers(name):
            if L[0] != "conv":
                continue
            (kh, kw), (sh, sw) = L[2], L[3]
            if L[4] == "SAME":
                oh, pt, pb = CO.same_padding(shape[0], kh, sh)
                ow, pl, pr = CO.same_padding(shape[1], kw, sw)
            else:
                oh, ow, pt, pb, pl, pr = (shape[0] - kh) // sh + 1, (shape[1] - kw) // sw + 1, 0, 0, 0, 0
            assert (oh, ow, L[1]) == nb.conv_output_shape(shape, nb.Conv2D(L[1], L[2], L[3], L[4]))
            shape = (oh, ow, L[1])
            convs.append((shape, (pt, pb), (pl, pr)))
        assert convs == CONVS[name], name
        assert int(np.prod(shape)) == FLAT[name]
        assert R.wgrad_shapes(G.layers(name), G.input_shape(name)) == WGRAD[name]
        assert G.layers(name)[-1 if G.layers(name)[-1][0] != "softmax" else -2] == ("linear", CLASSES[name])
    # what the cases are there for: an odd pad on one axis only with the extra column after; a kernel taller than the image
    assert CONVS["G1"][0][1:] == ((1, 1), (1, 2)) and CONVS["G3"][0][1] == (3, 3) and G.layers("G3")[1][2][0] > G.input_shape("G3")[0]
    # every kernel or stride pair of a first convolution is anisotropic, and no case has a square image
    for name in G.NAMES:
        first = [L for L in G.layers(name) if L[0] == "conv"][0]
        assert first[2][0] != first[2][1] and first[3][0] != first[3][1] and G.input_shape(name)[0] != G.input_shape(name)[1]


def test_layer_orders_the_zoo_does_not_have():
    kinds = {name: [L[0] for L in G.layers(name)] for name in G.NAMES}
    assert kinds["G2"][1:3] == ["relu", "relu"] and "softmax" not in kinds["G2"]          # a ReLU that cannot fold; no Softmax
    assert kinds["G3"][0] == "dropout" and kinds["G3"][3] == "dropout"                    # Dropout on the input and before Flatten
    assert kinds["G4"][0] == "relu"                                                       # a ReLU with no producer
    assert kinds["G4"][1:4] == ["conv", "dropout", "relu"]                                # the fold reaches across a Dropout
    assert kinds["G4"][4:6] == ["conv", "flatten"]                                        # a convolution without a ReLU
    assert all(kinds[n][-1] == "softmax" for n in ("G1", "G3", "G4"))


def unread(name):
    """(rows, columns) of the input that no output of the first layer reads: where the input gradient of an all-ones kernel under
    an all-ones output gradient is zero."""
    L = G.layers(name)[0]
    H, W, Cc = G.input_shape(name)
    g = np.ones((1,) + nb.conv_output_shape((H, W, Cc), nb.Conv2D(L[1], L[2], L[3], L[4])))
    dx = CO.conv2d_backward_input(g, np.ones(L[2] + (Cc, L[1])), (1, H, W, Cc), L[3], L[4])[0].sum(axis=2)
    return [r for r in range(H) if not dx[r].any()], [c for c in range(W) if not dx[:, c].any()]


def test_g2_leaves_four_rows_and_a_column_unread():
    assert unread("G2") == ([2, 5, 8, 11], [7])
    assert unread("G1") == ([], [])


def test_regimes_of_the_weight_gradient_reached():
    reached = {}
    for name in G.NAMES:
        for B in G.BATCH_SIZES:
            for i, (kind, M, N, pos) in enumerate(WGRAD[name]):
                reached[name, B, i] = R.regimes(kind, M, N, pos, B)
    # at B = 11 every first convolution has at least two slots, and their length is no multiple of the chunk of 16
    plans = {name: R.slot_plan(WGRAD[name][0][1], WGRAD[name][0][2], 11 * WGRAD[name][0][3]) for name in G.NAMES}
    assert plans == {"G1": (1, 4, 69, 4), "G2": (1, 2, 66, 2), "G3": (1, 2, 83, 2), "G4": (2, 5, 66, 5)}
    for name in G.NAMES:
        assert "slot start off a chunk boundary" in reached[name, 11, 0]
    assert "ragged last N-tile" in reached["G4", 5, 0] and "ragged last N-tile" in reached["G4", 5, 2]      # N = 66, 65
    assert {"ragged last M-tile", "N < 4"} <= reached["G4", 5, 1]                                           # M = 594, N = 2
    assert "N < 4" in reached["G1", 5, 3] and "N < 4" in reached["G3", 5, 0]
    # a convolution whose whole reduction is shorter than one chunk, and every last Linear at every batch size
    assert "K < 16" in reached["G2", 1, 0] and "K < 16" in reached["G4", 1, 1]
    assert all("K < 16" in reached[name, B, len(WGRAD[name]) - 1] for name in G.NAMES for B in G.BATCH_SIZES)


@pytest.mark.parametrize("name", G.NAMES)
def test_the_two_float64_references_agree(name):
    """classifier_oracle.forward / input_gradient against train_reference.logits and autograd, at evaluation (Dropout the
    identity), with labels and with the model's own argmax."""
    layers = G.layers(name)
    p64 = [(W.astype(np.float64), b.astype(np.float64)) for W, b in G.params(name)]
    rs = np.random.RandomState(7)
    x = G.images(name, 5, rs).astype(np.float64)
    labels = rs.randint(0, CLASSES[name], 5)
    lo, po = CO.forward(layers, p64, x)
    xt = torch.tensor(x, requires_grad=True)
    z = R.logits(layers, R.as_params(p64), xt)
    assert lo.shape == (5, CLASSES[name])
    np.testing.assert_allclose(lo, z.detach().numpy(), rtol=0, atol=1e-12)
    if layers[-1][0] == "softmax":
        np.testing.assert_allclose(po, torch.softmax(z, dim=1).detach().numpy(), rtol=0, atol=1e-12)
    else:
        assert po is lo or np.array_equal(po, lo)
    for lab in (labels, None):
        y = torch.as_tensor(labels if lab is not None else lo.argmax(axis=1), dtype=torch.long)
        (want,) = torch.autograd.grad(F.cross_entropy(z, y, reduction="sum"), xt, retain_graph=True)
        got = CO.input_gradient(layers, p64, x, lab)
        assert np.abs(want.numpy()).max() > 1e-3
        np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12)
