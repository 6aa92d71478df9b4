"""The classifier cases with anisotropic geometry and unusual layer orders, shared by tests/test_geometry_cpu.py (which asserts
the properties they were chosen for) and tests/test_gpu_geometry.py (which compares the device with float64 on them).  The zoo of
network_builder.MODELS has square images, kernels and strides, folds every ReLU into its producer and always ends in Softmax;
these four do not.  Layers are written as tests/support/train_reference.describe gives them.

    G1  9 x 14 x 3: (3,5)/(2,3) SAME with an odd column pad (1 before, 2 after), (2,1)/(1,2) VALID, Dropout between the Linears
    G2  12 x 8 x 2: (2,3)/(3,2) VALID whose row stride exceeds the kernel (input rows 2, 5, 8, 11 and column 7 are read by no
        output), a second ReLU that cannot fold and runs the stand-alone kernels, no Softmax
    G3  5 x 7 x 1: Dropout on the input, a (7,2)/(1,3) SAME kernel taller than the image (row pads 3 / 3, column pads 0 / 1)
    G4  6 x 10 x 2: a ReLU as the first layer, 66 output channels (a ragged last N-tile of the weight gradient), a ReLU that folds
        into its convolution across a Dropout, a (3,3)/(2,2) VALID convolution with M = 594 (a ragged last M-tile), N = 2 < 4 and
        no ReLU after it
"""
import numpy as np

RELU, FLATTEN, SOFTMAX = ("relu",), ("flatten",), ("softmax",)

CASES = {
    "G1": ((9, 14, 3), [("conv", 5, (3, 5), (2, 3), "SAME"), RELU, ("conv", 6, (2, 1), (1, 2), "VALID"), RELU, FLATTEN,
                        ("linear", 7), RELU, ("dropout", 0.5), ("linear", 3), SOFTMAX]),
    "G2": ((12, 8, 2), [("conv", 4, (2, 3), (3, 2), "VALID"), RELU, RELU, FLATTEN, ("linear", 5)]),
    "G3": ((5, 7, 1), [("dropout", 0.8), ("conv", 3, (7, 2), (1, 3), "SAME"), RELU, ("dropout", 0.5), FLATTEN, ("linear", 4), SOFTMAX]),
    "G4": ((6, 10, 2), [RELU, ("conv", 66, (1, 4), (2, 1), "SAME"), ("dropout", 0.5), RELU, ("conv", 2, (3, 3), (2, 2), "VALID"), FLATTEN,
                        ("linear", 65), RELU, ("linear", 6), SOFTMAX]),
}
NAMES = tuple(sorted(CASES))
BATCH_SIZES = (1, 5, 11)
BIAS_WIDTH = 0.1


def input_shape(name):
    return CASES[name][0]


def layers(name):
    return list(CASES[name][1])


def model(name):
    """The case as a network_builder.MLP (no device is touched before its first use)."""
    from defensegan_amd import network_builder as nb
    out = []
    for L in layers(name):
        if L[0] == "conv":
            out.append(nb.Conv2D(L[1], L[2], L[3], L[4]))
        elif L[0] == "linear":
            out.append(nb.Linear(L[1]))
        elif L[0] == "dropout":
            out.append(nb.Dropout(L[1]))
        else:
            out.append({"relu": nb.ReLU, "flatten": nb.Flatten, "softmax": nb.Softmax}[L[0]]())
    return nb.MLP(out, (None,) + input_shape(name))


def params(name):
    """MLP.init_like_reference's weights (its own code, with the installation on the device left out, so that the CPU tests can
    call it) and biases uniform in +-BIAS_WIDTH, float32."""
    m = model(name)
    m.set_weights = lambda p: None
    seed = sum(map(ord, name))
    rs = np.random.RandomState(seed + 1)
    return [(W, rs.uniform(-BIAS_WIDTH, BIAS_WIDTH, size=b.shape).astype(np.float32)) for W, b in m.init_like_reference(seed=seed)]


def images(name, n, rs):
    """n inputs uniform in [-1, 1]."""
    return rs.uniform(-1, 1, (n,) + input_shape(name)).astype(np.float32)
