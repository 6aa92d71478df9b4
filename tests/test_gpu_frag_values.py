"""-m gpu: the fragment-order forward path (option frag_path = 1: one workgroup per job, K split over its waves; 2: persistent
waves, no K split -- dg_fgemm.hip, the fragment-order Linear of dg_linear.hip, the gate bits the backward GEMMs of dg_gemm.hip
consume, unfrag_kernel) value for value against tests/support/path_reference.py (float64): checks (1) - (5) of
tests/test_gpu_path_values.py, unchanged -- layer by layer, per tap class, every row, 2e-6 forward, 1e-5 backward and loss, the
numpy float32 yardstick rule as it stands there -- with that module's weights and input recipe.

Shapes (tests/support/frag_cases.py; tests/test_frag_lds_cpu.py holds the table against the planner): MNIST and CelebA at NET_DIM
64 with 1, 33 and 47 rows (padded last 32-row block, partial last wave tile, two row blocks) and MNIST with 129 rows (5 row
blocks: last jobs with fewer M blocks than a full job at every K split).  (K split, output form) pairs run by frag_path = 1:
MNIST (4, fragment order) (2, fragment order) (2, NHWC) (1, NHWC); CelebA adds (1, fragment order) and repeats (4 | 2, fragment
order) and (1, NHWC).  (4, NHWC) is reached by no generator the path accepts (frag_cases.UNREACHED).  frag_path = 2 runs K split 1
in both output forms on every layer.

What is read: under frag_path "act<d>" is always the forward activation, converted from fragment order by unfrag_kernel (so every
forward check also checks that kernel and the fragment-order Linear output); the gradient a backward pass leaves is read through
"raw<d>", the gate words through "gate<d>", the count of dg_fgemm.hip launches through "frag_launches" (dg_debug_read).

Every handle is made with two_streams = 0: concurrent row groups switch the path off (dg_engine.cpp frag_active), and CelebA's
default is two_streams = auto -- with it frag_path changes nothing, which the launch count below would report.

Beyond (1) - (5), per case:
 * the fragment-order kernels RAN: the forward-only call and the all-outputs call each add at least one dg_fgemm.hip launch per
   GEMM layer to the handle's count -- a case that stayed on dg_gemm.hip fails;
 * gate bits: bit f % 32 of word f / 32 of "gate<d>" equals (act<d> > 0), exactly, on all real rows, every layer that has gates;
 * the backward pass leaves the fragment-order activations alone (act<d> reads the same bits before and after).
Per shape: frag_path 1 and 2 agree BIT FOR BIT wherever the K split is 1 and the two runs fed the layer the same bits: every output
(row, position) of a class with K split 1 whose whole input window is bit-identical between the runs.  The first deconv (K = 256:
the classes of 1 and 2 taps) reads the output of the same Linear kernel, so all of those are compared on every row, and the count
is asserted; deeper layers (K = 128: up to 4 taps; K = 64: all) are compared where their windows happen to hold the same bits,
and the test prints how many elements that was.
NET_DIM 128 (first deconv K = 512) falls back: no dg_fgemm.hip launch, everything bit-identical to frag_path = 0.
Determinism: 50 generate calls on one handle at 512 MNIST rows, frag_path = 1: act2 and y of every call equal the first call's
bit for bit.  This pins the documented claim; it does not reliably catch an LDS race and is not meant to (the layout itself is
checked without a GPU, tests/test_frag_lds_cpu.py).

Measured on MI355X, worst case of each group over all 14 runs (device error | float32 yardstick error | bound | bound / error; all
relative to max|float64| of the class):
  (1) forward GEMM layers, frag_path = 1   9.50e-07 | 1.05e-07 | 2e-06    | x2.1   CelebA 47 rows, act2 class 11 (MNIST: 8.66e-07, x2.3,
                                                                                   129 rows, act2 class 7): the K split shortens the chains
  (1) forward GEMM layers, frag_path = 2   1.57e-06 | 1.18e-07 | 2e-06    | x1.3   CelebA 47 rows, act1 class 1 (MNIST: 1.44e-06, x1.4, 1 row,
                                                                                   act1 class 0): one chain of K = 256 x 9 taps, the default
                                                                                   path's figure
  (1) y, MNIST                             1.80e-07 | 1.08e-07 | 2e-06    | x11.1  47 rows, frag_path = 1, class 4
  (1) y, CelebA                            1.72e-06 | 4.98e-07 | 2e-06    | x1.2   1 row, frag_path = 2, class 0 (the tail kernel of the default
                                                                                   path on this run's act3; tanh saturates: three classes of the
                                                                                   33- and 47-row runs take their bound from the yardstick,
                                                                                   2.27e-06 .. 2.82e-06, device 1.37e-06 .. 1.45e-06)
  (2) gates                                at most 1 of 413952 differs from float64 (MNIST 33 rows, frag_path = 2, act2), |pre| there 1.3e-08
  (3) backward GEMM layers                 2.21e-06 | 2.23e-07 | 1e-05    | x4.5   CelebA 47 rows, frag_path = 1, grad2 class 4 (MNIST: 1.32e-06, x7.6)
  (3) tail backward                        3.85e-07 | 2.55e-07 | 1e-05    | x26.0  CelebA 47 rows, frag_path = 2 (MNIST: 2.8e-07, x35.7)
  (3) dz from da0                          2.56e-07 | 2.72e-07 | 1e-05    | x39.1  MNIST 47 rows, frag_path = 2
  (4) dz end to end                        7.98e-07 of 1e-05 (CelebA 33 rows, frag_path = 2); loss 1.93e-07 of 1e-05 (CelebA 33 rows)
  (5) dz-only call                         no NaN; every figure equals the all-outputs call's
Gate words: 0 of up to 25284 (MNIST) / 24064 (CelebA) words per layer differ from (act > 0) in every run.  Launch counts: exactly one
dg_fgemm.hip launch per GEMM layer and call.  Elements compared bit for bit between the two forms: act1 9 (MNIST) / 11 (CelebA)
positions x 128 channels on every row; deeper layers e.g. 27072 (MNIST 47 rows, act2), 39104 and 63168 (CelebA 47 rows, act2, act3).
No class of a GEMM layer exceeded the project's figures, so no bound was taken from an emulation of the K-split tree.  Every case
runs in under a second (the 50-call determinism test: 0.2 s)."""

import numpy as np
import pytest

from tests.support import frag_cases as FC
from tests.support import path_reference as PR
from tests.test_gpu_path_values import _gan, _inputs, _weights

pytestmark = pytest.mark.gpu

_MEMO, _REC, _ACTS = {}, {}, {}


def _shape(arch, p, d, N):
    if d == 0:
        return (N, 4, 4, p["Generator.Input.W"].shape[1] // 16)
    name, _, e, _, _ = PR.O._arch_layers(arch)[d - 1]
    return (N, e, e, p[name + ".Filters"].shape[2])


def _read(gan, what, n):
    t = gan.debug_read(what, n)
    assert t.numel() == n, (what, t.numel(), n)
    return t.cpu().numpy()


def _read_all(gan, arch, p, N, prefix):
    return [_read(gan, "%s%d" % (prefix, d), int(np.prod(_shape(arch, p, d, N)))).reshape(_shape(arch, p, d, N)) for d in range(PR.n_act(arch))]


def _launches(gan):
    return int(_read(gan, "frag_launches", 1)[0])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _record(gan, arch, p, z, x, R, frag_runs):
    """The record of path_reference.run_checks, read the way the fragment-order path needs it, plus rec["extra"]: the launch counts,
    the gate words and the activations as they read after the backward."""
    import torch
    N, nd = len(z), PR.n_act(arch)
    rec = {"z": z, "x": x, "R": R}
    n0 = _launches(gan)
    rec["y_generate"] = np.asarray(gan.generate(z))
    n1 = _launches(gan)
    rec["acts"] = _read_all(gan, arch, p, N, "act")
    gates = []
    if frag_runs:
        for d in range(nd - 1):
            words = int(np.prod(_shape(arch, p, d, N)[1:])) // 32
            gates.append(_bits(_read(gan, "gate%d" % d, N * words)).reshape(N, words))
    rec["y"], rec["loss"], rec["dz"] = (np.asarray(v) for v in gan.loss_grad(x, z))
    n2 = _launches(gan)
    rec["grads"] = _read_all(gan, arch, p, N, "raw")
    acts_after = _read_all(gan, arch, p, N, "act")[:nd - 1] if frag_runs else []
    xd, zd = torch.as_tensor(x).cuda(), torch.as_tensor(z).cuda()
    dz = torch.full_like(zd, float("nan"))
    gan._check(gan._lib().dg_loss_grad(gan._handle, xd.data_ptr(), zd.data_ptr(), N // R, R, None, None, dz.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    rec["only"] = {"dz": dz.cpu().numpy(), "grads": _read_all(gan, arch, p, N, "raw")}
    rec["extra"] = {"launches": (n1 - n0, n2 - n1, _launches(gan) - n2), "gates": gates, "acts_after": acts_after}
    return rec


def _memo(key):
    if key not in _MEMO:
        _MEMO.clear()
        _MEMO[key] = PR.Memo()
    return _MEMO[key]


def _rec_of(case, frag):
    """One record per (shape, frag_path); only the last shape's records are kept whole, of the others the forward activations
    (_ACTS: what the comparison of the two forms needs, so that it launches nothing again)."""
    if (case, frag) not in _REC:
        for k in [k for k in _REC if k[0] != case]:
            del _REC[k]
        arch, net_dim, rows = case
        p = _weights(arch, net_dim)
        z, x, R = _inputs(arch, rows)
        _REC[(case, frag)] = _record(_gan(arch, net_dim, {"two_streams": 0, "frag_path": frag}), arch, p, z, x, R, frag_runs=bool(frag) and FC.generator_supported(arch, net_dim))
        _ACTS[(case, frag)] = _REC[(case, frag)]["acts"]
    return _REC[(case, frag)]


def _acts_of(case, frag):
    return _ACTS[(case, frag)] if (case, frag) in _ACTS else _rec_of(case, frag)["acts"]


def _id(c):
    return "%s-%d-rows%d" % c


@pytest.mark.parametrize("frag", [1, 2])
@pytest.mark.parametrize("case", FC.CASES, ids=_id)
def test_fragment_order_path_layer_by_layer(case, frag):
    """(1) - (5), the launch count, the gate bits and the untouched activations of the module docstring."""
    arch, net_dim, rows = case
    nd = PR.n_act(arch)
    lines = []
    try:
        p = _weights(arch, net_dim)
        rec = _rec_of(case, frag)
        ex = rec["extra"]
        lines.append("dg_fgemm.hip launches: generate %d, loss_grad %d, dz-only %d (GEMM layers: %d)" % (ex["launches"] + (nd - 1,)))
        assert all(n >= nd - 1 for n in ex["launches"]), "the fragment-order kernels did not run: %s" % (ex["launches"],)
        for d, words in enumerate(ex["gates"]):
            want = np.packbits(rec["acts"][d].reshape(rows, -1) > 0, axis=1, bitorder="little").view("<u4")
            bad = int((words != want).sum())
            lines.append("gate%d: %d of %d words differ from (act%d > 0)" % (d, bad, want.size, d))
            assert bad == 0, lines[-1]
        assert len(ex["gates"]) == nd - 1
        for d, a in enumerate(ex["acts_after"]):
            assert np.array_equal(_bits(a), _bits(rec["acts"][d])), "act%d changed under the backward pass" % d
        res = PR.run_checks(rec, p, arch, _memo(case))
        lines += res.lines + ["--"] + res.summary()
        assert res.fails == [], "\n".join(l for _, _, l in res.fails)
    finally:
        print("\n[%s frag_path=%d]\n  " % (_id(case), frag) + "\n  ".join(lines))


@pytest.mark.parametrize("case", FC.CASES, ids=_id)
def test_both_forms_agree_bit_for_bit_where_the_k_split_is_one(case):
    arch, net_dim, rows = case
    r1, r2 = {"acts": _acts_of(case, 1)}, {"acts": _acts_of(case, 2)}
    assert np.array_equal(_bits(r1["acts"][0]), _bits(r2["acts"][0]))          # the same Linear kernel on the same z
    compared = {}
    for d in range(1, PR.n_act(arch)):
        mask, classes = PR.tap_class_masks(arch, d, "fwd")
        same_in = (_bits(r1["acts"][d - 1]) == _bits(r2["acts"][d - 1])).all(axis=3)          # [N, h, h]
        h_in = same_in.shape[1]
        n = 0
        for c, ks in enumerate(FC.class_ksplits(arch, net_dim, d)):
            if ks != 1:
                continue
            for i, j in np.argwhere(mask == c):
                win = [((i + 1 - kh) // 2, (j + 1 - kw) // 2) for kh in classes[c]["kh"] for kw in classes[c]["kw"]]
                assert all(0 <= a < h_in and 0 <= b < h_in for a, b in win)
                ok = np.logical_and.reduce([same_in[:, a, b] for a, b in win])
                assert np.array_equal(_bits(r1["acts"][d][ok, i, j]), _bits(r2["acts"][d][ok, i, j])), (d, c, i, j)
                n += int(ok.sum()) * r1["acts"][d].shape[3]
        compared[d] = n
    print("\n[%s] elements compared bit for bit per layer: %s" % (_id(case), compared))
    # act1's classes of 1 and 2 taps (K = 256: 8 and 16 chunks), on every row
    k1 = sum(c["positions"] for c, ks in zip(PR.tap_class_masks(arch, 1, "fwd")[1], FC.class_ksplits(arch, net_dim, 1)) if ks == 1)
    assert k1 > 0 and compared[1] == rows * k1 * r1["acts"][1].shape[3]


def test_net_dim_128_falls_back_and_equals_the_position_batched_path():
    arch, net_dim, rows = FC.FALLBACK
    assert not FC.generator_supported(arch, net_dim)
    r1, r0 = _rec_of(FC.FALLBACK, 1), _rec_of(FC.FALLBACK, 0)
    assert r1["extra"]["launches"] == (0, 0, 0) == r0["extra"]["launches"]
    for k in ("y_generate", "y", "loss", "dz"):
        assert np.array_equal(_bits(r1[k]), _bits(r0[k])), k
    for k in ("acts", "grads"):
        for d in range(PR.n_act(arch)):
            assert np.array_equal(_bits(r1[k][d]), _bits(r0[k][d])), (k, d)
    assert np.array_equal(_bits(r1["only"]["dz"]), _bits(r0["only"]["dz"]))


def test_repeated_calls_are_bit_identical():
    """50 generate calls on one handle, MNIST, 512 rows, frag_path = 1 (the shape of the one wrong act2 on record)."""
    import torch
    arch, rows = "mnist", 512
    p = _weights(arch, 64)
    z, _, _ = _inputs(arch, rows)
    gan = _gan(arch, 64, {"two_streams": 0, "frag_path": 1})
    n = int(np.prod(_shape(arch, p, 2, rows)))
    first = None
    for k in range(50):
        y = torch.as_tensor(gan.generate(z)).cuda().view(torch.int32)
        a2 = gan.debug_read("act2", n).view(torch.int32)
        if first is None:
            first = (y.clone(), a2.clone())
            assert _launches(gan) >= 2
            continue
        assert torch.equal(a2, first[1]), "act2 of call %d differs from the first call's" % k
        assert torch.equal(y, first[0]), "y of call %d differs from the first call's" % k
