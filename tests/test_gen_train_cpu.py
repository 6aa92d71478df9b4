"""-m "not gpu": the float64 reference of the generator's training step checks itself, the gather maps of the derived weight layouts
(defensegan_amd/csrc/dg_pack.h, through the host-only tests/support/pack_host_exec.cpp), and the host logic of train_gan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from defensegan_amd import archs
from defensegan_amd import gan as G
from tests.support import generator_reference as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "defensegan_amd", "csrc")
SUP = os.path.join(ROOT, "tests", "support")
SO = os.path.join(SUP, "_build", "libdgpack_test.so")


def _layer_io(p, z, dy):
    """float64 (dpre on the materialised map, input activation NHWC, used extent) of the three deconvs and of the Linear layer."""
    import torch
    g = GR._gen(p, torch.float64)
    zt = torch.as_tensor(np.asarray(z, np.float64))
    a1 = (zt @ g.W + g.b).requires_grad_(True)
    h = torch.relu(a1).view(-1, 4, 4, g.W.shape[1] // 16).permute(0, 3, 1, 2)
    io = []
    for (w, b, used, act, _bn) in g.layers:
        hin = h.shape[-1]
        a = torch.nn.functional.conv_transpose2d(h, w, bias=b, stride=2, padding=1)[..., :2 * hin, :2 * hin]
        a.retain_grad()
        io.append((a, h, used if act == "relu" else 2 * hin))
        h = torch.relu(a)[..., :used, :used] if act == "relu" else torch.sigmoid(a)
    y = h.permute(0, 2, 3, 1)
    (torch.as_tensor(np.asarray(dy, np.float64)).reshape(y.shape) * y).sum().backward()
    return a1.grad.numpy(), [(a.grad.permute(0, 2, 3, 1).numpy(), hh.detach().permute(0, 2, 3, 1).numpy(), u) for a, hh, u in io]


def test_the_hand_written_filter_gradient_equals_autograd_and_the_trap_does_not():
    """The NumPy formula (taps inside the USED extent) equals autograd's dF and db on TorchGenerator for the three deconvs and the
    Linear layer at B = 2; a random gradient placed on the cropped row / column contributes nothing; the SAME-conv-on-7x7 form is
    right where nothing is cropped and off by O(1) on Generator.2."""
    p = GR.weights()
    z, dy = GR.draw(GR.find_seed(p, 2, 128), 2, 128)
    ref = GR.gradient(p, z, dy)["grads"]
    dpre1, io = _layer_io(p, z, dy)
    assert np.allclose(z.astype(np.float64).T @ dpre1, ref["Generator.Input.W"], rtol=1e-12, atol=1e-12)
    assert np.allclose(dpre1.sum(0), ref["Generator.Input.b"], rtol=1e-12, atol=1e-12)
    rs = np.random.RandomState(0)
    for i, (dpre, a_in, used) in enumerate(io):
        name = "Generator.%d" % (2, 3, 5)[i]
        dF, db = GR.numpy_filter_grad(dpre, a_in, used)
        scale = np.abs(ref[name + ".Filters"]).max()
        assert np.abs(dF - ref[name + ".Filters"]).max() <= 1e-12 * scale, name
        assert np.abs(db - ref[name + ".Biases"]).max() <= 1e-12 * max(1.0, np.abs(ref[name + ".Biases"]).max()), name
        if used < dpre.shape[1]:                      # Generator.2: autograd left zero there; garbage there changes nothing
            assert not dpre[:, used:].any() and not dpre[:, :, used:].any()
            noisy = dpre.copy()
            noisy[:, used:] = rs.standard_normal(noisy[:, used:].shape)
            noisy[:, :, used:] = rs.standard_normal(noisy[:, :, used:].shape)
            dF2, db2 = GR.numpy_filter_grad(noisy, a_in, used)
            assert np.abs(dF2 - dF).max() <= 1e-13 * scale and np.abs(db2 - db).max() <= 1e-13 * max(1.0, np.abs(db).max())      # (BLAS rounds a copy's layout differently)
        trap = GR.same_conv_filter_grad(dpre[:, :used, :used], a_in)
        rel = np.abs(trap - ref[name + ".Filters"]).max() / scale
        if used < dpre.shape[1]:
            assert rel > 0.1, rel                      # O(1): the trap
        else:
            assert rel <= 1e-12


def test_valid_taps_match_the_kernel_ranges():
    """dg_gen_train.hip's tap_range (lo = 1 for k = 0 else 0, hi = min(h - 1, (used - k) / 2)) counts archs.valid_taps_1d."""
    for h, used in ((4, 7), (7, 14), (14, 28), (1, 1)):
        n = 0
        for k in range(5) if h > 1 else [1]:
            lo, hi = (1 if k == 0 else 0), min(h - 1, (used - k) // 2)
            assert all(0 <= 2 * o + k - 1 < used for o in range(lo, hi + 1))
            assert not (lo > 0 and 0 <= 2 * (lo - 1) + k - 1 < used) and not (hi + 1 < h and 0 <= 2 * (hi + 1) + k - 1 < used)
            n += hi - lo + 1
        if h > 1:
            assert n == archs.valid_taps_1d(h, used)


def test_the_seed_search_at_the_smallest_shape():
    p = GR.weights()
    assert GR.find_seed(p, 1, 128) == 0
    assert GR.find_seed(GR.weights(64, 64), 3, 64) == 1


def test_every_recorded_seed_is_the_first_accepted_draw():
    """generator_reference.SEEDS, from which the GPU tests draw: a change to synth or draw cannot silently invalidate the table."""
    for (latent, nd, N), seed in GR.SEEDS.items():
        assert GR.find_seed(GR.weights(latent, nd), N, latent) == seed, (latent, nd, N)


def test_the_learning_reference_meets_its_test_with_room():
    """The float64 reference alone: 20 Adam steps against the fixed critic lower the held-out cost from 0.146 to -1.815 -- the figures
    the device test (tests/test_gpu_gen_train.py) is held to."""
    before, after = GR.learning_reference(GR.weights())
    assert after < before - 1.0
    assert abs(before - GR.LEARNING_REFERENCE[0]) <= 1e-9 and abs(after - GR.LEARNING_REFERENCE[1]) <= 1e-9


@pytest.fixture(scope="module")
def packlib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(SUP, "pack_host_exec.cpp")
    deps = [src, os.path.join(CSRC, "dg_pack.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", CSRC, "-o", SO, src])
    l = C.CDLL(SO)
    l.dgk_size.restype = C.c_longlong
    l.dgk_size.argtypes = [C.c_int] * 3
    l.dgk_pack_values.restype = C.c_longlong
    l.dgk_pack_values.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    l.dgk_pack_map.restype = C.c_longlong
    l.dgk_pack_map.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int]
    return l


@pytest.mark.parametrize("nd", [64, 128])
def test_gather_maps_reproduce_every_derived_layout(packlib, nd):
    """The packers run on an index array give maps; applied in NumPy to a random master copy (dst = map < 0 ? 0 : src[map]) they
    give what the value-packing path produces, for every derived layout; every non-padding map entry is a source index used once."""
    K, F = 128, 64 * nd
    rs = np.random.RandomState(nd)
    cases = [(0, K, F, 0, K * F), (1, K, F, 0, K * F), (2, K, F, 16, K * F), (2, K, F, 8, K * F)]
    for cout, cin in ((2 * nd, 4 * nd), (nd, 2 * nd), (1, nd)):
        cases += [(3, cout, cin, 0, 25 * cout * cin)]
        if cout % 32 == 0:
            cases += [(4, cout, cin, 0, 25 * cout * cin)]
    cases += [(5, 1, nd, 0, 25 * nd), (5, 3, nd, 0, 75 * nd), (6, 3, nd, 0, 75 * nd)]
    for which, a, b, c, n_src in cases:
        n = packlib.dgk_size(which, a, b)
        src = rs.standard_normal(n_src).astype(np.float32)
        dst = np.zeros(n, np.float32)
        m = np.empty(n, np.int32)
        packlib.dgk_pack_values(which, src.ctypes.data, dst.ctypes.data, a, b, c)
        packlib.dgk_pack_map(which, m.ctypes.data, n_src, a, b, c)
        assert m.max() < n_src and m.min() >= -1
        got = np.where(m < 0, np.float32(0), src[np.maximum(m, 0)])
        assert np.array_equal(got, dst), (which, a, b, c)
        used = m[m >= 0]
        if which != 6:
            assert np.array_equal(np.sort(used), np.arange(n_src)), which
        else:
            assert len(np.unique(used)) == len(used)


def test_train_gan_bookkeeping():
    """gan_iteration_plan: iteration it starts with a generator step unless it is the run's first; its critic steps continue the
    running index; a resumed run continues both."""
    plan = G.gan_iteration_plan(0, 3, 5)
    assert plan == [(0, 0, False), (1, 5, True), (2, 10, True)]
    assert G.gan_iteration_plan(2, 2, 2) == [(2, 4, True), (3, 6, True)]
    assert G.gan_iteration_plan(0, 4, 2)[2:] == G.gan_iteration_plan(2, 2, 2)


def test_generator_state_round_trip_on_arrays(tmp_path):
    names = list(archs.weight_shapes(archs.make_arch("mnist"), False))
    rs = np.random.RandomState(0)
    shapes = archs.weight_shapes(archs.make_arch("mnist"), False)
    w = {n: rs.standard_normal(s).astype(np.float32) for n, s in shapes.items()}
    m = {n: rs.standard_normal(s).astype(np.float32) for n, s in shapes.items()}
    v = {n: rs.uniform(0, 1, s).astype(np.float32) for n, s in shapes.items()}
    arrays = dict(w)
    arrays.update(G.generator_state_arrays(m, v, 17))
    path = str(tmp_path / "generator.npz")
    np.savez(path, **arrays)
    with np.load(path) as f:
        back = {k: f[k] for k in f.files}
    m2, v2, t2 = G.split_generator_state(back, names)
    assert t2 == 17 and all(np.array_equal(m[n], m2[n]) and np.array_equal(v[n], v2[n]) for n in names)
    assert G.split_generator_state(w, names) is None
    with pytest.raises(ValueError, match="optimiser state lacks"):
        G.split_generator_state({"adam_t": np.asarray(1)}, names)
    # the file loads through load_generator (what --init_path reads): the optimiser's keys are ignored there
    g = G.MnistDefenseGAN(cfg={"USE_BN": False}, test_mode=True)
    assert g.load_generator(path) and all(np.array_equal(g._weights[n], w[n]) for n in names)


def test_refusals():
    z = np.zeros((1, 128), np.float32)
    with pytest.raises(NotImplementedError, match="CelebA generator"):
        G.CelebADefenseGAN(cfg={"USE_BN": False}, test_mode=True).train_gan(None, train_iters=1)
    with pytest.raises(NotImplementedError, match="USE_BN"):
        G.MnistDefenseGAN(cfg={"USE_BN": True}, test_mode=True).generator_step(z)
    for mode in ("wgan", "dcgan"):
        with pytest.raises(NotImplementedError, match="MODE"):
            G.MnistDefenseGAN(cfg={"USE_BN": False, "MODE": mode}, test_mode=True).generator_gradient(z)
    with pytest.raises(NotImplementedError, match="generator step"):
        G.MnistDefenseGAN(cfg={"USE_BN": False}, test_mode=True).train(None, phase=None)


def test_the_cli_saves_every_500_iterations_and_at_the_end():
    from defensegan_amd import train_gan as T
    assert T.chunks(0, 1200, 500) == [(0, 500), (500, 500), (1000, 200)]
    assert T.chunks(700, 1200, 500) == [(700, 300), (1000, 200)] and T.chunks(1200, 1200, 500) == []
    a = T.build_parser().parse_args(["--data_dir", "d", "--out_dir", "o", "--resume", "--train_iters", "7"])
    assert a.cfg == "mnist" and a.resume and a.train_iters == 7


def test_resume_without_a_saved_run_is_an_error(tmp_path):
    from defensegan_amd import train_gan as T
    with pytest.raises(SystemExit):
        T.main(["--data_dir", str(tmp_path), "--out_dir", str(tmp_path / "none"), "--resume"])
    assert not (tmp_path / "none").exists()
