"""-m "not gpu": the host-side front end the attack classes share (defensegan_amd/attacks.py) -- both import orders and the
forwarding of every moved name from network_builder, the label / clip / start-point helpers on CPU tensors, and the checks that
must refuse a bad argument before a model's native handle (and with it the device) is touched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from defensegan_amd import attacks, network_builder as nb, whitebox as wb

MOVED = ("FastGradientMethod", "CarliniWagnerL2", "_AttackDeviceOps", "BpdaDeviceOps", "BPDA", "ProjectedGradientDescent", "SpsaDeviceOps",
         "SPSA", "LatentAttack", "_attack_ord", "ball_project_noise", "_row_norms", "_philox4x32_10", "bpda_rand_noise",
         "bpda_seed_schedule", "rand_fgsm_prestep", "BPDA_NOISE_TAG", "BPDA_DEFAULT_SEED", "LATENT_DEFAULT_SEED", "_CW_REC_NOTE",
         "_L1_ITERATIVE_NOTE")


# ---------------------------------------------------------------------- the move
@pytest.mark.parametrize("code", [
    "import defensegan_amd.attacks",
    "import defensegan_amd.network_builder as nb; nb.BPDA; nb.FastGradientMethod; nb._attack_ord"])
def test_both_import_orders_work_in_a_fresh_interpreter_and_touch_no_device(code):
    code += "; import sys; t = sys.modules.get('torch'); assert t is None or not t.cuda.is_initialized()"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert done.returncode == 0, done.stderr


def test_every_moved_name_resolves_on_network_builder_and_nothing_else_does():
    with open(nb.__file__) as fh:
        source = fh.read()
    for name in MOVED:
        assert getattr(nb, name) is getattr(attacks, name), name
    for cls in MOVED[:9]:
        assert getattr(nb, cls).__module__ == "defensegan_amd.attacks" and "class %s(" % cls not in source
    with pytest.raises(AttributeError, match="no attribute 'NoSuchAttack'"):
        nb.NoSuchAttack
    assert not hasattr(nb, "__wrapped__")
    assert nb.MLP.input_gradient.__qualname__ == "MLP.input_gradient" and nb.MLP.jacobian.__qualname__ == "MLP.jacobian"
    assert callable(nb._jacobian_input) and callable(nb._class_indices) and "BPDA" in nb._REC_GRADIENT_NOTE


def test_a_patched_name_is_what_whitebox_sees_and_is_undone_cleanly():
    class Stub(object):
        pass
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(nb, "SPSA", Stub)
        assert wb.network_builder.SPSA is Stub and attacks.SPSA is not Stub
    assert wb.network_builder.SPSA is attacks.SPSA


# ---------------------------------------------------------------------- labels
def test_labels_from_lists_arrays_tensors_and_one_hot_rows():
    import torch
    cpu = torch.device("cpu")
    want = [2, 0, 3]
    for y in (want, np.array(want, np.int64), torch.tensor(want), np.eye(4, dtype=np.float32)[want], torch.eye(4)[want]):
        for policy in (None, "cw", "latent"):
            got = attacks._labels(y, 3, cpu, range_words=policy, nb_classes=4)
            assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == want
    assert attacks._labels(None, 3, cpu, required=False) is None
    assert attacks._labels(np.array(want), None, cpu, required=False).tolist() == want          # FGSM: no length asked for
    assert attacks._labels(np.array([0, 1]), None, cpu, required=False).tolist() == [0, 1]


def test_labels_refuse_in_each_policys_own_words():
    import torch
    cpu = torch.device("cpu")
    words = {None: "y must be 3 class indices or one-hot rows", "latent": "y must be 3 class indices or one-hot rows",
             "cw": "labels must be 3 class indices in [0, 4) or one-hot rows"}
    for policy, text in words.items():
        for bad in ([0, 1], np.zeros(4, np.int64), np.eye(4)[[0, 1]], None):
            with pytest.raises(ValueError) as e:
                attacks._labels(bad, 3, cpu, range_words=policy, nb_classes=4)
            assert str(e.value) == text
    # an index outside the classes: passed on as it is (a zero gradient / zero step on the device), or refused by name
    assert attacks._labels([0, 4, 1], 3, cpu).tolist() == [0, 4, 1] and attacks._labels([0, -1, 1], 3, cpu).tolist() == [0, -1, 1]
    for bad in ([0, 4, 1], [0, -1, 1]):
        with pytest.raises(ValueError) as e:
            attacks._labels(bad, 3, cpu, range_words="cw", nb_classes=4)
        assert str(e.value) == words["cw"]
        with pytest.raises(ValueError) as e:
            attacks._labels(bad, 3, cpu, range_words="latent", nb_classes=4)
        assert str(e.value) == "y holds a class index outside [0, 4)"


# ---------------------------------------------------------------------- clip bounds, budget, chunks
def test_clip_bounds():
    inf = float("inf")
    assert attacks._clip_bounds(None, None) == (-inf, inf) == attacks._clip_bounds(None, None, ordered=False)
    assert attacks._clip_bounds(0, None) == (0.0, inf) and attacks._clip_bounds(None, np.float32(1)) == (-inf, 1.0)
    assert attacks._clip_bounds(0.5, 0.5) == (0.5, 0.5)
    assert attacks._clip_bounds(1.0, 0.0, ordered=False) == (1.0, 0.0)                           # FGSM's: never checked
    lo, hi = attacks._clip_bounds(float("nan"), 1.0, ordered=False)
    assert lo != lo and hi == 1.0
    for bad in ((1.0, 0.0), (float("nan"), 1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError) as e:
            attacks._clip_bounds(*bad)
        assert str(e.value) == "clip_min must not exceed clip_max"


def test_budget_checks_and_chunks():
    attacks._check_iterative(1, 0.0, 0.0, 1)
    attacks._check_iterative()
    for kw, text in ((dict(nb_iter=0), "nb_iter must be >= 1, got 0"), (dict(eps=-0.1), "eps and eps_iter must be >= 0"),
                     (dict(eps_iter=float("nan")), "eps and eps_iter must be >= 0"), (dict(batch_size=0), "batch_size must be >= 1"),
                     (dict(rand_init=True, x_init=np.zeros(1)), "give rand_init or x_init, not both")):
        with pytest.raises(ValueError) as e:
            attacks._check_iterative(**kw)
        assert str(e.value) == text
    assert attacks._chunks(5) == [(0, 5)] and attacks._chunks(5, 2) == [(0, 2), (2, 4), (4, 5)] and attacks._chunks(4, 9) == [(0, 4)]


# ---------------------------------------------------------------------- the start point
def test_start_point_draw_is_bit_equal_to_the_noise_functions():
    """3 images of 7 elements: the last Philox quad of every image is cut."""
    import torch
    rs = np.random.RandomState(2)
    x = rs.uniform(-0.4, 1.4, (3, 7, 1, 1)).astype(np.float32)
    t = torch.from_numpy(x)
    noise = nb.bpda_rand_noise(3, 7, 0.3, 5)
    for ord, drawn in ((np.inf, noise), (2, nb.ball_project_noise(noise, 0.3))):
        got = attacks._start_point(t, None, True, 0.3, 5, ord, 0.0, 1.0)
        want = np.clip(x + drawn.reshape(x.shape), np.float32(0.0), np.float32(1.0))
        assert got.dtype == torch.float32 and got.numpy().tobytes() == want.tobytes()
        assert (want == 0).any() and (want == 1).any() and ((want > 0) & (want < 1)).any()       # the clip took part
    assert not np.array_equal(noise, nb.ball_project_noise(noise, 0.3))
    plain = attacks._start_point(t, None, False, 0.3, 5, np.inf, 0.25, 0.75)
    assert plain.numpy().tobytes() == np.clip(x, np.float32(0.25), np.float32(0.75)).tobytes() and np.array_equal(t.numpy(), x)


def test_start_point_takes_x_init_as_given_cloned_only_on_request():
    import torch
    t = torch.zeros(3, 7, 1, 1)
    x_init = torch.full((3, 7, 1, 1), 5.0)                                                        # outside the clip range: not clipped
    same = attacks._start_point(t, x_init, False, 0.3, 5, np.inf, 0.0, 1.0)
    assert same.data_ptr() == x_init.data_ptr() and float(same.max()) == 5.0
    own = attacks._start_point(t, x_init, False, 0.3, 5, 2, 0.0, 1.0, clone=True)
    assert own.data_ptr() != x_init.data_ptr() and torch.equal(own, x_init)
    from_numpy = attacks._start_point(t, np.full((3, 7, 1, 1), 0.5), False, 0.3, 5, np.inf, 0.0, 1.0)
    assert from_numpy.dtype == torch.float32 and float(from_numpy.min()) == 0.5
    with pytest.raises(ValueError) as e:
        attacks._start_point(t, x_init, True, 0.3, 5, np.inf, 0.0, 1.0)
    assert str(e.value) == "give rand_init or x_init, not both"
    with pytest.raises(ValueError) as e:
        attacks._start_point(t, torch.zeros(3, 7), False, 0.3, 5, np.inf, 0.0, 1.0)
    assert str(e.value) == "x_init must have x's shape"


# ---------------------------------------------------------------------- return packing
def test_pack_gives_numpy_for_numpy_and_leaves_tensors_alone():
    import torch
    a, b = torch.arange(3.0), torch.arange(3, dtype=torch.int32)
    assert attacks._pack(False, False, a, b) is a
    out = attacks._pack(False, True, a, b, 7, {"k": b})
    assert out[0] is a and out[1] is b and out[2] == 7 and out[3]["k"] is b
    assert isinstance(attacks._pack(True, False, a, b), np.ndarray)
    out = attacks._pack(True, True, a, b, 7, {"k": b})
    assert [type(v) for v in out] == [np.ndarray, np.ndarray, int, dict] and out[1].dtype == np.int32 and out[3]["k"].tolist() == [0, 1, 2]


# ---------------------------------------------------------------------- checks before the device
_X, _Y = np.zeros((2, 28, 28, 1), np.float32), np.zeros(2, np.int32)


def _gan(**cfg):
    from defensegan_amd.gan import MnistDefenseGAN
    return MnistDefenseGAN(cfg=dict({"USE_BN": False, "LATENT_DIM": 128, "NET_DIM": 64}, **cfg), test_mode=True, rec_rr=2, rec_iters=5,
                           rec_lr=10.0)


def _refused(model, call, exc, text):
    with pytest.raises(exc) as e:
        call()
    assert text in str(e.value), str(e.value)
    assert model._handle is None


@pytest.mark.parametrize("kw,exc,text", [
    (dict(nb_iter=0), ValueError, "nb_iter must be >= 1, got 0"),
    (dict(eps=-0.1), ValueError, "eps and eps_iter must be >= 0"),
    (dict(eps_iter=-0.1), ValueError, "eps and eps_iter must be >= 0"),
    (dict(rand_init=True, x_init=_X), ValueError, "give rand_init or x_init, not both"),
    (dict(clip_min=1.0, clip_max=0.0), ValueError, "clip_min must not exceed clip_max"),
    (dict(batch_size=0), ValueError, "batch_size must be >= 1"),
    (dict(ord=1), NotImplementedError, "needs a sort"),
    (dict(ord=3), ValueError, "ProjectedGradientDescent: ord must be one of np.inf, 2, got 3")])
def test_pgd_refuses_before_the_device(kw, exc, text):
    m = nb.model_e()
    _refused(m, lambda: nb.ProjectedGradientDescent(m).generate(_X, _Y, **kw), exc, text)


def test_pgd_and_cw_refuse_a_defended_model_before_the_device():
    m = nb.model_e()
    m.add_rec_model(_gan(), None, 50)
    _refused(m, lambda: nb.ProjectedGradientDescent(m).generate(_X, _Y), ValueError, "use BPDA")
    _refused(m, lambda: nb.CarliniWagnerL2(m).generate(_X), NotImplementedError, nb._CW_REC_NOTE)


@pytest.mark.parametrize("kw,exc,text", [
    (dict(steps=3), TypeError, "unknown CarliniWagnerL2 parameters: ['steps']"),
    (dict(y=_Y, y_target=_Y), ValueError, "give y or y_target, not both")])
def test_cw_refuses_before_the_device(kw, exc, text):
    m = nb.model_e()
    _refused(m, lambda: nb.CarliniWagnerL2(m).generate(_X, **kw), exc, text)


@pytest.mark.parametrize("kw,exc,text", [
    (dict(rec_rr=0), ValueError, "rec_rr must be >= 1 and nb_iter >= 0"),
    (dict(nb_iter=-1), ValueError, "rec_rr must be >= 1 and nb_iter >= 0"),
    (dict(confidence=-1.0), ValueError, "confidence and c must be >= 0"),
    (dict(c=-1.0), ValueError, "confidence and c must be >= 0"),
    (dict(batch_size=0), ValueError, "batch_size must be >= 1")])
def test_latent_refuses_before_the_device(kw, exc, text):
    m = nb.model_f()
    _refused(m, lambda: nb.LatentAttack(m, _gan()).generate(_X, _Y, **kw), exc, text)


def test_latent_refuses_a_batchnorm_generator_before_the_device():
    m = nb.model_f()
    _refused(m, lambda: nb.LatentAttack(m, _gan(USE_BN=True)).generate(_X, _Y), NotImplementedError, "not implemented for use_bn")


@pytest.mark.parametrize("attack", ["BPDA", "SPSA"])
def test_bpda_and_spsa_refuse_before_their_device_operations_are_built(attack):
    m = nb.model_e()
    m.add_rec_model(_gan(), None, 50)
    gen = lambda **kw: getattr(nb, attack)(m).generate(_X, _Y, **kw)
    for kw, text in ((dict(nb_iter=0), "nb_iter"), (dict(eps=-1.0), "eps and eps_iter"), (dict(clip_min=1.0, clip_max=0.0), "clip_min"),
                     (dict(batch_size=-1), "batch_size")):
        _refused(m, lambda: gen(**kw), ValueError, text)
    m.rec_layer.z_init = np.zeros((4, 128), np.float32)
    _refused(m, gen, ValueError, "fixed z_init")
    if attack == "SPSA":
        bn = nb.model_e()
        bn.add_rec_model(_gan(USE_BN=True), None, 50)
        _refused(bn, lambda: nb.SPSA(bn).generate(_X, _Y), NotImplementedError, "USE_BN")
