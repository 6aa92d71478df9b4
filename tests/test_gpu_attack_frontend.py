"""-m gpu: what the attacks' shared return packing promises (defensegan_amd/attacks.py, ``_pack``) -- NumPy in gives NumPy out, a
device tensor in gives tensors on its device, and the two agree bit for bit, with ``return_info`` on and off.  The values
themselves are pinned by each attack's own GPU tests; this runs 3 images through the smallest classifier of
tests/support/cw_cases.py (model T: 60 pixels, 6 classes) and, for the latent attack, tests/support/latent_device.py's models."""
import numpy as np
import pytest

from defensegan_amd import network_builder as nb
from tests.support import cw_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    import torch
    model = C.model("T")
    model.set_weights(C.params("T"))
    x = np.array(C.images("T", 3, 61))
    yield model, x, np.zeros(3, np.int64)       # the model's own class on all three: every attack has something to move
    torch.cuda.synchronize()
    model.close()


def _flat(out):
    """The values of a result, in order: x_adv, then the info (a dict's values by key)."""
    out = out if isinstance(out, tuple) else (out,)
    return [w for v in out for w in ([v[k] for k in sorted(v)] if isinstance(v, dict) else [v])]


def _both_ways(generate, x, n_values, infos=(False, True)):
    """``generate(x, return_info=...)`` on the array and on a device tensor: kinds, device, and the same bits."""
    import torch
    xt = torch.from_numpy(x).cuda()
    for info in infos:
        a, t = generate(x, return_info=info), generate(xt, return_info=info)
        assert isinstance(a, tuple) == isinstance(t, tuple) == info
        a, t = _flat(a), _flat(t)
        assert len(a) == len(t) == (n_values if info else 1)
        assert isinstance(a[0], np.ndarray) and a[0].dtype == np.float32 and a[0].shape == x.shape
        for va, vt in zip(a, t):
            if isinstance(vt, torch.Tensor):
                assert isinstance(va, np.ndarray) and vt.device == xt.device
                assert va.dtype == vt.cpu().numpy().dtype and va.shape == tuple(vt.shape) and va.tobytes() == vt.cpu().numpy().tobytes()
            else:
                assert va == vt and type(va) is type(vt)
        assert not np.array_equal(a[0], x)                          # an attack ran: the agreement is not that of two copies of x
    assert np.array_equal(xt.cpu().numpy(), x)


@pytest.mark.parametrize("ord", [np.inf, 2])
def test_fgsm(small, ord):
    model, x, y = small
    fgsm = nb.FastGradientMethod(model)
    _both_ways(lambda v, return_info: fgsm.generate(v, eps=0.1, ord=ord, y=y, clip_min=0.0, clip_max=1.0), x, 1, infos=(False,))


@pytest.mark.parametrize("ord,n_values", [(np.inf, 2), (2, 3)])
def test_pgd(small, ord, n_values):
    model, x, y = small
    pgd = nb.ProjectedGradientDescent(model)
    _both_ways(lambda v, return_info: pgd.generate(v, y, eps=0.3, eps_iter=0.1, nb_iter=2, clip_min=0.0, clip_max=1.0, rand_init=True, seed=3,
                                                   batch_size=2, ord=ord, return_info=return_info), x, n_values)


@pytest.mark.parametrize("search,n_values", [(False, 3), (True, 5)])
def test_cw(small, search, n_values):
    model, x, y = small
    cw = nb.CarliniWagnerL2(model)
    _both_ways(lambda v, return_info: cw.generate(v, y=y, binary_search_steps=1, max_iterations=3, learning_rate=0.1, initial_const=100.0,
                                                  batch_size=2, return_info=return_info, return_search=search), x, n_values)


def test_latent():
    import torch
    from tests.support import latent_device as LD, latent_reference as LR
    g, model, atk = LD.build(128, "conv10", 0)
    x, lab, _ = LR.draw(128, 3, 2, 3)
    _both_ways(lambda v, return_info: atk.generate(v, lab % 10, rec_rr=2, nb_iter=2, seed=1, batch_size=2, return_info=return_info), x, 6)
    torch.cuda.synchronize()
    g.close()
    model.close()
