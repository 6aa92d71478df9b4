"""The WGAN-GP critic of the reference (models/dataset_models.py:74-97, models/gan.py:167-199) on the device.

    critic = mnist_discriminator(net_dim=128)              # Conv2D x 3 with LeakyReLU, Flatten, Linear(1); no Softmax
    critic.init_like_tflib(seed=0)                         # or critic.set_named_weights({"Discriminator.1.Filters": ...})
    d = critic.discriminate(x)                             # D(x) [B]
    cost, grads, slopes = critic.gradient(real, fake, alpha)       # dg_critic_gradient
    cost = critic.step(real, fake, alpha)                  # dg_critic_step: one Adam step (1e-4, 0.5, 0.9)

The container is network_builder.MLP with one more layer kind; the arithmetic is the HIP library's (csrc/dg_critic.hip).  Parameters
carry tflib's names, so that a weight pack (.npz) or -- through tf_checkpoint -- a reference checkpoint fills them.  A Batchnorm
critic (USE_BN: True) and the CelebA critic are not implemented.  The generator's half of the loop is gan.train_gan / generator_step.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import numpy as np

from . import _native
from . import network_builder as nb

PENALTY_AXES = {"reference": 0, "image": 1, 0: 0, 1: 1}
# the reference's critic optimiser (gan.py:194-199)
LEARNING_RATE, BETA1, BETA2 = 1e-4, 0.5, 0.9


def penalty_axes_id(penalty_axes) -> int:
    """0 ("reference": the sum over the height axis alone, what reduction_indices=[1] does to an NHWC tensor) or 1 ("image")."""
    if isinstance(penalty_axes, (bool, float)) or penalty_axes not in PENALTY_AXES:
        raise ValueError("penalty_axes must be 'reference' (0) or 'image' (1), got %r" % (penalty_axes,))
    return PENALTY_AXES[penalty_axes]


def tflib_conv_stdev(cin: int, cout: int, k: int, stride: int) -> float:
    """tflib Conv2D's he_init (its default): sqrt(4 / (fan_in + fan_out)), fan_in = cin k^2, fan_out = cout k^2 / stride^2
    (tflib/ops/conv2d.py:69-77); the filters are uniform in +-sqrt(3) stdev."""
    fan_in = cin * k ** 2
    fan_out = cout * k ** 2 / float(stride ** 2)
    return float(np.sqrt(4.0 / (fan_in + fan_out)))


def tflib_linear_stdev(n_in: int, n_out: int) -> float:
    """tflib Linear's default (glorot): sqrt(2 / (in + out)) (tflib/ops/linear.py:55-60)."""
    return float(np.sqrt(2.0 / (n_in + n_out)))


class Critic(nb.MLP):
    """An MLP with one output and tflib parameter names (``param_names``: one (W name, b name) per Conv2D / Linear layer)."""

    def __init__(self, layers, input_shape, param_names: List[Tuple[str, str]]):
        super(Critic, self).__init__(layers, input_shape=input_shape)
        if len(param_names) != len(self._param_layers):
            raise ValueError("expected %d parameter name pairs, got %d" % (len(self._param_layers), len(param_names)))
        self.param_names = [tuple(p) for p in param_names]

    # ------------------------------------------------------------------ parameters by tflib name
    def named_shapes(self) -> Dict[str, Tuple[int, ...]]:
        out = {}
        for (wn, bn), (ws, bs) in zip(self.param_names, self.param_shapes()):
            out[wn], out[bn] = tuple(ws), tuple(bs)
        return out

    def set_named_weights(self, weights: Dict[str, np.ndarray]) -> None:
        shapes = self.named_shapes()
        missing = [k for k in shapes if k not in weights]
        if missing:
            raise ValueError("critic weights lack %s" % ", ".join(missing))
        for k, shp in shapes.items():
            if tuple(np.shape(weights[k])) != shp:
                raise ValueError("%s: shape %r, expected %r" % (k, tuple(np.shape(weights[k])), shp))
        self.set_weights([(weights[wn], weights[bn]) for wn, bn in self.param_names])

    def named_weights(self) -> Dict[str, np.ndarray]:
        out = {}
        for (wn, bn), (W, b) in zip(self.param_names, self.get_weights()):
            out[wn], out[bn] = W, b
        return out

    def tflib_init(self, seed: int = 0) -> Dict[str, np.ndarray]:
        """tflib's initial values restated with a seeded NumPy stream (TF's and NumPy's streams differ: the draw is not the
        reference's, its distribution is): Conv2D uniform +-sqrt(3) stdev with tflib_conv_stdev, Linear glorot, zero biases."""
        rs = np.random.RandomState(seed)
        out = {}
        convs = [l for l in self.layers if isinstance(l, (nb.Conv2D, nb.Linear))]
        for layer, (wn, bn), (ws, bs) in zip(convs, self.param_names, self.param_shapes()):
            if isinstance(layer, nb.Conv2D):
                sd = tflib_conv_stdev(ws[2], ws[3], ws[0], layer.strides[0])
            else:
                sd = tflib_linear_stdev(ws[0], ws[1])
            out[wn] = rs.uniform(-sd * np.sqrt(3), sd * np.sqrt(3), ws).astype(np.float32)
            out[bn] = np.zeros(bs, np.float32)
        return out

    def init_like_tflib(self, seed: int = 0) -> Dict[str, np.ndarray]:
        w = self.tflib_init(seed)
        self.set_named_weights(w)
        return w

    # ------------------------------------------------------------------ the device calls
    def _dev(self, a, dtype=None):
        import torch
        dev = torch.device("cuda", self._device)
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        return t.to(device=dev, dtype=dtype or torch.float32).contiguous()

    def _batches(self, real, fake, alpha):
        r, f, a = self._dev(real), self._dev(fake), self._dev(alpha).reshape(-1)
        B = int(r.shape[0])
        if tuple(f.shape) != tuple(r.shape) or tuple(r.shape[1:]) != tuple(self.input_shape[1:]):
            raise ValueError("real %r and fake %r must both be [B,%d,%d,%d]" % ((tuple(r.shape), tuple(f.shape)) + tuple(self.input_shape[1:])))
        if int(a.numel()) != B:
            raise ValueError("alpha must hold one value per image (%d), got %d" % (B, int(a.numel())))
        return r, f, a, B

    def discriminate(self, x):
        """D(x) [B] (mnist_discriminator's tf.reshape(output, [-1]))."""
        return self.get_logits(x).reshape(-1)

    def n_params(self) -> int:
        return sum(int(np.prod(ws)) + int(np.prod(bs)) for ws, bs in self.param_shapes())

    def split_grads(self, flat: np.ndarray):
        """dg_critic_gradient's flat gradient as [(dW, db)] per Conv2D / Linear layer."""
        out, off = [], 0
        for ws, bs in self.param_shapes():
            nw, nbias = int(np.prod(ws)), int(np.prod(bs))
            out.append((flat[off:off + nw].reshape(ws), flat[off + nw:off + nw + nbias]))
            off += nw + nbias
        return out

    def gradient(self, real, fake, alpha, gp_lambda: float = 10.0, penalty_axes="reference", sync: bool = True):
        """dg_critic_gradient: (cost [3] = cost, w, P; grads flat; slopes [B,W,C] or [B]).  ``sync``: NumPy results (grads split per
        layer); otherwise device tensors and no wait."""
        import torch
        self._ensure()
        if not self._weights_set:
            raise _native.NativeError("critic weights not set")
        axes = penalty_axes_id(penalty_axes)
        r, f, a, B = self._batches(real, fake, alpha)
        dev = r.device
        _, H, W, Cc = self.input_shape
        grads = torch.empty(self.n_params(), dtype=torch.float32, device=dev)
        cost = torch.empty(3, dtype=torch.float32, device=dev)
        slopes = torch.empty((B, W, Cc) if axes == 0 else (B,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check(_native.load().dg_critic_gradient(self._handle, r.data_ptr(), f.data_ptr(), a.data_ptr(), B, float(gp_lambda), axes,
                                                            grads.data_ptr(), cost.data_ptr(), slopes.data_ptr(),
                                                            torch.cuda.current_stream(dev).cuda_stream))
        if not sync:
            return cost, grads, slopes
        torch.cuda.synchronize(dev)
        return cost.cpu().numpy(), self.split_grads(grads.cpu().numpy()), slopes.cpu().numpy()

    def step(self, real, fake, alpha, gp_lambda: float = 10.0, penalty_axes="reference", learning_rate: float = LEARNING_RATE,
             beta1: float = BETA1, beta2: float = BETA2, cost=None):
        """dg_critic_step: one Adam step; returns the device tensor [3] (cost, w, P before the update) without waiting.  ``cost``: a
        device tensor [3] to write into instead of a new one."""
        import torch
        self._ensure()
        if not self._weights_set:
            raise _native.NativeError("critic weights not set")
        axes = penalty_axes_id(penalty_axes)
        r, f, a, B = self._batches(real, fake, alpha)
        dev = r.device
        if cost is None:
            cost = torch.empty(3, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _native.check(_native.load().dg_critic_step(self._handle, r.data_ptr(), f.data_ptr(), a.data_ptr(), B, float(gp_lambda), axes,
                                                        float(learning_rate), float(beta1), float(beta2), cost.data_ptr(),
                                                        torch.cuda.current_stream(dev).cuda_stream))
        return cost

    # ------------------------------------------------------------------ Adam state
    def adam_reset(self) -> None:
        self._ensure()
        _native.check(_native.load().dg_clf_adam_reset(self._handle))

    def adam_state(self):
        """[((mW, mb), (vW, vb), t)] per Conv2D / Linear layer (dg_clf_get_adam)."""
        from . import utils_tf
        return [utils_tf.adam_state(self, i) for i in range(len(self.param_names))]


def mnist_discriminator(net_dim: int = 128, input_shape=(None, 28, 28, 1), use_bn: bool = False) -> Critic:
    """models/dataset_models.py:74-97: Conv2D(net_dim, 5x5, stride 2, SAME), LeakyReLU, Conv2D(2 net_dim), LeakyReLU,
    Conv2D(4 net_dim), LeakyReLU, the reshape, Linear(1).  28 -> 14 -> 7 -> 4."""
    if use_bn:
        raise NotImplementedError("a Batchnorm critic (USE_BN: True) is not implemented: its batch statistics couple the images of "
                                  "the gradient penalty's double backward")
    net_dim = int(net_dim)
    layers = [nb.Conv2D(net_dim, (5, 5), (2, 2), "SAME"), nb.LeakyReLU(),
              nb.Conv2D(2 * net_dim, (5, 5), (2, 2), "SAME"), nb.LeakyReLU(),
              nb.Conv2D(4 * net_dim, (5, 5), (2, 2), "SAME"), nb.LeakyReLU(),
              nb.Flatten(), nb.Linear(1)]
    names = [("Discriminator.%d.Filters" % i, "Discriminator.%d.Biases" % i) for i in (1, 2, 3)] + [("Discriminator.Output.W", "Discriminator.Output.b")]
    return Critic(layers, input_shape, names)


def celeba_discriminator(*args, **kwargs):
    raise NotImplementedError("the CelebA critic (models/dataset_models.py celeba_discriminator) is not implemented; only "
                              "mnist_discriminator is")
