"""Host-side mirror of the reference's classifier container (/root/reference/utils/network_builder.py:129-331, models
A-F :333-521) for the step AFTER the projection -- SURVEY.md section 8f row N2.  The layers only describe the network;
the arithmetic runs in the HIP library (dg_clf_* in include/defensegan_hip.h), never on the host.

    model = model_a()                      # same builders, same argument names as the reference
    model.set_weights([(kernels, b), ...]) # one (W, b) per Conv2D / Linear layer, reference layouts
    probs = model(x)                       # = get_probs(x); x NumPy or torch [B,H,W,C]; returns the same kind
    model.add_rec_model(gan, z_init, batch_size)   # prepend the Defense-GAN projection (network_builder.py:179-183)
    model.save_weights("clf.npz"); model.load_weights("clf.npz")   # trained parameters (utils_tf.model_train)

Differences from the reference that follow from having no TF graph: ``fprop`` exposes only 'logits' and 'probs' (and
'reconstruction' after add_rec_model), not every hidden layer; Dropout is the identity in evaluation and active only in
training (utils_tf.model_train)."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native

KIND = {"Conv2D": 0, "ReLU": 1, "Linear": 2, "Flatten": 3, "Softmax": 4, "Dropout": 5, "LeakyReLU": 6}


class Layer(object):
    has_params = False

    def spec(self) -> Tuple[int, ...]:
        return (KIND[self.__class__.__name__], 0, 0, 0, 0, 0, 0)


class Conv2D(Layer):
    """network_builder.py:206-236: tf.nn.conv2d(x, kernels[kh,kw,cin,cout], (1,)+strides+(1,), padding) + b."""
    has_params = True

    def __init__(self, output_channels, kernel_shape, strides, padding):
        assert padding in ("SAME", "VALID")
        self.output_channels, self.kernel_shape, self.strides, self.padding = int(output_channels), tuple(kernel_shape), tuple(strides), padding

    def spec(self):
        return (KIND["Conv2D"], self.output_channels, self.kernel_shape[0], self.kernel_shape[1], self.strides[0], self.strides[1],
                1 if self.padding == "SAME" else 0)


class Linear(Layer):
    """network_builder.py:190-203: tf.matmul(x, W[in,out]) + b."""
    has_params = True

    def __init__(self, num_hid):
        self.num_hid = int(num_hid)

    def spec(self):
        return (KIND["Linear"], self.num_hid, 0, 0, 0, 0, 0)


class ReLU(Layer):
    pass


class LeakyReLU(Layer):
    """The critic's activation, tf.maximum(0.2 * x, x) (models/dataset_models.py:10-11).  The slope 0.2 is the reference's only
    value and is fixed in the kernel; the gradient at x == 0 is 0.2 (TF's MaximumGrad gives a tie to its first argument)."""


class Flatten(Layer):
    pass


class Softmax(Layer):
    pass


class Dropout(Layer):
    """Identity at evaluation (tf.cond(K.learning_phase(), ...), network_builder.py:296-297).  In training, ``prob`` is TF 1.x
    tf.nn.dropout's KEEP probability, as the reference passes it: Dropout(0.25) keeps 25 % of the units and scales them by 4."""

    def __init__(self, prob):
        self.prob = prob


class MLP(object):
    """network_builder.py:129-183."""

    def __init__(self, layers: Sequence[Layer], input_shape=(None, 28, 28, 1), rec_model=None, device: int = 0):
        self.layers = list(layers)
        self.input_shape = tuple(input_shape)
        self.rec_model = rec_model
        self.rec_layer = None
        self._device = int(device)
        self._handle = None
        self.layer_names: List[str] = []
        for i, layer in enumerate(self.layers):
            self.layer_names.append(layer.__class__.__name__ + str(i))
        if isinstance(self.layers[-1], Softmax):
            self.layer_names[-1], self.layer_names[-2] = "probs", "logits"
        else:
            self.layer_names[-1] = "logits"
        self._param_layers = [i for i, l in enumerate(self.layers) if l.has_params]
        self._weights_set = False

    # ------------------------------------------------------------------ native handle
    def _ensure(self):
        if self._handle is not None:
            return
        lib = _native.load()
        _, H, W, Cc = self.input_shape
        h = C.c_void_p()
        _native.check(lib.dg_clf_create(self._device, int(H), int(W), int(Cc), C.byref(h)))
        self._handle = h
        self._native_index = []
        for layer in self.layers:
            rc = lib.dg_clf_add_layer(h, *layer.spec())
            if rc < 0:
                _native.check(rc)
            self._native_index.append(rc)
            if isinstance(layer, Dropout):
                _native.check(lib.dg_clf_set_dropout(h, rc, float(layer.prob)))
        self.nb_classes = int(lib.dg_clf_output_width(h))

    def close(self):
        if self._handle is not None:
            _native.load().dg_clf_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_layer_names(self):
        return (["reconstruction"] if self.rec_layer is not None else []) + self.layer_names

    def set_weights(self, params: Sequence[Tuple[np.ndarray, np.ndarray]]) -> None:
        """One (W, b) per Conv2D / Linear layer, in order; kernels [kh,kw,cin,cout], W [in,out] (reference layouts)."""
        self._ensure()
        if len(params) != len(self._param_layers):
            raise ValueError("expected %d (W, b) pairs, got %d" % (len(self._param_layers), len(params)))
        lib = _native.load()
        for li, (W, b) in zip(self._param_layers, params):
            W = np.ascontiguousarray(W, np.float32)
            b = np.ascontiguousarray(b, np.float32)
            shp = (C.c_int64 * W.ndim)(*W.shape)
            _native.check(lib.dg_clf_set_weights(self._handle, self._native_index[li], W.ctypes.data_as(C.c_void_p), shp, W.ndim,
                                                 b.ctypes.data_as(C.c_void_p), b.size, 0))
        self._weights_set = True

    def param_shapes(self) -> List[Tuple[Tuple[int, ...], Tuple[int]]]:
        """((W shape), (b shape)) per Conv2D / Linear layer, in order, in the reference layouts."""
        _, H, W, Cc = self.input_shape
        shape, flat, out = (H, W, Cc), None, []
        for layer in self.layers:
            if isinstance(layer, Conv2D):
                out.append((tuple(layer.kernel_shape) + (shape[2], layer.output_channels), (layer.output_channels,)))
                shape = conv_output_shape(shape, layer)
            elif isinstance(layer, Flatten):
                flat = int(np.prod(shape))
            elif isinstance(layer, Linear):
                out.append(((flat, layer.num_hid), (layer.num_hid,)))
                flat = layer.num_hid
        return out

    def get_weights(self) -> List[Tuple[np.ndarray, np.ndarray]]:
        """The device parameters as NumPy (W, b) pairs, one per Conv2D / Linear layer, in the layouts set_weights takes."""
        self._ensure()
        if not self._weights_set:
            raise _native.NativeError("classifier weights not set")
        lib = _native.load()
        out = []
        for li, (ws, bs) in zip(self._param_layers, self.param_shapes()):
            W, b = np.empty(ws, np.float32), np.empty(bs, np.float32)
            _native.check(lib.dg_clf_get_weights(self._handle, self._native_index[li], W.ctypes.data_as(C.c_void_p),
                                                 b.ctypes.data_as(C.c_void_p), 0))
            out.append((W, b))
        return out

    def save_weights(self, path: str) -> None:
        """Writes get_weights() to ``path`` (.npz: W0, b0, W1, b1, ... in layer order)."""
        arrays = {}
        for i, (W, b) in enumerate(self.get_weights()):
            arrays["W%d" % i], arrays["b%d" % i] = W, b
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    def load_weights(self, path: str) -> None:
        """Installs the parameters save_weights wrote; the file must hold exactly this model's (W, b) pairs and shapes."""
        shapes = self.param_shapes()
        with np.load(path) as f:
            keys = set(f.files)
            want = {"%s%d" % (k, i) for i in range(len(shapes)) for k in "Wb"}
            if keys != want:
                raise ValueError("%s holds %s, this model needs %s" % (path, sorted(keys), sorted(want)))
            params = [(f["W%d" % i], f["b%d" % i]) for i in range(len(shapes))]
        for i, ((W, b), (ws, bs)) in enumerate(zip(params, shapes)):
            if W.shape != ws or b.shape != bs:
                raise ValueError("%s: parameter pair %d is %s / %s, this model needs %s / %s" % (path, i, W.shape, b.shape, ws, bs))
        self.set_weights(params)

    def init_like_reference(self, seed: int = 0) -> List[Tuple[np.ndarray, np.ndarray]]:
        """The reference's initialisers (normal, normalised per output unit, zero bias: network_builder.py:196-203, 217-224)
        with a NumPy stream; returns and installs the parameters.  For tests and synthetic benchmarks."""
        rs = np.random.RandomState(seed)
        _, H, W, Cc = self.input_shape
        shape, flat, params = (H, W, Cc), None, []
        for layer in self.layers:
            if isinstance(layer, Conv2D):
                kh, kw = layer.kernel_shape
                k = rs.standard_normal((kh, kw, shape[2], layer.output_channels)).astype(np.float32)
                k = k / np.sqrt(1e-7 + np.square(k).sum(axis=(0, 1, 2)))
                params.append((k.astype(np.float32), np.zeros(layer.output_channels, np.float32)))
                shape = conv_output_shape(shape, layer)
            elif isinstance(layer, Flatten):
                flat = int(np.prod(shape))
            elif isinstance(layer, Linear):
                w = rs.standard_normal((flat, layer.num_hid)).astype(np.float32)
                w = w / np.sqrt(1e-7 + np.square(w).sum(axis=0, keepdims=True))
                params.append((w.astype(np.float32), np.zeros(layer.num_hid, np.float32)))
                flat = layer.num_hid
        self.set_weights(params)
        return params

    # ------------------------------------------------------------------ forward
    def add_rec_model(self, model, z_init, batch_size):
        """network_builder.py:179-183: prepend the Defense-GAN projection."""
        from .gan import ReconstructionLayer
        self.rec_layer = ReconstructionLayer(model, z_init, self.input_shape, batch_size)

    def model_eval(self, test_images, test_labels, batch_size: int, **kw):
        """Accuracy of this classifier over ``test_images`` -- behind the Defense-GAN projection when ``add_rec_model`` installed
        one -- as ``(correct, n, roc_info)``: ``gan_defense.model_eval_gan`` with the layer's model, ``z_init`` and ``rec_rr``.  THE
        way to evaluate a defended classifier here: ``fprop`` / ``get_probs`` project whatever single batch they are handed in ONE
        engine call and cannot coalesce across calls (the reference's ``ReconstructionLayer.fprop`` sits inside one session.run per
        BATCH_SIZE = 50 images, utils/network_builder.py:266-271: 500 latent rows, where the loop runs at 0.67 of the peak), while
        this routes the same per-batch semantics through runs of whole batches (0.85)."""
        from . import gan_defense
        rl = self.rec_layer
        if rl is None:
            return gan_defense.model_eval_gan(None, self, test_images, test_labels, batch_size, **kw)
        kw.setdefault("same_init_z", rl.z_init)
        return gan_defense.model_eval_gan(rl.rec_model.reconstruct, self, test_images, test_labels, batch_size,
                                          rec_rr=int(rl.rec_model.rec_rr), **kw)

    def _forward(self, x, no_rec=False):
        import torch
        self._ensure()
        if not self._weights_set:
            raise _native.NativeError("classifier weights not set")
        was_numpy = isinstance(x, np.ndarray)
        dev = torch.device("cuda", self._device)
        t = torch.from_numpy(np.ascontiguousarray(x, np.float32)) if was_numpy else x
        t = t.to(device=dev, dtype=torch.float32).contiguous()
        rec = None
        if self.rec_layer is not None and not no_rec:
            rec = self.rec_layer.fprop(t)
            t = rec if not isinstance(rec, np.ndarray) else torch.from_numpy(rec).to(dev)
            t = t.to(device=dev, dtype=torch.float32).contiguous()
        B = int(t.shape[0])
        logits = torch.empty(B, self.nb_classes, dtype=torch.float32, device=dev)
        probs = torch.empty_like(logits)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _native.check(_native.load().dg_clf_forward(self._handle, t.data_ptr(), B, logits.data_ptr(), probs.data_ptr(), stream))
        out = {"logits": logits, "probs": probs}
        if rec is not None:
            out["reconstruction"] = t
        if was_numpy:
            torch.cuda.synchronize(dev)
            out = {k: v.cpu().numpy() for k, v in out.items()}
        return out

    def fprop(self, x, set_ref=False, no_rec=False):
        return self._forward(x, no_rec=no_rec)

    def get_logits(self, x):
        return self._forward(x)["logits"]

    def get_probs(self, x):
        return self._forward(x)["probs"]

    def __call__(self, x):
        return self.get_probs(x)

    def eval_batch(self, rec, orig=None, labels=None, sync=True):
        """One batch of model_eval_gan on the device (gan_defense.py:113-179): returns (n_correct, preds [B], diffs [B] or None);
        with ``sync=False`` n_correct stays a device tensor [1] (int32) and the call does not wait for the stream.
        ``rec`` = the classifier's input (reconstructions), ``orig`` = the images they are compared with (diff_op,
        blackbox.py:569-572), ``labels`` int class indices."""
        import torch
        self._ensure()
        dev = torch.device("cuda", self._device)
        to = lambda a, dt: (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(device=dev, dtype=dt).contiguous()
        r = to(rec, torch.float32)
        B = int(r.shape[0])
        o = to(orig, torch.float32) if orig is not None else None
        lab = to(labels, torch.int32) if labels is not None else None
        preds = torch.empty(B, dtype=torch.int32, device=dev)
        diffs = torch.empty(B, dtype=torch.float32, device=dev) if o is not None else None
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _native.check(_native.load().dg_eval_batch(
                self._handle, r.data_ptr(), o.data_ptr() if o is not None else None, lab.data_ptr() if lab is not None else None, B,
                preds.data_ptr(), diffs.data_ptr() if diffs is not None else None, cnt.data_ptr(), stream))
        if sync:
            return int(cnt.item()), preds, diffs
        return cnt, preds, diffs          # device tensors: nothing waits for the stream (gan_defense.model_eval_gan sums at the end)


def conv_output_shape(shape, layer: Conv2D):
    H, W, _ = shape
    (kh, kw), (sh, sw) = layer.kernel_shape, layer.strides
    if layer.padding == "SAME":
        return (-(-H // sh), -(-W // sw), layer.output_channels)
    return ((H - kh) // sh + 1, (W - kw) // sw + 1, layer.output_channels)


# ---------------------------------------------------------------------- the reference's model zoo (network_builder.py:333-521)
# Architectures are data: (channels, kernel, stride, padding) per Conv2D+ReLU stage, hidden widths per Linear+ReLU(+Dropout)
# stage; the builders keep the reference's names and signatures.
def _conv_zoo(convs, hidden, nb_classes, input_shape, rec_model, drop_after_flatten=None, drop_input=None, drop_before_flatten=None,
              hidden_dropout=True):
    layers: List[Layer] = []
    if drop_input is not None:
        layers.append(Dropout(drop_input))
    for (ch, k, s, pad) in convs:
        layers += [Conv2D(ch, (k, k), (s, s), pad), ReLU()]
    if drop_before_flatten is not None:
        layers.append(Dropout(drop_before_flatten))
    layers.append(Flatten())
    if drop_after_flatten is not None:
        layers.append(Dropout(drop_after_flatten))
    for h in hidden:
        layers += [Linear(h), ReLU()] + ([Dropout(0.5)] if hidden_dropout else [])
    layers += [Linear(nb_classes), Softmax()]
    return MLP(layers, input_shape, rec_model=rec_model)


_BF_CONVS = lambda f: [(f, 8, 2, "SAME"), (2 * f, 6, 2, "VALID"), (2 * f, 5, 1, "VALID")]


def model_f(nb_filters=64, nb_classes=10, input_shape=(None, 28, 28, 1), rec_model=None):
    return _conv_zoo(_BF_CONVS(nb_filters), [], nb_classes, input_shape, rec_model)


def model_b(nb_filters=64, nb_classes=10, input_shape=(None, 28, 28, 1), rec_model=None):
    return _conv_zoo(_BF_CONVS(nb_filters), [], nb_classes, input_shape, rec_model, drop_input=0.2, drop_before_flatten=0.5)


def model_e(input_shape=(None, 28, 28, 1), nb_classes=10):
    return _conv_zoo([], [200, 200], nb_classes, input_shape, None, hidden_dropout=False)


def model_d(input_shape=(None, 28, 28, 1), nb_classes=10):
    m = _conv_zoo([], [200, 200], nb_classes, input_shape, None, hidden_dropout=False)
    layers = list(m.layers)
    layers.insert(3, Dropout(0.5))          # Flatten, Linear(200), ReLU, Dropout(0.5), Linear(200), ReLU, Linear, Softmax
    return MLP(layers, input_shape)


def model_a(nb_filters=64, nb_classes=10, input_shape=(None, 28, 28, 1), rec_model=None):
    return _conv_zoo([(nb_filters, 5, 1, "SAME"), (nb_filters, 5, 2, "VALID")], [128], nb_classes, input_shape, rec_model, 0.25)


def model_c(nb_filters=64, nb_classes=10, input_shape=(None, 28, 28, 1), rec_model=None):
    return _conv_zoo([(nb_filters * 2, 3, 1, "SAME"), (nb_filters, 5, 2, "VALID")], [128], nb_classes, input_shape, rec_model, 0.25)


def model_y(nb_filters=64, nb_classes=10, input_shape=(None, 28, 28, 1), rec_model=None):
    return _conv_zoo([(nb_filters, 3, 1, "SAME"), (nb_filters, 3, 2, "VALID"), (2 * nb_filters, 3, 2, "VALID"),
                      (2 * nb_filters, 3, 2, "VALID")], [256, 256], nb_classes, input_shape, rec_model)


def model_q(nb_filters=32, nb_classes=10, input_shape=(None, 28, 28, 1), rec_model=None):
    return _conv_zoo([(nb_filters, 3, 1, "SAME"), (nb_filters, 3, 2, "VALID"), (2 * nb_filters, 3, 1, "VALID"),
                      (2 * nb_filters, 3, 2, "VALID")], [256, 256], nb_classes, input_shape, rec_model)


def model_z(nb_filters=32, nb_classes=10, input_shape=(None, 28, 28, 1), rec_model=None):
    return _conv_zoo([(nb_filters, 3, 1, "SAME"), (nb_filters, 3, 2, "VALID"), (2 * nb_filters, 3, 1, "VALID"),
                      (2 * nb_filters, 3, 2, "VALID"), (4 * nb_filters, 3, 1, "VALID"), (4 * nb_filters, 3, 2, "VALID")],
                     [600, 600], nb_classes, input_shape, rec_model)


MODELS = {"A": model_a, "B": model_b, "C": model_c, "D": model_d, "E": model_e, "F": model_f, "Y": model_y, "Q": model_q,
          "Z": model_z}


# ---------------------------------------------------------------------- the step BEFORE the path: FGSM
_REC_GRADIENT_NOTE = (
    "the model has the Defense-GAN reconstruction layer attached (add_rec_model): the reference differentiates "
    "THROUGH ReconstructionLayer (whitebox.py:185-214, network_builder.py:266-271), whose gradient w.r.t. its input is "
    "identically zero (the projected latents live in variables updated by ApplyMomentum; the selected restart comes "
    "from an argmin) -- the input gradient is 0 and FGSM returns clip(x).  Build the attack before add_rec_model (or "
    "pass no_rec=True) to differentiate the bare classifier.  For a white-box attack that uses the defense, see BPDA "
    "(the real projection forward, the identity backward, averaged over its random restarts).")


def _mlp_input_gradient(self, x, labels=None, no_rec=False):
    """d(sum_b CE(softmax(logits_b), y_b))/dx on the device; y = ``labels`` (class indices) or the model's own prediction.
    With the reconstruction layer attached the result is the reference's: zeros (see _REC_GRADIENT_NOTE)."""
    import torch
    if self.rec_layer is not None and not no_rec:
        import warnings
        warnings.warn(_REC_GRADIENT_NOTE, stacklevel=2)
        return np.zeros_like(x) if isinstance(x, np.ndarray) else torch.zeros_like(x)
    self._ensure()
    if not self._weights_set:
        raise _native.NativeError("classifier weights not set")
    was_numpy = isinstance(x, np.ndarray)
    dev = torch.device("cuda", self._device)
    t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if was_numpy else x).to(device=dev, dtype=torch.float32).contiguous()
    lab = None
    if labels is not None:
        lab = (torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels).to(device=dev, dtype=torch.int32).contiguous()
    g = torch.empty_like(t)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _native.check(_native.load().dg_clf_input_gradient(self._handle, t.data_ptr(), lab.data_ptr() if lab is not None else None,
                                                           int(t.shape[0]), g.data_ptr(), stream))
    return g.cpu().numpy() if was_numpy else g


MLP.input_gradient = _mlp_input_gradient


def _mlp_backward(self, x, dlogits):
    """d(sum_{b,k} dlogits[b,k] * logits(x)[b,k])/dx on the device (``dg_clf_backward``): the input gradient of any loss on
    the logits, given its seed ``dlogits`` [B, nb_classes].  Bare classifier only (the reconstruction layer is not entered).
    NumPy in gives NumPy out, torch in gives torch out on the caller's current stream."""
    import torch
    self._ensure()
    if not self._weights_set:
        raise _native.NativeError("classifier weights not set")
    was_numpy = isinstance(x, np.ndarray)
    dev = torch.device("cuda", self._device)
    t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if was_numpy else x).to(device=dev, dtype=torch.float32).contiguous()
    d = (torch.from_numpy(np.ascontiguousarray(dlogits, np.float32)) if isinstance(dlogits, np.ndarray) else dlogits)
    d = d.to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() != 4 or tuple(t.shape[1:]) != tuple(self.input_shape[1:]):
        raise ValueError("x must be [B, %s], got %s" % (", ".join(str(v) for v in self.input_shape[1:]), tuple(t.shape)))
    B = int(t.shape[0])
    if tuple(d.shape) != (B, self.nb_classes):
        raise ValueError("dlogits must be [%d, %d], got %s" % (B, self.nb_classes, tuple(d.shape)))
    g = torch.empty_like(t)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _native.check(_native.load().dg_clf_backward(self._handle, t.data_ptr(), d.data_ptr(), B, g.data_ptr(), stream))
    return g.cpu().numpy() if was_numpy else g


MLP.backward = _mlp_backward


_JAC_REC_NOTE = (
    "class_gradient / jacobian on a model with the Defense-GAN reconstruction layer attached (add_rec_model) is not implemented: "
    "the reference takes the Jacobian of the SUBSTITUTE (blackbox.py:170-174), a bare classifier, and the gradient through "
    "ReconstructionLayer is identically zero there (network_builder.py:266-271).  Differentiate the model before add_rec_model.")


def _jacobian_input(self, x):
    """(device tensor [B, H, W, C], was_numpy) for the class-gradient entries: the checks of ``backward``."""
    import torch
    if self.rec_layer is not None:
        raise NotImplementedError(_JAC_REC_NOTE)
    self._ensure()
    if not self._weights_set:
        raise _native.NativeError("classifier weights not set")
    was_numpy = isinstance(x, np.ndarray)
    dev = torch.device("cuda", self._device)
    t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if was_numpy else x).to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() != 4 or tuple(t.shape[1:]) != tuple(self.input_shape[1:]) or int(t.shape[0]) == 0:
        raise ValueError("x must be [B, %s] with B > 0, got %s" % (", ".join(str(v) for v in self.input_shape[1:]), tuple(t.shape)))
    return t, was_numpy


def _class_indices(self, classes, B, what="classes"):
    """int32 device tensor [B].  Class indices on the host are checked against [0, nb_classes); a device tensor is taken as it
    is (an index outside the range gives a zero gradient there, as training's out-of-range label does)."""
    import torch
    dev = torch.device("cuda", self._device)
    if not isinstance(classes, torch.Tensor):
        c = np.asarray(classes)
        if c.ndim == 0:
            c = np.full(B, c)
        if c.shape != (B,) or not (c == np.round(c)).all() or (c < 0).any() or (c >= self.nb_classes).any():
            raise ValueError("%s must be %d class indices in [0, %d)" % (what, B, self.nb_classes))
        classes = torch.from_numpy(np.ascontiguousarray(c.astype(np.int32)))
    elif tuple(classes.shape) != (B,):
        raise ValueError("%s must be [%d], got %s" % (what, B, tuple(classes.shape)))
    return classes.to(device=dev, dtype=torch.int32).contiguous()


def _mlp_class_gradient(self, x, classes, of_probs=True):
    """d out(x)[b, classes[b]] / dx on the device (``dg_clf_class_gradient``): one row of cleverhans' ``jacobian_graph`` per image.
    ``out`` is what ``model(x)`` returns -- the probabilities -- when ``of_probs`` and the model ends in Softmax, otherwise the
    logits.  ``classes``: [B] class indices (or one index for every image).  NumPy in gives NumPy out, torch in gives torch out on
    the caller's current stream.  Bare classifier only (NotImplementedError with the reconstruction layer attached)."""
    import torch
    t, was_numpy = _jacobian_input(self, x)
    B = int(t.shape[0])
    c = _class_indices(self, classes, B)
    g = torch.empty_like(t)
    stream = torch.cuda.current_stream(t.device).cuda_stream
    with torch.cuda.device(t.device):
        _native.check(_native.load().dg_clf_class_gradient(self._handle, t.data_ptr(), c.data_ptr(), B, 1 if of_probs else 0,
                                                           g.data_ptr(), stream))
    return g.cpu().numpy() if was_numpy else g


def _mlp_jacobian(self, x, of_probs=True):
    """[B, nb_classes, H, W, C]: d out(x)[b, k] / dx for every class (``dg_clf_jacobian``: one forward, nb_classes backwards) --
    cleverhans' ``jacobian_graph`` evaluated at ``x``, list index k on axis 1.  Same conventions as ``class_gradient``."""
    import torch
    t, was_numpy = _jacobian_input(self, x)
    B = int(t.shape[0])
    jac = torch.empty((B, self.nb_classes) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
    stream = torch.cuda.current_stream(t.device).cuda_stream
    with torch.cuda.device(t.device):
        _native.check(_native.load().dg_clf_jacobian(self._handle, t.data_ptr(), B, 1 if of_probs else 0, jac.data_ptr(), stream))
    return jac.cpu().numpy() if was_numpy else jac


MLP.class_gradient = _mlp_class_gradient
MLP.jacobian = _mlp_jacobian


_L1_ITERATIVE_NOTE = ("ord = 1 is not implemented for the iterative attacks: the projection onto an L1 ball needs a sort per image; "
                      "ord = np.inf and ord = 2 are")


def _attack_ord(ord, allowed, who):
    """``ord`` as np.inf, 1 or 2 ('inf' and float('inf') are np.inf); anything else, or a value not in ``allowed``, is refused."""
    if isinstance(ord, str):
        ord = {"inf": np.inf, "1": 1, "2": 2}.get(ord.lower(), ord)
    if not isinstance(ord, str) and ord in (np.inf, 1, 2):
        ord = np.inf if ord == np.inf else int(ord)
        if ord in allowed:
            return ord
        if ord == 1:
            raise NotImplementedError("%s: %s" % (who, _L1_ITERATIVE_NOTE))
    raise ValueError("%s: ord must be one of %s, got %r" % (who, ", ".join("np.inf" if a == np.inf else str(a) for a in allowed), ord))


def ball_project_noise(noise, eps):
    """The ``rand_init`` draw for ord = 2: ``noise`` [n, P] (``bpda_rand_noise``, uniform in the L-infinity cube) scaled per image by
    ``min(1, eps / max(1e-12, ||noise||_2))`` onto the L2 ball, in float32 on the host (the norm in float64, rounded once)."""
    noise = np.asarray(noise, np.float32)
    norm = np.sqrt(np.square(noise.astype(np.float64)).sum(axis=1))
    scale = np.minimum(1.0, float(eps) / np.maximum(1e-12, norm)).astype(np.float32)
    return noise * scale[:, None]


def _row_norms(v, w, ord=2):
    """[n] float32 on the device: the per-image ``ord``-norm of ``v - w`` (of ``v`` when ``w`` is None), ``dg_row_norms``; device
    tensors [n, ...] on torch's current stream, not waited for."""
    import torch
    n = int(v.shape[0])
    out = torch.empty(n, dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        _native.check(_native.load().dg_row_norms(v.data_ptr(), w.data_ptr() if w is not None else None, n, int(v.numel() // n), int(ord),
                                                  out.data_ptr(), torch.cuda.current_stream(v.device).cuda_stream))
    return out


class FastGradientMethod(object):
    """The cleverhans attack object the reference instantiates (whitebox.py:198-200, blackbox.py:530-534) with ord = inf:
    ``adv = clip(x + eps * sign(grad_x CE(model(x), y)), clip_min, clip_max)``; without ``y`` the model's own prediction is
    the label (cleverhans' default).  ``ord`` 1 and 2 are cleverhans' as well, the norm per image over its H W C elements
    (``dg_fgm``): ``adv = clip(x + eps * g / max(1e-12, sum|g|), ...)`` and ``adv = clip(x + eps * g / max(1e-12, sqrt(sum g^2)), ...)``;
    a zero gradient gives a zero step.  ``sess`` / ``back`` are accepted for signature compatibility and ignored.

    White-box use on a DEFENDED model (whitebox.py:185-200 attaches the reconstruction layer first, then builds the attack
    on that model): the gradient through the projection is identically zero in the reference, so ``generate`` returns
    ``clip(x, clip_min, clip_max)`` -- reproduced here, with a warning."""

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    def generate(self, x, eps=0.3, ord=np.inf, y=None, clip_min=None, clip_max=None, **kwargs):
        import torch
        ord = _attack_ord(ord, (np.inf, 1, 2), "FastGradientMethod")
        m = self.model
        m._ensure()
        was_numpy = isinstance(x, np.ndarray)
        dev = torch.device("cuda", m._device)
        t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if was_numpy else x).to(device=dev, dtype=torch.float32).contiguous()
        lo = float("-inf") if clip_min is None else float(clip_min)
        hi = float("inf") if clip_max is None else float(clip_max)
        if m.rec_layer is not None:
            import warnings
            warnings.warn(_REC_GRADIENT_NOTE, stacklevel=2)
            out = torch.clamp(t, lo, hi)                 # x + eps * sign(0)
            return out.cpu().numpy() if was_numpy else out
        lab = None
        if y is not None:
            yy = y if isinstance(y, np.ndarray) else y.detach().cpu().numpy()
            if yy.ndim > 1:
                yy = yy.argmax(axis=-1)                            # one-hot labels as cleverhans takes them
            lab = torch.from_numpy(np.ascontiguousarray(yy)).to(device=dev, dtype=torch.int32)
        out = torch.empty_like(t)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            if ord == np.inf:
                _native.check(_native.load().dg_fgsm(m._handle, t.data_ptr(), lab.data_ptr() if lab is not None else None,
                                                     int(t.shape[0]), float(eps), lo, hi, out.data_ptr(), stream))
            else:
                _native.check(_native.load().dg_fgm(m._handle, t.data_ptr(), lab.data_ptr() if lab is not None else None,
                                                    int(t.shape[0]), float(eps), int(ord), lo, hi, out.data_ptr(), stream))
        return out.cpu().numpy() if was_numpy else out


_CW_REC_NOTE = (
    "CarliniWagnerL2 on a model with the Defense-GAN reconstruction layer attached (add_rec_model) is not implemented: in the "
    "reference the gradient through ReconstructionLayer is identically zero (network_builder.py:266-271), so the attack "
    "there reduces to repeated defended evaluations of the tanh round trip of x, whose per-iteration latent draws cannot be "
    "pinned.  Build the attack before add_rec_model, or on a model without it (no_rec), as bench.py's --strong flow does for "
    "FGSM.  The white-box attack that does use the defense is BPDA (L-infinity, projected sign gradient).")


class CarliniWagnerL2(object):
    """cleverhans' CarliniWagnerL2 (the reference's ``--attack_type cw``, whitebox.py:201-209), restated and run as ONE
    asynchronous device call (``dg_cw``; the algorithm is in defensegan_amd/csrc/dg_cw.hip's header comment and DESIGN.md
    section 7).  ``sess`` / ``back`` are accepted for signature compatibility and ignored.

    ``generate(x, y=None, y_target=None, **params)``: NumPy in gives NumPy out, a torch tensor in gives a tensor out (on the
    caller's current stream, not waited for); ``y`` / ``y_target`` one-hot or class indices; without either the label is the
    model's own first argmax on ``x``.  ``return_info=True`` also returns ``(best_l2, best_class)`` (1e10 / -1 where no step
    succeeded); ``return_search=True`` then also ``(final_const [B] float64, chunk_stop [binary_search_steps, chunks] int32)``:
    the constants after the last binary-search update and the iteration at whose check each chunk stopped (-1: it ran to
    max_iterations).  ``nb_classes`` and ``feed`` are accepted and ignored.

    ``abort_early`` changes which iterations count, not how long the call takes: a stopped chunk skips the attack's own
    kernels, but the classifier's forward and backward keep running over every image until max_iterations.

    The defaults are those of cleverhans 2.x ``generate`` as remembered (batch_size=1, confidence=0, learning_rate=5e-3,
    binary_search_steps=5, max_iterations=1000, abort_early=True, initial_const=1e-2, clip_min=0, clip_max=1): nothing in the
    reference pins them (cleverhans is an empty, un-pinned submodule).  Only the white-box setting is pinned:
    ``binary_search_steps=1, max_iterations=100, learning_rate=10, initial_const=100, batch_size=BATCH_SIZE`` and no clip
    bounds, so CelebA inputs are clipped to [0, 1] as well -- a quirk of the reference kept here.

    A model with the reconstruction layer attached raises NotImplementedError (see _CW_REC_NOTE)."""

    DEFAULTS = dict(batch_size=1, confidence=0.0, learning_rate=5e-3, binary_search_steps=5, max_iterations=1000, abort_early=True,
                    initial_const=1e-2, clip_min=0.0, clip_max=1.0)

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    def generate(self, x, y=None, y_target=None, return_info=False, return_search=False, nb_classes=None, feed=None, **params):
        import torch
        unknown = set(params) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("unknown CarliniWagnerL2 parameters: %s" % sorted(unknown))
        p = dict(self.DEFAULTS, **params)
        m = self.model
        if m.rec_layer is not None:
            raise NotImplementedError(_CW_REC_NOTE)
        if y is not None and y_target is not None:
            raise ValueError("give y or y_target, not both")
        m._ensure()
        if not m._weights_set:
            raise _native.NativeError("classifier weights not set")
        was_numpy = isinstance(x, np.ndarray)
        dev = torch.device("cuda", m._device)
        t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if was_numpy else x).to(device=dev, dtype=torch.float32).contiguous()
        if t.dim() != 4 or tuple(t.shape[1:]) != tuple(m.input_shape[1:]):
            raise ValueError("x must be [B, %s], got %s" % (", ".join(str(d) for d in m.input_shape[1:]), tuple(t.shape)))
        B = int(t.shape[0])
        if B == 0:
            raise ValueError("x holds no images")
        lab, targeted = None, y_target is not None
        yy = y_target if targeted else y
        if yy is not None:
            yy = np.asarray(yy if isinstance(yy, np.ndarray) else yy.detach().cpu().numpy())
            if yy.ndim > 1:
                yy = yy.argmax(axis=-1)                            # one-hot labels as cleverhans takes them
            if yy.shape != (B,) or (yy < 0).any() or (yy >= m.nb_classes).any():
                raise ValueError("labels must be %d class indices in [0, %d) or one-hot rows" % (B, m.nb_classes))
            lab = torch.from_numpy(np.ascontiguousarray(yy)).to(device=dev, dtype=torch.int32)
        out = torch.empty_like(t)
        best_l2 = torch.empty(B, dtype=torch.float32, device=dev)
        best_class = torch.empty(B, dtype=torch.int32, device=dev)
        nsteps, chunks = max(int(p["binary_search_steps"]), 0), -(-B // max(int(p["batch_size"]), 1))
        final_const = torch.empty(B, dtype=torch.float64, device=dev)
        chunk_stop = torch.empty(nsteps, chunks, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _native.check(_native.load().dg_cw(
                m._handle, t.data_ptr(), lab.data_ptr() if lab is not None else None, B, 1 if targeted else 0, int(p["batch_size"]),
                float(p["confidence"]), float(p["learning_rate"]), int(p["binary_search_steps"]), int(p["max_iterations"]),
                1 if p["abort_early"] else 0, float(p["initial_const"]), float(p["clip_min"]), float(p["clip_max"]), out.data_ptr(),
                best_l2.data_ptr(), best_class.data_ptr(), final_const.data_ptr() if return_search else None,
                chunk_stop.data_ptr() if return_search else None, stream))
        res = (out, best_l2, best_class) + ((final_const, chunk_stop) if return_search else ())
        if was_numpy:
            res = tuple(r.cpu().numpy() for r in res)
        if not return_info:
            return res[0]
        return res if return_search else res[:3]


# ---------------------------------------------------------------------- the attack that sees the defense: BPDA / EOT
BPDA_NOISE_TAG = 0x42504441          # "BPDA": word 3 of the rand_init counter (the latents' draw has 0 there, dg_small.hip)
BPDA_DEFAULT_SEED = 11241990         # model_eval_gan's default: without ``seed`` iteration 0 sees the evaluation's own latents


def _philox4x32_10(ctr, key):
    """Random123's Philox4x32-10 on the host: ctr [N, 4] uint32 values, key (k0, k1) -> [N, 4] uint64 arrays holding uint32
    words.  The generator of the latent init and of Dropout (csrc/dg_shared_math.h), restated for the one draw made on the host."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(ctr[:, i], np.uint64) & M for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, axis=1)


def bpda_rand_noise(n_images: int, row_elems: int, eps: float, seed: int, first_image: int = 0) -> np.ndarray:
    """The ``rand_init`` draw of BPDA, float32 [n_images, row_elems] in [-eps, eps): element e of the image with GLOBAL index
    i = first_image + row takes word e % 4 of Philox4x32-10(key = (seed lo, seed hi), counter = (e // 4, i lo, i hi,
    BPDA_NOISE_TAG)); u = (word >> 8) * 2^-24 in [0, 1); noise = float32(eps) * (2 u - 1), one float32 rounding (2 u - 1 is exact).
    Keyed by the image, so the draw does not depend on how the images are batched.  Drawn once per attack, on the host."""
    n_images, row_elems, seed = int(n_images), int(row_elems), int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (row_elems + 3) // 4
    img = (np.arange(n_images, dtype=np.uint64) + np.uint64(int(first_image)))[:, None]
    ctr = np.empty((n_images, nq, 4), np.uint64)
    ctr[:, :, 0] = np.arange(nq, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = img & np.uint64(0xFFFFFFFF)
    ctr[:, :, 2] = img >> np.uint64(32)
    ctr[:, :, 3] = BPDA_NOISE_TAG
    words = _philox4x32_10(ctr.reshape(-1, 4), (seed & 0xFFFFFFFF, seed >> 32)).reshape(n_images, nq * 4)[:, :row_elems]
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (np.float32(eps) * (np.float32(2.0) * u - np.float32(1.0))).astype(np.float32)


def bpda_seed_schedule(seed: int, nb_iter: int, eot_samples: int):
    """``(per_iteration, final)``: ``per_iteration[k][s] = seed + k * eot_samples + s`` is the latent seed of EOT sample s of
    iteration k, ``final = seed + nb_iter * eot_samples`` that of the projection that judges the last iterate."""
    m = int(eot_samples)
    return [[int(seed) + k * m + s for s in range(m)] for k in range(int(nb_iter))], int(seed) + int(nb_iter) * m


class _AttackDeviceOps(object):
    """What the device operations of the iterative attacks on a (defended) model share: the classifier, its projection's model (or
    None), the device; the prediction on a batch; the best tracking."""

    def __init__(self, model: MLP):
        import torch
        model._ensure()
        if not model._weights_set:
            raise _native.NativeError("classifier weights not set")
        self.model, self.gan = model, (model.rec_layer.rec_model if model.rec_layer is not None else None)
        self.device = torch.device("cuda", model._device)

    def predict(self, rec):
        """[B] int32: the classifier's first argmax on ``rec`` (dg_eval_batch)."""
        return self.model.eval_batch(rec, None, None, sync=False)[1]

    def track(self, preds, labels, k, x_iter, x_best, first_success):
        """dg_bpda_track: images still without a success take iterate k as their best, and k as their first success where
        ``preds != labels``."""
        import torch
        B = int(preds.shape[0])
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_bpda_track(
                preds.data_ptr(), labels.data_ptr(), B, int(k), x_iter.data_ptr(), x_best.data_ptr(), first_success.data_ptr(),
                int(x_iter.numel() // B), torch.cuda.current_stream(self.device).cuda_stream))


class BpdaDeviceOps(_AttackDeviceOps):
    """The device operations ``BPDA.generate`` is made of (``step_ball`` and ``dist`` only with ``ord = 2``), on tensors of the classifier's device and torch's current stream;
    none of them waits for the device.  (``BPDA`` takes any object with these methods and a ``device``: the tests drive the loop
    with a recording stand-in.)  ``predict`` and ``track`` are the base class's."""

    def project(self, x, seed, first_row):
        """gan.reconstruct: latents drawn as dg_init_latents does for (seed, first_row + row)."""
        return self.gan.reconstruct(x, seed=int(seed), first_row=int(first_row))

    def step(self, rec, labels, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, clip_min, clip_max, x_next):
        """dg_bpda_step: the classifier's input gradient at ``rec``, then ``gsum += g`` (accumulate_only) or the projected sign
        step of ``gsum + g`` from ``x_cur`` around ``x_orig`` into ``x_next``."""
        import torch
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_bpda_step(
                self.model._handle, rec.data_ptr(), labels.data_ptr(), int(rec.shape[0]), ptr(x_cur), ptr(x_orig), ptr(gsum),
                1 if accumulate_only else 0, float(eps), float(eps_iter), float(clip_min), float(clip_max), ptr(x_next),
                torch.cuda.current_stream(self.device).cuda_stream))

    def step_ball(self, rec, labels, x_cur, x_orig, gsum, accumulate_only, eps, eps_iter, ord, clip_min, clip_max, x_next):
        """dg_bpda_step_ball: ``step`` with the L2 step (``ord`` = 2) in the projected sign step's place."""
        import torch
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_bpda_step_ball(
                self.model._handle, rec.data_ptr(), labels.data_ptr(), int(rec.shape[0]), ptr(x_cur), ptr(x_orig), ptr(gsum),
                1 if accumulate_only else 0, float(eps), float(eps_iter), int(ord), float(clip_min), float(clip_max), ptr(x_next),
                torch.cuda.current_stream(self.device).cuda_stream))

    def dist(self, x_adv, x_orig):
        """dg_row_norms: [n] float32, the per-image L2 distance of ``x_adv`` from ``x_orig``."""
        return _row_norms(x_adv, x_orig, 2)


class BPDA(object):
    """The white-box attack that uses the defense: BPDA with EOT (Athalye, Carlini, Wagner 2018), L-infinity, on a model with
    the Defense-GAN projection attached (``add_rec_model``).  Not in the reference, whose attacks differentiate through
    ``ReconstructionLayer`` and see a zero gradient (_REC_GRADIENT_NOTE).  The projection runs for real in the forward pass and
    counts as the identity in the backward pass; the gradient is summed over ``eot_samples`` projections with fresh latents:

        x_0 = clip(x)            (``rand_init``: clip(x + bpda_rand_noise(...)); or ``x_init`` as given)
        for k < nb_iter:   g_k = sum_{s < m} grad_r CE(logits(r), y) at r = reconstruct(x_k; latents of seed + k m + s)
                           x_{k+1} = clip(x + clamp(x_k + eps_iter sign(g_k) - x, -eps, eps), clip_min, clip_max),  sign(0) = 0

    Best tracking on the device: iterate k + 1 succeeds for an image when the defended prediction on it is not ``y``; that
    prediction is read off the next iteration's first projection (s = 0), the last iterate's off one more projection with seed
    ``seed + nb_iter m`` -- ``nb_iter * m + 1`` projections in all, enqueued with no host read in between.  ``generate`` returns
    per image the first successful iterate, or the last iterate; ``return_info=True`` adds ``first_success`` [n] int32 (the
    iterate's index in 1 .. nb_iter, or -1).

    ``ord = 2`` (default np.inf) bounds the perturbation in L2 instead, every norm per image over its H W C elements:
    ``u = g_k / max(1e-12, ||g_k||)``, ``d = (x_k + eps_iter u) - x``, ``x_{k+1} = clip(x + d min(1, eps / max(1e-12, ||d||)), ...)``
    (``dg_bpda_step_ball``; a zero gradient gives a zero step); ``rand_init`` then draws ``ball_project_noise(bpda_rand_noise(...))``,
    the same draw scaled onto the L2 ball on the host; and ``return_info=True`` returns a third value, ``dist`` [n] float32, the
    distance ``||x_adv - x||_2`` (``dg_row_norms``).  ``ord = 1`` raises NotImplementedError: its projection needs a sort.

    ``x`` NumPy or a device tensor [n, H, W, C] in generator range (NumPy in gives NumPy out; a tensor gives tensors on the
    caller's current stream, not waited for); ``y`` class indices or one-hot rows, required.  ``seed`` defaults to
    BPDA_DEFAULT_SEED.  The latents of image i are rows ``i * rec_rr + r`` of the seeded stream and every classifier output is
    one thread's fixed-order sum, so the result does not depend on ``batch_size``, bit for bit: ``batch_size`` (default: the
    reconstruction layer's) only bounds the images per engine call, and consecutive batches are coalesced into engine calls as
    in ``gan_defense.model_eval_gan``.  With a USE_BN generator the rows of an engine call share its Batchnorm statistics: the
    calls are then cut on ``batch_size`` exactly, and the result DOES depend on it.

    A bare model raises ValueError: projected gradient descent on an undefended classifier is ``ProjectedGradientDescent``.  A
    reconstruction layer with a fixed ``z_init`` is refused as well (the attack draws fresh latents for every projection)."""

    def __init__(self, model: MLP, back="tf", sess=None, ops=None):
        self.model = model
        self._ops = ops

    def generate(self, x, y, eps=0.3, eps_iter=0.05, nb_iter=10, eot_samples=1, clip_min=None, clip_max=None, rand_init=False,
                 seed=None, x_init=None, batch_size=None, return_info=False, ord=np.inf):
        import torch
        from . import gan_defense
        ord = _attack_ord(ord, (np.inf, 2), "BPDA")
        m = self.model
        rl = m.rec_layer
        if rl is None:
            raise ValueError("BPDA attacks a model with the Defense-GAN projection attached (add_rec_model); projected gradient "
                             "descent on a bare classifier (PGD-on-bare) is ProjectedGradientDescent")
        if rl.z_init is not None:
            raise ValueError("BPDA draws fresh latents for every projection; the reconstruction layer has a fixed z_init")
        nb_iter, mm = int(nb_iter), int(eot_samples)
        if nb_iter < 1:
            raise ValueError("nb_iter must be >= 1, got %d" % nb_iter)
        if mm < 1:
            raise ValueError("eot_samples must be >= 1, got %d" % mm)
        if not (float(eps) >= 0 and float(eps_iter) >= 0):
            raise ValueError("eps and eps_iter must be >= 0")
        if rand_init and x_init is not None:
            raise ValueError("give rand_init or x_init, not both")
        lo = float("-inf") if clip_min is None else float(clip_min)
        hi = float("inf") if clip_max is None else float(clip_max)
        if not lo <= hi:
            raise ValueError("clip_min must not exceed clip_max")
        seed = BPDA_DEFAULT_SEED if seed is None else int(seed)
        ops = self._ops if self._ops is not None else BpdaDeviceOps(m)
        dev = ops.device
        was_numpy = isinstance(x, np.ndarray)
        to = lambda a: (torch.from_numpy(np.ascontiguousarray(a, np.float32)) if isinstance(a, np.ndarray) else a).to(device=dev, dtype=torch.float32).contiguous()
        t = to(x)
        if t.dim() != 4 or tuple(t.shape[1:]) != tuple(m.input_shape[1:]) or int(t.shape[0]) == 0:
            raise ValueError("x must be [n, %s] with n > 0, got %s" % (", ".join(str(d) for d in m.input_shape[1:]), tuple(t.shape)))
        n, P = int(t.shape[0]), int(t[0].numel())
        yy = np.asarray(y if isinstance(y, np.ndarray) else (y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y))
        if yy.ndim > 1:
            yy = yy.argmax(axis=-1)                                # one-hot labels as cleverhans takes them
        if yy.shape != (n,):
            raise ValueError("y must be %d class indices or one-hot rows" % n)
        lab = torch.from_numpy(np.ascontiguousarray(yy.astype(np.int32))).to(dev)
        if x_init is not None:
            x_cur = to(x_init).clone()
            if tuple(x_cur.shape) != tuple(t.shape):
                raise ValueError("x_init must have x's shape")
        elif rand_init:
            noise = bpda_rand_noise(n, P, eps, seed)
            noise = torch.from_numpy(noise if ord == np.inf else ball_project_noise(noise, eps)).to(dev).view_as(t)
            x_cur = torch.clamp(t + noise, lo, hi)
        else:
            x_cur = torch.clamp(t, lo, hi)
        gan = rl.rec_model
        R = int(gan.rec_rr)
        bs = int(batch_size or rl.batch_size or n)
        if bs < 1:
            raise ValueError("batch_size must be >= 1")
        step_n = gan_defense.engine_step(gan.reconstruct, bs, R, n)
        cuts = [(a, min(n, a + step_n)) for a in range(0, n, step_n)]
        x_next, x_best = torch.empty_like(x_cur), torch.empty_like(x_cur)
        first_success = torch.full((n,), -1, dtype=torch.int32, device=dev)
        gsum = torch.empty_like(x_cur) if mm > 1 else None
        seeds, final_seed = bpda_seed_schedule(seed, nb_iter, mm)
        for k in range(nb_iter):
            if gsum is not None:
                gsum.zero_()
            for s in range(mm):
                for a, b in cuts:
                    rec = ops.project(x_cur[a:b], seeds[k][s], a * R)
                    if s == 0 and k > 0:                           # rec_{k,0} is the defended view of iterate k
                        ops.track(ops.predict(rec), lab[a:b], k, x_cur[a:b], x_best[a:b], first_success[a:b])
                    gs = gsum[a:b] if gsum is not None else None
                    if ord == np.inf:
                        ops.step(rec, lab[a:b], x_cur[a:b], t[a:b], gs, s < mm - 1, eps, eps_iter, lo, hi, x_next[a:b])
                    else:
                        ops.step_ball(rec, lab[a:b], x_cur[a:b], t[a:b], gs, s < mm - 1, eps, eps_iter, ord, lo, hi, x_next[a:b])
            x_cur, x_next = x_next, x_cur
        for a, b in cuts:
            rec = ops.project(x_cur[a:b], final_seed, a * R)
            ops.track(ops.predict(rec), lab[a:b], nb_iter, x_cur[a:b], x_best[a:b], first_success[a:b])
        info = (first_success,) if ord == np.inf or not return_info else (first_success, ops.dist(x_best, t))
        if was_numpy:
            x_best, info = x_best.cpu().numpy(), tuple(v.cpu().numpy() for v in info)
        return (x_best,) + info if return_info else x_best


class ProjectedGradientDescent(object):
    """Projected gradient descent (Madry et al. 2018), L-infinity, on a BARE classifier: ``BPDA`` with the identity as the projection
    and ``eot_samples = 1``, run as ONE asynchronous device call per ``batch_size`` images (``dg_pgd``, defensegan_amd/csrc/dg_pgd.hip):

        x_0 = clip(x)            (``rand_init``: clip(x + bpda_rand_noise(...)); or ``x_init`` as given)
        for k < nb_iter:   g_k = grad_x CE(logits(x_k), y)                     (``input_gradient``'s bits)
                           x_{k+1} = clip(x + clamp(x_k + eps_iter sign(g_k) - x, -eps, eps), clip_min, clip_max),  sign(0) = 0

    Best tracking as BPDA's: iterate k + 1 succeeds for an image when the model's prediction on it is not ``y``; ``generate``
    returns per image the first successful iterate, or the last one; ``return_info=True`` adds ``first_success`` [n] int32 (the
    iterate's index in 1 .. nb_iter, or -1).  The prediction is read off the logits the next iteration's forward keeps:
    ``nb_iter + 1`` forwards and ``nb_iter`` backwards in all.

    ``ord = 2`` (default np.inf) is the L2 attack, as ``BPDA``'s: the step ``u = g_k / max(1e-12, ||g_k||)``, ``d = (x_k + eps_iter u) - x``,
    ``x_{k+1} = clip(x + d min(1, eps / max(1e-12, ||d||)), ...)`` with every norm per image (``dg_pgd_ball``, still one device call);
    ``rand_init`` draws ``ball_project_noise(bpda_rand_noise(...))`` on the host; ``return_info=True`` returns a third value, ``dist`` [n]
    float32 = ``||x_adv - x||_2`` (``dg_row_norms``).  ``ord = 1`` raises NotImplementedError: its projection needs a sort.

    ``x`` NumPy or a device tensor [n, H, W, C] (NumPy in gives NumPy out; a tensor gives tensors on the caller's current stream,
    not waited for); ``y`` class indices or one-hot rows, required; a class index outside [0, nb_classes) gives that image a zero
    gradient (training's policy): it stays at x_0.  ``seed`` (default BPDA_DEFAULT_SEED) keys the ``rand_init`` draw, by the
    image.  ``batch_size`` only bounds the images per device call (default: all): every output element is one thread's
    fixed-order arithmetic on its own image, so the result does not depend on it, bit for bit.

    A model with the reconstruction layer attached raises ValueError: the attack that uses the defense is ``BPDA``."""

    def __init__(self, model: MLP, back="tf", sess=None):
        self.model = model

    def generate(self, x, y, eps=0.3, eps_iter=0.05, nb_iter=10, clip_min=None, clip_max=None, rand_init=False, seed=None, x_init=None,
                 batch_size=None, return_info=False, ord=np.inf):
        import torch
        ord = _attack_ord(ord, (np.inf, 2), "ProjectedGradientDescent")
        m = self.model
        if m.rec_layer is not None:
            raise ValueError("ProjectedGradientDescent attacks a bare classifier; this model has the Defense-GAN projection attached "
                             "(add_rec_model), through which the gradient is identically zero: use BPDA")
        nb_iter = int(nb_iter)
        if nb_iter < 1:
            raise ValueError("nb_iter must be >= 1, got %d" % nb_iter)
        if not (float(eps) >= 0 and float(eps_iter) >= 0):
            raise ValueError("eps and eps_iter must be >= 0")
        if rand_init and x_init is not None:
            raise ValueError("give rand_init or x_init, not both")
        lo = float("-inf") if clip_min is None else float(clip_min)
        hi = float("inf") if clip_max is None else float(clip_max)
        if not lo <= hi:
            raise ValueError("clip_min must not exceed clip_max")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        seed = BPDA_DEFAULT_SEED if seed is None else int(seed)
        m._ensure()
        if not m._weights_set:
            raise _native.NativeError("classifier weights not set")
        dev = torch.device("cuda", m._device)
        was_numpy = isinstance(x, np.ndarray)
        to = lambda a: (torch.from_numpy(np.ascontiguousarray(a, np.float32)) if isinstance(a, np.ndarray) else a).to(device=dev, dtype=torch.float32).contiguous()
        t = to(x)
        if t.dim() != 4 or tuple(t.shape[1:]) != tuple(m.input_shape[1:]) or int(t.shape[0]) == 0:
            raise ValueError("x must be [n, %s] with n > 0, got %s" % (", ".join(str(d) for d in m.input_shape[1:]), tuple(t.shape)))
        n, P = int(t.shape[0]), int(t[0].numel())
        yy = np.asarray(y if isinstance(y, np.ndarray) else (y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y))
        if yy.ndim > 1:
            yy = yy.argmax(axis=-1)                                # one-hot labels as cleverhans takes them
        if yy.shape != (n,):
            raise ValueError("y must be %d class indices or one-hot rows" % n)
        lab = torch.from_numpy(np.ascontiguousarray(yy.astype(np.int32))).to(dev)
        if x_init is not None:
            x0 = to(x_init)
            if tuple(x0.shape) != tuple(t.shape):
                raise ValueError("x_init must have x's shape")
        elif rand_init:
            noise = bpda_rand_noise(n, P, eps, seed)
            x0 = torch.clamp(t + torch.from_numpy(noise if ord == np.inf else ball_project_noise(noise, eps)).to(dev).view_as(t), lo, hi)
        else:
            x0 = torch.clamp(t, lo, hi)
        x_adv = torch.empty_like(t)
        first_success = torch.empty(n, dtype=torch.int32, device=dev)
        bs = n if batch_size is None else int(batch_size)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            for a in range(0, n, bs):
                b = min(n, a + bs)
                if ord == np.inf:
                    _native.check(_native.load().dg_pgd(m._handle, t[a:b].data_ptr(), x0[a:b].data_ptr(), lab[a:b].data_ptr(), b - a, float(eps),
                                                        float(eps_iter), nb_iter, lo, hi, x_adv[a:b].data_ptr(), first_success[a:b].data_ptr(),
                                                        stream))
                else:
                    _native.check(_native.load().dg_pgd_ball(m._handle, t[a:b].data_ptr(), x0[a:b].data_ptr(), lab[a:b].data_ptr(), b - a,
                                                             float(eps), float(eps_iter), nb_iter, ord, lo, hi, x_adv[a:b].data_ptr(),
                                                             first_success[a:b].data_ptr(), stream))
        info = (first_success,) if ord == np.inf or not return_info else (first_success, _row_norms(x_adv, t, 2))
        if was_numpy:
            x_adv, info = x_adv.cpu().numpy(), tuple(v.cpu().numpy() for v in info)
        return (x_adv,) + info if return_info else x_adv


# ---------------------------------------------------------------------- the score-based black-box attack: SPSA
class SpsaDeviceOps(_AttackDeviceOps):
    """The device operations ``SPSA.generate`` is made of, on tensors of the classifier's device and torch's current stream; none
    of them waits for the device.  (``SPSA`` takes any object with these methods and a ``device``: the tests drive the loop with a
    recording stand-in.)  ``predict`` and ``track`` are the base class's."""

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def queries(self, x_cur, n, delta, seed, first_image, k, clip_min, clip_max, q):
        """dg_spsa_queries: the 2 n + 1 queries of every image of ``x_cur`` [B, ...] into ``q`` [B (2 n + 1), ...]."""
        import torch
        B = int(x_cur.shape[0])
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_spsa_queries(
                x_cur.data_ptr(), B, int(x_cur.numel() // B), int(n), float(delta), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image), int(k),
                float(clip_min), float(clip_max), q.data_ptr(), self._stream()))

    def project(self, q, seed, first_row, row_step=None):
        """The defended model's projection of ``q``: row j takes the latents ``first_row + j * row_step + r``, r < rec_rr, of the
        stream of ``seed``.  ``row_step`` None = rec_rr, consecutive rows: one ``gan.reconstruct``; any other step (the closing
        pass, whose images lie 2 n + 1 queries apart) draws each row's latents with ``init_latents`` and hands them over as z0 --
        the values ``reconstruct`` would have drawn.  On a bare model: the identity."""
        import torch
        if self.gan is None:
            return q
        R = int(self.gan.rec_rr)
        if row_step is None or int(row_step) == R or int(q.shape[0]) == 1:
            return self.gan.reconstruct(q, seed=int(seed), first_row=int(first_row))
        z0 = torch.cat([self.gan.init_latents(R, seed=int(seed), first_row=int(first_row) + j * int(row_step)) for j in range(int(q.shape[0]))])
        return self.gan.reconstruct(q, z_init_val=z0, seed=int(seed))

    def logits(self, rec):
        """[B, classes] float32: the classifier's logits on ``rec`` (dg_clf_forward)."""
        import torch
        B = int(rec.shape[0])
        out = torch.empty(B, self.model.nb_classes, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_clf_forward(self.model._handle, rec.data_ptr(), B, out.data_ptr(), None, self._stream()))
        return out

    def step(self, logits, labels, n, delta, seed, first_image, k, x_cur, x_orig, eps, eps_iter, clip_min, clip_max, x_next, out_grad=None):
        """dg_spsa_step: margins, the estimate and the projected sign step from ``x_cur`` around ``x_orig`` into ``x_next``."""
        import torch
        B = int(x_cur.shape[0])
        with torch.cuda.device(self.device):
            _native.check(_native.load().dg_spsa_step(
                logits.data_ptr(), labels.data_ptr(), B, int(logits.shape[1]), int(x_cur.numel() // B), int(n), float(delta),
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_image), int(k), x_cur.data_ptr(), x_orig.data_ptr(), float(eps), float(eps_iter),
                float(clip_min), float(clip_max), x_next.data_ptr(), out_grad.data_ptr() if out_grad is not None else None, self._stream()))


class SPSA(object):
    """The score-based black-box attack: SPSA (Uesato et al. 2018) with Rademacher directions and the projected sign step of
    ``ProjectedGradientDescent`` and ``BPDA``, L-infinity.  It reads only the attacked model's logits, so it attacks the DEFENDED
    model (``add_rec_model``), whose gradient is identically zero (_REC_GRADIENT_NOTE), as well as a bare classifier, where the
    identity stands in for the projection.  Not in the reference.  With ``n = spsa_samples``, ``g`` an image's index in ``x``:

        x_0 = clip(x)
        for k < nb_iter:   u_i[e] = +-1 by bit (i & 31) of word (e & 3) of Philox4x32-10(key = seed, counter = (e >> 2, g,
                                    k ceil(n / 32) + (i >> 5), 0x53505341))                                            i < n
                           q_0 = x_k,  q+_i = clip(x_k + delta u_i),  q-_i = clip(x_k - delta u_i)     (2 n + 1 queries, clipped)
                           L(q) = max_{j != y} Z_j - Z_y  on the logits Z of the model (through the projection) at q
                           ghat = (1 / (2 delta n)) sum_i (L(q+_i) - L(q-_i)) u_i          (float32, ascending i; dg_spsa_step)
                           x_{k+1} = clip(x + clamp(x_k + eps_iter sign(ghat) - x, -eps, eps), clip_min, clip_max),  sign(0) = 0

    A label outside [0, classes) gives L = 0 and a zero step; a pair whose loss difference is not finite contributes 0.  Best
    tracking as BPDA's: iterate j = 1 .. nb_iter succeeds when the model's first arg-max on ITS query 0 is not ``y`` (iteration j's
    query 0 is x_j; iterate nb_iter is judged by one closing query per image); ``generate`` returns per image the first successful
    iterate, or else the last one.  ``return_info=True`` adds ``first_success`` [n] int32 (1 .. nb_iter, or -1) and ``queries``,
    the queries spent per image: ``nb_iter * (2 n + 1) + 1``.

    Defended model: iteration k projects with latent seed ``seed + k``, the closing pass with ``seed + nb_iter``; the latents of
    query c of image g are rows ``(g (2 n + 1) + c) rec_rr + r`` of that stream.  ``batch_size`` (default: the reconstruction
    layer's, else all) bounds the images whose queries are alive at once, and their flat query range is cut into engine calls by
    ``gan_defense.engine_step``; every row of the engine and every element of the two kernels is computed independently of its
    batch, so the result depends on neither, bit for bit.  On a bare model no latent seeds are used.

    ``x`` NumPy or a device tensor [n, H, W, C] (NumPy in gives NumPy out; a tensor gives tensors on the caller's current stream,
    not waited for); ``y`` class indices or one-hot rows, required.  ``seed`` defaults to BPDA_DEFAULT_SEED.  No host read is made
    inside the attack.  A reconstruction layer with a fixed ``z_init`` is a ValueError (every projection draws fresh latents); a
    USE_BN generator a NotImplementedError (its batch statistics would couple an image's queries to the cut)."""

    def __init__(self, model: MLP, back="tf", sess=None, ops=None):
        self.model = model
        self._ops = ops

    def generate(self, x, y, eps=0.3, eps_iter=0.05, nb_iter=10, spsa_samples=32, delta=0.01, clip_min=None, clip_max=None, seed=None,
                 batch_size=None, return_info=False):
        import torch
        from . import gan_defense
        m = self.model
        rl = m.rec_layer
        gan = rl.rec_model if rl is not None else None
        if rl is not None and rl.z_init is not None:
            raise ValueError("SPSA draws fresh latents for every projection; the reconstruction layer has a fixed z_init")
        if gan is not None and bool(getattr(gan, "use_bn", False)):
            raise NotImplementedError("SPSA on a USE_BN generator: its batch statistics would couple an image's queries to how the "
                                      "engine calls are cut")
        nb_iter, ns = int(nb_iter), int(spsa_samples)
        if nb_iter < 1:
            raise ValueError("nb_iter must be >= 1, got %d" % nb_iter)
        if ns < 1:
            raise ValueError("spsa_samples must be >= 1, got %d" % ns)
        if not float(delta) > 0:
            raise ValueError("delta must be > 0")
        if not (float(eps) >= 0 and float(eps_iter) >= 0):
            raise ValueError("eps and eps_iter must be >= 0")
        lo = float("-inf") if clip_min is None else float(clip_min)
        hi = float("inf") if clip_max is None else float(clip_max)
        if not lo <= hi:
            raise ValueError("clip_min must not exceed clip_max")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        seed = BPDA_DEFAULT_SEED if seed is None else int(seed)
        ops = self._ops if self._ops is not None else SpsaDeviceOps(m)
        dev = ops.device
        was_numpy = isinstance(x, np.ndarray)
        t = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if was_numpy else x).to(device=dev, dtype=torch.float32).contiguous()
        if t.dim() != 4 or tuple(t.shape[1:]) != tuple(m.input_shape[1:]) or int(t.shape[0]) == 0:
            raise ValueError("x must be [n, %s] with n > 0, got %s" % (", ".join(str(d) for d in m.input_shape[1:]), tuple(t.shape)))
        n = int(t.shape[0])
        yy = np.asarray(y if isinstance(y, np.ndarray) else (y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y))
        if yy.ndim > 1:
            yy = yy.argmax(axis=-1)                                # one-hot labels as cleverhans takes them
        if yy.shape != (n,):
            raise ValueError("y must be %d class indices or one-hot rows" % n)
        lab = torch.from_numpy(np.ascontiguousarray(yy.astype(np.int32))).to(dev)
        Q = 2 * ns + 1                                             # queries per image and iteration
        R = int(gan.rec_rr) if gan is not None else 1
        bs = min(n, int(batch_size or (rl.batch_size if rl is not None else None) or n))
        chunks = [(a, min(n, a + bs)) for a in range(0, n, bs)]

        def cuts(count):
            """An engine call's share [c0, c1) of ``count`` consecutive rows; a bare model takes them in one."""
            step = gan_defense.engine_step(gan.reconstruct, 1, R, count) if gan is not None else count
            return [(c0, min(count, c0 + step)) for c0 in range(0, count, step)]

        x_cur = torch.clamp(t, lo, hi)
        x_next, x_best = torch.empty_like(x_cur), torch.empty_like(x_cur)
        first_success = torch.full((n,), -1, dtype=torch.int32, device=dev)
        q = torch.empty((bs * Q,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        for k in range(nb_iter):
            for a, b in chunks:
                nq = (b - a) * Q
                ops.queries(x_cur[a:b], ns, delta, seed, a, k, lo, hi, q[:nq])
                Z, rec0 = [], []
                for c0, c1 in cuts(nq):
                    rec = ops.project(q[c0:c1], (seed + k) if gan is not None else None, (a * Q + c0) * R)
                    Z.append(ops.logits(rec))
                    if k > 0 and -c0 % Q < c1 - c0:                # the cut holds query 0 of an image: the defended view of iterate k
                        rec0.append(rec[-c0 % Q::Q])
                if k > 0:
                    ops.track(ops.predict(rec0[0] if len(rec0) == 1 else torch.cat(rec0)), lab[a:b], k, x_cur[a:b], x_best[a:b],
                              first_success[a:b])
                ops.step(Z[0] if len(Z) == 1 else torch.cat(Z), lab[a:b], ns, delta, seed, a, k, x_cur[a:b], t[a:b], eps, eps_iter, lo, hi,
                         x_next[a:b])
            x_cur, x_next = x_next, x_cur
        for a, b in chunks:                                        # the closing query of every image judges iterate nb_iter
            preds = [ops.predict(ops.project(x_cur[a + c0:a + c1], (seed + nb_iter) if gan is not None else None, (a + c0) * Q * R, Q * R))
                     for c0, c1 in cuts(b - a)]
            ops.track(preds[0] if len(preds) == 1 else torch.cat(preds), lab[a:b], nb_iter, x_cur[a:b], x_best[a:b], first_success[a:b])
        if not return_info:
            return x_best.cpu().numpy() if was_numpy else x_best
        return (x_best.cpu().numpy() if was_numpy else x_best), (first_success.cpu().numpy() if was_numpy else first_success), nb_iter * Q + 1


def rand_fgsm_prestep(test_images, eps: float, alpha: float, min_val: float = 0.0, max_val: float = 1.0, rng=None):
    """The ``rand`` half of ``--attack_type rand+fgsm`` (/root/reference/whitebox.py:191-195): one random sign step of size
    ``alpha`` before the FGSM step, whose budget shrinks by it:

        x' = clip(x + alpha * sign(N(0, 1)), min_val, 1),   eps' = eps - alpha

    Returns ``(x', eps')``; feed both to ``FastGradientMethod.generate``.  ``rng``: a ``numpy.random.RandomState`` (the reference
    draws from the global NumPy generator it seeded with [11, 24, 1990], whitebox.py:143-144)."""
    rng = np.random if rng is None else rng
    x = np.asarray(test_images, np.float32)
    out = np.clip(x + np.float32(alpha) * np.sign(rng.randn(*x.shape)).astype(np.float32), min_val, max_val).astype(np.float32)
    return out, float(eps) - float(alpha)


LATENT_DEFAULT_SEED = 11241990


class LatentAttack(object):
    """The latent-space attack (Athalye, Carlini, Wagner 2018, section 5), the attack that breaks Defense-GAN: search the generator's
    range for ``z`` such that ``G(z)`` is misclassified and close to ``x``.  ``G(z)`` lies on the manifold, so the projection returns
    it almost unchanged and the defence does not help.  One asynchronous device call per ``batch_size`` images (``dg_latent_attack``,
    defensegan_amd/csrc/dg_latent.hip; DESIGN.md section 7 gives the definition): ``rec_rr`` restarts per image, TF's Adam
    (0.9, 0.999, 1e-8) on ``z`` for ``nb_iter`` steps of the loss

        mean_pixels (G(z) - x)^2 + c max(logits[y] - max_{k != y} logits[k] + confidence, 0)

    and per image the successful iterate (margin < -confidence) of the smallest distance, or -- with no success -- the final iterate
    of the smallest margin.

    ``model``: an MLP whose output before Softmax is the logits, without Dropout.  A model with the reconstruction layer attached
    (``add_rec_model``) is accepted: the attack uses its BARE classifier and, when ``gan`` is None, the layer's generator.  ``gan``:
    a DefenseGANBase of the MNIST / F-MNIST architecture with ``USE_BN: False``; a CelebA or Batchnorm generator raises
    NotImplementedError with the library's words.

    ``generate`` returns ``x_adv`` (NumPy in, NumPy out; a device tensor in, a device tensor out on the caller's current stream, not
    waited for); ``return_info=True`` adds a dict of best_dist, best_margin [n], best_iter, best_row [n] int32 (best_iter = -1: no
    success) and z [n rec_rr, latent].  ``y``: class indices or one-hot rows, required, checked on the host against the class count.
    ``z_init`` [n rec_rr, latent] or None: the rows are then drawn as ``init_latents(seed)`` draws them, keyed by the GLOBAL row
    (image index x rec_rr + restart), so the result does not depend on ``batch_size``, which only bounds the images per call."""

    def __init__(self, model: MLP, gan=None, back="tf", sess=None):
        self.model = model
        if gan is None and model.rec_layer is not None:
            gan = model.rec_layer.rec_model
        if gan is None:
            raise ValueError("LatentAttack needs the generator: pass gan, or a model with the reconstruction layer attached")
        self.gan = gan

    def _check_gan(self):
        from . import archs
        g = self.gan
        if g._arch.arch_id == archs.ARCH_CELEBA:
            raise NotImplementedError("dg_latent_attack: not implemented for the CelebA generator (only the MNIST / F-MNIST one)")
        if g.use_bn:
            raise NotImplementedError("dg_latent_attack: not implemented for use_bn (a Batchnorm generator)")

    def call(self, x, labels, R, nb_iter, learning_rate=0.05, c=1.0, confidence=0.0, z0=None, seed=0, first_row=0, beta1=0.9, beta2=0.999,
             m=None, v=None, t_start=0, keep_state=False, state=None, traces=False, want_dz=False):
        """One ``dg_latent_attack`` call on device tensors: ``x`` [B,28,28,1] float32, ``labels`` [B] int32.  ``state``: the dict a
        call before returned, whose x_adv / best_* buffers this call continues (``t_start`` > 0).  Returns a dict of device tensors:
        x_adv, best_dist, best_margin, best_iter, best_row, z, and with ``traces`` margin and dist [nb_iter + 1, B R], with
        ``want_dz`` dz [B R, latent].  Nothing is waited for."""
        import torch
        g, mdl = self.gan, self.model
        self._check_gan()
        g._ensure_handle()
        if not g.initialized:
            raise _native.NativeError("generator weights not loaded (load_generator / set_weights)")
        mdl._ensure()
        dev = x.device
        B, N, latent = int(x.shape[0]), int(x.shape[0]) * int(R), int(g.latent_dim)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out = dict(state) if state is not None else {
            "x_adv": torch.empty_like(x), "best_dist": f32(B), "best_margin": f32(B),
            "best_iter": torch.empty(B, dtype=torch.int32, device=dev), "best_row": torch.empty(B, dtype=torch.int32, device=dev)}
        out["z"] = f32(N, latent)
        if traces:
            out["margin"], out["dist"] = f32(int(nb_iter) + 1, N), f32(int(nb_iter) + 1, N)
        if want_dz:
            out["dz"] = f32(N, latent)
        ptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(dev):
            _native.check(g._lib().dg_latent_attack(
                g._handle, mdl._handle, x.data_ptr(), labels.data_ptr(), B, int(R), ptr(z0), int(seed), int(first_row), int(nb_iter),
                float(learning_rate), float(beta1), float(beta2), float(c), float(confidence), ptr(m), ptr(v), int(t_start),
                1 if keep_state else 0, out["x_adv"].data_ptr(), out["best_dist"].data_ptr(), out["best_margin"].data_ptr(),
                out["best_iter"].data_ptr(), out["best_row"].data_ptr(), out["z"].data_ptr(), ptr(out.get("margin")), ptr(out.get("dist")),
                ptr(out.get("dz")), torch.cuda.current_stream(dev).cuda_stream), g._lib())
        return out

    def generate(self, x, y, rec_rr=None, nb_iter=100, learning_rate=0.05, c=1.0, confidence=0.0, z_init=None, seed=None, batch_size=None,
                 return_info=False):
        import torch
        self._check_gan()
        mdl, g = self.model, self.gan
        R = int(g.rec_rr if rec_rr is None else rec_rr)
        nb_iter = int(nb_iter)
        if R < 1 or nb_iter < 0:
            raise ValueError("rec_rr must be >= 1 and nb_iter >= 0")
        if not (float(confidence) >= 0 and float(c) >= 0):
            raise ValueError("confidence and c must be >= 0")
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        seed = LATENT_DEFAULT_SEED if seed is None else int(seed)
        mdl._ensure()
        if not mdl._weights_set:
            raise _native.NativeError("classifier weights not set")
        g._ensure_handle()
        dev = torch.device("cuda", mdl._device)
        was_numpy = isinstance(x, np.ndarray)
        to = lambda a: (torch.from_numpy(np.ascontiguousarray(a, np.float32)) if isinstance(a, np.ndarray) else a).to(device=dev, dtype=torch.float32).contiguous()
        t = to(x)
        if t.dim() != 4 or tuple(t.shape[1:]) != tuple(mdl.input_shape[1:]) or int(t.shape[0]) == 0:
            raise ValueError("x must be [n, %s] with n > 0, got %s" % (", ".join(str(d) for d in mdl.input_shape[1:]), tuple(t.shape)))
        n = int(t.shape[0])
        yy = np.asarray(y if isinstance(y, np.ndarray) else (y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y))
        if yy.ndim > 1:
            yy = yy.argmax(axis=-1)
        if yy.shape != (n,):
            raise ValueError("y must be %d class indices or one-hot rows" % n)
        if (yy < 0).any() or (yy >= mdl.nb_classes).any():
            raise ValueError("y holds a class index outside [0, %d)" % mdl.nb_classes)
        lab = torch.from_numpy(np.ascontiguousarray(yy.astype(np.int32))).to(dev)
        z0 = None
        if z_init is not None:
            z0 = to(z_init)
            if tuple(z0.shape) != (n * R, int(g.latent_dim)):
                raise ValueError("z_init must be [%d, %d], got %s" % (n * R, int(g.latent_dim), tuple(z0.shape)))
        bs = n if batch_size is None else int(batch_size)
        parts = []
        for a in range(0, n, bs):
            b = min(n, a + bs)
            parts.append(self.call(t[a:b], lab[a:b], R, nb_iter, learning_rate, c, confidence, None if z0 is None else z0[a * R:b * R],
                                   seed, a * R))
        info = {k: torch.cat([p[k] for p in parts]) for k in ("x_adv", "best_dist", "best_margin", "best_iter", "best_row", "z")}
        x_adv = info.pop("x_adv")
        if was_numpy:
            x_adv, info = x_adv.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
        return (x_adv, info) if return_info else x_adv
