"""The training half of cleverhans 2.x utils_tf, which the reference calls to train every classifier it attacks
(whitebox.py:120-170; cleverhans is an empty, un-pinned submodule of the reference, its published functions are
restated).  The arithmetic runs in the HIP library (dg_clf_train in include/defensegan_hip.h), one asynchronous call per epoch;
only the batch schedule is built here, with NumPy, exactly as cleverhans builds it.

    model = network_builder.model_f()
    model.init_like_reference(seed=0)
    model_train(model, X_train, Y_train, args={"nb_epochs": 10, "batch_size": 128, "learning_rate": 0.001},
                rng=np.random.RandomState([11, 24, 1990]), adv_eps=0.15)      # adv_eps: --defense_type adv_tr
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native
from . import network_builder as nb

WHITEBOX_RNG_SEED = [11, 24, 1990]          # whitebox.py: rng = np.random.RandomState([11, 24, 1990])


def batch_indices(batch_nb, data_length, batch_size):
    """cleverhans utils.batch_indices: the [start, end) of batch ``batch_nb``; the last batch is shifted back so that it is full
    (data_length 5, batch_size 2: [0, 2), [2, 4), [3, 5))."""
    start = int(batch_nb * batch_size)
    end = int((batch_nb + 1) * batch_size)
    if end > data_length:
        shift = end - data_length
        start -= shift
        end -= shift
    return start, end


def epoch_indices(rng, n, batch_size):
    """One epoch of model_train's schedule: ``index_shuf = list(range(n)); rng.shuffle(index_shuf)``, then batch b =
    index_shuf[batch_indices(b, n, batch_size)] for b < ceil(n / batch_size).  Returns the concatenated batches (int32)."""
    index_shuf = list(range(n))
    rng.shuffle(index_shuf)
    nb_batches = int(math.ceil(float(n) / batch_size))
    out = np.empty(nb_batches * batch_size, np.int32)
    for b in range(nb_batches):
        start, end = batch_indices(b, n, batch_size)
        out[b * batch_size:(b + 1) * batch_size] = index_shuf[start:end]
    return out


def _arg(args, name):
    v = args.get(name) if isinstance(args, dict) else getattr(args, name, None)
    if v is None:
        raise ValueError("%s was not given in args" % name)
    return v


def _nb_classes(model):
    for layer in reversed(model.layers):
        if isinstance(layer, nb.Linear):
            return layer.num_hid
        if isinstance(layer, nb.Conv2D):
            return None
    return None


def labels_of(Y, n, nb_classes):
    """int32 class indices from one-hot rows [n, nb_classes] (exactly one 1, zeros elsewhere) or class indices [n]."""
    Y = Y if isinstance(Y, np.ndarray) else Y.detach().cpu().numpy()
    Y = np.asarray(Y)
    if Y.ndim == 2:
        if Y.shape != (n, nb_classes):
            raise ValueError("one-hot labels must be [%d, %d], got %s" % (n, nb_classes, Y.shape))
        ok = ((Y == 0) | (Y == 1)).all(axis=1) & (Y.sum(axis=1) == 1)
        if not ok.all():
            raise ValueError("label row %d is not one-hot" % int(np.flatnonzero(~ok)[0]))
        return Y.argmax(axis=1).astype(np.int32)
    if Y.ndim != 1 or Y.shape[0] != n:
        raise ValueError("labels must be [%d] class indices or [%d, %d] one-hot rows, got %s" % (n, n, nb_classes, Y.shape))
    if not np.issubdtype(Y.dtype, np.integer):
        if not (Y == np.round(Y)).all():
            raise ValueError("class indices must be integers")
    Y = Y.astype(np.int64)
    if (Y < 0).any() or (Y >= nb_classes).any():
        raise ValueError("class indices must lie in [0, %d)" % nb_classes)
    return Y.astype(np.int32)


def model_train(model, X_train, Y_train, args=None, rng=None, adv_eps=None, adv_clip=(0., 1.), evaluate=None, seed=11241990,
                return_losses=False):
    """cleverhans utils_tf.model_train on the device: a fresh Adam (the moments and the step count reset), ``nb_epochs`` epochs of
    ceil(n / batch_size) steps over the permutation ``rng`` draws per epoch (``rng`` default: whitebox's RandomState([11, 24,
    1990])), the training phase (Dropout active, masks drawn with ``seed``), softmax cross-entropy on the logits.

    ``args``: dict or object with nb_epochs, batch_size, learning_rate.  ``X_train`` [n, H, W, C] NumPy or device tensor, kept on
    the device for the whole run; ``Y_train`` one-hot rows (as the reference feeds them) or class indices.  ``adv_eps`` > 0 adds
    the adversarial half of whitebox's adv_tr (loss = (clean + FGSM(adv_eps, clipped to ``adv_clip``)) / 2, the FGSM label the
    model's own prediction).  ``evaluate()`` runs after every epoch, as in cleverhans.  Returns True, or with ``return_losses``
    the per-step losses (NumPy float32 [nb_epochs * ceil(n / batch_size)]).

    A model with the reconstruction layer attached raises NotImplementedError: the reference's training through it
    (online_training / train_on_recs) is not reproduced; training on a cache of reconstructions is a different ``X_train``."""
    import torch
    if getattr(model, "rec_layer", None) is not None:
        raise NotImplementedError("model_train through the Defense-GAN reconstruction layer (add_rec_model) is not implemented; "
                                  "train the bare classifier, or on reconstructed images as X_train")
    if args is None:
        raise ValueError("args (nb_epochs, batch_size, learning_rate) must be given")
    nb_epochs, batch_size, lr = int(_arg(args, "nb_epochs")), int(_arg(args, "batch_size")), float(_arg(args, "learning_rate"))
    if nb_epochs < 0 or batch_size <= 0 or not lr > 0:
        raise ValueError("need nb_epochs >= 0, batch_size > 0 and learning_rate > 0 (got %d, %d, %g)" % (nb_epochs, batch_size, lr))
    shape = tuple(int(d) for d in X_train.shape)
    if len(shape) != 4 or shape[1:] != tuple(model.input_shape[1:]):
        raise ValueError("X_train must be [n, %s], got %s" % (", ".join(str(d) for d in model.input_shape[1:]), shape))
    n = shape[0]
    if n < batch_size:
        raise ValueError("the training set (%d images) is smaller than one batch (%d)" % (n, batch_size))
    nb_classes = _nb_classes(model)
    if nb_classes is None:
        raise ValueError("the model does not end in a Linear layer")
    lab = labels_of(Y_train, n, nb_classes)
    eps = float(adv_eps) if adv_eps is not None else 0.0
    lo, hi = float(adv_clip[0]), float(adv_clip[1])
    if eps > 0 and not hi > lo:
        raise ValueError("adv_clip %s is empty" % (adv_clip,))
    rng = np.random.RandomState(WHITEBOX_RNG_SEED) if rng is None else rng

    model._ensure()
    if not model._weights_set:
        raise _native.NativeError("classifier weights not set")
    lib = _native.load()
    dev = torch.device("cuda", model._device)
    X = (torch.from_numpy(np.ascontiguousarray(X_train, np.float32)) if isinstance(X_train, np.ndarray) else X_train)
    X = X.to(device=dev, dtype=torch.float32).contiguous()
    y = torch.from_numpy(lab).to(dev)
    nb_batches = int(math.ceil(float(n) / batch_size))
    losses = []
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _native.check(lib.dg_clf_adam_reset(model._handle))
        for _ in range(nb_epochs):
            idx = torch.from_numpy(epoch_indices(rng, n, batch_size)).to(dev)
            loss = torch.empty(nb_batches, dtype=torch.float32, device=dev)
            _native.check(lib.dg_clf_train(model._handle, X.data_ptr(), y.data_ptr(), n, idx.data_ptr(), nb_batches, batch_size, lr,
                                           eps, lo, hi, int(seed) & 0xFFFFFFFFFFFFFFFF, loss.data_ptr(), stream))
            losses.append(loss)
            if evaluate is not None:
                evaluate()
    if return_losses:
        torch.cuda.synchronize(dev)
        return torch.cat(losses).cpu().numpy() if losses else np.zeros(0, np.float32)
    return True


def batch_eval(fn, X, batch_size=128):
    """cleverhans utils_tf.batch_eval for one input and one output (blackbox.py:205-207): ``fn`` over the consecutive batches
    X[0:bs], X[bs:2bs], ...; the last one is partial (NOT shifted back as model_train's is).  ``fn`` maps a batch to an array or
    device tensor with the batch on axis 0; the outputs are concatenated in order, as the kind ``fn`` returned."""
    batch_size = int(batch_size)
    if batch_size <= 0:
        raise ValueError("batch_size must be positive, got %d" % batch_size)
    n = len(X)
    outs = [fn(X[start:start + batch_size]) for start in range(0, n, batch_size)]
    if not outs:
        raise ValueError("X holds no rows")
    if isinstance(outs[0], np.ndarray):
        return np.concatenate(outs, axis=0)
    import torch
    return torch.cat(outs, dim=0)


def batch_eval_labels(fn, X, batch_size=128):
    """``np.argmax(batch_eval(...), axis=1)`` (blackbox.py:211): the labels an adversary reads off an oracle, NumPy int64 [n]."""
    out = batch_eval(fn, X, batch_size)
    if isinstance(out, np.ndarray):
        return np.argmax(out, axis=1).astype(np.int64)
    return out.argmax(dim=1).cpu().numpy().astype(np.int64)


def adam_state(model, layer_nb):
    """(m, v, t) of the ``layer_nb``-th Conv2D / Linear layer: each moment as the (W, b) pair of its parameters."""
    model._ensure()
    lib = _native.load()
    ws, bs = model.param_shapes()[layer_nb]
    nw, nbias = int(np.prod(ws)), int(np.prod(bs))
    m, v, t = np.empty(nw + nbias, np.float32), np.empty(nw + nbias, np.float32), C.c_int64()
    _native.check(lib.dg_clf_get_adam(model._handle, model._native_index[model._param_layers[layer_nb]], m.ctypes.data_as(C.c_void_p),
                                      v.ctypes.data_as(C.c_void_p), C.byref(t), 0))
    return (m[:nw].reshape(ws), m[nw:]), (v[:nw].reshape(ws), v[nw:]), int(t.value)
