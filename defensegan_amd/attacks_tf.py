"""cleverhans 2.x ``attacks_tf``, the part the reference's black-box flow calls (blackbox.py:174, 193-194; cleverhans is an empty,
un-pinned submodule of the reference, its published functions are restated).  The arithmetic runs in the HIP library
(``dg_jacobian_augment`` in include/defensegan_hip.h), one asynchronous call per augmentation.

    X_sub = jacobian_augmentation(sub_model, X_sub, Y_sub, lmbda=0.1)        # [n, ...] -> [2n, ...]

``jacobian_graph(preds_sub, x, nb_classes)`` has no counterpart object: without a TF graph the Jacobian is a method of the model,
``MLP.jacobian(x)`` / ``MLP.class_gradient(x, classes)`` (network_builder.py)."""
from __future__ import annotations

import numpy as np

from . import _native
from . import network_builder as nb


def jacobian_augmentation(model, X_sub, Y_sub, lmbda, batch_size=128):
    """Papernot's Jacobian-based dataset augmentation (arxiv.org/abs/1602.02697, cleverhans ``jacobian_augmentation``):

        X_out[:n] = X_sub,   X_out[n + i] = X_sub[i] + lmbda * sign(d model(X_sub[i])[Y_sub[i]] / dx)

    ``model(x)`` is the substitute's PROBABILITIES (MLP.__call__), so the direction is the gradient of softmax(logits)[label]; a
    model without Softmax is differentiated at its logits.  sign(0) = 0 and the new half is NOT clipped, as in cleverhans.
    ``X_sub`` [n, H, W, C] NumPy or device tensor (the same kind is returned), ``Y_sub`` [n] class indices.  ``batch_size`` is the
    number of images per device launch and does not change the result (cleverhans evaluates one image per session.run)."""
    import torch
    if getattr(model, "rec_layer", None) is not None:
        raise NotImplementedError(nb._JAC_REC_NOTE)
    if int(batch_size) <= 0:
        raise ValueError("batch_size must be positive, got %r" % (batch_size,))
    t, was_numpy = nb._jacobian_input(model, X_sub)
    n = int(t.shape[0])
    y = nb._class_indices(model, Y_sub, n, what="Y_sub")
    out = torch.empty((2 * n,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
    stream = torch.cuda.current_stream(t.device).cuda_stream
    with torch.cuda.device(t.device):
        _native.check(_native.load().dg_jacobian_augment(model._handle, t.data_ptr(), y.data_ptr(), n, float(lmbda), int(batch_size),
                                                         out.data_ptr(), stream))
    return out.cpu().numpy() if was_numpy else out
