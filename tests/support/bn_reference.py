"""Float64 restatement of the generator's Batchnorm path (USE_BN: True) for value checks of the device kernels.

Three things the NumPy oracle (oracle/defensegan_oracle.py) does not offer:

* the LAYER form with every intermediate exposed: mean, biased variance, rstd (eps 1e-5), xhat, relu(xhat * scale + offset), and
  for the backward mean(dy * gate), mean(dy * gate * xhat), da;
* the WHOLE generator with PRESCRIBED gates: the forward is the oracle's, the backward takes every ReLU mask as an argument
  instead of forming it from its own pre-activations.  ReLU is continuous, so a forward comparison needs no exclusion at a gate
  that sits at rounding distance from zero; the backward is discontinuous there -- but handed the gates the device used, the
  reference differentiates the same piecewise-linear function and needs no exclusion either;
* the statistics in FLOAT32 in the tf.nn.moments form (mean, then mean of squared differences): the yardstick a float32
  implementation is measured against (tolerances of tests/test_gpu_bn_values.py).

Layout: activations NHWC; a Batchnorm layer's statistics run over every axis but the last (BN1: the [N, 4096] Linear output,
one statistic per feature)."""
from __future__ import annotations

import numpy as np

from oracle import defensegan_oracle as O

EPS = 1e-5


def _axes(a):
    return tuple(range(a.ndim - 1))


# ---- layer form ---------------------------------------------------------------------------------------------------------------
def layer_forward(pre, scale, offset):
    """pre [..., C] -> dict(mean [C], var [C] (biased), rstd [C], xhat, bn = xhat * scale + offset, out = relu(bn)); float64."""
    a = np.asarray(pre, np.float64)
    ax = _axes(a)
    mean = a.mean(axis=ax)
    var = ((a - mean) ** 2).mean(axis=ax)
    rstd = 1.0 / np.sqrt(var + EPS)
    xhat = (a - mean) * rstd
    bn = xhat * np.asarray(scale, np.float64) + np.asarray(offset, np.float64)
    return {"mean": mean, "var": var, "rstd": rstd, "xhat": xhat, "bn": bn, "out": np.maximum(bn, 0.0)}


def layer_backward(dy, gate, xhat, rstd, scale):
    """dy: gradient w.r.t. relu(bn(pre)); gate: the ReLU mask (bool, same shape).  Returns (mean(dy * gate) [C],
    mean(dy * gate * xhat) [C], da = gradient w.r.t. pre); float64."""
    g = np.asarray(dy, np.float64) * np.asarray(gate, bool)
    ax = _axes(g)
    m1 = g.mean(axis=ax)
    m2 = (g * xhat).mean(axis=ax)
    da = (np.asarray(scale, np.float64) * rstd) * (g - m1 - xhat * m2)
    return m1, m2, da


# ---- float32 two-pass statistics (the yardstick) ------------------------------------------------------------------------------
def moments_f32(pre):
    """mean, biased variance and rstd of float32 `pre` as tf.nn.moments forms them, every operation in float32."""
    a = np.asarray(pre, np.float32)
    ax = _axes(a)
    mean = a.mean(axis=ax, dtype=np.float32)
    var = ((a - mean) ** 2).mean(axis=ax, dtype=np.float32)
    rstd = (np.float32(1.0) / np.sqrt(var + np.float32(EPS))).astype(np.float32)
    return mean, var, rstd


def backward_sums_f32(g, xhat):
    """mean(g), mean(g * xhat) over the statistics axes, every operation in float32 (g = the masked dy)."""
    g = np.asarray(g, np.float32)
    ax = _axes(g)
    return g.mean(axis=ax, dtype=np.float32), (g * np.asarray(xhat, np.float32)).mean(axis=ax, dtype=np.float32)


# ---- whole generator ----------------------------------------------------------------------------------------------------------
def bn_names(arch):
    """Batchnorm layer d (index of the activation buffer it writes) -> parameter name."""
    return ["Generator.BN1"] + [bn for (_, _, _, _, bn) in O._arch_layers(arch) if bn]


def layer_pre(p, arch, d, prev):
    """Pre-activations of Batchnorm layer d in float64 from the activation in front of it: d = 0: prev = z [N, latent] -> [N, 4096];
    d >= 1: prev = activation d - 1 on its full stored map [N, pitch, pitch, C] (the crop is taken here) -> [N, 2h, 2h, Cout]."""
    prev = np.asarray(prev, np.float64)
    if d == 0:
        return O.linear(prev, p["Generator.Input.W"].astype(np.float64), p["Generator.Input.b"].astype(np.float64))
    name, h_in, _, _, _ = O._arch_layers(arch)[d - 1]
    return O.deconv2d(prev[:, :h_in, :h_in, :], p[name + ".Filters"].astype(np.float64), p[name + ".Biases"].astype(np.float64), None)


def generator_forward(p, z, arch):
    """Float64 forward with Batchnorm.  Returns dict: pre[d], bn[d] (layer_forward records) and act[d] (relu(bn), FULL map, not
    cropped) per Batchnorm layer d, tail (list of the remaining layers' outputs), y."""
    layers = O._arch_layers(arch)
    names = bn_names(arch)
    out = {"pre": [], "bn": [], "act": [], "tail": []}
    a = np.asarray(z, np.float64)
    for d, bn in enumerate(names):
        pre = layer_pre(p, arch, d, a)
        rec = layer_forward(pre, p[bn + ".scale"], p[bn + ".offset"])
        out["pre"].append(pre); out["bn"].append(rec)
        a = rec["out"] if d else rec["out"].reshape(len(pre), 4, 4, -1)
        out["act"].append(a)
    for (name, h_in, h_used, act, bn) in layers[len(names) - 1:]:
        a = O.deconv2d(a[:, :h_in, :h_in, :], p[name + ".Filters"].astype(np.float64), p[name + ".Biases"].astype(np.float64), h_used)
        a = {"none": lambda v: v, "sigmoid": lambda v: 1.0 / (1.0 + np.exp(-v)), "tanh": np.tanh}[act](a)
        out["tail"].append(a)
    out["y"] = a
    return out


def generator_backward(p, fwd, dy, arch, gates, want=False):
    """dL/dz from dL/dy with PRESCRIBED ReLU masks: gates[d] (bool, shape of fwd['act'][d]) replaces (act[d] > 0) of Batchnorm
    layer d.  `want`: also return per layer the masked gradient g[d], the sums (m1[d], m2[d]) and da[d]."""
    layers = O._arch_layers(arch)
    names = bn_names(arch)
    nb = len(names)
    g = np.asarray(dy, np.float64)
    tail_layers = layers[nb - 1:]
    for k in range(len(tail_layers) - 1, -1, -1):
        name, h_in, h_used, act, _ = tail_layers[k]
        out = fwd["tail"][k]
        if act == "sigmoid":
            g = g * out * (1 - out)
        elif act == "tanh":
            g = g * (1 - out * out)
        g = O.deconv2d_backward_input(g, p[name + ".Filters"].astype(np.float64), h_in)
    rec = {"g": [None] * nb, "m1": [None] * nb, "m2": [None] * nb, "da": [None] * nb}
    for d in range(nb - 1, -1, -1):
        bnr = fwd["bn"][d]
        shape = bnr["xhat"].shape
        if d:
            gp = np.zeros(shape, np.float64)                   # gradient of the crop = zero padding
            gp[:, :g.shape[1], :g.shape[2], :] = g
        else:
            gp = g.reshape(shape)
        gate = np.asarray(gates[d], bool).reshape(shape)
        m1, m2, da = layer_backward(gp, gate, bnr["xhat"], bnr["rstd"], p[names[d] + ".scale"])
        rec["g"][d], rec["m1"][d], rec["m2"][d], rec["da"][d] = gp * gate, m1, m2, da
        if d:
            name, h_in, _, _, _ = layers[d - 1]
            g = O.deconv2d_backward_input(da, p[name + ".Filters"].astype(np.float64), h_in)
    dz = da @ p["Generator.Input.W"].astype(np.float64).T
    return (dz, rec) if want else dz


def own_gates(fwd):
    return [a > 0 for a in fwd["act"]]


def loss_and_dy(y, x, R):
    """Per-row mean squared error against image row // R, and its gradient w.r.t. y."""
    xt = np.repeat(np.asarray(x, np.float64), R, axis=0)
    diff = np.asarray(y, np.float64) - xt
    P = diff[0].size
    return (diff ** 2).reshape(len(diff), -1).mean(axis=1), 2.0 / P * diff
