"""Float64 restatement of the generator's default path (USE_BN: False), layer by layer, for value checks of the device kernels,
and the checks themselves (shared by tests/test_gpu_path_values.py, which feeds them the device, and
tests/test_path_reference_cpu.py, which feeds them a float32 emulation with and without seeded defects).

Built from the oracle's own layer functions (oracle/defensegan_oracle.py: linear, deconv2d, deconv2d_backward_input); what the
oracle does not offer:

* TEACHER FORCING: every layer as a function of a GIVEN input (the device's previous activation, the device's gradient of the
  layer behind it), so that a layer's error is seen by itself and not through the layers around it;
* PRESCRIBED GATES: the backward takes every ReLU mask as an argument.  Handed the gates the device used, the reference
  differentiates the same piecewise-linear function and no "kink" row has to be left out;
* TAP CLASSES: the positions of a layer's output grouped by their relative pattern of valid taps (index map i = 2 * o + k - 1 of
  dg_plan.h, derived here, not read from the planner), so that an error is measured against the size of ITS class -- a few-tap
  border class is small beside the 25-tap interior, and a wrong tap or offset shows there;
* the same layers in FLOAT32 (dtype = np.float32): the yardstick of the tolerances.

Numbering: activation buffer d of the engine ("act<d>" of dg_debug_read) is the output of layer d: d = 0 the Linear layer as
[N, 4, 4, C] (feature f = (oh * 4 + ow) * C + c), d >= 1 Deconv2D number d - 1 of the architecture; layer n_act(arch) is the tail
(its output is the image y).  After a backward pass act<d> holds the gradient w.r.t. layer d's pre-activation (the ReluGrad mask
applied; CelebA's last GEMM layer has no activation function).

Geometry: without Batchnorm the engine stores exactly the used grid of every layer (describe_activations in dg_engine.cpp:
pitch = e_used; the 8 x 8 pitch of MNIST's 7 x 7 map exists only with Batchnorm, whose statistics cover the cropped row and
column -- tests/support/bn_reference.py).  The crop is therefore part of the tap classes (the 7 x 7 map's last row / column reads
fewer taps) and there is NO stored position outside the used grid on this path: nothing to compare with 0 and nothing left out."""
from __future__ import annotations

import hashlib

import numpy as np

from oracle import defensegan_oracle as O

FWD_TOL = 2e-6       # teacher-forced forward layers (rule (b) of tests/test_gpu_bn_values.py)
GRAD_TOL = 1e-5      # gradients (the project's backward gate)
GATE_EPS = 1e-5      # a gate may differ from float64's only where the float64 |pre-activation| is below this
LOSS_RTOL = 1e-5


# ---- layers -------------------------------------------------------------------------------------------------------------------
def n_act(arch):
    """Number of activation buffers: the Linear layer and every Deconv2D but the last."""
    return len(O._arch_layers(arch))


def layer_is_relu(arch, d):
    return d == 0 or O._arch_layers(arch)[d - 1][3] == "relu"


def _w(p, name, dtype):
    return np.asarray(p[name]).astype(dtype)


def layer_pre(p, arch, d, prev, dtype=np.float64):
    """Pre-activation of layer d from the activation in front of it (d = 0: prev = z [N, latent]) -> [N, h, h, C]."""
    prev = np.asarray(prev).astype(dtype)
    if d == 0:
        W = _w(p, "Generator.Input.W", dtype)
        return O.linear(prev, W, _w(p, "Generator.Input.b", dtype)).reshape(len(prev), 4, 4, W.shape[1] // 16)
    name, h_in, h_used, _, _ = O._arch_layers(arch)[d - 1]
    assert prev.shape[1] == h_in and prev.shape[2] == h_in, (prev.shape, h_in)
    return O.deconv2d(prev, _w(p, name + ".Filters", dtype), _w(p, name + ".Biases", dtype), h_used)


def layer_out(arch, d, pre):
    return np.maximum(pre, 0) if layer_is_relu(arch, d) else pre


def tail_forward(p, arch, prev, dtype=np.float64):
    """The last layer with its sigmoid / tanh: the image y from the last activation."""
    name, h_in, h_used, act, _ = O._arch_layers(arch)[-1]
    a = O.deconv2d(np.asarray(prev).astype(dtype), _w(p, name + ".Filters", dtype), _w(p, name + ".Biases", dtype), h_used)
    return dtype(1.0) / (dtype(1.0) + np.exp(-a)) if act == "sigmoid" else np.tanh(a)


def loss_and_dy(y, x, R, dtype=np.float64):
    """Per-row mean squared error against image row // R, and its gradient w.r.t. y."""
    xt = np.repeat(np.asarray(x).astype(dtype), R, axis=0)
    diff = np.asarray(y).astype(dtype) - xt
    P = diff[0].size
    return (diff ** 2).reshape(len(diff), -1).mean(axis=1, dtype=dtype), dtype(2.0) / dtype(P) * diff


def layer_backward(p, arch, d, g_next, gate, dtype=np.float64):
    """Gradient w.r.t. layer d's pre-activation from the gradient w.r.t. layer d + 1's pre-activation and layer d's ReLU mask
    (gate = None: no mask, as for a layer without activation function or to look at the sum in front of the mask)."""
    name, h_in, _, _, _ = O._arch_layers(arch)[d]
    g = O.deconv2d_backward_input(np.asarray(g_next).astype(dtype), _w(p, name + ".Filters", dtype), h_in)
    return g if gate is None else g * np.asarray(gate, bool)


def tail_backward(p, arch, y, x, R, gate, dtype=np.float64):
    """Gradient w.r.t. the last GEMM layer's pre-activation from the image y: dL/dy through sigmoid' / tanh' (formed from y, as
    ReluGrad-style gradients are), through the last Deconv2D, then the mask."""
    act = O._arch_layers(arch)[-1][3]
    _, dy = loss_and_dy(y, x, R, dtype)
    y = np.asarray(y).astype(dtype)
    g = dy * y * (dtype(1.0) - y) if act == "sigmoid" else dy * (dtype(1.0) - y * y)
    return layer_backward(p, arch, n_act(arch) - 1, g, gate, dtype)


def linear_backward(p, da0, dtype=np.float64):
    da0 = np.asarray(da0).astype(dtype)
    return da0.reshape(len(da0), -1) @ _w(p, "Generator.Input.W", dtype).T


def forward_from_z(p, arch, z, dtype=np.float64):
    """The chained forward: dict(pre [n_act], act [n_act], y)."""
    out = {"pre": [], "act": []}
    a = np.asarray(z).astype(dtype)
    for d in range(n_act(arch)):
        pre = layer_pre(p, arch, d, a, dtype)
        a = layer_out(arch, d, pre)
        out["pre"].append(pre); out["act"].append(a)
    out["y"] = tail_forward(p, arch, a, dtype)
    return out


def backward_with_gates(p, arch, y, x, R, gates, dtype=np.float64):
    """The chained backward with prescribed masks: (dz, [gradient at every layer])."""
    nd = n_act(arch)
    gate = lambda d: gates[d] if layer_is_relu(arch, d) else None
    grads = [None] * nd
    grads[nd - 1] = tail_backward(p, arch, y, x, R, gate(nd - 1), dtype)
    for d in range(nd - 2, -1, -1):
        grads[d] = layer_backward(p, arch, d, grads[d + 1], gate(d), dtype)
    return linear_backward(p, grads[0], dtype), grads


# ---- tap classes --------------------------------------------------------------------------------------------------------------
def _taps_1d(h_in, h_out, direction):
    """Per position of one dimension the tuple of valid kernel indices k under i = 2 * o + k - 1 (i: the h_out side, o: the h_in
    side).  'fwd': positions are the outputs i; 'bwd': positions are the inputs o (the stride-2 conv of the backward)."""
    if direction == "fwd":
        return [tuple(k for k in range(O.KS) if (i + 1 - k) % 2 == 0 and 0 <= (i + 1 - k) // 2 < h_in) for i in range(h_out)]
    return [tuple(k for k in range(O.KS) if 0 <= 2 * o + k - 1 < h_out) for o in range(h_in)]


def tap_class_masks(arch, d, direction):
    """(mask [h, h] of class numbers, classes) for the stored positions of act<d> (d = n_act: the image y, 'fwd' only).
    'fwd': as the output of the forward layer d; 'bwd': as the output of the backward layer that reads the gradient of layer
    d + 1.  A class is the set of positions with the same valid taps (kh set x kw set): with the same filter taps valid, the input
    offsets relative to the position are the same too (o = (i + 1 - k) / 2, resp. i = 2 * o + k - 1).  classes[c] = dict(kh, kw,
    taps, positions), ordered by descending tap count as the planner orders them.  The Linear layer (d = 0, 'fwd') is one class."""
    layers = O._arch_layers(arch)
    if direction == "fwd" and d == 0:
        return np.zeros((4, 4), np.int64), [{"kh": (), "kw": (), "taps": 1, "positions": 16}]
    if direction == "fwd":
        _, h_in, h_used, _, _ = layers[d - 1]
        one = _taps_1d(h_in, h_used, "fwd")
    else:
        _, h_in, h_used, _, _ = layers[d]
        one = _taps_1d(h_in, h_used, "bwd")
    keys = sorted({(a, b) for a in one for b in one}, key=lambda k: (-len(k[0]) * len(k[1]), k))
    index = {k: c for c, k in enumerate(keys)}
    mask = np.array([[index[(a, b)] for b in one] for a in one], np.int64)
    classes = [{"kh": a, "kw": b, "taps": len(a) * len(b), "positions": int((mask == c).sum())} for c, (a, b) in enumerate(keys)]
    return mask, classes


# ---- the checks ---------------------------------------------------------------------------------------------------------------
def _ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


class Result:
    """What a run of the checks found: `fails` = [(check number, label, line)], `lines` = the full table, `worst` = per group the
    line with the smallest bound / error."""

    def __init__(self):
        self.fails, self.lines, self.worst = [], [], {}

    def add(self, check, group, label, err, yard, bound, scale, from_yard):
        margin = bound / max(err, 1e-300)
        line = ("(%d) %-34s device %.3g | float32 %.3g | bound %.3g%s | x%.1f   (of max|float64| = %.3g)"
                % (check, label, err / scale, yard / scale, bound / scale, " [4 x float32 + 2 ulp]" if from_yard else "", min(margin, 9999.0), scale))
        self.lines.append(line)
        w = self.worst.get(group)
        if w is None or margin < w[0]:
            self.worst[group] = (margin, line, from_yard)
        if not err <= bound:
            self.fails.append((check, label, line))

    def note(self, check, label, ok, line):
        self.lines.append("(%d) %-34s %s" % (check, label, line))
        if not ok:
            self.fails.append((check, label, line))

    def labels(self, check):
        return sorted(l for c, l, _ in self.fails if c == check)

    def summary(self):
        return ["worst %-12s %s" % (g, w[1]) for g, w in sorted(self.worst.items())]


def class_check(res, check, group, what, dev, ref, yard, mask, figure):
    """Per tap class c: max|dev - ref| over the class <= figure * max|ref| over the class -- unless the float32 yardstick's own
    error in the class exceeds a quarter of that: then 4 x the yardstick's worst error in the class + 2 ulp (of the class
    maximum).  mask = None: the whole tensor is one class.  A class whose float64 values are all 0 must be exactly 0."""
    dev, ref, yard = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(yard, np.float64)
    assert dev.shape == ref.shape == yard.shape, (what, dev.shape, ref.shape, yard.shape)
    finite = bool(np.isfinite(dev).all())
    if not finite:
        res.note(check, what, False, "device values are not all finite")
        return
    ed, ey, ar = np.abs(dev - ref), np.abs(yard - ref), np.abs(ref)
    n_cls = 1 if mask is None else int(mask.max()) + 1
    for c in range(n_cls):
        if mask is None:
            e, y, s, label = ed.max(), ey.max(), ar.max(), what
        else:
            sel = mask == c
            e, y, s, label = ed[:, sel].max(), ey[:, sel].max(), ar[:, sel].max(), "%s class %d" % (what, c)
        if s == 0.0:
            res.note(check, label, e == 0.0, "float64 is 0 on the whole class; device max %.3g" % e)
            continue
        from_yard = y > 0.25 * figure * s
        bound = 4.0 * y + 2.0 * _ulp(s) if from_yard else figure * s
        res.add(check, group, label, float(e), float(y), float(bound), float(s), from_yard)


class Memo:
    """Results of the float64 / float32 layer functions by the bytes of their array arguments: option settings that leave a
    layer's input bit for bit the same (the job-list options do) share one evaluation.  Entries are never modified."""

    def __init__(self):
        self.d = {}

    @staticmethod
    def _feed(h, a):
        if isinstance(a, dict):
            h.update(b"dict%d" % id(a))                                           # the weight dict: by identity
        elif isinstance(a, np.ndarray):
            h.update(str((a.shape, a.dtype)).encode()); h.update(np.ascontiguousarray(a).tobytes())
        elif isinstance(a, (list, tuple)):
            h.update(b"seq%d" % len(a))
            for v in a:
                Memo._feed(h, v)
        else:
            h.update(repr(a).encode())

    def __call__(self, fn, *args, **kw):
        h = hashlib.blake2b(digest_size=16)
        h.update(fn.__name__.encode())
        self._feed(h, list(args) + sorted(kw.items()))
        k = h.digest()
        if k not in self.d:
            self.d[k] = fn(*args, **kw)
        return self.d[k]


def _both(memo, fn, *args):
    return memo(fn, *args, dtype=np.float64), memo(fn, *args, dtype=np.float32)


def check_forward(res, rec, p, arch, memo):
    """(1) act<d> against the float64 layer fed the record's act<d - 1>, y against the float64 tail fed the last activation, per tap
    class.  Returns the float64 pre-activations (for (2))."""
    pres, prev = [], rec["z"]
    for d in range(n_act(arch)):
        pre64, pre32 = _both(memo, layer_pre, p, arch, d, prev)
        mask = tap_class_masks(arch, d, "fwd")[0]
        class_check(res, 1, "forward", "act%d" % d, rec["acts"][d], layer_out(arch, d, pre64), layer_out(arch, d, pre32), mask if d else None, FWD_TOL)
        pres.append(pre64)
        prev = rec["acts"][d]
    y64, y32 = _both(memo, tail_forward, p, arch, prev)
    class_check(res, 1, "y", "y", rec["y"], y64, y32, tap_class_masks(arch, n_act(arch), "fwd")[0], FWD_TOL)
    if rec.get("y_generate") is not None:                    # the forward-only call's image (another launch of the tail)
        class_check(res, 1, "y", "y (generate)", rec["y_generate"], y64, y32, tap_class_masks(arch, n_act(arch), "fwd")[0], FWD_TOL)
    return pres


def check_gates(res, rec, arch, pres):
    """(2) where (act<d> > 0) differs from the float64 layer's gate, the float64 |pre-activation| is below GATE_EPS."""
    for d in range(n_act(arch)):
        if not layer_is_relu(arch, d):
            continue
        flip = (rec["acts"][d] > 0) != (pres[d] > 0)
        worst = float(np.abs(pres[d][flip]).max()) if flip.any() else 0.0
        res.note(2, "act%d gates" % d, worst < GATE_EPS, "%d of %d differ from float64, largest |pre| there %.3g (< %.0e)" % (int(flip.sum()), flip.size, worst, GATE_EPS))


def check_backward(res, rec, p, arch, memo, grads, dz, check=3, tag=""):
    """(3) the gradient at every layer against the float64 layer fed the record's gradient of the layer behind it and the record's
    gate; the tail's from the record's y; dz from the record's da0.  Per tap class."""
    nd = n_act(arch)
    gate = lambda d: (rec["acts"][d] > 0) if layer_is_relu(arch, d) else None
    g64, g32 = _both(memo, tail_backward, p, arch, rec["y"], rec["x"], rec["R"], gate(nd - 1))
    class_check(res, check, "tail bwd" + tag, "grad%d%s (tail)" % (nd - 1, tag), grads[nd - 1], g64, g32, tap_class_masks(arch, nd - 1, "bwd")[0], GRAD_TOL)
    for d in range(nd - 2, -1, -1):
        g64, g32 = _both(memo, layer_backward, p, arch, d, grads[d + 1], gate(d))
        class_check(res, check, "backward" + tag, "grad%d%s" % (d, tag), grads[d], g64, g32, tap_class_masks(arch, d, "bwd")[0], GRAD_TOL)
    z64, z32 = _both(memo, linear_backward, p, grads[0])
    class_check(res, check, "dz Linear" + tag, "dz%s from da0" % tag, dz, z64, z32, None, GRAD_TOL)


def end_to_end(p, arch, z, x, R, gates):
    """Float64 from z: (per-row loss, dz with the given gates).  The forward is shared by every gate set of an input set."""
    fwd = forward_from_z(p, arch, z)
    loss, _ = loss_and_dy(fwd["y"], x, R)
    return loss, backward_with_gates(p, arch, fwd["y"], x, R, gates)[0]


def check_end_to_end(res, rec, p, arch, memo, dz, loss=None, check=4, tag=""):
    """(4) every row of dz against the float64 backward run from z with the record's gates, GRAD_TOL of max|dz|; the per-row loss
    against float64 at LOSS_RTOL.  No row is left out."""
    loss64, dz64 = memo(end_to_end, p, arch, rec["z"], rec["x"], rec["R"], [a > 0 for a in rec["acts"]])
    dz = np.asarray(dz, np.float64)
    scale = float(np.abs(dz64).max())
    ok = bool(np.isfinite(dz).all())
    err = np.abs(dz - dz64).max(axis=1) if ok else np.full(len(dz64), np.inf)
    res.note(check, "dz%s every row" % tag, ok and bool((err < GRAD_TOL * scale).all()),
             "worst row %.3g of max|dz| = %.3g (gate %.0e), row %d of %d" % (err.max() / scale, scale, GRAD_TOL, int(err.argmax()), len(err)))
    if loss is not None:
        rel = np.abs(np.asarray(loss, np.float64) - loss64) / loss64
        res.note(check, "loss every row", bool((rel < LOSS_RTOL).all()), "worst row rel %.3g (rtol %.0e)" % (rel.max(), LOSS_RTOL))


def run_checks(rec, p, arch, memo=None):
    """Checks (1) - (5) on a record dict(z, x, R, acts [n_act] (after the forward), y, grads [n_act] (act<d> after the backward),
    loss, dz, and optionally y_generate (the image of the forward-only call) and only = dict(grads, dz): the dz-only call on the
    same inputs)."""
    memo = memo or Memo()
    res = Result()
    pres = check_forward(res, rec, p, arch, memo)
    check_gates(res, rec, arch, pres)
    check_backward(res, rec, p, arch, memo, rec["grads"], rec["dz"])
    check_end_to_end(res, rec, p, arch, memo, rec["dz"], rec["loss"])
    if rec.get("only"):
        # the dz-only call runs the same GEMM layers on the same z: its gates are the all-outputs call's, bit for bit (the tails form
        # their ReluGrad bits from the activation the last GEMM layer stored); its y is never stored: the all-outputs call's y
        # stands in (two correct tails differ by roundings of y, ~1e-7 of a gradient term, far inside GRAD_TOL)
        o = rec["only"]
        nan = sum(int(np.isnan(np.asarray(a)).sum()) for a in [o["dz"]] + list(o["grads"]))
        res.note(5, "dz-only NaN", nan == 0, "%d NaN left" % nan)
        check_backward(res, rec, p, arch, memo, o["grads"], o["dz"], check=5, tag=" (dz-only)")
        check_end_to_end(res, rec, p, arch, memo, o["dz"], None, check=5, tag=" (dz-only)")
    return res
