"""tests/support/path_reference.py (the float64 reference and the checks of tests/test_gpu_path_values.py) without a GPU:
the teacher-forced pieces chain to the NumPy oracle, the tap classes partition every layer and agree with what tests/test_plan.py
asserts for the planner, and the checks accept a float32 emulation of the path and reject it with one seeded defect at a time --
each defect by the check, the layer and the tap class it was seeded in.  Two of the defects are the fragment-order path's own
(tests/test_gpu_frag_values.py): gate bits read from the neighbouring 32-channel word, and a K-split partial sum replaced by
another tile's stored outputs (the LDS overlap of DESIGN.md section 4.5)."""
import numpy as np
import pytest

from defensegan_amd import archs, synth
from oracle import defensegan_oracle as O
from tests.support import path_reference as PR


def _case(arch, N, seed, R=1):
    p = synth.make_weights(arch, seed=1234, gain=2.0, bias_range=0.1)
    a = archs.make_arch(arch)
    rs = np.random.RandomState(seed)
    z = (rs.standard_normal((N, a.latent_dim)) * 0.3).astype(np.float32)
    x = (rs.rand(N // R, *a.image_dim) * (a.in_hi - a.in_lo) + a.in_lo).astype(np.float32)
    return p, z, x


# ---- the reference against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,N", [("mnist", 5), ("celeba", 3)])
def test_teacher_forced_pieces_chain_to_the_oracle(arch, N):
    p, z, x = _case(arch, N, 3)
    z = z.astype(np.float64)
    fwd = PR.forward_from_z(p, arch, z)
    yo, cache = O.generator_forward(p, z, arch)
    np.testing.assert_allclose(fwd["y"], yo, rtol=1e-13, atol=1e-15)
    for d in range(PR.n_act(arch)):
        np.testing.assert_allclose(fwd["act"][d], cache["acts"][d], rtol=1e-13, atol=1e-15)
        prev = z if d == 0 else fwd["act"][d - 1]
        np.testing.assert_array_equal(PR.layer_pre(p, arch, d, prev), fwd["pre"][d])             # teacher forcing = the chain's own step
    loss, dy = PR.loss_and_dy(fwd["y"], x, 1)
    np.testing.assert_allclose(loss, ((yo - x) ** 2).reshape(N, -1).mean(axis=1), rtol=1e-14)
    go = O.generator_backward(p, cache, dy, arch)
    dz, grads = PR.backward_with_gates(p, arch, fwd["y"], x, 1, [a > 0 for a in fwd["act"]])
    np.testing.assert_allclose(dz, go, rtol=1e-11, atol=1e-14 * np.abs(go).max())
    # a prescribed gate is what is used: flipping one changes the result; the piece behind it is untouched
    gates = [a > 0 for a in fwd["act"]]
    gates[1] = gates[1].copy()
    gates[1].flat[0] ^= True
    dz2, grads2 = PR.backward_with_gates(p, arch, fwd["y"], x, 1, gates)
    assert np.abs(dz2 - dz).max() > 0 and np.array_equal(grads2[-1], grads[-1])
    # R > 1: row j is compared with image j // R
    l2, _ = PR.loss_and_dy(np.repeat(fwd["y"][:1], 2, axis=0), np.stack([x[0]]), 2)
    np.testing.assert_allclose(l2, [loss[0], loss[0]], rtol=1e-14)


def _literal_tap_sets(h_in, h_out, direction):
    """Valid (kh, kw) per position by running the index map forwards over every (o, k), as deconv2d_literal does."""
    n = h_out if direction == "fwd" else h_in
    sets = [[set() for _ in range(n)] for _ in range(n)]
    for oh in range(h_in):
        for ow in range(h_in):
            for kh in range(5):
                for kw in range(5):
                    i, j = 2 * oh + kh - 1, 2 * ow + kw - 1
                    if 0 <= i < h_out and 0 <= j < h_out:
                        (sets[i][j] if direction == "fwd" else sets[oh][ow]).add((kh, kw))
    return sets


@pytest.mark.parametrize("arch", ["mnist", "celeba"])
def test_tap_classes_partition_every_layer(arch):
    layers = O._arch_layers(arch)
    nd = PR.n_act(arch)
    for direction, ds in (("fwd", range(1, nd + 1)), ("bwd", range(nd))):
        for d in ds:
            _, h_in, h_used, _, _ = layers[d - 1] if direction == "fwd" else layers[d]
            mask, classes = PR.tap_class_masks(arch, d, direction)
            n = h_used if direction == "fwd" else h_in
            assert mask.shape == (n, n) and sorted(np.unique(mask)) == list(range(len(classes)))       # every position in one class
            assert sum(c["positions"] for c in classes) == n * n
            assert [c["taps"] for c in classes] == sorted((c["taps"] for c in classes), reverse=True)
            assert sum(c["taps"] * c["positions"] for c in classes) == archs.valid_taps_1d(h_in, h_used) ** 2
            sets = _literal_tap_sets(h_in, h_used, direction)
            for i in range(n):
                for j in range(n):
                    c = classes[mask[i, j]]
                    assert sets[i][j] == {(kh, kw) for kh in c["kh"] for kw in c["kw"]}, (arch, d, direction, i, j)
            # two classes never share a tap pattern
            assert len({(c["kh"], c["kw"]) for c in classes}) == len(classes)
    mask, classes = PR.tap_class_masks(arch, 0, "fwd")
    assert mask.shape == (4, 4) and len(classes) == 1


def test_tap_classes_match_the_planner_figures():
    """The figures tests/test_plan.py asserts for the planner's classes (test_classes_of_the_mnist_layers,
    test_k_pair_jobs_split_the_taps_of_the_long_classes_in_two)."""
    big = lambda cl: (cl[0]["positions"], cl[0]["taps"])
    _, c = PR.tap_class_masks("mnist", 1, "fwd")            # Generator.2 forward, 4x4 -> 7x7 used
    assert len(c) == 16 and big(c) == (4, 9)
    _, c = PR.tap_class_masks("mnist", 2, "fwd")            # Generator.3 forward, 7 -> 14
    assert len(c) == 25 and big(c) == (25, 9)
    _, c = PR.tap_class_masks("mnist", 1, "bwd")            # Generator.3 backward: 7x7 grid reading 14x14
    assert len(c) == 9 and big(c) == (25, 25)
    _, c = PR.tap_class_masks("mnist", 0, "bwd")            # Generator.2 backward: 100 / 80 / 64 / 40 / 32 / 16 chunks of 32 at K = 128 per tap
    assert sorted({k["taps"] * 4 for k in c}, reverse=True) == [100, 80, 64, 40, 32, 16]
    _, c = PR.tap_class_masks("celeba", 0, "bwd")           # 4x4 <- 8x8: the interior class is 4 positions x 25 taps
    assert len(c) == 9 and big(c) == (4, 25)


# ---- the checks against a float32 emulation, clean and with seeded defects ---------------------------------------------------
def _one_tap(F, taps):
    G = np.zeros_like(F)
    for kh, kw in taps:
        G[kh, kw] = F[kh, kw]
    return G


def _keep_last_rows(new, old, sel):
    """The class's M axis (row-major over latent row x position of the class) computed but for its last M % 32 rows."""
    a, b = new[:, sel], old[:, sel]                          # [N, positions, C]
    M = a.shape[0] * a.shape[1]
    assert M % 32, "the case must leave a partial 32-row block"
    flat = a.reshape(M, -1).copy()
    flat[M - M % 32:] = b.reshape(M, -1)[M - M % 32:]
    new[:, sel] = flat.reshape(a.shape)


def emulate(p, arch, z, x, R, defect=(), stale=None, x_prev=None):
    """The path in float32 on the CPU with the record layout of the device (path_reference.run_checks).  Every matrix product
    runs over the channels in REVERSED order, so the emulation is another float32 summation than the checks' yardstick, as the
    device is.  defect: one of
      ("fwd_tap", d, c)    forward layer d: the last valid tap of class c is not added
      ("bwd_tap", d, c)    the backward that writes grad<d>: likewise
      ("kpair", d, c)      the backward that writes grad<d>: taps 12 .. 24 of the 25-tap class c are not added
      ("stale_fwd", d, c)  forward layer d: the last (rows * positions) % 32 rows of class c keep the contents of `stale`
      ("stale_bwd", d, c)  the backward that writes grad<d>: ... keep the forward activation (the backward works in place)
      ("gate", d, n)       the backward that writes grad<d> masks row n with row n + 1's gate
      ("only_prev_x",)     the dz-only call differentiates against x_prev
      ("gate_word", d)     the backward that writes grad<d> takes the gate bits of every 32-channel word from the NEXT word of the
                           row (feature f masked by the gate of feature f + 32): a wrong word index into the fragment-order
                           path's gate bits
      ("overlap", d, c)    forward layer d (K = 128: a K split of 2): at one position of class c, channels 32 .. 63, the second
                           K part's partial sum is replaced by the STORED OUTPUTS (bias and ReLU applied) of another wave tile --
                           what dg_fgemm.hip's wave 0 summed when wave 2's epilogue slice lay inside tile 0's image"""
    f32 = np.float32
    layers = O._arch_layers(arch)
    nd = PR.n_act(arch)
    kind = defect[0] if defect else None
    W = lambda name: np.asarray(p[name], f32)

    def fwd_layer(d, prev):
        if d == 0:
            Wl = W("Generator.Input.W")
            return (prev[:, ::-1] @ Wl[::-1] + W("Generator.Input.b")).reshape(len(prev), 4, 4, -1)
        name, h_in, h_used, _, _ = layers[d - 1]
        F = W(name + ".Filters")
        pre = O.deconv2d(np.ascontiguousarray(prev[..., ::-1]), np.ascontiguousarray(F[..., ::-1]), W(name + ".Biases"), h_used)
        if kind == "fwd_tap" and defect[1] == d:
            mask, classes = PR.tap_class_masks(arch, d, "fwd")
            c = classes[defect[2]]
            sel = mask == defect[2]
            pre[:, sel] -= O.deconv2d(prev, _one_tap(F, [(c["kh"][-1], c["kw"][-1])]), None, h_used)[:, sel]
        if kind == "overlap" and defect[1] == d:
            mask, classes = PR.tap_class_masks(arch, d, "fwd")
            c = classes[defect[2]]
            taps = [(kh, kw) for kh in c["kh"] for kw in c["kw"]]
            cin = F.shape[3]
            half = len(taps) * cin // 2                      # K part 0: the first half of the flattened (tap, k) sequence
            G = np.zeros_like(F)
            for t, (kh, kw) in enumerate(taps):
                n = min(max(half - t * cin, 0), cin)
                G[kh, kw, :, :n] = F[kh, kw, :, :n]
            part0 = O.deconv2d(prev, G, None, h_used)
            pos = np.argwhere(mask == defect[2])
            (i, j), (i2, j2) = pos[0], pos[-1]               # the hit position and one of another tile
            other = np.maximum(pre[:, i2, j2, 0:32], 0)      # that tile's stored outputs
            pre[:, i, j, 32:64] = part0[:, i, j, 32:64] + other + W(name + ".Biases")[32:64]
        return pre

    def bwd_layer(d, g_next, gate):
        name, h_in, _, _, _ = layers[d]
        F = W(name + ".Filters")
        g = O.deconv2d_backward_input(np.ascontiguousarray(g_next[..., ::-1]), np.ascontiguousarray(F[:, :, ::-1, :]), h_in)
        if kind in ("bwd_tap", "kpair") and defect[1] == d:
            mask, classes = PR.tap_class_masks(arch, d, "bwd")
            c = classes[defect[2]]
            taps = [(kh, kw) for kh in c["kh"] for kw in c["kw"]]
            assert kind == "bwd_tap" or len(taps) == 25
            drop = taps[-1:] if kind == "bwd_tap" else taps[25 // 2:]
            sel = mask == defect[2]
            g[:, sel] -= O.deconv2d_backward_input(g_next, _one_tap(F, drop), h_in)[:, sel]
        if gate is not None:
            gate = gate.copy()
            if kind == "gate" and defect[1] == d:
                gate[defect[2]] = gate[defect[2] + 1]
            if kind == "gate_word" and defect[1] == d:
                gate = np.roll(gate.reshape(len(gate), -1), -32, axis=1).reshape(gate.shape)
            g = g * gate
        return g

    def backward(acts, y, xx):
        _, dy = PR.loss_and_dy(y, xx, R, f32)
        g = dy * y * (f32(1) - y) if layers[-1][3] == "sigmoid" else dy * (f32(1) - y * y)
        grads = [None] * nd
        for d in range(nd - 1, -1, -1):
            grads[d] = bwd_layer(d, g, (acts[d] > 0) if PR.layer_is_relu(arch, d) else None)
            if kind == "stale_bwd" and defect[1] == d:
                _keep_last_rows(grads[d], acts[d], PR.tap_class_masks(arch, d, "bwd")[0] == defect[2])
            g = grads[d]
        da0 = grads[0].reshape(len(z), -1)
        return grads, da0[:, ::-1] @ W("Generator.Input.W").T[::-1]

    acts, prev = [], np.asarray(z, f32)
    for d in range(nd):
        a = PR.layer_out(arch, d, fwd_layer(d, prev))
        if kind == "stale_fwd" and defect[1] == d:
            _keep_last_rows(a, stale["acts"][d], PR.tap_class_masks(arch, d, "fwd")[0] == defect[2])
        acts.append(a)
        prev = a
    name, h_in, h_used, act, _ = layers[-1]
    t = O.deconv2d(np.ascontiguousarray(prev[..., ::-1]), np.ascontiguousarray(W(name + ".Filters")[..., ::-1]), W(name + ".Biases"), h_used)
    y = f32(1) / (f32(1) + np.exp(-t)) if act == "sigmoid" else np.tanh(t)
    loss, _ = PR.loss_and_dy(y, x, R, f32)
    grads, dz = backward(acts, y, x)
    rec = {"z": np.asarray(z, f32), "x": np.asarray(x, f32), "R": R, "acts": acts, "y": y, "grads": grads, "loss": loss, "dz": dz}
    og, odz = backward(acts, y, x_prev if kind == "only_prev_x" else x)
    rec["only"] = {"grads": og, "dz": odz}
    assert all(a.dtype == f32 for a in acts + grads + [y, dz, odz, loss])
    return rec


def _border_class(arch, d, direction):
    """A few-tap border class: the one with the fewest taps among those with at least two."""
    _, classes = PR.tap_class_masks(arch, d, direction)
    return max(c for c, k in enumerate(classes) if k["taps"] >= 2)


_STATE = {}


def _setup(arch):
    """One input set per architecture, its clean emulation and the memo of reference evaluations, shared by the defect cases
    (a defect changes what is behind it; everything in front of it is evaluated once)."""
    if arch not in _STATE:
        N = {"mnist": 5, "celeba": 3}[arch]
        p, z, x = _case(arch, N, 11)
        _, z_prev, x_prev = _case(arch, N, 12)
        _STATE[arch] = dict(p=p, z=z, x=x, x_prev=x_prev, memo=PR.Memo(), stale=emulate(p, arch, z_prev, x_prev, 1), clean=emulate(p, arch, z, x, 1))
    return _STATE[arch]


@pytest.mark.parametrize("arch", ["mnist", "celeba"])
def test_checks_accept_the_clean_float32_emulation(arch):
    s = _setup(arch)
    res = PR.run_checks(s["clean"], s["p"], arch, s["memo"])
    print("\n  " + "\n  ".join(res.lines + res.summary()))
    assert res.fails == [], res.fails
    assert {c for c in (1, 2, 3, 4, 5) if any(l.startswith("(%d)" % c) for l in res.lines)} == {1, 2, 3, 4, 5}      # every check ran


def _cases():
    out = []
    for arch, nd in (("mnist", 3), ("celeba", 4)):
        # one tap dropped in one border class: every GEMM layer of MNIST, the first and last of CelebA
        for d in ((1, 2) if arch == "mnist" else (1, nd - 1)):
            out.append((arch, ("fwd_tap", d, _border_class(arch, d, "fwd")), 1, "act%d class %%d" % d))
        for d in ((0, 1) if arch == "mnist" else (0, nd - 2)):
            out.append((arch, ("bwd_tap", d, _border_class(arch, d, "bwd")), 3, "grad%d class %%d" % d))
        out.append((arch, ("kpair", 0, 0), 3, "grad0 class %d"))                      # the 4x4 <- 7x7 / 8x8 backward's 25-tap class
        out.append((arch, ("stale_fwd", 1, _border_class(arch, 1, "fwd")), 1, "act1 class %d"))
        out.append((arch, ("stale_bwd", 1, 0), 3, "grad1 class %d"))
        out.append((arch, ("gate", 1, 1), 3, None))
        out.append((arch, ("only_prev_x",), 5, None))
        out.append((arch, ("gate_word", 1), 3, None))
    out.append(("mnist", ("kpair", 1, 0), 3, "grad1 class %d"))                       # 7x7 <- 14x14: 25 positions x 25 taps
    # the K = 128 layers the fragment-order path splits in two: MNIST's writes act2 as NHWC rows (where the overlap was), CelebA's
    # writes fragment order
    out.append(("mnist", ("overlap", 2, 0), 1, "act2 class %d"))
    out.append(("celeba", ("overlap", 2, 1), 1, "act2 class %d"))
    return out


@pytest.mark.parametrize("arch,defect,check,label", _cases(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_checks_reject_one_seeded_defect(arch, defect, check, label):
    s = _setup(arch)
    rec = emulate(s["p"], arch, s["z"], s["x"], 1, defect, stale=s["stale"], x_prev=s["x_prev"])
    res = PR.run_checks(rec, s["p"], arch, s["memo"])
    got = res.labels(check)
    print("\n  " + "\n  ".join(l for _, _, l in res.fails))
    assert got, "defect %s was not rejected by check (%d)" % (defect, check)
    if defect[0] in ("gate", "gate_word"):
        # one row of grad<d> (gate_word: every row) is masked wrongly: the layer's own teacher-forced check fails, the layers behind it (computed from what
        # the record holds) do not
        assert {l.split(" class")[0] for l in got} == {"grad%d" % defect[1]}
    elif defect[0] == "only_prev_x":
        # the all-outputs call is untouched; the dz-only call's tail gradient (teacher-forced from y and x) and its dz end to end fail
        assert not [f for f in res.fails if f[0] != 5]
        assert any(l.startswith("grad%d (dz-only) (tail)" % (PR.n_act(arch) - 1)) for l in got) and "dz (dz-only) every row" in got
    else:
        # teacher forcing localises: among the per-class comparisons of this check exactly the seeded layer and class fail
        assert [l for l in got if "class" in l] == [label % defect[2]], got
        # the forward checks are untouched by a backward defect
        if check == 3:
            assert not res.labels(1) and not res.labels(2)


def test_a_border_defect_hides_behind_the_whole_tensor_maximum():
    """Why the scale is the class and not the layer: the class of Generator.3's backward on MNIST with the smallest values gets an
    error in its last tap that sits between the gradient gate (1e-5) of the class's own maximum and of the whole tensor's: it
    passes when errors are divided by the maximum of the whole tensor and is rejected per class."""
    s = _setup("mnist")
    rec = s["clean"]
    mask, classes = PR.tap_class_masks("mnist", 1, "bwd")
    gate = rec["acts"][1] > 0
    full = PR.layer_backward(s["p"], "mnist", 1, rec["grads"][2], gate)
    yard = PR.layer_backward(s["p"], "mnist", 1, rec["grads"][2], gate, np.float32)
    scales = [np.abs(full[:, mask == c]).max() for c in range(len(classes))]
    c = int(np.argmin(scales))
    scale_c, scale_all = scales[c], np.abs(full).max()
    assert classes[c]["taps"] < 25 and scale_all > 2 * scale_c                 # a border class, well below the interior
    F = np.asarray(s["p"]["Generator.3.Filters"], np.float64)
    k = classes[c]
    tap = O.deconv2d_backward_input(rec["grads"][2].astype(np.float64), _one_tap(F, [(k["kh"][-1], k["kw"][-1])]), 7) * gate
    sel = mask == c
    target = PR.GRAD_TOL * np.sqrt(scale_c * scale_all)                        # between the two gates
    bad = rec["grads"][1].copy()
    bad[:, sel] = (full[:, sel] + target / np.abs(tap[:, sel]).max() * tap[:, sel]).astype(np.float32)
    err = np.abs(bad - full).max()
    assert err / scale_all < PR.GRAD_TOL < err / scale_c
    res = PR.Result()
    PR.class_check(res, 3, "backward", "grad1", bad, full, yard, mask, PR.GRAD_TOL)
    assert res.labels(3) == ["grad1 class %d" % c], res.labels(3)
    res = PR.Result()
    PR.class_check(res, 3, "backward", "grad1", bad, full, yard, None, PR.GRAD_TOL)      # one scale for the whole tensor: not seen
    assert res.fails == []
