"""-m "not gpu": what tests/test_gpu_jsma_edges.py rests on, shown on the CPU.  Every input set of the saliency-map edge cases
(tests/support/jsma_reference.py: the all-ties and the dyadic linear families, EDGE_CASES, EXIT_CASE) has the property it was chosen
for -- the domain patterns reach the threads and waves they name, the dyadic sets are mostly exact ties whose tied pairs lie 64
columns apart and in rows of different waves, class 0's bias keeps every image of the linear families away from its target, the
reference sets are at least 75 % decidable -- and the pair rule restated with one fault at a time gives another result on them, so
the inputs can tell the faults apart.  No device code runs here."""
import os

import numpy as np
import pytest
import torch

from tests.support import jsma_reference as JR

DECIDABLE_CAP = 0.75
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "defensegan_amd", "csrc")


def _chw(f, shape):
    """The index of HWC feature f had the row been flattened channel first: (c H + h) W + w."""
    H, W, C = shape
    f = np.asarray(f)
    return np.where(f < 0, f, ((f % C) * H + f // (W * C)) * W + (f // C) % W)


# ---------------------------------------------------------------------- 1a. the all-ties family
def test_the_chunks_and_patterns_stand_where_the_all_ties_family_was_chosen_for():
    with open(os.path.join(CSRC, "dg_jsma.hip")) as fh:
        src = fh.read()
    assert "const int chunk = ((P + 255) / 256 + V - 1) / V * V;" in src and "for (int i = wave; i < D - 1; i += 4) {" in src
    assert "for (int j = i + 1 + lane; j < D; j += 64) {" in src
    assert {F: JR.pair_chunk(F) for F in JR.TIE_SHAPES} == JR.TIE_CHUNKS
    assert sorted(set(JR.TIE_CHUNKS.values())) == [1, 4, 5, 8, 12, 20]
    assert any(F % c and -(-F // c) > 1 for F, c in JR.TIE_CHUNKS.items())          # a last thread with a partial chunk (F = 1300)
    for F, shape in JR.TIE_SHAPES.items():
        assert int(np.prod(shape)) == F
        c = JR.TIE_CHUNKS[F]
        doms = dict(zip(JR.TIE_PATTERNS, JR.tie_domains(F)))
        assert len(doms) == len(JR.TIE_PATTERNS) == 8
        assert len(doms["full"]) == F and doms["last_two"].tolist() == [F - 2, F - 1] and doms["first_and_last"].tolist() == [0, F - 1]
        assert len(doms["three"]) == 3 and len(doms["thirteen"]) == 13 and (np.diff(doms["every_third"]) == 3).all()
        owner = doms["wave0_empty"] // c
        assert (owner >= 64).all() and (len(owner) > 0) == (F > 64 * c)
        if F > 64 * c:
            assert owner.min() == 64                                # wave 0's total is 0, wave 1 starts the list
        odd = np.unique(doms["odd_threads"] // c)
        assert (odd % 2 == 1).all() and len(odd) == -(-F // c) // 2
        for d in doms.values():
            assert (np.diff(d) > 0).all()
    assert sum(F > 64 * c for F, c in JR.TIE_CHUNKS.items()) >= 5


@pytest.mark.parametrize("theta", JR.TIE_THETAS)
@pytest.mark.parametrize("F", sorted(JR.TIE_SHAPES))
def test_all_ties_expectation_and_margin(F, theta):
    """The expectation written down from the patterns is the float64 reference's where the reference's table fits (F <= 784), every
    score of it is 4.0, and class 0 keeps its lead for the whole run at every F."""
    m, p, x, t, doms = JR.tie_case(F, theta)
    want = JR.tie_expected(x, doms, theta, JR.TIE_ITERS)
    mg = JR.linear_margins(p, x, t, want["choices"], theta)
    print("F %d theta %g: iters %s, smallest margin of class 0 %.1f" % (F, theta, want["iters"].tolist(), mg.min()))
    assert mg.min() > 0 and (t == 1).all()
    assert want["iters"].tolist()[:4] == [6, 1, 1, 1] and want["iters"][7] == 6 and want["iters"][4] == min(6, len(doms[4]) // 2)
    assert (want["x_adv"] != x).reshape(len(x), -1).sum(axis=1).tolist() == want["n_changed"].tolist()
    a, b = p[0][0][:, 1].astype(np.float64), p[0][0][:, 0].astype(np.float64)
    for d in doms:
        if len(d) >= 2 and F <= 784:
            S = JR.pair_choice(a, b, np.isin(np.arange(F), d), theta)[4]
            assert (S[np.triu_indices(len(d), 1)] == 4.0).all()
    if F <= 784:
        ref = JR.run(m, p, x, t, theta, JR.TIE_ITERS, 0.0, 1.0, False)
        for k in ("choices", "iters", "n_changed", "final_class"):
            assert np.array_equal(ref[k], want[k]), k
        assert np.array_equal(ref["x_adv"].astype(np.float32), want["x_adv"])


# ---------------------------------------------------------------------- 1b. the dyadic family
def _tied(params, x, t, ref, theta):
    """Per step taken of a linear run: (image, D, compacted (i, j) of every pair at the best score, the first being the one taken)."""
    W = params[0][0].astype(np.float64)
    B = len(x)
    with np.errstate(invalid="ignore"):
        dom = (x.reshape(B, -1) < 1.0) if theta > 0 else (x.reshape(B, -1) > 0.0)
    out = []
    for k in range(len(ref["choices"])):
        for i in np.flatnonzero(ref["choices"][k][:, 0] >= 0):
            a, b = W[:, t[i]], W.sum(axis=1) - W[:, t[i]]
            p, q, best, second, S = JR.pair_choice(a, b, dom[i], theta)
            assert (p, q) == tuple(ref["choices"][k][i])
            S32 = JR.pair_choice(a.astype(np.float32), b.astype(np.float32), dom[i], theta)[4]
            assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), S)          # nothing rounds: an exact oracle
            ii, jj = np.nonzero(S == best)
            assert (best - second == 0) == (len(ii) > 1) and ref["score_gap"][k, i] == best - second
            out.append((i, len(S), ii, jj))
            dom[i, [p, q]] = False
    return out


def test_dyadic_sets_are_mostly_ties_across_lanes_trips_and_waves():
    steps = ties = 0
    far = same_lane = waves = 0
    for F, n, theta in JR.DYADIC_CASES:
        m, p, x, t = JR.dyadic_case(F, n, theta)
        W = p[0][0]
        assert np.array_equal(W * 8, np.round(W * 8)) and np.abs(W * 8).max() <= 16 and (t >= 1).all() and (t < n).all()
        out_share = ((x == 1.0) if theta > 0 else (x == 0.0)).mean()
        assert 0.4 < out_share < 0.6
        ref = JR.dyadic_run(F, n, theta)
        mg = JR.linear_margins(p, x, t, ref["choices"], theta)
        assert mg.min() > 0 and (ref["final_class"] == 0).all()     # the bias margin holds for the whole run
        st = _tied(p, x, t, ref, theta)
        tied = [s for s in st if len(s[2]) > 1]
        steps += len(st)
        ties += len(tied)
        for _, D, ii, jj in tied:
            row = ii == ii[0]
            far += bool((row & (jj - jj[0] >= 64)).any())
            same_lane += bool((row & (jj > jj[0]) & ((jj - jj[0]) % 64 == 0)).any())
            waves += bool((ii % 4 != ii[0] % 4).any())
        print("F %d n %d theta %g: %d steps, %d exact ties, iters %s" % (F, n, theta, len(st), len(tied), ref["iters"].tolist()))
        assert len(st) >= len(x)                                    # the set attacks something
    print("dyadic family: %d steps, %d exact ties; tied with the pair taken: a column >= 64 further in its row %d, in its lane's later "
          "trip %d, a row of another wave %d" % (steps, ties, far, same_lane, waves))
    assert 2 * ties >= steps
    assert far > 0 and same_lane > 0 and waves > 0


# ---------------------------------------------------------------------- 2.-5. the sets compared with the float64 reference
@pytest.mark.parametrize("name", sorted(JR.EDGE_CASES))
def test_every_edge_set_is_mostly_decidable(name):
    c = JR.EDGE_CASES[name]
    out = JR.edge_run(name)
    dec = JR.decidable(out)
    print("%s: decidable %d/%d, iters %s, success rate %.3f" % (name, dec.sum(), dec.size, out["iters"].tolist(),
                                                               (out["final_class"] == out["target"]).mean()))
    assert dec.mean() >= DECIDABLE_CAP
    assert out["iters"].max() >= 1 and (out["n_changed"] <= 2 * out["iters"]).all()


def test_sparse_sets_are_sparse_and_cover_both_endings():
    x = JR.edge_inputs(JR.SPARSE_CASES[0])[2]
    assert 0.40 < (x == 0.0).mean() < 0.50 and 0.10 < (x == 1.0).mean() < 0.20
    for name in JR.SPARSE_CASES:
        c, out = JR.EDGE_CASES[name], JR.edge_run(name)
        ok = out["final_class"] == out["target"]
        assert JR.decidable(out).all()
        assert 2 <= out["iters"].min() and out["iters"].max() <= 20 and 0.25 <= ok.mean() <= 1.0
        assert (out["n_changed"] == 2 * out["iters"]).all()
        xf = x.reshape(len(x), -1)
        for i in range(len(x)):
            f = out["choices"][:, i][out["choices"][:, i] >= 0]
            assert (xf[i, f] != (1.0 if c["theta"] > 0 else 0.0)).all()
    ok = np.concatenate([JR.edge_run(n)["final_class"] == JR.edge_run(n)["target"] for n in JR.SPARSE_CASES])
    assert ok.any() and not ok.all()
    its = np.concatenate([JR.edge_run(n)["iters"] for n in JR.SPARSE_CASES])
    assert its.min() == 2 and its.max() == 20


def test_range_sets_bind_where_they_were_chosen_for():
    for th in (0.5, -0.5):
        s, u, pt, o = (JR.edge_run("%s_th%g" % (k, th)) for k in ("signed", "unbounded", "point", "outside"))
        x = JR.edge_inputs("signed_th%g" % th)[2]
        assert x.min() == -1.0 and x.max() == 1.0
        assert s["x_adv"].min() == -1.0 and s["x_adv"].max() == 1.0
        assert (np.abs(u["x_adv"]).max() == 1.5) and not np.array_equal(u["choices"], s["choices"])     # without bounds a feature at 1 moves on
        moved = pt["x_adv"] != x
        assert moved.any() and (pt["x_adv"][moved] == 0.5).all() and ((x[moved] < 0.5) if th > 0 else (x[moved] > 0.5)).all()
        xo = JR.edge_inputs("outside_th%g" % th)[2]
        away = (xo < 0.0) | (xo > 1.0)
        assert away.reshape(2, -1).sum(axis=1).tolist() == [3, 3]
        hit = (o["x_adv"] != xo) & away
        print("theta %g: %d of the 6 elements outside [0, 1] are moved, to %s" % (th, hit.sum(), o["x_adv"][hit].tolist()))
        assert hit.any() and (away & ~hit).any()                    # one is moved (and clipped into the range), one keeps its value
        assert (o["x_adv"][hit] == (0.0 if th > 0 else 1.0)).all()
        assert np.array_equal(o["x_adv"][away & ~hit], xo[away & ~hit].astype(np.float64))
        assert JR.decidable(o).all()


def test_channel_sets_tell_the_flatten_orders_apart():
    for name in JR.CONV_CASES:
        c, out = JR.EDGE_CASES[name], JR.edge_run(name)
        assert JR.decidable(out).all() and 1 <= out["iters"].min() and out["iters"].max() <= 9
        f = out["choices"][out["choices"] >= 0]
        assert (f % 3 > 0).any() and (_chw(f, c["shape"]) != f).mean() > 0.5
        assert (int(np.prod(c["shape"])) % 4 == 0) == (c["shape"] == (4, 6, 3))
    assert all(JR.decidable(JR.edge_run(n)).all() for n in JR.MANY_CLASS_CASES)
    assert JR.edge_inputs("mlp200_p0")[0].param_shapes()[-1][0][1] == 200


def test_exit_batches_are_decidable_and_not_empty():
    m, p, x, t, ref, bat = JR.exit_batches()
    print("images done after exactly 1 step: %d, after exactly 2: %d" % (len(bat[1]), len(bat[2])))
    dec = JR.decidable(ref)
    for k in (1, 2):
        assert len(bat[k]) >= 1 and dec[bat[k]].all() and (ref["iters"][bat[k]] == k).all()
        assert (ref["final_class"][bat[k]] == t[bat[k]]).all()
        assert (ref["choices"][k:, bat[k]] == -1).all()


@pytest.mark.parametrize("sign", [1, -1])
def test_the_infinite_pixel_keeps_its_logits_infinite_and_its_image_going(sign):
    m, p, bad, x, t, theta = JR.inf_case(sign)
    W = p[0][0]
    i, f = JR.INF_PIXEL
    assert (W != 0).all() and np.array_equal(W * 8, np.round(W * 8)) and np.abs(W * 8).max() <= 16 and (p[0][1] == 0).all()
    assert np.isinf(bad).sum() == 1 and bad[i].reshape(-1)[f] == sign * JR.INF and np.array_equal(np.delete(bad.reshape(-1), 16 * i + f), np.delete(x.reshape(-1), 16 * i + f))
    with np.errstate(invalid="ignore"):
        z = bad[i].reshape(-1).astype(np.float64) @ W.astype(np.float64)
    assert z.tolist() == ([JR.INF, -JR.INF, JR.INF] if sign > 0 else [-JR.INF, JR.INF, -JR.INF]) and t[i] == 2
    on_logits = JR.run(m, p, bad, t, theta, JR.INF_ITERS, 0.0, 1.0, False)
    on_probs = JR.run(m, p, bad, t, theta, JR.INF_ITERS, 0.0, 1.0, True)
    print("pixel %g: pairs on the logits %s, final_class %d" % (sign * JR.INF, on_logits["choices"][:, i].tolist(), on_logits["final_class"][i]))
    assert on_logits["iters"][i] >= 2 and (on_logits["choices"][:, i] != f).all() and on_logits["final_class"][i] == (0 if sign > 0 else 1)
    assert on_probs["iters"][i] == 0 and on_probs["n_changed"][i] == 0 and on_probs["final_class"][i] == on_logits["final_class"][i]
    assert on_logits["x_adv"][i].reshape(-1)[f] == sign * JR.INF


# ---------------------------------------------------------------------- 9. the tests have teeth
FAULTS = ("last_maximum", "q_before_p", "other_bound", "no_clip", "channel_first")


def _pick(a, b, dom, theta, fault):
    idx = np.flatnonzero(dom)
    D = len(idx)
    if D < 2:
        return -1, -1
    with np.errstate(invalid="ignore", over="ignore"):
        A, Bs = a[idx][:, None] + a[idx][None, :], b[idx][:, None] + b[idx][None, :]
        adm = ((A > 0) & (Bs < 0)) if theta > 0 else ((A < 0) & (Bs > 0))
        S = np.where(adm & np.triu(np.ones((D, D), bool), 1), -(A * Bs), 0.0)
    S = np.where(np.isnan(S), 0.0, S)
    if not S.max() > 0:
        return -1, -1
    ii, jj = np.nonzero(S == S.max())                               # in row-major order
    k = {"last_maximum": len(ii) - 1, "q_before_p": int(np.lexsort((ii, jj))[0])}.get(fault, 0)
    return int(idx[ii[k]]), int(idx[jj[k]])


def rule_run(m, p, x, t, theta, max_iters, lo, hi, of_probs, fault=None):
    """DESIGN.md's loop restated once more, in float64, with at most one fault: {choices, x_adv}."""
    net = JR.logits_fn(m, p)
    adv = torch.tensor(np.asarray(x), dtype=torch.float64)
    B = adv.shape[0]
    flat = adv.reshape(B, -1)
    xf = flat.numpy().copy()
    with np.errstate(invalid="ignore"):
        if fault == "other_bound":
            dom = (xf > lo) if theta > 0 else (xf < hi)
        else:
            dom = (xf < hi) if theta > 0 else (xf > lo)
    active = np.ones(B, bool)
    choices = np.full((max_iters, B, 2), -1, np.int32)
    for k in range(max_iters):
        if not active.any():
            break
        O, a, b = JR.gradients(net, adv, t, of_probs)
        active = active & ~np.isnan(O).any(axis=1) & (JR._first_argmax(O) != t) & (dom.sum(axis=1) >= 2)
        for i in np.flatnonzero(active):
            pq = _pick(a[i], b[i], dom[i], theta, fault)
            if pq[0] < 0:
                active[i] = False
                continue
            for f in pq:
                flat[i, f] = flat[i, f] + theta if fault == "no_clip" else torch.clamp(flat[i, f] + theta, lo, hi)
                dom[i, f] = False
            choices[k, i] = pq
    if fault == "channel_first":
        choices = _chw(choices, np.shape(x)[1:]).astype(np.int32)
    return {"choices": choices, "x_adv": adv.numpy()}


def _teeth_sets():
    """name -> (inputs of rule_run, the expected result): a few sets of each of sections 1 to 4, the small ones."""
    sets = {}
    for F in (16, 25):
        for th in JR.TIE_THETAS:
            m, p, x, t, doms = JR.tie_case(F, th)
            sets["ties%d_th%g" % (F, th)] = ((m, p, x, t, th, JR.TIE_ITERS, 0.0, 1.0, False), JR.tie_expected(x, doms, th, JR.TIE_ITERS))
    for F, n, th in ((25, 2, 1.0), (25, 3, -1.0), (784, 2, -1.0), (784, 3, 0.25)):
        m, p, x, t = JR.dyadic_case(F, n, th)
        sets["dyadic%d_n%d_th%g" % (F, n, th)] = ((m, p, x, t, th, JR.DYADIC_ITERS, 0.0, 1.0, False), JR.dyadic_run(F, n, th))
    for name in ("sparse_th1_p0", "signed_th0.5", "signed_th-0.5", "point_th0.5", "outside_th-0.5", "conv6x5x3_p0", "conv4x6x3_p1"):
        c = JR.EDGE_CASES[name]
        m, p, x, t = JR.edge_inputs(name)
        sets[name] = ((m, p, x, t, c["theta"], c["max_iters"], c["lo"], c["hi"], bool(c["of_probs"])), JR.edge_run(name))
    return sets


@pytest.fixture(scope="module")
def teeth():
    sets = _teeth_sets()
    for name, (args, want) in sets.items():                         # the restatement without a fault is the expectation
        got = rule_run(*args)
        assert np.array_equal(got["choices"], want["choices"]), name
        assert np.array_equal(got["x_adv"].astype(np.float32), np.asarray(want["x_adv"]).astype(np.float32)), name
    return sets


@pytest.mark.parametrize("fault,must", [("last_maximum", ("ties16_th1", "dyadic784_n2_th-1")), ("q_before_p", ("dyadic25_n2_th1", "dyadic25_n3_th-1")),
                                        ("other_bound", ("ties25_th-0.5", "sparse_th1_p0", "signed_th-0.5", "point_th0.5")),
                                        ("no_clip", ("ties16_th1", "sparse_th1_p0", "outside_th-0.5")),
                                        ("channel_first", ("conv6x5x3_p0", "conv4x6x3_p1"))])
def test_each_fault_changes_the_expected_result(teeth, fault, must):
    assert fault in FAULTS
    seen = []
    for name, (args, want) in teeth.items():
        got = rule_run(*args, fault=fault)
        if not (np.array_equal(got["choices"], want["choices"]) and
                np.array_equal(got["x_adv"].astype(np.float32), np.asarray(want["x_adv"]).astype(np.float32))):
            seen.append(name)
    print("%s shows on %s" % (fault, seen))
    assert set(must) <= set(seen)
