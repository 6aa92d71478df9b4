"""-m gpu: the SPSA attack on the device (dg_spsa_queries, dg_spsa_step, network_builder.SPSA) against the CPU restatement in
tests/support/spsa_reference.py: queries and step bit for bit, the estimate within the fixed-order float32 sum bound, and the
driver's compositions.  The cases (S.KERNEL, S.COMPOSE) are fixed on the CPU, tests/test_spsa_cpu.py."""
import numpy as np
import pytest

from defensegan_amd import _native, gan_defense, network_builder as nb
from tests.helpers import make_gan
from tests.support import spsa_reference as S
from tests.support.bpda_reference import init_params

pytestmark = pytest.mark.gpu
K = S.KERNEL
Q = 2 * K["n"] + 1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _queries(x_cur, first_image, B=None, n=K["n"], k=K["k"], lo=K["lo"], hi=K["hi"], delta=K["delta"], seed=K["seed"]):
    import torch
    t = _dev(x_cur)
    B = len(x_cur) if B is None else B
    P = t[0].numel()
    q = torch.full((B, 2 * n + 1, P), -7.0, device="cuda")
    _native.check(_native.load().dg_spsa_queries(t.data_ptr(), B, P, n, delta, seed, first_image, k, lo, hi, q.data_ptr(), None))
    return q.cpu().numpy()


def _step(Z, y, x_cur, x_orig, first_image, eps, eps_iter, want_grad=True, n=K["n"], k=K["k"], lo=K["lo"], hi=K["hi"]):
    import torch
    tz, ty, tc, to = _dev(Z), _dev(y), _dev(x_cur), _dev(x_orig)
    B, P = x_cur.shape
    nxt, g = torch.full_like(tc, -7.0), (torch.full_like(tc, -7.0) if want_grad else None)
    _native.check(_native.load().dg_spsa_step(tz.data_ptr(), ty.data_ptr(), B, Z.shape[1], P, n, K["delta"], K["seed"], first_image, k,
                                              tc.data_ptr(), to.data_ptr(), eps, eps_iter, lo, hi, nxt.data_ptr(),
                                              g.data_ptr() if want_grad else None, None))
    return nxt.cpu().numpy(), (g.cpu().numpy() if want_grad else None)


def _step32(g, xc, xo, eps, eps_iter, lo, hi):
    f = np.float32
    d = (xc + f(eps_iter) * np.sign(g).astype(f)) - xo
    return np.clip(xo + np.clip(d, -f(eps), f(eps)), f(lo), f(hi)).astype(f)


# ---------------------------------------------------------------------- 1, 2. the queries
@pytest.mark.parametrize("P", [784, 25])
def test_queries_bit_for_bit_and_independent_of_batching(P):
    """B = 3, n = 33 (a second Philox group with one live bit), first_image = 5, iter = 2; 784 elements take the float4 path, 25 the
    scalar one; x_cur has elements at both clip bounds.  Each image alone, with its own first_image, equals its rows of the batch."""
    x_cur = S.kernel_inputs(P)[0]
    got = _queries(x_cur, K["first_image"])
    want = S.queries(x_cur, K["n"], K["delta"], K["seed"], K["first_image"], K["k"], K["lo"], K["hi"])
    assert got.shape == want.shape == (K["B"], Q, P)
    assert got.tobytes() == want.tobytes()
    assert got[:, 0].tobytes() == x_cur.tobytes() and got.min() == 0.0 and got.max() == 1.0
    for b in range(K["B"]):
        assert _queries(x_cur[b:b + 1], K["first_image"] + b).tobytes() == got[b:b + 1].tobytes()
    assert _queries(x_cur, K["first_image"], k=K["k"] + 1)[:, 1:].tobytes() != got[:, 1:].tobytes()


def test_queries_scalar_path_on_a_misaligned_pointer():
    """P = 784 from a pointer 4 bytes off a 16-byte boundary: the scalar path, the same values."""
    import torch
    x_cur = S.kernel_inputs(784)[0]
    buf = torch.zeros(K["B"] * 784 + 1, device="cuda")
    buf[1:] = _dev(x_cur).reshape(-1)
    q = torch.empty(K["B"] * Q * 784 + 1, device="cuda")
    _native.check(_native.load().dg_spsa_queries(buf.data_ptr() + 4, K["B"], 784, K["n"], K["delta"], K["seed"], K["first_image"], K["k"],
                                                 K["lo"], K["hi"], q.data_ptr() + 4, None))
    want = S.queries(x_cur, K["n"], K["delta"], K["seed"], K["first_image"], K["k"], K["lo"], K["hi"])
    assert q[1:].cpu().numpy().tobytes() == want.tobytes()


# ---------------------------------------------------------------------- 3, 4. estimate and step
@pytest.mark.parametrize("P", [784, 25])
def test_estimate_within_the_float32_sum_bound_and_step_bit_for_bit(P):
    """Teacher-forced random logits, 10 classes, image 1's label out of range.  out_grad is within (n + 2) 2^-24 sum|dL| / (2 delta n)
    of the float64 estimate per element; where |ghat| exceeds that bound (all but at most 1 %) its sign is the reference's; the
    out-of-range image has a zero gradient; x_next is the float32 rule on the device's own out_grad, bit for bit, with the clamp
    binding (eps = 0.04 against |x_cur - x_orig| up to 0.1) and not (eps = 0.3)."""
    x_cur, x_orig, Z, y = S.kernel_inputs(P)
    B, n = K["B"], K["n"]
    dL = S.delta_losses(Z.reshape(B, Q, -1), y)
    want = S.estimate(dL, S.directions(B, P, n, K["seed"], K["first_image"], K["k"]), K["delta"])
    bound = S.estimate_bound(dL, K["delta"])
    nxt, g = _step(Z, y, x_cur, x_orig, K["first_image"], 0.04, 0.05)
    err = np.abs(g.astype(np.float64) - want)
    for b in (0, 2):
        print("P %d image %d: worst share of the estimate bound %.4f (max |err| %.3e, bound %.3e, max |ghat| %.3e)" %
              (P, b, (err[b] / bound[b]).max(), err[b].max(), bound[b], np.abs(want[b]).max()))
        assert (err[b] <= bound[b]).all()
        decided = np.abs(want[b]) > bound[b]
        assert 1 - decided.mean() <= 0.01
        assert np.array_equal(np.sign(g[b])[decided], np.sign(want[b])[decided])
    assert (g[1] == 0).all()
    assert nxt[1].tobytes() == _step32(np.zeros(P, np.float32), x_cur[1], x_orig[1], 0.04, 0.05, 0.0, 1.0).tobytes()
    assert nxt.tobytes() == _step32(g, x_cur, x_orig, 0.04, 0.05, 0.0, 1.0).tobytes()
    assert (np.abs(nxt - x_orig) >= np.float32(0.04) - 1e-6).mean() > 0.1 and np.abs(nxt - x_orig).max() <= 0.04 + 1e-6
    wide, g2 = _step(Z, y, x_cur, x_orig, K["first_image"], 0.3, 0.05)
    assert g2.tobytes() == g.tobytes() and wide.tobytes() == _step32(g, x_cur, x_orig, 0.3, 0.05, 0.0, 1.0).tobytes()
    assert _step(Z, y, x_cur, x_orig, K["first_image"], 0.3, 0.05, want_grad=False)[0].tobytes() == wide.tobytes()
    for b in range(B):                                      # each image alone, with its own first_image
        one, g1 = _step(Z[b * Q:(b + 1) * Q], y[b:b + 1], x_cur[b:b + 1], x_orig[b:b + 1], K["first_image"] + b, 0.3, 0.05)
        assert one.tobytes() == wide[b:b + 1].tobytes() and g1.tobytes() == g[b:b + 1].tobytes()


# ---------------------------------------------------------------------- 5. composition on a bare classifier
def test_generate_on_a_bare_classifier_is_the_schedule_call_by_call():
    """S.COMPOSE (exact in float32 and float64 alike): SPSA.generate equals dg_spsa_queries, dg_clf_forward, dg_eval_batch,
    dg_bpda_track and dg_spsa_step driven from here, bit for bit, for any batch_size; first_success, queries and -- the case being
    exact -- x_adv equal the float64 loop's."""
    import torch
    c = S.COMPOSE
    x, y, W, b = S.compose_inputs()
    m = nb.MLP([nb.Flatten(), nb.Linear(c["classes"])], input_shape=(None, 5, 5, 1))
    m.set_weights([(W, b)])
    kw = dict(eps=c["eps"], eps_iter=c["eps_iter"], nb_iter=c["nb_iter"], spsa_samples=c["n"], delta=c["delta"], clip_min=c["lo"],
              clip_max=c["hi"], seed=c["seed"], return_info=True)
    adv, first, queries = nb.SPSA(m).generate(x, y, **kw)
    lib, B, n, P = _native.load(), c["B"], c["n"], 25
    qn = 2 * n + 1
    t, lab = _dev(x), _dev(y)
    cur, nxt, best = torch.clamp(t, c["lo"], c["hi"]), torch.empty_like(t), torch.empty_like(t)
    fs = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    q, Z, preds = torch.empty(B * qn, 5, 5, 1, device="cuda"), torch.empty(B * qn, c["classes"], device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    for k in range(c["nb_iter"] + 1):
        if k > 0:
            _native.check(lib.dg_eval_batch(m._handle, cur.data_ptr(), None, None, B, preds.data_ptr(), None, None, None))
            _native.check(lib.dg_bpda_track(preds.data_ptr(), lab.data_ptr(), B, k, cur.data_ptr(), best.data_ptr(), fs.data_ptr(), P, None))
        if k == c["nb_iter"]:
            break
        _native.check(lib.dg_spsa_queries(cur.data_ptr(), B, P, n, c["delta"], c["seed"], 0, k, c["lo"], c["hi"], q.data_ptr(), None))
        _native.check(lib.dg_clf_forward(m._handle, q.data_ptr(), B * qn, Z.data_ptr(), None, None))
        _native.check(lib.dg_spsa_step(Z.data_ptr(), lab.data_ptr(), B, c["classes"], P, n, c["delta"], c["seed"], 0, k, cur.data_ptr(),
                                       t.data_ptr(), c["eps"], c["eps_iter"], c["lo"], c["hi"], nxt.data_ptr(), None, None))
        cur, nxt = nxt, cur
    assert adv.tobytes() == best.cpu().numpy().tobytes() and first.tolist() == fs.cpu().tolist()
    ref = S.spsa(lambda qq, what: qq.astype(np.float64) @ W.astype(np.float64) + b, x, y, c["eps"], c["eps_iter"], c["nb_iter"], n,
                 c["delta"], c["lo"], c["hi"], c["seed"])
    assert first.tolist() == ref["first_success"].tolist() and queries == ref["queries"] == c["nb_iter"] * qn + 1
    assert np.array_equal(adv.astype(np.float64), ref["x_adv"])
    for bs in (1, 4):
        a2, f2, _ = nb.SPSA(m).generate(x, y, batch_size=bs, **kw)
        assert a2.tobytes() == adv.tobytes() and f2.tobytes() == first.tobytes()
    t_adv, t_first, _ = nb.SPSA(m).generate(t, y, batch_size=4, **kw)                  # tensors in, tensors out
    assert t_adv.is_cuda and t_first.dtype == torch.int32 and t_adv.cpu().numpy().tobytes() == adv.tobytes()
    torch.cuda.synchronize()
    m.close()


# ---------------------------------------------------------------------- 6. the defended model
def test_defended_model_logits_are_the_projection_of_the_queries(monkeypatch):
    """MNIST generator with synthetic weights, L = 3, R = 2, B = 2, n = 2, nb_iter = 2.  The logits every iteration hands to the step
    equal dg_clf_forward(gan.reconstruct(queries, seed + k, first_row)) computed here in one call per iteration; the closing pass's
    projection (one engine call for both images, their latents 2 n + 1 queries apart), its logits and its predictions equal those of
    reconstruct(x_2[g], seed + 2, first_row = g (2 n + 1) R) image by image -- all bit for bit, while the driver cuts its engine calls
    every 3 queries (mid-image).  batch_size 1 and 2 give the same bits."""
    import torch
    R_, n, nb_iter, seed = 2, 2, 2, 5100
    qn = 2 * n + 1
    gan, p = make_gan("mnist", rec_rr=R_, rec_iters=3, rec_lr=10.0)
    m = nb.model_e()
    m.set_weights(init_params(m, 9))
    m.add_rec_model(gan, None, 50)
    from tests.helpers import clean_targets
    x, _ = clean_targets(p, "mnist", 2, 17)
    y = np.array([3, 8], np.int32)
    kw = dict(eps=0.3, eps_iter=0.05, nb_iter=nb_iter, spsa_samples=n, delta=0.01, clip_min=0.0, clip_max=1.0, seed=seed, return_info=True)

    class Recording(nb.SpsaDeviceOps):
        def __init__(self, model):
            super().__init__(model)
            self.steps, self.closing, self.closing_recs, self.calls = [], [], [], 0

        def project(self, q, seed_, first_row, row_step=None):
            self.calls += 1
            rec = super().project(q, seed_, first_row, row_step)
            if row_step is not None:
                self.closing_recs.append((int(seed_), int(first_row), int(row_step), rec.clone()))
            return rec

        def queries(self, x_cur, n_, delta, seed_, first_image, k, lo, hi, q):
            super().queries(x_cur, n_, delta, seed_, first_image, k, lo, hi, q)
            self.q = q[:x_cur.shape[0] * qn].clone()

        def step(self, logits, labels, n_, delta, seed_, first_image, k, x_cur, *a):
            self.steps.append((k, int(first_image), self.q, logits.clone(), x_cur.clone()))
            super().step(logits, labels, n_, delta, seed_, first_image, k, x_cur, *a)

        def track(self, preds, labels, k, x_iter, *a):
            if k == nb_iter:
                self.closing.append((x_iter.clone(), preds.clone()))
            super().track(preds, labels, k, x_iter, *a)
    monkeypatch.setattr(gan_defense, "COALESCE_ROWS", 3 * R_)
    ops = Recording(m)
    adv, first, queries = nb.SPSA(m, ops=ops).generate(x, y, batch_size=2, **kw)
    assert queries == nb_iter * qn + 1 and ops.calls == nb_iter * 4 + 1 and len(ops.steps) == nb_iter
    plain = nb.SpsaDeviceOps(m)
    for k, first_image, q, logits, x_cur in ops.steps:
        assert first_image == 0 and q[0::qn].cpu().numpy().tobytes() == x_cur.cpu().numpy().tobytes()
        want = plain.logits(gan.reconstruct(q, seed=seed + k, first_row=0))
        assert logits.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    (x_last, preds), = ops.closing
    (c_seed, c_first, c_step, c_rec), = ops.closing_recs                       # both images in one call: the row_step path
    assert (c_seed, c_first, c_step) == (seed + nb_iter, 0, qn * R_) and c_rec.shape[0] == 2
    c_logits = plain.logits(c_rec)
    for g in range(2):
        rec = gan.reconstruct(x_last[g:g + 1], seed=seed + nb_iter, first_row=g * qn * R_)
        assert c_rec[g:g + 1].cpu().numpy().tobytes() == rec.cpu().numpy().tobytes()
        assert c_logits[g:g + 1].cpu().numpy().tobytes() == plain.logits(rec).cpu().numpy().tobytes()
        assert plain.predict(rec).cpu().tolist() == preds[g:g + 1].cpu().tolist()
    # the latents matter: image 1 projected with image 0's rows is another reconstruction
    assert gan.reconstruct(x_last[1:2], seed=seed + nb_iter, first_row=0).cpu().numpy().tobytes() != c_rec[1:2].cpu().numpy().tobytes()
    assert np.abs(adv - x).max() <= 0.3 + 1e-6 and adv.min() >= 0 and adv.max() <= 1 and not np.array_equal(adv, np.clip(x, 0, 1))
    a1, f1, _ = nb.SPSA(m).generate(x, y, batch_size=1, **kw)
    assert a1.tobytes() == adv.tobytes() and f1.tobytes() == first.tobytes()
    monkeypatch.setattr(gan_defense, "COALESCE_ROWS", 12800)
    a2, f2, _ = nb.SPSA(m).generate(x, y, **kw)
    assert a2.tobytes() == adv.tobytes() and f2.tobytes() == first.tobytes()
    torch.cuda.synchronize()
    m.close()
    gan.close()


# ---------------------------------------------------------------------- 7. refusals
def test_refusals_are_errors():
    import torch
    lib = _native.load()
    # every buffer is large enough for the largest shape named below (B = 2, n = 65, 8 elements, 4 classes), refused or not
    buf, out, lab = torch.zeros(64, device="cuda"), torch.zeros(2 * 131 * 8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    Z = torch.zeros(2 * 131 * 4, device="cuda")
    p, o, z, l = buf.data_ptr(), out.data_ptr(), Z.data_ptr(), lab.data_ptr()
    qargs = dict(x=p, B=2, P=8, n=1, delta=0.01, seed=1, first=0, k=0, lo=0.0, hi=1.0, q=o)
    call_q = lambda **kw: (lambda a: lib.dg_spsa_queries(a["x"], a["B"], a["P"], a["n"], a["delta"], a["seed"], a["first"], a["k"], a["lo"], a["hi"],
                                                         a["q"], None))(dict(qargs, **kw))
    assert call_q() == 0
    for kw in (dict(x=None), dict(q=None), dict(B=0), dict(n=0), dict(P=0), dict(delta=0.0), dict(delta=-1.0), dict(k=-1), dict(first=-1),
               dict(lo=1.0, hi=0.0), dict(first=2 ** 32 - 1), dict(n=65, k=2 ** 31 - 1), dict(P=2 ** 31)):
        assert call_q(**kw) == -1, kw
        assert b"dg_spsa_queries" in lib.dg_last_error()
    assert call_q(first=2 ** 32 - 2) == 0 and call_q(k=2 ** 31 - 1) == 0            # the last image and iteration that fit
    sargs = dict(z=z, l=l, B=2, C=4, P=8, n=1, delta=0.01, seed=1, first=0, k=0, xc=p, xo=p + 64, eps=0.1, ei=0.05, lo=0.0, hi=1.0, xn=o, g=None)
    call_s = lambda **kw: (lambda a: lib.dg_spsa_step(a["z"], a["l"], a["B"], a["C"], a["P"], a["n"], a["delta"], a["seed"], a["first"], a["k"],
                                                      a["xc"], a["xo"], a["eps"], a["ei"], a["lo"], a["hi"], a["xn"], a["g"], None))(dict(sargs, **kw))
    assert call_s() == 0 and call_s(g=o + 256) == 0                                  # out_grad: a buffer of its own
    for kw in (dict(z=None), dict(l=None), dict(xc=None), dict(xo=None), dict(xn=None), dict(B=0), dict(n=0), dict(C=1), dict(delta=0.0),
               dict(eps=-0.1), dict(ei=-0.1), dict(lo=1.0, hi=0.0), dict(k=-1), dict(xn=p), dict(first=2 ** 32 - 1), dict(n=65, k=2 ** 31 - 1),
               dict(P=2 ** 31), dict(g=o), dict(g=p), dict(g=p + 64)):
        assert call_s(**kw) == -1, kw
        assert b"dg_spsa_step" in lib.dg_last_error()
    torch.cuda.synchronize()
    # the Python refusals
    gan, _ = make_gan("mnist", rec_rr=2, rec_iters=3)
    m = nb.model_e()
    m.set_weights(init_params(m, 9))
    x, y = np.zeros((1, 28, 28, 1), np.float32), np.zeros(1, np.int32)
    m.add_rec_model(gan, np.zeros((2, 128), np.float32), 50)
    with pytest.raises(ValueError, match="z_init"):
        nb.SPSA(m).generate(x, y)
    bn, _ = make_gan("mnist", rec_rr=2, rec_iters=3, use_bn=True)
    m.add_rec_model(bn, None, 50)
    with pytest.raises(NotImplementedError, match="USE_BN"):
        nb.SPSA(m).generate(x, y)
    m.close()
    gan.close()
    bn.close()
