"""-m "not gpu": the SPSA definition as restated in tests/support/spsa_reference.py -- direction keying, queries, margin, estimate,
the non-finite rule -- and the host side of network_builder.SPSA: argument checks and the driver loop run on CPU tensors over a
recording stand-in (which queries, projections, seeds and rows it asks for, in which order, and what it tracks); the whitebox
driver's plumbing; and what the GPU cases' inputs promise.  The device kernels are tests/test_gpu_spsa.py's."""
import numpy as np
import pytest

from defensegan_amd import gan_defense, network_builder as nb, whitebox as wb
from tests.support import spsa_reference as S
from tests.support.bpda_reference import philox4x32_10


# ---------------------------------------------------------------------- by hand: one image, P = 4, n = 1
def test_hand_written_case():
    """seed 1, image 0, iteration 0: the counter (0, 0, 0, "SPSA") under the key (1, 0) gives the words 0x272cb2c6, 0x130d0967,
    0x384c9b4c, 0x954128e1, whose lowest bits are 0, 1, 0, 1: u_0 = (-1, +1, -1, +1).  Two classes, Z = (0, w.q), y = 0, so
    L = w.q with w = (1, 2, 3, 4)."""
    words = philox4x32_10(np.array([[0, 0, 0, 0x53505341]], np.uint64), (1, 0))[0]
    assert [hex(int(v)) for v in words] == ["0x272cb2c6", "0x130d0967", "0x384c9b4c", "0x954128e1"]
    assert S.direction_bits(1, 4, 1, seed=1).tolist() == [[[False, True, False, True]]]
    u = S.directions(1, 4, 1, seed=1)
    assert u.tolist() == [[[-1.0, 1.0, -1.0, 1.0]]]
    x_k = np.array([[0.5, 0.995, 0.0, 0.25]], np.float32)
    q = S.queries(x_k, 1, 0.01, 1, 0, 0, 0.0, 1.0)
    f = np.float32
    assert q.dtype == np.float32 and q.shape == (1, 3, 4)
    assert q[0, 0].tolist() == x_k[0].tolist()                                   # query 0 is the iterate itself
    #                           -delta             +delta, clipped at 1   -delta, clipped at 0   +delta
    assert q[0, 1].tolist() == [f(0.5) - f(0.01), 1.0, 0.0, f(0.25) + f(0.01)]
    assert q[0, 2].tolist() == [f(0.5) + f(0.01), f(0.995) - f(0.01), f(0.01), f(0.25) - f(0.01)]
    w = np.array([1.0, 2.0, 3.0, 4.0])
    Z = np.stack([np.zeros(3), q[0].astype(np.float64) @ w], axis=1)[None]       # [1, 3, 2]
    L = S.margins(Z, [0])
    np.testing.assert_allclose(L[0], [0.5 + 1.99 + 0 + 1.0, 0.49 + 2.0 + 0 + 1.04, 0.51 + 1.97 + 0.03 + 0.96], rtol=0, atol=1e-6)
    dL = S.delta_losses(Z, [0])
    np.testing.assert_allclose(dL, [[0.06]], rtol=0, atol=1e-6)
    g = S.estimate(dL, u, 0.01)                                                   # 0.06 / (2 * 0.01 * 1) * u: u, not the clipped difference
    np.testing.assert_allclose(g, [[-3.0, 3.0, -3.0, 3.0]], rtol=0, atol=1e-4)
    nxt = S.step_rule(x_k.astype(np.float64), x_k.astype(np.float64), g, 0.1, 0.05, 0.0, 1.0)
    np.testing.assert_allclose(nxt, [[0.45, 1.0, 0.0, 0.30]], rtol=0, atol=1e-6)
    # the margin takes the best OTHER class, and an out-of-range label gives 0
    Z3 = np.array([[[1.0, 5.0, 2.0], [4.0, 0.0, 3.0]]])
    assert S.margins(Z3, [1]).tolist() == [[-3.0, 4.0]] and S.margins(Z3, [0]).tolist() == [[4.0, -1.0]]
    assert S.margins(Z3, [3]).tolist() == [[0.0, 0.0]] and S.margins(Z3, [-1]).tolist() == [[0.0, 0.0]]


def test_linear_loss_identity():
    """L(q) = w.q inside the clip interior: L(q+) - L(q-) = 2 delta w.u_i, so ghat = (1 / n) sum_i (w.u_i) u_i."""
    rs = np.random.RandomState(2)
    B, P, n, delta = 2, 25, 7, 1.0 / 64
    x = (rs.randint(16, 48, (B, P)) / 64.0).astype(np.float32)                    # the 1/64 grid: every query is exact
    w = rs.randint(-8, 9, P) / 8.0
    q = S.queries(x, n, delta, 11, 3, 1, 0.0, 1.0)
    Z = np.stack([np.zeros((B, 2 * n + 1)), q.astype(np.float64) @ w], axis=2)
    u = S.directions(B, P, n, 11, 3, 1)
    got = S.estimate(S.delta_losses(Z, np.zeros(B, int)), u, delta)
    want = np.einsum("bi,bip->bp", u @ w, u) / n
    assert np.array_equal(got, want)                                              # dyadic values: exact


def test_keying():
    n, P, seed = 40, 25, (5 << 32) | 17
    all_ = S.direction_bits(4, P, n, seed, first_image=10, k=3)
    assert all_.shape == (4, n, P) and 0.4 < all_.mean() < 0.6
    # an image's directions depend on its global index, not on B or its position in the batch
    for r in range(4):
        assert np.array_equal(S.direction_bits(1, P, n, seed, first_image=10 + r, k=3)[0], all_[r])
    assert np.array_equal(S.direction_bits(2, P, n, seed, first_image=11, k=3), all_[1:3])
    assert not np.array_equal(all_[0], all_[1])
    # directions 31 and 32 come from different blocks: counter word 2 is k G + (i >> 5), bits 31 and 0
    G = 2
    for i, blk, bit in ((31, 3 * G, 31), (32, 3 * G + 1, 0), (39, 3 * G + 1, 7)):
        ctr = np.array([[e >> 2, 12, blk, S.SPSA_TAG] for e in range(P)], np.uint64)
        words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
        want = [bool((int(words[e, e & 3]) >> bit) & 1) for e in range(P)]
        assert all_[2, i].tolist() == want
    # iterations differ, and iteration k + 1's first group is not iteration k's second one shifted: k G + group is unique per (k, group)
    assert not np.array_equal(S.direction_bits(1, P, n, seed, 10, k=4)[0], all_[0])
    assert np.array_equal(S.direction_bits(1, P, 64, seed, 10, k=1)[0, :32], S.direction_bits(1, P, 32, seed, 10, k=2)[0])
    with pytest.raises(ValueError, match="wrap"):
        S.direction_bits(1, 4, 1, 0, first_image=2 ** 32)
    with pytest.raises(ValueError, match="wrap"):
        S.direction_bits(1, 4, 33, 0, k=2 ** 31)


def test_non_finite_loss_rule():
    """A NaN logit makes its query's L NaN; a pair whose dL is not finite as a float32 contributes 0, the divisor stays n."""
    big = np.float32(3e38)
    Z = np.zeros((1, 9, 2), np.float32)                       # n = 4, y = 0, L = Z_1 - Z_0
    Z[0, 1:, 1] = [3.0, 1.0, np.nan, 0.0, np.inf, 0.0, big, -big]
    assert np.isnan(S.margins(Z, [0])[0, 3])
    dL = S.delta_losses(Z, [0])
    assert dL.tolist() == [[2.0, 0.0, 0.0, 0.0]]              # NaN, +inf, and 6e38 (finite in float64, not in float32) are dropped
    Z[0, 5:7, 1] = [np.inf, np.inf]                           # inf - inf
    assert S.delta_losses(Z, [0])[0, 2] == 0.0
    Znan = np.zeros((1, 3, 3), np.float32)
    Znan[0, 1] = [0.0, np.nan, 5.0]                           # the NaN is not the label's nor the largest: the maximum still propagates it
    assert np.isnan(S.margins(Znan, [0])[0, 1]) and S.delta_losses(Znan, [0]).tolist() == [[0.0]]
    u = np.ones((1, 4, 3))
    assert S.estimate(dL, u, 0.25).tolist() == [[1.0, 1.0, 1.0]]          # 2 / (2 * 0.25 * 4)


# ---------------------------------------------------------------------- the host class
def _defended(R_=2, batch_size=50, use_bn=False, shape=(None, 28, 28, 1)):
    from defensegan_amd.gan import MnistDefenseGAN
    gan = MnistDefenseGAN(cfg={"USE_BN": use_bn, "LATENT_DIM": 128, "NET_DIM": 64}, test_mode=True, rec_rr=R_, rec_iters=5, rec_lr=10.0)
    m = nb.model_e(input_shape=shape)
    m.add_rec_model(gan, None, batch_size)
    return m


class _StandIn(object):
    """The six operations of SpsaDeviceOps on CPU tensors: queries and step by the restatement, an identity 'projection', a linear
    classifier with dyadic weights -- and a log of every call."""

    def __init__(self, W):
        import torch
        self.device, self.W, self.log, self.cur, self.saw_query0 = torch.device("cpu"), W, [], None, []

    def queries(self, x_cur, n, delta, seed, first_image, k, lo, hi, q):
        import torch
        self.log.append(("queries", int(first_image), int(k), int(x_cur.shape[0]), int(n)))
        self.cur = x_cur.clone()
        q.copy_(torch.from_numpy(S.queries(x_cur.numpy(), n, delta, seed, first_image, k, lo, hi)).view_as(q))

    def project(self, q, seed, first_row, row_step=None):
        self.log.append(("project", seed, int(first_row), int(q.shape[0]), row_step))
        return q.clone()

    def logits(self, rec):
        import torch
        self.log.append(("logits", int(rec.shape[0])))
        return torch.from_numpy((rec.numpy().reshape(len(rec), -1).astype(np.float64) @ self.W).astype(np.float32))

    def predict(self, rec):
        import torch
        self.log.append(("predict", int(rec.shape[0])))
        self.saw_query0.append(bool(torch.equal(rec, self.cur)))                  # query 0: the chunk's iterate itself
        return self.logits(rec).argmax(dim=1).to(torch.int32)

    def step(self, logits, labels, n, delta, seed, first_image, k, x_cur, x_orig, eps, eps_iter, lo, hi, x_next, out_grad=None):
        import torch
        B = int(x_cur.shape[0])
        self.log.append(("step", int(first_image), int(k), B, int(logits.shape[0])))
        P = x_cur[0].numel()
        Z = logits.numpy().astype(np.float64).reshape(B, 2 * n + 1, -1)
        g = S.estimate(S.delta_losses(Z, labels.numpy()), S.directions(B, P, n, seed, first_image, k), delta)
        nxt = S.step_rule(x_orig.numpy().reshape(B, P).astype(np.float64), x_cur.numpy().reshape(B, P).astype(np.float64), g, eps, eps_iter, lo, hi)
        x_next.copy_(torch.from_numpy(nxt.astype(np.float32)).view_as(x_next))

    def track(self, preds, labels, k, x_iter, x_best, first_success):
        self.log.append(("track", int(k), int(preds.shape[0])))
        open_ = first_success < 0
        x_best[open_] = x_iter[open_]
        first_success[open_ & (preds != labels)] = k


@pytest.mark.parametrize("batch_size,coalesce_rows", [(None, 12800), (2, 6), (3, 2)])
def test_driver_loop_over_a_recording_stand_in(batch_size, coalesce_rows, monkeypatch):
    """network_builder.SPSA.generate on CPU tensors: per iteration and image chunk one ``queries``, the flat query range cut into
    ``project`` calls (latent seed + k, first_row = global query x rec_rr) each followed by ``logits``, from k = 1 on one ``predict``
    on the chunk's query-0 rows and ``track``, then ``step``; at the end one closing ``project`` per cut with seed + nb_iter, the
    images 2 n + 1 queries apart.  The result equals the restatement's, whatever the chunks and cuts."""
    monkeypatch.setattr(gan_defense, "COALESCE_ROWS", coalesce_rows)
    n_img, ns, nb_iter, R_, seed, Q = 5, 2, 3, 2, (1 << 33) + 900, 5
    rs = np.random.RandomState(4)
    x = (rs.randint(8, 57, (n_img, 28, 28, 1)) / 64.0).astype(np.float32)
    W = rs.randint(-8, 9, (784, 3)) / 64.0
    y = (x.reshape(n_img, -1).astype(np.float64) @ W).argmax(axis=1).astype(np.int32)
    kw = dict(eps=0.125, eps_iter=0.0625, nb_iter=nb_iter, spsa_samples=ns, delta=1.0 / 64, clip_min=0.0, clip_max=1.0, seed=seed)
    ops = _StandIn(W)
    adv, first, queries = nb.SPSA(_defended(R_), ops=ops).generate(x, y, batch_size=batch_size, return_info=True, **kw)

    bs = n_img if batch_size is None else batch_size
    per_call = max(1, coalesce_rows // R_)                      # queries (or closing images) per engine call
    want = []
    for k in range(nb_iter):
        for a in range(0, n_img, bs):
            b = min(n_img, a + bs)
            nq = (b - a) * Q
            want.append(("queries", a, k, b - a, ns))
            for c0 in range(0, nq, per_call):
                c1 = min(nq, c0 + per_call)
                want += [("project", seed + k, (a * Q + c0) * R_, c1 - c0, None), ("logits", c1 - c0)]
            if k > 0:
                want += [("predict", b - a), ("logits", b - a), ("track", k, b - a)]
            want.append(("step", a, k, b - a, nq))
    for a in range(0, n_img, bs):
        b = min(n_img, a + bs)
        for c0 in range(0, b - a, per_call):
            c1 = min(b - a, c0 + per_call)
            want += [("project", seed + nb_iter, (a + c0) * Q * R_, c1 - c0, Q * R_), ("predict", c1 - c0), ("logits", c1 - c0)]
        want.append(("track", nb_iter, b - a))
    assert ops.log == want
    n_chunks = len(range(0, n_img, bs))
    assert ops.saw_query0[:(nb_iter - 1) * n_chunks] == [True] * ((nb_iter - 1) * n_chunks)      # tracking reads query 0
    assert queries == nb_iter * Q + 1 == 16

    ref = S.spsa(lambda q, what: q.astype(np.float64) @ W, x, y, 0.125, 0.0625, nb_iter, ns, 1.0 / 64, 0.0, 1.0, seed)
    assert first.dtype == np.int32 and first.tolist() == ref["first_success"].tolist()
    assert adv.dtype == np.float32 and np.array_equal(adv.astype(np.float64), ref["x_adv"])
    assert np.abs(adv - x).max() <= 0.125 and adv.min() >= 0 and adv.max() <= 1
    assert (ref["first_success"] > 0).any() and (ref["first_success"] < 0).any()


def test_bare_model_uses_no_latent_seeds():
    rs = np.random.RandomState(5)
    x = (rs.randint(8, 57, (3, 5, 5, 1)) / 64.0).astype(np.float32)
    W = rs.randint(-8, 9, (25, 3)) / 8.0
    ops = _StandIn(W)
    m = nb.MLP([nb.Flatten(), nb.Linear(3)], input_shape=(None, 5, 5, 1))
    nb.SPSA(m, ops=ops).generate(x, np.zeros(3, np.int32), nb_iter=2, spsa_samples=2, delta=1.0 / 64, clip_min=0.0, clip_max=1.0, batch_size=2)
    proj = [e for e in ops.log if e[0] == "project"]
    assert len(proj) == 2 * 2 + 2 and all(e[1] is None for e in proj)           # per iteration and chunk one, plus the closing ones
    assert [e[3] for e in proj] == [10, 5, 10, 5, 2, 1]


def test_argument_errors():
    x, y = np.zeros((2, 28, 28, 1), np.float32), np.zeros(2, np.int32)
    m = _defended()
    ops = _StandIn(np.zeros((784, 3)))
    for kw, match in ((dict(nb_iter=0), "nb_iter"), (dict(spsa_samples=0), "spsa_samples"), (dict(delta=0.0), "delta"),
                      (dict(eps=-0.1), "eps"), (dict(eps_iter=-1.0), "eps"), (dict(clip_min=1.0, clip_max=0.0), "clip_min"),
                      (dict(batch_size=0), "batch_size")):
        with pytest.raises(ValueError, match=match):
            nb.SPSA(m, ops=ops).generate(x, y, **kw)
    with pytest.raises(ValueError, match="x must be"):
        nb.SPSA(m, ops=ops).generate(np.zeros((2, 5, 5, 1), np.float32), y)
    with pytest.raises(ValueError, match="y must be"):
        nb.SPSA(m, ops=ops).generate(x, np.zeros(3, np.int32))
    assert ops.log == []
    with pytest.raises(NotImplementedError, match="USE_BN"):
        nb.SPSA(_defended(use_bn=True), ops=ops).generate(x, y)
    m.rec_layer.z_init = np.zeros((4, 128), np.float32)
    with pytest.raises(ValueError, match="z_init"):
        nb.SPSA(m, ops=ops).generate(x, y)


# ---------------------------------------------------------------------- the whitebox driver
def test_whitebox_driver_plumbing(monkeypatch):
    log = []

    class Attack(object):
        def __init__(self, model):
            log.append(("build", model.rec_layer is not None))

        def generate(self, x, y, **kw):
            log.append(("generate", len(x), kw))
            return np.asarray(x)

    class Model(object):
        _device, _weights_set, rec_layer = 0, True, None

        def _ensure(self):
            pass

        def add_rec_model(self, gan, z_init, batch_size):
            self.rec_layer = (gan, z_init)

    class Gan(object):
        dataset_name, arch_name, rec_rr, latent_dim = "mnist", "mnist", 5, 8

        def reconstruct(self, *a, **k):
            raise AssertionError("the stubbed evaluation never projects")
    monkeypatch.setattr(wb.utils_tf, "model_train", lambda *a, **kw: None)
    monkeypatch.setattr(wb, "_accuracy", lambda *a: 0.75)
    monkeypatch.setattr(wb.gan_defense, "model_eval_gan", lambda rec, model, X, Y, bs, **kw: (2, len(X), ["l", "p", "d"]))
    monkeypatch.setattr(wb.network_builder, "SPSA", Attack)
    data = (np.full((8, 2, 2, 1), 0.5, np.float32), np.arange(8) % 3, np.full((4, 2, 2, 1), 0.5, np.float32), np.arange(4) % 3)
    for defense, gan in (("none", None), ("adv_tr", None), ("defense_gan", Gan())):
        del log[:]
        out = wb.whitebox(gan, Model(), data, batch_size=4, nb_epochs=1, attack_type="spsa", defense_type=defense,
                          attack_params={"spsa_samples": 8, "nb_iter": 3})
        assert out[0] == 0.5 and (out[2] is not None) == (defense == "defense_gan")
        assert log[0] == ("build", defense == "defense_gan")
        assert log[1] == ("generate", 4, dict(eps=0.3, eps_iter=0.05, nb_iter=3, spsa_samples=8, delta=0.01, clip_min=0.0, clip_max=1.0,
                                              seed=wb.SEED, batch_size=4))
    assert wb.attack_kind("spsa") == ("spsa", False) and "spsa" in wb.ATTACKS
    with pytest.raises(ValueError, match="^unknown attack_type"):
        wb.attack_kind("rand_spsa")
    with pytest.raises(ValueError, match="same_init"):
        wb.whitebox(Gan(), Model(), data, attack_type="spsa", defense_type="defense_gan", same_init=True)
    with pytest.raises(ValueError, match="attack_ord"):
        wb.whitebox(None, Model(), data, attack_type="spsa", attack_ord=2)
    assert wb.SPSA_DEFAULTS == {"spsa_samples": 32, "spsa_delta": 0.01}
    assert wb._attack_params("spsa", None) == {"eps_iter": 0.05, "nb_iter": 10, "spsa_samples": 32, "spsa_delta": 0.01}
    assert wb._attack_params("pgd", {"spsa_samples": 4}) == {"eps_iter": 0.05, "nb_iter": 10}
    a = wb.build_parser().parse_args(["--data_dir", "d", "--attack_type", "spsa", "--spsa_samples", "16", "--spsa_delta", "0.02"])
    assert (a.spsa_samples, a.spsa_delta) == (16, 0.02)
    b = wb.build_parser().parse_args(["--data_dir", "d"])
    assert (b.spsa_samples, b.spsa_delta) == (None, None)
    a.dataset_name, a.fgsm_eps_tr = "mnist", 0.15
    assert wb.get_results_dir_filename(a, None)[1] == "model=F_nodefense_attack=spsa.txt"          # bpda's naming rule


# ---------------------------------------------------------------------- what the GPU cases' inputs promise
@pytest.mark.parametrize("P", [784, 25])
def test_gpu_estimate_case_leaves_few_signs_undecided_on_the_reference_alone(P):
    """tests/test_gpu_spsa.py compares sign(ghat) and x_next with the float64 values only where |ghat| exceeds the float32 error
    bound, and may skip at most 1 % of the elements of a labelled image: the draw (S.kernel_inputs) is chosen so that the reference
    alone satisfies this.  It also promises live clips, both of the queries and of the step."""
    c = S.KERNEL
    x_cur, x_orig, Z, y = S.kernel_inputs(P)
    B, n = c["B"], c["n"]
    assert x_cur.shape == (B, P) and Z.shape == (B * (2 * n + 1), c["classes"]) and Z.dtype == np.float32
    assert (x_cur == 0.0).any() and (x_cur == 1.0).any() and ((x_cur > 0) & (x_cur < 1)).any()
    assert y[1] == c["classes"] and 0 <= y[0] < c["classes"] and 0 <= y[2] < c["classes"]
    dL = S.delta_losses(Z.reshape(B, 2 * n + 1, -1), y)
    assert (dL[1] == 0).all() and np.abs(dL[0]).min() > 0
    g = S.estimate(dL, S.directions(B, P, n, c["seed"], c["first_image"], c["k"]), c["delta"])
    bound = S.estimate_bound(dL, c["delta"])
    assert (g[1] == 0).all() and bound[1] == 0
    for b in (0, 2):
        undecided = float((np.abs(g[b]) <= bound[b]).mean())
        assert undecided <= 0.01, undecided
        assert bound[b] < 1e-3 * np.abs(g[b]).max()
    q = S.queries(x_cur, n, c["delta"], c["seed"], c["first_image"], c["k"], c["lo"], c["hi"])
    raw = x_cur[:, None, :] + np.where(S.direction_bits(B, P, n, c["seed"], c["first_image"], c["k"]), 1, -1) * np.float32(c["delta"])
    assert (raw > 1).any() and (raw < 0).any() and q.min() == 0.0 and q.max() == 1.0


def test_gpu_composition_case_is_exact_and_away_from_ties():
    """S.COMPOSE: every logit is a dyadic rational that float32 holds exactly (so the device's float32 loop and the float64 loop
    compute the same numbers), no judged iterate has a zero margin, and the outcome has successes at several iterates and failures."""
    c = S.COMPOSE
    x, y, W, b = S.compose_inputs()
    seen = []

    def logits_of(q, what):
        z = q.astype(np.float64) @ W.astype(np.float64) + b
        assert np.array_equal(z, z.astype(np.float32)) and np.array_equal(q * 64, np.round(q * 64))
        seen.append(what)
        return z
    out = S.spsa(logits_of, x, y, c["eps"], c["eps_iter"], c["nb_iter"], c["n"], c["delta"], c["lo"], c["hi"], c["seed"])
    assert seen == [0, 1, 2, 3, "closing"]
    assert 1.0 / (2 * c["delta"] * c["n"]) == 8.0
    for j in range(1, c["nb_iter"] + 1):
        assert np.abs(out["margin0"][j]).min() >= 2.0 ** -10, (j, out["margin0"][j])
        assert ((out["margin0"][j] > 0) == (out["preds"][j] != y)).all()
    assert out["first_success"].tolist() == [-1, 3, -1, 1, -1, -1] and out["queries"] == 37
    for g in out["grads"]:
        assert np.array_equal(g * 64, np.round(g * 64))
    assert any((g == 0).any() for g in out["grads"])                              # sign(0) = 0 is exercised
