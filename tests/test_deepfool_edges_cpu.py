"""-m "not gpu": what tests/test_gpu_deepfool_edges.py rests on, shown on the CPU.  Every input set of the edge cases
(tests/support/deepfool_reference.py: TILE_CASES, MANY_STEP_CASES, MANY_RUN, SIGNED_CASE, takeback_case) has at least 75 % decidable
images, and each case has the property it was chosen for: the tiled batch reaches the second trip of every image-strided loop with
the images the case names, the signed range binds at both bounds, and the take-back image overflows float32 exactly where it should."""
import os

import numpy as np
import pytest
import torch

from tests.support import deepfool_reference as DR

DECIDABLE_CAP = 0.75
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "defensegan_amd", "csrc")
FLT_MAX = float(np.finfo(np.float32).max)


def test_the_caps_and_strides_stand_where_the_cases_were_chosen_for():
    for name, text in DR.CAP_SOURCES:
        with open(os.path.join(CSRC, name)) as fh:
            assert text in fh.read(), (name, text)
    assert (DR.IMAGE_CAP, DR.WAVE_CAP, DR.TILE_B) == (65536, 4096 * 4, 65538)
    assert DR.IMAGE_CAP % 67 == 10                                  # workgroup 0's second image is base image 10, workgroup 1's 11
    assert -(-DR.TILE_B // DR.WAVE_CAP) == 5                        # the wave-strided kernels make five trips
    assert max(nc for _, _, _, nc in DR.MANY_STEP_CASES) == 2048 and {257, 258} <= {nc for _, _, _, nc in DR.MANY_STEP_CASES}


@pytest.mark.parametrize("name", sorted(DR.TILE_CASES))
def test_tile_base_sets(name):
    c = DR.TILE_CASES[name]
    m, p, x = DR.tile_inputs(name)
    out = DR.edge_run(name, m, p, x, c)
    dec = DR.decidable(out)
    print("%s: decidable %d/%d, iters %s" % (name, dec.sum(), dec.size, out["iters"].tolist()))
    assert len(x) == 67 and np.isnan(x[0]).sum() == 1 and np.isfinite(x[1:]).all()
    assert dec.mean() >= DECIDABLE_CAP
    assert out["iters"][0] == 0 and (out["choices"][:, 0] == -1).all() and not dec[0]      # inactive from the start
    assert dec[10] and dec[11] and out["choices"][0, 10] >= 0 and out["choices"][0, 11] >= 0
    assert out["choices"][0, 1] >= 0                                # workgroup 1's first image takes a step too
    assert (out["iters"] > 1).any() and (out["iters"][1:] >= 1).all()
    assert (np.prod(c["shape"]) % 4 == 0) == (name == "tile4x4")    # one case per vector width
    o32 = DR.run(m, p, x, c["nc"], 0.02, c["max_iter"], 0.0, 1.0, dtype=torch.float32)
    assert (o32["choices"][:, dec] == out["choices"][:, dec]).all() and (o32["final_class"][dec] == out["final_class"][dec]).all()


def test_many_candidate_sets_are_decidable():
    for name, shape, B, nc in DR.MANY_STEP_CASES:
        m, p, x = DR.case_inputs(dict(model=name, shape=shape, B=B, **DR.MANY_SEEDS[name]))
        out = DR.run(m, p, x, nc, 0.0, 1, 0.0, 1.0, shadow=torch.float32)
        assert DR.decidable(out).mean() >= DECIDABLE_CAP, (name, nc)
        assert (out["choices"][0] >= 0).all()
        # with B = 2 or 3 one image less is under the cap, and the float32 error that sets the bar differs from CPU to CPU: the
        # seeds were searched for twice the margin, and every image has it
        room = DR.margin_room(out)
        print("%s nc %d: margins at %s times what decidable asks" % (name, nc, room.round(2).tolist()))
        assert (room >= 2.0).all(), (name, nc, room)
    c = DR.MANY_RUN
    m, p, x = DR.case_inputs(c)
    out = DR.edge_run("many_run", m, p, x, c)
    assert DR.decidable(out).mean() >= DECIDABLE_CAP and (out["iters"] >= 1).all()
    assert (DR.margin_room(out) >= 2.0).all()
    assert c["nc"] >= 258 and m.param_shapes()[-1][0][1] == 300


def test_signed_range_binds_at_both_bounds():
    c = DR.SIGNED_CASE
    m, p, x = DR.case_inputs(c)
    out = DR.edge_run("signed", m, p, x, c)
    dec = DR.decidable(out)
    assert dec.mean() >= DECIDABLE_CAP
    assert x.min() == -1.0 and x.max() == 1.0 and (x[::3] == -1).any() and (x[::3] == 1).any() and (x < -0.5).mean() > 0.15
    free = x.astype(np.float64) + 1.02 * out["r_tot"]               # before the clip
    stepped = out["choices"][0] >= 0
    both = stepped & (free.reshape(len(x), -1) < -1.0).any(axis=1) & (free.reshape(len(x), -1) > 1.0).any(axis=1)
    print("signed: decidable %d/%d, %d images clipped at both bounds" % (dec.sum(), dec.size, both.sum()))
    assert (both & dec).any()
    assert out["x_adv"].min() == -1.0 and out["x_adv"].max() == 1.0


def _forward32(params, x):
    """The three Linear layers in float32 torch: (h2, logits)."""
    h = torch.as_tensor(np.asarray(x, np.float32).reshape(len(x), -1))
    hs = []
    for W, b in params:
        h = h @ torch.as_tensor(W) + torch.as_tensor(b)
        hs.append(h)
    return hs[1].numpy(), hs[2].numpy()


def test_takeback_image_overflows_float32_on_its_first_step_and_not_before():
    m, p, x = DR.takeback_case()
    ref = DR.run(m, p, x, 3, 0.02, 5, 0.0, 1.0)                     # float64: nothing overflows there
    assert ref["choices"][0].tolist()[1] == 1 and ref["orig"].tolist() == [0, 0, 0]
    net = DR.logits_fn(m, p)
    st = DR.start(net, torch.tensor(x, dtype=torch.float64), 3)
    new, info = DR.step(net, st, 0.0, 1.0)
    adv = new["adv"].numpy()
    assert np.array_equal(adv[1], x[1].astype(np.float64) + new["r_tot"].numpy()[1])       # the clip does not bind on that step
    h2_x, z_x = _forward32(p, x)
    h2_a, z_a = _forward32(p, adv)
    assert np.isfinite(z_x).all() and np.isfinite(h2_x).all() and np.abs(h2_x).max() < 0.95 * FLT_MAX
    assert 1e6 <= np.abs(z_x).max() <= 1e7                          # logits of order 1e6: the way back stays in normal numbers
    assert np.isnan(z_a[1]).any() and np.isinf(h2_a[1][:2]).all()
    with torch.no_grad():                                           # in float64 the same point lies 1.2 x past the float32 range
        h64 = (torch.tensor(adv.reshape(3, -1)) @ torch.tensor(p[0][0], dtype=torch.float64)) @ torch.tensor(p[1][0], dtype=torch.float64)
    assert (h64[1, :2].numpy() > 1.2 * FLT_MAX).all()
    assert np.isfinite(z_a[[0, 2]]).all() and np.abs(h2_a[[0, 2]]).max() < 0.95 * FLT_MAX  # the neighbours stay finite
    # the smallest partial product of the way back: the seed 1 through W3, then W2
    w3 = np.abs(p[2][0][:2]).min()
    assert w3 > 1e-36 and w3 * DR.TAKEBACK_S > 1e-36
    # the restatement in float32 applies the NaN rule as the device must
    o32 = DR.run(m, p, x, 3, 0.02, 5, 0.0, 1.0, dtype=torch.float32)
    assert o32["iters"][1] == 1 and o32["choices"][:, 1].tolist() == [1, -1, -1, -1, -1] and o32["final_class"][1] == 0
    assert np.array_equal(o32["x_adv"][1], x[1]) and o32["r_norm"][1] == 0.0
