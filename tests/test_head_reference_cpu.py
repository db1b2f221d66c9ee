"""The float64 reference of the segmentation tail (tests/head_reference.py) against torch and against the oracle, and the share of
pixels its acceptance rule leaves uncounted on the inputs the GPU test uses.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_reference as HR
from oracle import segment as OS

POTSDAM_QIDX = [0, 0, 1, 2, 3, 4, 5, 5]


@pytest.mark.parametrize("n_in,n_out", [(3, 42), (5, 48), (4, 46), (37, 518), (7, 7), (9, 4)])
def test_taps_are_torch_align_corners_false(n_in, n_out):
    x = torch.randn(1, 2, n_in, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(n_in * 100 + n_out))
    want = F.interpolate(x, size=(n_out, 3), mode="bilinear", align_corners=False)[0].numpy()
    got = np.einsum("yg,qgh->qyh", HR.taps(n_in, n_out), x[0].numpy())
    assert np.abs(got - want).max() < 1e-13


@pytest.mark.parametrize("geom", ["a", "b"])
def test_stitch_is_interpolate_plus_the_reference_add_count_loop(geom):
    c = HR.make_case(geom, 5, False)
    H, W = c["hw"]
    tl = torch.from_numpy(c["tile_logits"]).double()
    preds = torch.zeros(5, H, W, dtype=torch.float64)
    count = torch.zeros(1, H, W, dtype=torch.float64)
    for t, (y1, y2, x1, x2) in enumerate(c["windows"].tolist()):           # segmentor.py:436-447
        lg = F.interpolate(tl[t][None], size=c["up_hw"], mode="bilinear")[0]
        lg = lg[:, c["pad_tl"][0]:c["pad_tl"][0] + (y2 - y1), c["pad_tl"][1]:c["pad_tl"][1] + (x2 - x1)]
        preds[:, y1:y2, x1:x2] += lg
        count[:, y1:y2, x1:x2] += 1
    assert (count == 0).sum() == 0
    assert {1.0, 2.0, 4.0} <= set(count.unique().tolist())
    want = (preds / count).numpy()
    got = HR.stitch(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
    assert np.abs(got - want).max() < 1e-13


def test_a_band_is_a_canvas_with_shifted_windows():
    c = HR.make_case("a", 3, False)
    full = HR.stitch(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
    y0, y1 = 28, 61
    w = c["windows"].copy()
    w[:, 0:2] -= y0
    band = HR.stitch(c["tile_logits"], w, c["up_hw"], c["pad_tl"], (y1 - y0, c["hw"][1]))
    assert np.array_equal(band, full[:, y0:y1])


@pytest.mark.parametrize("name,thd,bg", [("ex_base", 0.1, 5), ("ex_pad", 0.0, 0), ("se_plain", 0.0, 0), ("ex_small", 0.0, 0)])
def test_tail_reproduces_the_oracle_labels_on_the_fixture(golden, name, thd, bg):
    g = golden("segment")
    lg = g[f"{name}.logits"][0]
    ref = HR.tail(lg, POTSDAM_QIDX, 6, 50.0, thd, bg)
    assert np.array_equal(ref["labels"], g[f"{name}.pred"][0])
    o = OS.SegOracle(None, None, torch.zeros(8, 4), torch.tensor(POTSDAM_QIDX), prob_thd=thd, bg_idx=bg)
    p, pred = o.postprocess(torch.from_numpy(lg).double())
    assert np.array_equal(ref["labels"], pred[0].numpy())
    assert np.abs(ref["probs"] - p.numpy()).max() < 1e-14


def test_tail_without_synonyms_and_with_one_class():
    rng = np.random.default_rng(3)
    lg = rng.standard_normal((4, 5, 6))
    ref = HR.tail(lg, [0, 1, 2, 3], 4, 50.0, 0.0, 0)
    p = torch.softmax(torch.from_numpy(lg) * 50.0, 0)
    assert np.array_equal(ref["labels"], p.argmax(0).numpy()) and np.abs(ref["probs"] - p.numpy()).max() < 1e-14
    one = HR.tail(lg[:1], [0], 1, 50.0, 0.3, 2)
    assert np.array_equal(one["labels"], np.zeros((5, 6), dtype=np.int64)) and np.all(one["conf"] == 1.0)
    o = OS.SegOracle(None, None, torch.zeros(4, 4), torch.tensor([1, 1, 1, 1]))       # every query in class 1 of K = 2
    ps, pred = o.postprocess(torch.from_numpy(lg))
    same = HR.tail(lg, [1, 1, 1, 1], 2, 50.0, 0.0, 0)
    assert np.array_equal(same["labels"], pred[0].numpy()) and np.abs(same["probs"] - ps.numpy()).max() < 1e-14


@pytest.mark.parametrize("Q", HR.QS)
@pytest.mark.parametrize("geom", ["a", "b"])
def test_uncounted_share_stays_under_the_cap(geom, Q):
    """The GPU test's cap, confirmed on the real reference and the real inputs before any kernel runs."""
    for merge in (False, True):
        c = HR.make_case(geom, Q, merge)
        canvas = HR.stitch(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
        for thd in (0.0, 0.3):
            ref = HR.tail(canvas, c["query_idx"], c["K"], 50.0, thd, 3)
            frac = 1.0 - HR.counted(ref, thd).mean()
            print(f"{geom} Q={Q} K={c['K']} thd={thd}: uncounted {100 * frac:.3f} %")
            assert frac <= HR.CAP
            if merge and Q > 1:
                assert not np.all(np.diff(c["query_idx"]) >= 0) or Q <= 3          # query_idx is not sorted


def test_dense_case_stays_under_the_cap_at_the_q_the_gpu_test_uses():
    """More than 64 tiles over one block: a pixel is the mean of up to 80 tiles, the logits are flat and near-ties frequent.  Q = 9 is under
    the cap; larger vocabularies are not, in the reference itself."""
    shares = {}
    for Q, merge in ((9, True), (65, False)):
        c = HR.make_case("dense", Q, merge)
        assert len(c["windows"]) == 100
        ref = HR.label_head(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"], c["query_idx"], c["K"], 50.0, 0.3, 3)
        shares[Q] = 1.0 - HR.counted(ref, 0.3).mean()
        print(f"dense Q={Q}: uncounted {100 * shares[Q]:.3f} %")
    assert shares[9] <= HR.CAP < shares[65]
