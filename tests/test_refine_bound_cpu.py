"""The refiner / fusion / CTD bounds of tests/refine_reference.py on the CPU (no GPU needed): on every case generator the GPU modules use,
an f32 emulation of each op -- the oracle run in f32, and for the refiners also a 64-lane strided summation order -- stays inside its
bound, and each listed mutation of the arithmetic or of the write order -- the kind of slip a kernel makes -- fails on a named case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_reference as R                                            # noqa: E402
from refine_reference import check_within                               # noqa: E402
from rowops_reference import lane_sum                                   # noqa: E402  (the kernels' 64-lane strided sum + butterfly)
from oracle import refine as OR, ctd as OC                              # noqa: E402

TEMPS = (0.1, 5.0)


# ---- refiners --------------------------------------------------------------------------------------------------------------------
def emulate_refine(feats, idx, gh, gw, temp, decontaminate, dtype=torch.float32, lane=True, mut=None):
    """refine_compute_kernel + refine_scatter_kernel in `dtype`, with the mutations of the module docstring."""
    B, n, D = feats.shape
    src = feats.to(dtype)
    out = src.clone()
    summ = lane_sum if lane else (lambda v: v.sum(-1))
    for b in range(B):
        ib = idx[b].long()
        if mut == "swap_hw":                                             # gh for gw in the cell arithmetic
            rows, cols = ib // gh, ib % gh
            ny = (rows[:, None] + R.NEIGHBOURS[None, :, 0]).clamp(0, gh - 1)
            nx = (cols[:, None] + R.NEIGHBOURS[None, :, 1]).clamp(0, gw - 1)
            tgt = (ny * gh + nx).clamp(max=n - 1)
        else:
            _, _, tgt = R.neighbour_cells(ib, gh, gw)
        c, nb = src[b, ib], src[b, tgt]
        dot, nn, cc = summ(nb * c[:, None]), summ(nb * nb), summ(c * c)[:, None]
        cos = dot / (nn.sqrt().clamp_min(1e-12) * cc.sqrt().clamp_min(1e-12))
        w = torch.softmax((1.0 - cos).clamp(min=0.0), 1)
        rep = torch.zeros_like(c)
        for j in range(8):
            rep = rep + nb[:, j] * w[:, j:j + 1]
        sigma = cos * torch.tensor(temp, dtype=dtype)
        if mut != "no_sigma_clamp":
            sigma = sigma.clamp(0, 1)
        cleaned = nb - c[:, None] * sigma[:, :, None]
        cells, t = ib.tolist(), tgt.tolist()
        if mut == "nbr_over_outlier":                                    # replacements first: neighbour writes land on outlier cells
            out[b, ib] = rep
        written = set()
        if decontaminate:
            for i, cell in enumerate(cells):
                for j in range(8):
                    if t[i][j] == cell or (mut == "first_wins" and t[i][j] in written):
                        continue
                    out[b, t[i][j]] = (out[b, t[i][j]] - c[i] * sigma[i, j]) if mut == "from_modified" else cleaned[i, j]
                    written.add(t[i][j])
        if mut != "nbr_over_outlier":
            out[b, ib] = rep
    return out


_REFINE = {}


def refine_case(ci, weak, temp):
    """(case, reference) of REFINE_CASES[ci] -- or the tie case for ci = -1 --, computed once."""
    key = (ci, weak, temp)
    if key not in _REFINE:
        if ci < 0:
            case = R.make_tie_case(weak, seed=7)
            shape = case["shape"]
        else:
            shape = R.REFINE_CASES[ci]
            case = R.make_refine_case(*shape, weak, seed=ci)
        ref = R.neighbour_refine_reference(case["feats"], case["idx"], shape[1], shape[2], R.f32(temp), not weak)
        _REFINE[key] = (shape, case, ref)
    return _REFINE[key]


def refine_ok(got, case, ref):
    written = ref["kind"] > 0
    if not torch.equal(got[~written], case["feats"][~written]):
        return False
    try:
        check_within(got[written], ref["out"][written], ref["bound"][written])
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("weak", [False, True])
@pytest.mark.parametrize("ci", [-1] + list(range(len(R.REFINE_CASES))))
def test_refiner_f32_emulations_stay_inside_the_bound(ci, weak):
    for temp in (TEMPS if not weak else TEMPS[:1]):
        (B, gh, gw, D, k), case, ref = refine_case(ci, weak, temp)
        untouched = int((ref["kind"] == R.UNTOUCHED).sum())
        assert untouched >= 1 or (gh, gw) == R.CONTESTED_GRID
        grid = case["feats"].permute(0, 2, 1).reshape(B, D, gh, gw)
        orc = OR.suppress_outliers(grid, case["idx"], R.f32(temp)) if not weak else OR.replace_weak_tokens(grid, case["idx"])
        assert orc.dtype == torch.float32
        got = {"oracle f32": orc.reshape(B, D, gh * gw).permute(0, 2, 1),
               "lane-strided f32": emulate_refine(case["feats"], case["idx"], gh, gw, R.f32(temp), not weak),
               "plain f32": emulate_refine(case["feats"], case["idx"], gh, gw, R.f32(temp), not weak, lane=False)}
        written = ref["kind"] > 0
        for name, g in got.items():
            assert torch.equal(g[~written], case["feats"][~written]), name
            worst = check_within(g[written], ref["out"][written], ref["bound"][written], f"{name} {(B, gh, gw, D, k)} temp {temp}")
            assert worst <= 1.0
        exact = emulate_refine(case["feats"], case["idx"], gh, gw, R.f32(temp), not weak, dtype=torch.float64, lane=False)
        assert bool(((exact - ref["out"]).abs() <= 1e-6 * ref["bound"]).all())      # the emulation is the reference's arithmetic


def test_selection_reference_and_rank_gap():
    s = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, 0.5]], dtype=torch.float64)
    assert R.selection_reference(s, 4).tolist() == [[1, 2, 4, 3]]              # exact ties: lowest index first
    assert R.rank_gap(s, 3) == pytest.approx(1.0 / 3.0)                       # 3 -> 2 among the first four, the ties ignored
    assert R.rank_gap(s, 4) == pytest.approx(1.0 / 3.0) and R.rank_gap(s, 5) == pytest.approx(1.0 / 3.0)
    for weak in (False, True):
        case = R.make_tie_case(weak, seed=7)
        k = case["shape"][4]
        assert case["idx"][0, k - 2:].tolist() == case["tied"][:2]
        f32_scores = (-case["a_diag"][:, 1:]) if weak else case["a_cls"][:, 1:] / (case["a_diag"][:, 1:] + 1e-8)
        assert torch.equal(R.selection_reference(f32_scores.double(), k), case["idx"])   # the f32 scores keep the order at this gap


# (mutation, weak, the REFINE_CASES index it must fail on, why there)
REFINE_MUTATIONS = [
    ("swap_hw", False, 0), ("swap_hw", True, 1),            # non-square grids: 5 x 9 and 9 x 5
    ("first_wins", False, 1),                               # 40 outliers on 9 x 5: most neighbour cells are targeted more than once
    ("nbr_over_outlier", False, 2),                         # 300 outliers on 20 x 20: most outliers neighbour an outlier
    ("from_modified", False, 2),                            # ... and most neighbour cells were written before their last writer
    ("no_sigma_clamp", False, 0),                           # temp 5: sigma beyond 1; temp 0.1: negative cosines below 0
]


@pytest.mark.parametrize("mut,weak,ci", REFINE_MUTATIONS)
def test_refiner_mutations_fail(mut, weak, ci):
    for temp in (TEMPS if not weak else TEMPS[:1]):
        (B, gh, gw, D, k), case, ref = refine_case(ci, weak, temp)
        got = emulate_refine(case["feats"], case["idx"], gh, gw, R.f32(temp), not weak, mut=mut)
        assert not refine_ok(got, case, ref), (mut, temp)
        assert refine_ok(emulate_refine(case["feats"], case["idx"], gh, gw, R.f32(temp), not weak), case, ref)


# ---- cross-tile fusion -------------------------------------------------------------------------------------------------------------
def fuse_weighted(cur, nbr, s, eps, biased=False):
    cn, nn_ = cur / (cur.norm(dim=-1, keepdim=True) + eps), nbr / (nbr.norm(dim=-1, keepdim=True) + eps)
    sim = cn @ nn_.T
    thr = sim.mean(-1, keepdim=True) + sim.std(-1, keepdim=True, unbiased=not biased)
    margin = torch.relu(sim - thr)
    raw = margin.pow(2)
    wts = raw / (raw.sum(-1, keepdim=True) + eps)
    sf = s * margin.mean(-1, keepdim=True).clamp(0.0, 1.0)
    return cur * (1 - sf) + (wts @ nbr) * sf


def fuse_attention(cur, nbr, s, scaled=True):
    both = torch.cat([cur, nbr], 0)
    sc = cur @ both.T
    a = torch.softmax(sc / (cur.shape[-1] ** 0.5) if scaled else sc, -1)
    return cur * (1 - s) + (a @ both) * s


def emulate_fusion(tokens, hg, wg, gh, gw, bw, mode, s, dtype=torch.float32, mut=None):
    """The kernels' data flow (pack / fuse left / pack / fuse top / apply) in `dtype`, with the mutations of the module docstring."""
    T, n, C = tokens.shape
    x = tokens.to(dtype).view(T, gh, gw, C)
    eps = R.f32(1e-6)
    if mode == "attention":
        fuse = lambda c, nb: fuse_attention(c, nb, s, scaled=mut != "no_sqrt_c")        # noqa: E731
    else:
        fuse = lambda c, nb: fuse_weighted(c, nb, s, eps, biased=mut == "biased_std")   # noqa: E731
    out = x.clone()
    left = {}
    for t in range(T):
        if t % wg > 0:
            cur = x[t][:, :bw].reshape(-1, C)
            if mut == "swap_strips":                          # the left strip walked with the top strip's row length
                e = torch.arange(gh * bw)
                cur = x[t].reshape(n, C)[((e // bw) * gh + e % bw) % n]
            left[t] = fuse(cur, x[t - 1][:, gw - bw:].reshape(-1, C)).view(gh, bw, C)
    for t in range(T):
        if t // wg > 0:
            up = t - wg
            bottom = x[up][gh - bw:].clone()
            if up % wg > 0 and mut != "top_original":
                bottom[:, :bw] = left[up][gh - bw:]
            out[t][:bw] = fuse(x[t][:bw].reshape(-1, C), bottom.reshape(-1, C)).view(bw, gw, C)
        if t in left:
            out[t][:, :bw] = left[t]
    return out.view(T, n, C)


_FUSION = {}


def fusion_tokens(ci):
    if ci not in _FUSION:
        hg, wg, gh, gw, bw, C = R.FUSION_CASES[ci]
        _FUSION[ci] = R.make_fusion_case(hg, wg, gh, gw, C, seed=ci)
    return _FUSION[ci]


def fusion_ok(got, tok, ci, mode, s):
    hg, wg, gh, gw, bw, C = R.FUSION_CASES[ci]
    ref = R.cross_tile_reference(tok, hg, wg, gh, gw, bw, mode, s, final_left=got)
    st = ref["strip"]
    if not torch.equal(got[~st], tok[~st]):
        return False, 0.0
    if not bool(st.any()):
        return True, 0.0
    try:
        return True, check_within(got[st], ref["out"][st], ref["bound"][st])
    except AssertionError:
        return False, float("inf")


@pytest.mark.parametrize("mode", ["weighted", "attention"])
@pytest.mark.parametrize("ci", range(len(R.FUSION_CASES)))
def test_fusion_f32_emulations_stay_inside_the_bound(ci, mode):
    hg, wg, gh, gw, bw, C = R.FUSION_CASES[ci]
    tok = fusion_tokens(ci)
    for strength in (0.3, 1.0):
        s = R.f32(strength)
        o = OR.CrossTileFusionOracle(mode, bw, s)
        orc = torch.stack([o(tok[t:t + 1].clone(), t // wg, t % wg, gh, gw)[0] for t in range(hg * wg)], 0)
        assert orc.dtype == torch.float32
        for name, got in (("oracle f32", orc), ("data-flow f32", emulate_fusion(tok, hg, wg, gh, gw, bw, mode, s))):
            ok, worst = fusion_ok(got, tok, ci, mode, s)
            assert ok and worst <= 1.0, (name, strength, worst)
        # without final_left the reference is the oracle itself
        o64 = OR.CrossTileFusionOracle(mode, bw, s)
        want = torch.stack([o64(tok[t:t + 1].double(), t // wg, t % wg, gh, gw)[0] for t in range(hg * wg)], 0)
        ref = R.cross_tile_reference(tok, hg, wg, gh, gw, bw, mode, s)
        assert (ref["out"] - want).abs().max().item() <= 1e-9 * want.abs().max().item()


# (mutation, mode, the FUSION_CASES index it must fail on)
FUSION_MUTATIONS = [
    ("swap_strips", "weighted", 0), ("swap_strips", "attention", 1),   # 6 x 10 and 10 x 6 grids
    ("top_original", "weighted", 1), ("top_original", "attention", 0),  # 3 x 2 and 2 x 3 scenes: tiles with both a left and an upper neighbour
    ("biased_std", "weighted", 0),                                      # S = 6: sqrt(6 / 5) on the std
    ("no_sqrt_c", "attention", 3),                                      # C = 72
]


@pytest.mark.parametrize("mut,mode,ci", FUSION_MUTATIONS)
def test_fusion_mutations_fail(mut, mode, ci):
    hg, wg, gh, gw, bw, C = R.FUSION_CASES[ci]
    tok = fusion_tokens(ci)
    for strength in (0.3, 1.0):
        s = R.f32(strength)
        assert fusion_ok(emulate_fusion(tok, hg, wg, gh, gw, bw, mode, s), tok, ci, mode, s)[0]
        assert not fusion_ok(emulate_fusion(tok, hg, wg, gh, gw, bw, mode, s, mut=mut), tok, ci, mode, s)[0], (mut, strength)


# ---- Cluster-Then-Debias -----------------------------------------------------------------------------------------------------------
def dbscan_variant(points, eps, min_samples, border="lowest_cluster", numbering="smallest_core"):
    """DBSCAN as ctd.hip states it (min-label propagation over core points, clusters numbered by their smallest core index, a border
    point joins the lowest-numbered neighbouring cluster), with the two mutations: border = 'lowest_core_index' (the cluster of the
    border point's lowest-index core neighbour), numbering = 'any_member' (clusters numbered by their first member of any kind)."""
    nb, _ = OC.neighbour_matrix(points, eps)
    n = points.shape[0]
    core = nb.sum(1) >= min_samples
    big = np.iinfo(np.int64).max
    lab = np.where(core, np.arange(n), big)
    A = nb & core[None, :] & core[:, None]
    while True:
        new = np.minimum(lab, np.where(A, lab[None, :], big).min(1))
        new[core] = np.minimum(new[core], new[new[core]])
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab[core])
    cid = {int(r): k for k, r in enumerate(roots)}
    out = np.full(n, -1, np.int64)
    for i in range(n):
        if core[i]:
            out[i] = cid[int(lab[i])]
        else:
            cn = np.nonzero(nb[i] & core)[0]
            if cn.size:
                out[i] = cid[int(lab[cn[0]])] if border == "lowest_core_index" else min(cid[int(lab[j])] for j in cn)
    if numbering == "any_member":
        first = {}
        for i in range(n):
            if out[i] >= 0 and int(out[i]) not in first:
                first[int(out[i])] = len(first)
        out = np.array([first[int(v)] if v >= 0 else -1 for v in out], np.int64)
    return out


def ctd_inputs():
    """(name, x [B, n, C], eps, min_samples) of every generator the GPU module uses, the n = 8192 chain and n = 1025 blobs aside (the
    same generators at sizes the CPU handles in a second)."""
    ch, co, nr = R.make_chain(2048), R.make_contested(), R.make_near_radius()
    yield "chain", ch["x"], ch["eps"], ch["min_samples"]
    yield "contested", co["x"], co["eps"], co["min_samples"]
    yield "near-radius", nr["x"], nr["eps"], nr["min_samples"]
    for n, C, eps, ms in ((64, 4, 0.4, 5), (65, 200, 1.1, 11)):
        yield f"blobs {n}x{C}", R.make_blobs(n, C, eps, seed=n + C), eps, ms


def test_ctd_generators_have_the_structure_they_claim():
    ch = R.make_chain(2048)
    ref = R.ctd_reference(ch["x"], torch.ones(1, 8), ch["eps"], ch["min_samples"], -1.5)
    assert bool((ref["labels"] == 0).all()) and 1e-5 < ref["radius_margin"] < 1e-4          # every adjacent pair is re-evaluated in f64
    nbm, _ = OC.neighbour_matrix(OC.ctd_points(ch["x"])[0].numpy(), ch["eps"])
    assert sorted(np.nonzero(nbm.sum(1) < 3)[0].tolist()) == sorted(ch["ends"])             # the two ends are the only non-core points
    co = R.make_contested()
    lab = R.ctd_reference(co["x"], torch.ones(3, 8), co["eps"], co["min_samples"], -1.5)["labels"]
    assert lab[0, co["z"]] == 0 and lab[0, co["tX"]] == 1 and lab[0, 0] == 0 and int(lab[0].max()) == 1 and int((lab[0] < 0).sum()) == 2
    assert bool((lab[1] == -1).all())
    assert lab[2, co["e"]] == 1 and lab[2, 1] == 0 and int(lab[2].max()) == 1
    nr = R.make_near_radius()
    ref = R.ctd_reference(nr["x"], torch.ones(1, 32), nr["eps"], nr["min_samples"], -1.5)
    assert R.RADIUS_MARGIN <= ref["radius_margin"] < 5e-6
    assert bool((ref["labels"][0, nr["inside"]] >= 0).all()) and bool((ref["labels"][0, nr["outside"]] == -1).all())
    _, d2 = OC.neighbour_matrix(OC.ctd_points(nr["x"])[0].numpy(), nr["eps"])
    near = np.abs(d2 - nr["eps"] ** 2) < 1e-4
    assert int(near.sum()) // 2 >= 16 and int((near & (d2 < nr["eps"] ** 2)).sum()) >= 16    # both sides of the radius


def test_ctd_mutations_fail_and_the_variant_is_the_oracle():
    for name, x, eps, ms in ctd_inputs():
        if name == "chain":
            continue
        for b in range(x.shape[0]):
            p = OC.ctd_points(x)[b].numpy()
            assert np.array_equal(dbscan_variant(p, eps, ms), OC.dbscan_labels(p, eps, ms)), name
    co = R.make_contested()
    p = OC.ctd_points(co["x"]).numpy()
    want = [OC.dbscan_labels(p[b], co["eps"], co["min_samples"]) for b in range(3)]
    got = dbscan_variant(p[0], co["eps"], co["min_samples"], border="lowest_core_index")
    assert got[co["z"]] == 1 and not np.array_equal(got, want[0])                            # fails on the contested tile
    got = dbscan_variant(p[2], co["eps"], co["min_samples"], numbering="any_member")
    assert got[co["e"]] == 0 and not np.array_equal(got, want[2])                            # fails on the numbering tile


def test_ctd_debias_f32_emulation_stays_inside_the_bound():
    for name, x, eps, ms in ctd_inputs():
        B, n, C = x.shape
        cls = torch.from_numpy(np.random.default_rng(5).standard_normal((B, C)).astype(np.float32))
        ref = R.ctd_reference(x, cls, eps, ms, -1.5)
        got = OC.adaptive_debiasing(x, ref["labels"], cls, -1.5)
        assert got.dtype == torch.float32
        noise = ref["labels"] < 0
        assert torch.equal(got[noise], x[noise]) and bool((ref["bound"][noise] == 0).all())
        if bool((~noise).any()):
            assert check_within(got[~noise], ref["out"][~noise], ref["bound"][~noise], name) <= 1.0
            # teeth: 1.0 for the 1.1 the two norms add is outside the bound on every generator
            off = OC.adaptive_debiasing(x, ref["labels"], cls, -1.5, eps=1.0)
            assert not bool(((off.double() - ref["out"]).abs() <= ref["bound"])[~noise].all()), name


def test_ctd_debias_bound_has_teeth_on_the_longest_cluster():
    """One cluster of 8192 members: the index-order f32 sum is charged 2u 8192 mean|x|, the loosest prototype bound of the GPU module
    (its err / bound there is ~1e-4).  The f32 emulation passes and 1.0 for the norms' 1.1 still fails."""
    ch = R.make_chain(8192)
    cls = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 8)).astype(np.float32))
    labels = torch.zeros(1, 8192, dtype=torch.long)                      # the GPU module asserts them against the oracle
    ref, bound = R.debias_reference(ch["x"], cls, labels, -1.5)
    assert check_within(OC.adaptive_debiasing(ch["x"], labels, cls, -1.5), ref, bound, "chain 8192") <= 1.0
    off = OC.adaptive_debiasing(ch["x"], labels, cls, -1.5, eps=1.0)
    assert not bool(((off.double() - ref).abs() <= bound).all())


def test_oracle_dbscan_equals_scikit_learn():
    pytest.importorskip("sklearn")
    from sklearn import cluster
    for name, x, eps, ms in ctd_inputs():
        pts = OC.ctd_points(x)
        for b in range(x.shape[0]):
            p = pts[b].numpy()
            want = cluster.DBSCAN(eps=eps, min_samples=ms, algorithm="brute").fit(p).labels_
            assert np.array_equal(OC.dbscan_labels(p, eps, ms), want), (name, b)
