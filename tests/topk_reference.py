"""float64 numpy reference of the top-k head (sg_topk_head) and the acceptance rule its tests share.  Test infrastructure only.

The reference builds on head_reference.stitch: the scaled logit of a class is the maximum over the class's queries of canvas *
logit_scale (the synonym max of the class probabilities, since softmax is monotone); classes are sorted by (value descending, class
ascending); the probability of a slot is exp(value - logsumexp over ALL Q queries).  A class that owns no query is never listed; the
slots it leaves hold class -1 and probability 0.

Acceptance rule, per (pixel, slot).  Slot j COUNTS unless, in the reference, the scaled-logit gap to rank j - 1 or to rank j + 1
(rank k + 1 included, when it exists) is below GL = 5e-4: head_reference.py budgets about 5e-5 of f32 error on a scaled logit, two of
them move a gap by 1e-4, and GL is that with the module's 5x margin.  The rule is stated on the exponent because the lower slots'
probabilities are far below head_reference.G.  On a counted slot the class must equal the reference's and
|p - ref| <= REL * ref + 1e-30 with REL = 1e-3: 1e-4 on the exponent, 2 ulp of expf, about (Q + Q / 8) 2^-24 = 2e-5 for the online
sum at Q = 257 and one division are about 1.3e-4 relative; REL is about 7x that.  At most CAP = 1 % of a case's slots, and of any
single slot index, may be left uncounted; tests/test_topk_reference_cpu.py confirms that the reference alone meets the cap on every
case the GPU test runs.
"""
import functools

import numpy as np

import head_reference as HR

GL = 5e-4
REL, ABS = 1e-3, 1e-30
CAP = 0.01
KMAX = 8                                                                  # SG_TOPK_MAX
KS = (1, 2, 3, 5, 8)                                                      # every KTOP (1, 2, 4, 8) and both ragged dispatches (3, 5)

# (geometry, Q, merged class map): the cases of tests/test_gpu_topk_head.py; "dense" has more than 64 tiles over one block
CASES = [(g, Q, m) for g in ("a", "b") for Q in HR.QS for m in (False, True)]
DENSE = [("dense", 9, True), ("dense", 9, False)]


def ks_of(K: int):
    """The k values a case runs: KS clipped to K, without repeats."""
    return sorted({min(k, K) for k in KS})


def rank(canvas, query_idx, K: int, logit_scale: float, depth: int = KMAX + 1) -> dict:
    """canvas [Q,H,W] -> dict(order int64 [r,H,W], value [r,H,W], lse [H,W]), r = min(depth, K): the classes in (value descending,
    class ascending) order with their scaled logits (-inf: the class owns no query) and the log of the softmax denominator."""
    v = np.asarray(canvas, dtype=np.float64) * float(logit_scale)
    Q = v.shape[0]
    qi = np.arange(Q) if K == Q else np.asarray(query_idx).reshape(-1)
    cv = np.full((K,) + v.shape[1:], -np.inf)
    for q in range(Q):
        if 0 <= qi[q] < K:
            cv[qi[q]] = np.maximum(cv[qi[q]], v[q])
    m = v.max(0)
    lse = m + np.log(np.exp(v - m).sum(0))
    order = np.argsort(-cv, axis=0, kind="stable")[:min(depth, K)]         # stable on the negated values: equal values keep class order
    return dict(order=order, value=np.take_along_axis(cv, order, 0), lse=lse)


def topk(ranked: dict, k: int) -> dict:
    """-> dict(classes int64 [k,H,W] (-1 unfilled), probs [k,H,W], counted bool [k,H,W])"""
    val = ranked["value"]
    assert 1 <= k <= val.shape[0]
    top = val[:k]
    filled = np.isfinite(top)
    with np.errstate(invalid="ignore", over="ignore"):
        probs = np.where(filled, np.exp(np.where(filled, top, 0.0) - ranked["lse"]), 0.0)
        gap = val[:-1] - val[1:] if val.shape[0] > 1 else np.zeros((0,) + val.shape[1:])      # gap[j] = rank j to rank j + 1
    gap = np.where(np.isnan(gap), np.inf, gap)                              # two unfilled slots: both are -1 / 0, nothing to decide
    inf = np.full((1,) + val.shape[1:], np.inf)
    up = np.concatenate([inf, gap[:k - 1]], 0)
    down = np.concatenate([gap[:k], inf], 0)[:k]
    classes = np.where(filled, ranked["order"][:k], -1)
    return dict(classes=classes, probs=probs, counted=(up >= GL) & (down >= GL))


def shares(ref: dict):
    """(uncounted share of all slots, the largest uncounted share of one slot index)"""
    un = ~ref["counted"]
    return float(un.mean()), float(un.reshape(un.shape[0], -1).mean(1).max())


def check(ref: dict, classes, probs, what: str = "", cap: bool = True):
    """The acceptance rule; prints the uncounted shares and the worst err / bound, returns (share, worst slot share, worst ratio)."""
    classes = np.asarray(classes).astype(np.int64).reshape(ref["classes"].shape)
    probs = np.asarray(probs, dtype=np.float64).reshape(ref["probs"].shape)
    ok = ref["counted"]
    frac, worst = shares(ref)
    bad = int((classes[ok] != ref["classes"][ok]).sum())
    bound = REL * ref["probs"] + ABS
    ratio = float((np.abs(probs - ref["probs"])[ok] / bound[ok]).max()) if ok.any() else 0.0
    print(f"{what}: uncounted {100 * frac:.3f} % of the slots, {100 * worst:.3f} % of the worst slot index, class mismatches on counted "
          f"slots {bad}, worst err / bound {ratio:.3f}")
    if cap:
        assert frac <= CAP, f"{what}: {100 * frac:.2f} % of the slots are within {GL} of a tie"
        assert worst <= CAP, f"{what}: {100 * worst:.2f} % of one slot index are within {GL} of a tie"
    assert bad == 0, f"{what}: {bad} counted slots name another class than the float64 reference"
    assert np.isfinite(probs).all(), f"{what}: non-finite probabilities"
    assert ratio <= 1.0, f"{what}: a counted probability is off by {ratio:.3f} of its bound"
    return frac, worst, ratio


@functools.lru_cache(maxsize=None)
def case(geom: str, Q: int, merge: bool) -> dict:
    """head_reference.make_case with its float64 canvas and ranking, computed once and never modified."""
    c = HR.make_case(geom, Q, merge)
    c["canvas"] = HR.stitch(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
    c["ranked"] = rank(c["canvas"], c["query_idx"], c["K"], SCALE)
    return c


SCALE = 50.0
