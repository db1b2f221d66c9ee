"""Reference of area_thd, the per-image suppression of small-area classes (the definition: include/segearth_hip.h), in numpy: integer
counts, the comparison in Python doubles, and float64 probabilities on top of head_reference.stitch / tail.  Test infrastructure only;
shared by the CPU and the GPU tests of the feature.

Also the cases those tests run and their acceptance rule.  A case is head_reference.make_case plus a two-tier class bias, added to every
query of a class: classes c < (K + 2) // 3 and the background get 0, the others -0.05 (x logit_scale 50: a factor e^-2.5 on their
probabilities), so that the second tier wins small scattered areas -- what the option exists to remove.  The two small cases (K = 2, 3
with bg_idx = 0: the binary building / road shape) use -0.03 for class 1 and -0.04 for class 2, so that at K = 3 the two non-background
classes have areas that differ by more than noise.  area_thd is the midpoint of the widest gap between adjacent non-background areas of
the reference; at K = 2 there is no gap to take and the one non-background class has to go for the case to mean anything: area_thd = 1.5.

The acceptance rule.  A pixel COUNTS unless
  - its first-pass top-two gap is below G = head_reference.G (its first label, hence one unit of an area, may differ), or
  - the RELATIVE gap (p1 - p2) / p1 of its two best kept classes is below G (relative: a relabelled pixel's best kept probability can
    be 1e-4, and the device's error is relative there -- both probabilities carry the same softmax sum and a few ulp of expf each), or
  - |p1 - prob_thd| < G.
At most CAP = head_reference.CAP of a case's pixels may be left uncounted.  Two preconditions make the keep bits themselves safe, and a
test fails (never skips) when one does not hold: every non-background class's area differs from area_thd * total by more pixels than the
first pass leaves uncounted (no near-tie can flip a keep bit); and a class of positive area is dropped while -- where there is more than
one non-background class -- a non-background class is kept.
"""
import functools

import numpy as np

import head_reference as HR

G, CAP = HR.G, HR.CAP
LOGIT_SCALE, PROB_THD = 50.0, 0.3
# (geometry, Q, merge, bg_idx): the Q = 130 case of "dense" leaves 1.04 % of its pixels uncounted and is left out
CASES = [(g, Q, m, 3) for g in ("a", "b", "dense") for Q, m in ((8, False), (9, True), (65, True), (130, False)) if (g, Q) != ("dense", 130)] + \
        [(g, K, False, 0) for g in ("a", "dense") for K in (2, 3)]


def case_id(c):
    return f"{c[0]}-Q{c[1]}-{'merge' if c[2] else 'plain'}-bg{c[3]}"


def keep_of(area, bg_idx: int, area_thd: float) -> np.ndarray:
    """Steps 2-3: int64 areas [K] -> keep bool [K].  Python ints and doubles: the sum is exact, the comparison IEEE double."""
    area = [int(a) for a in np.asarray(area).reshape(-1)]
    total = sum(a for c, a in enumerate(area) if c != bg_idx)
    return np.array([c == bg_idx or float(a) > float(area_thd) * float(total) for c, a in enumerate(area)], dtype=bool)


def area_filter(probs: np.ndarray, area_thd: float, prob_thd: float, bg_idx: int, l0=None) -> dict:
    """Steps 1-5 on probs [K,H,W] in the dtype they come in (float64 for the reference, float32 for byte comparisons with the device:
    the function compares and selects, it computes nothing).  ``l0``: first-pass labels to use in place of the arg-max of step 1.
    -> dict(l0, area int64 [K], total, keep bool [K], probs, labels int64 [H,W], best = the largest kept probability)."""
    probs = np.asarray(probs)
    K = probs.shape[0]
    l0 = probs.argmax(0) if l0 is None else np.asarray(l0).reshape(probs.shape[1:])        # the first maximum: the lowest class index
    inside = (l0 >= 0) & (l0 < K)
    area = np.bincount(l0[inside].reshape(-1), minlength=K).astype(np.int64)
    keep = keep_of(area, bg_idx, area_thd)
    out = np.where(keep[:, None, None], probs, probs.dtype.type(0))
    masked = np.where(keep[:, None, None], probs, -np.inf)                                # dropped classes are excluded, not zeros
    labels = masked.argmax(0).astype(np.int64)
    best = masked.max(0)
    labels = np.where(best < probs.dtype.type(prob_thd), bg_idx, labels)
    return dict(l0=l0, area=area, total=int(area.sum() - area[bg_idx]), keep=keep, probs=out, labels=labels, best=best)


def widest_gap_thd(area, bg_idx: int) -> float:
    """area_thd as a share of the non-background total: the midpoint of the widest gap between adjacent non-background areas; 1.5 where
    there is a single non-background class (it is dropped)."""
    area = np.asarray(area, dtype=np.int64)
    nb = np.sort(np.delete(area, bg_idx))
    total = int(nb.sum())
    if nb.size < 2:
        return 1.5
    assert total > 0, "no non-background pixel: the case would show nothing"
    i = int(np.argmax(np.diff(nb)))
    return float(nb[i] + nb[i + 1]) / 2.0 / float(total)


def class_bias(K: int, bg_idx: int) -> np.ndarray:
    if K <= 3:
        return np.array([0.0, -0.03, -0.04][:K])
    b = np.full(K, -0.05)
    b[:(K + 2) // 3] = 0.0
    b[bg_idx] = 0.0
    return b


@functools.lru_cache(maxsize=None)
def make_case(geom: str, Q: int, merge: bool, bg_idx: int):
    """head_reference.make_case with the class bias on every query of the class, and its float64 reference:
    -> dict(the case's fields, bg_idx, first = head_reference.tail with prob_thd 0 (probs, labels = l0, conf, gap), area_thd, ref =
    area_filter of first['probs'], ok = the counted pixels, first_uncounted = pixels whose first label is undecided).  Computed once per
    case and shared; nobody may write into it."""
    c = HR.make_case(geom, Q, merge)
    K, qi = c["K"], c["query_idx"]
    bias = class_bias(K, bg_idx)
    c["tile_logits"] = (c["tile_logits"] + bias[qi][None, :, None, None].astype(np.float32)).astype(np.float32)
    canvas = HR.stitch(c["tile_logits"], c["windows"], c["up_hw"], c["pad_tl"], c["hw"])
    first = HR.tail(canvas, qi, K, LOGIT_SCALE, 0.0, bg_idx)
    thd = widest_gap_thd(np.bincount(first["labels"].reshape(-1), minlength=K), bg_idx)
    ref = area_filter(first["probs"], thd, PROB_THD, bg_idx)
    kp = np.where(ref["keep"][:, None, None], first["probs"], -np.inf)
    p1 = kp.max(0)
    if int(ref["keep"].sum()) > 1:
        p2 = np.partition(kp, K - 2, axis=0)[K - 2]
    else:
        p2 = np.full(p1.shape, -np.inf)                                                    # the background alone: nothing to tie with
    rel = np.where(p1 > 0, (p1 - np.maximum(p2, 0.0)) / np.where(p1 > 0, p1, 1.0), 0.0)
    first_ok = first["gap"] >= G
    ok = first_ok & (rel >= G) & (np.abs(p1 - PROB_THD) >= G)
    c.update(bg_idx=bg_idx, first=first, area_thd=thd, ref=ref, ok=ok, first_uncounted=int((~first_ok).sum()),
             relabelled=float((~ref["keep"][first["labels"]]).mean()))
    for v in (c["tile_logits"], first["probs"], first["labels"], ref["probs"], ref["labels"], ok):
        v.setflags(write=False)
    return c


def check_preconditions(c, what=""):
    """The cap and the two preconditions of the module docstring, asserted; returns the figures."""
    ref, bg, K = c["ref"], c["bg_idx"], c["K"]
    frac = 1.0 - float(c["ok"].mean())
    nb = [k for k in range(K) if k != bg]
    margin = min(abs(float(ref["area"][k]) - c["area_thd"] * ref["total"]) for k in nb)
    dropped = [k for k in nb if not ref["keep"][k] and ref["area"][k] > 0]
    kept = [k for k in nb if ref["keep"][k]]
    print(f"{what}: K {K}, area_thd {c['area_thd']:.4f}, uncounted {100 * frac:.3f} %, area margin {margin:.1f} px against "
          f"{c['first_uncounted']} undecided first labels, dropped {len(dropped)} kept {len(kept)}, relabelled {100 * c['relabelled']:.1f} %")
    assert frac <= CAP, f"{what}: {100 * frac:.2f} % of the pixels are uncounted"
    assert margin > c["first_uncounted"], f"{what}: an area lies {margin} px from the bound, {c['first_uncounted']} first labels are undecided"
    assert dropped, f"{what}: no class of positive area is dropped"
    assert kept or len(nb) == 1, f"{what}: no non-background class is kept"
    return frac, margin


def check_labels(c, labels, what=""):
    """The acceptance rule against the float64 reference: every counted pixel carries the reference's label."""
    labels = np.asarray(labels).reshape(c["ref"]["labels"].shape)
    ok = c["ok"]
    bad = int((labels[ok] != c["ref"]["labels"][ok]).sum())
    print(f"{what}: uncounted {100 * (1 - ok.mean()):.3f} %, label mismatches on counted pixels {bad}")
    assert 1.0 - ok.mean() <= CAP, what
    assert bad == 0, f"{what}: {bad} counted pixels differ from the float64 reference"
