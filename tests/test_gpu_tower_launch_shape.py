"""Both towers at machine-filling launch sizes against the oracle (cases: tests/tower_launch_cases.py).

A launch of one or two tiles (or 24 prompts) runs every linear on the 128 x 128 ring kernels with LayerNorm as a pass; production and the
benchmark launch enough rows for gemm_bf16_prefers_persistent(): persist_k64 / h2_persist, and in the vision tower the folded-LayerNorm
chain (producer epilogues -> ln_stats_finalize -> consumer GEMMs, handed from block to block by LnHandoff), plus the last block's
'Experimental' attention in its order=images workgroup order.  Each case asserts, in this order:

 a. the dispatch under test really ran (the restated rule with the device's CU count; launch counts per profile category; the last GEMM /
    attention record) -- a failure, never a skip;
 b. each of the three copies of the probe tile (or the five probe prompts) against the fixture / the oracle, on the default path and
    under tuning code 34 (persistent GEMMs, LayerNorm as a pass);
 c. the three copies agree with one another (1e-5, identical arg-max), and for V2 / V3 with the probe tile run alone on the same
    kernels (tuning code 36).

Folded launch counts (capi.hip std_block / mlp_block / ln1_qkv, L layers, every block foldable): blocks 0 .. L-2 run std_block.  Its
out-projection is a producer in every block and its mlp_block runs an fc consumer + a proj producer: 2 (L-1) producers, L-1 consumers.
ln1_qkv is a consumer where the previous block handed x on: blocks 1 .. L-2 (block 0 has no hand-off) and the last block's ln1_qkv:
L-1 more.  The last block's out-projection and (ignore_residual=False) mlp_block take a fresh hand-off and fold nothing.  So categories
5 (consumer) and 6 (producer) each show 2 (L-1) launches.  GEM (V5) runs std_block on its first F = L - 6 blocks only and the dual-stream
blocks fold nothing (gem_forward_tail: LayerNorm passes, mlp_block on a fresh hand-off): 2 F - 1 consumers, 2 F producers.

The f16x2 record: the profile has one category for all two-plane GEMMs, so the evidence is the restated rule, the last GEMM record and a
bit difference under code 34.  The last GEMM of a vision forward is `@ proj` with an f32 C and no residual, which is not one of the
two-plane persistent kernel's compile-time epilogue forms (gemm_bf16.hip gemm_h2: hot_form), so a big launch runs it on `h2_pingpong`
(a small launch: `h2_ring128`); the record asserted is therefore `h2_pingpong`, and the folded chain (which forces h2_persist) is
evidenced by the code-34 difference.  For the text tower in f16x2 (no folding, and a last GEMM of 241 rows) the restated rule is the
only evidence.

Bounds are the ones the one-tile tests carry (1e-3 + labels for f16x2, HALF_TOL of test_gpu_vit.py for bf16 / f16, the text bounds of
test_text_real_shape_vs_oracle); every measured value is printed.  The text cosine bounds were measured on the small-launch kernels
and hold on the persistent ones (min cosine bf16 0.9999834 for 0.99995, f16 0.9999996 for 0.999999).  All values measured on an
MI355X: DESIGN.md section 4, 'Towers at launch size'."""
import ctypes as C
import gc
import os

import pytest
import torch
import torch.nn.functional as F

import tower_launch_cases as TL
from test_gpu_batch import labels_match_up_to_ties
from test_gpu_vit import HALF_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECS = ("f16x2", "f16", "bf16")
CAT_RING, CAT_PERSIST, CAT_LN_CONSUMER, CAT_LN_PRODUCER = 0, 3, 5, 6
TEXT_COS = {"bf16": 0.99995, "f16": 0.999999}                  # test_gpu_text.py::test_text_real_shape_vs_oracle


def _lib():
    from clip_decontamination_amd import _lib as L
    return L.load()


def launches(cat):
    ms, fl, n, dr = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
    assert _lib().sg_profile_read(cat, C.byref(ms), C.byref(fl), C.byref(n), C.byref(dr)) == 0
    assert dr.value == 0
    return n.value


def profiled(fn):
    """fn() between sg_profile_enable and a synchronise: (result, launches per category)."""
    lib = _lib()
    assert lib.sg_profile_enable(4096) == 0
    out = fn()
    torch.cuda.synchronize()
    counts = {c: launches(c) for c in (CAT_RING, CAT_PERSIST, CAT_LN_CONSUMER, CAT_LN_PRODUCER)}
    lib.sg_profile_disable()
    return out, counts


@pytest.fixture(scope="module")
def towers():
    """One tower per (architecture, precision), shared by the model types and cases that run on it; batches stay on the device."""
    from clip_decontamination_amd import engine as E
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    held = {}

    class Towers:
        batches = {}

        def vision(self, case, prec):
            key = (case.cfg, prec)
            if key not in held:
                held.clear()
                gc.collect()
                held[key] = E.HipCLIP(E.HipVisionTower(case.cfg, TL.vit_weights(case.cfg), precision=prec, device=DEV))
            return held[key]

        def text(self, case, prec):
            key = (case.cfg, prec)
            if key not in held:
                held.clear()
                gc.collect()
                held[key] = E.HipTextTower(case.cfg, TL.text_weights(case.cfg), precision=prec, device=DEV)
            return held[key]

        def batch(self, case):
            if case.name not in self.batches:
                self.batches[case.name] = TL.vision_batch(case).to(DEV)
            return self.batches[case.name]

    yield Towers()
    held.clear()
    Towers.batches.clear()


REFS = {}


def reference(golden, case, mt, ign):
    """(logits [Q, g, g], arg-max [g, g], SegOracle) of the probe tile: the fixture minted from the reference, or the oracle run once."""
    key = (case.name, mt, ign)
    if key not in REFS:
        if case.reference == "fixture":
            lk, ak = TL.fixture_keys(case, mt)
            g = golden("real_logits")
            REFS[key] = (torch.from_numpy(g[lk]), torch.from_numpy(g[ak]).long())
        else:
            lg = TL.oracle_logits(case, mt, ign, TL.probe_tile(case))[0]
            REFS[key] = (lg, lg.argmax(0))
    return REFS[key] + (TL.seg_oracle(case, mt, ign),)


def tile_logits(net, case, mt, ign, img):
    """Patch-grid logits [B, Q, g, g] of ONE tower launch on `img`, as head_logits of test_gpu_vit.py computes them."""
    from clip_decontamination_amd import engine as E, ops
    v = net.visual
    text = TL.text_features(case).to(DEV)
    if mt == "GEM":
        v.similarity_enhancer = v.outlier_suppressor = None
        v.gem_ignore_residual = ign
        lg = ops.cosine_logits(v(img), None, text, 0.0, 0.0)
    else:
        v.similarity_enhancer = E.SimilarityEnhancementModule(**TL.SIM)
        v.outlier_suppressor = E.OutlierSuppressionModule(**TL.OUTLIER)
        cls, tok = net.encode_image(img, mt, ign, output_cls_token=True, apply_similarity_enhancement=True)
        lg = ops.cosine_logits(tok, cls, text, 0.2, 0.0)
    return lg.reshape(img.shape[0], -1, case.grid, case.grid)


def expected_folded(case):
    """(consumer, producer) launches of one forward: the derivation in the module docstring."""
    if case.reference == "gem":
        return 2 * case.folded_blocks - 1, 2 * case.folded_blocks
    return 2 * (case.cfg.layers - 1), 2 * (case.cfg.layers - 1)


def check_against_reference(tag, prec, case, lg, ref, ref_argmax, oracle):
    """(b) for one copy of the probe tile; prints the measured values, then asserts the bounds of the one-tile tests."""
    lg = lg.cpu()
    d = (lg - ref).abs()
    err, q99 = d.max().item(), torch.quantile(d.flatten(), 0.99).item()
    agree = (lg.argmax(0) == ref_argmax).float().mean().item()
    print(f"LAUNCH-SHAPE | {tag} | max|dlogit| {err:.2e} | q99 {q99:.2e} | agreement {agree:.4f}")
    if prec == "f16x2":
        assert err < 1e-3, (tag, err)
        if case.reference == "fixture":
            assert agree == 1.0, (tag, agree)
        else:
            assert labels_match_up_to_ties(oracle.postprocess(lg)[1], ref, oracle), f"{tag}: label mismatch away from a tie"
    else:
        tol = HALF_TOL[prec]
        assert err < tol["real_err"], (tag, err)
        assert q99 < tol["real_q99"], (tag, q99)
        assert agree > tol["real_agree"], (tag, agree)


VISION_PARAMS = [pytest.param(name, prec, mt, ign, id=f"{name}-{prec}-{mt}-{'ign' if ign else 'res'}")
                 for group in (("V1", "V2"), ("V3",), ("V4",), ("V5",)) for prec in PRECS for name in group
                 for (mt, ign) in TL.VISION_CASES[name].variants]


@pytest.mark.parametrize("name,prec,mt,ign", VISION_PARAMS)
def test_vision_tower_at_launch_size(towers, golden, name, prec, mt, ign):
    lib = _lib()
    case = TL.VISION_CASES[name]
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    # ---- a. the rule, before anything runs
    assert TL.rule_holds(case, cu), (f"{name}: {case.batch} tiles = {case.rows} rows do not pass gemm_bf16_prefers_persistent() at N = "
                                     f"{TL.rule_widths(case)} on this device's {cu} compute units: the small-launch kernels would run")
    net, batch = towers.vision(case, prec), towers.batch(case)
    at = TL.probe_indices(case.batch)
    try:
        lg, counts = profiled(lambda: tile_logits(net, case, mt, ign, batch))
        gemm_last, attn_last = lib.sg_gemm_last_kernel().decode(), lib.sg_attention_last_kernel().decode()
        assert lib.sg_set_gemm_config(34) == 0
        lg34, counts34 = profiled(lambda: tile_logits(net, case, mt, ign, batch))
        lone = None
        if name in ("V2", "V3"):
            assert lib.sg_set_gemm_config(36) == 0
            lone = tile_logits(net, case, mt, ign, batch[:1])[0]
            torch.cuda.synchronize()
    finally:
        lib.sg_profile_disable()
        lib.sg_set_gemm_config(-1)
    print(f"LAUNCH-SHAPE | {name} {prec} {mt} ign={ign} | CUs {cu} | launches {counts} | code 34 {counts34} | {gemm_last} | {attn_last}")
    # ---- a. the dispatch under test really ran
    if prec == "f16x2":
        assert gemm_last.startswith("h2_pingpong"), gemm_last           # `@ proj` of a big launch (module docstring); small: h2_ring128
        assert not torch.equal(lg, lg34), "code 34 changed no bit: the folded-LayerNorm chain did not run"
    else:
        want = expected_folded(case)
        assert (counts[CAT_LN_CONSUMER], counts[CAT_LN_PRODUCER]) == want, (counts, want)
        assert (counts34[CAT_LN_CONSUMER], counts34[CAT_LN_PRODUCER]) == (0, 0), counts34
        assert counts34[CAT_PERSIST] == counts[CAT_PERSIST] and counts34[CAT_RING] == counts[CAT_RING]   # the same GEMMs, unfolded
        assert gemm_last.startswith("persist_k64"), gemm_last
    if mt == "Experimental":
        assert "gk=2" in attn_last and "order=images" in attn_last, attn_last
    assert torch.isfinite(lg).all() and torch.isfinite(lg34).all()
    # ---- b. each copy against the reference, default path and code 34
    ref, ref_argmax, oracle = reference(golden, case, mt, ign)
    for path, out in (("folded", lg), ("code34", lg34)):
        for i in at:
            check_against_reference(f"{name} {prec} {mt} ign={ign} {path} copy@{i}", prec, case, out[i], ref, ref_argmax, oracle)
    # ---- c. position inside the launch does not matter
    for path, out in (("folded", lg), ("code34", lg34)):
        same = all(torch.equal(out[at[0]], out[i]) for i in at[1:])
        worst = max((out[at[0]] - out[i]).abs().max().item() for i in at[1:])
        print(f"LAUNCH-SHAPE | {name} {prec} {mt} ign={ign} {path} | copies bit-identical {same} | max|d| between copies {worst:.2e}")
        assert worst < 1e-5, (path, worst)
        for i in at[1:]:
            assert torch.equal(out[at[0]].argmax(0), out[i].argmax(0)), (path, i)
    if lone is not None:
        worst = max((lone - lg[i]).abs().max().item() for i in at)
        print(f"LAUNCH-SHAPE | {name} {prec} {mt} ign={ign} | alone (code 36) bit-identical {all(torch.equal(lone, lg[i]) for i in at)} | "
              f"max|d| to the copies {worst:.2e}")
        assert worst < 1e-5, worst
        for i in at:
            assert torch.equal(lone.argmax(0), lg[i].argmax(0)), i
        assert not any(torch.equal(lg[i], lg[j]) for i in at for j in range(case.batch) if j not in at)   # the other tiles are other tiles


TEXT_PARAMS = [pytest.param(name, prec, id=f"{name}-{prec}") for name in TL.TEXT_CASES for prec in PRECS]


@pytest.mark.parametrize("name,prec", TEXT_PARAMS)
def test_text_tower_at_launch_size(towers, name, prec):
    """241 prompts in one encode_text launch; the oracle on prompts 0, 1, 120, 239 and 240.  The text tower folds no LayerNorm, so code
    34 must change nothing; in f16x2 the restated rule is the only evidence of the dispatch (module docstring)."""
    lib = _lib()
    case = TL.TEXT_CASES[name]
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert TL.rule_holds(case, cu), (f"{name}: {case.prompts} prompts = {case.rows} rows do not pass gemm_bf16_prefers_persistent() at N = "
                                     f"{TL.rule_widths(case)} on this device's {cu} compute units: the small-launch kernels would run")
    tt = towers.text(case, prec)
    ids = TL.prompt_ids(case)
    tok = torch.from_numpy(ids)
    try:
        out, counts = profiled(lambda: tt.encode_text(tok))
        assert lib.sg_set_gemm_config(34) == 0
        out34 = tt.encode_text(tok)
        torch.cuda.synchronize()
    finally:
        lib.sg_profile_disable()
        lib.sg_set_gemm_config(-1)
    print(f"LAUNCH-SHAPE | {name} {prec} | CUs {cu} | launches {counts}")
    if prec != "f16x2":
        assert counts[CAT_PERSIST] == 4 * case.cfg.layers, counts
        assert counts[CAT_LN_CONSUMER] == 0 and counts[CAT_LN_PRODUCER] == 0, counts
        assert counts[CAT_RING] <= 1, counts                                 # at most the final projection (241 rows)
    assert out.shape == (case.prompts, case.cfg.embed_dim) and torch.isfinite(out).all()
    probes = list(case.probes)
    ref = TL.oracle_text(case, ids[probes])
    for path, o in (("default", out), ("code34", out34)):
        got = o.cpu()[probes]
        err = (got - ref).abs().max().item()
        cmin = F.cosine_similarity(got, ref, dim=-1).min().item()
        print(f"LAUNCH-SHAPE | {name} {prec} {path} | max|d| {err:.2e} (|ref| max {ref.abs().max().item():.2f}) | min cosine {cmin:.7f}")
        if prec == "f16x2":
            assert err < 2e-4 * max(1.0, ref.abs().max().item()), (path, err)
        else:
            assert cmin > TEXT_COS[prec], (path, cmin)
    assert torch.equal(out, out34)
