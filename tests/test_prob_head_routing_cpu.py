"""Which tail returns the class probabilities: SegPipeline.fused_prob_head() on a stub, no GPU.  "fused" and "canvas" are what they say;
"auto" is the canvas route up to 64 queries, and beyond it the fused head only if profiles/r08_bench_prob_head.jsonl shows its median not
above the canvas route's at both Q = 130 and Q = 256 -- otherwise the canvas everywhere.  The constant in pipeline.py must be what that
rule gives on the recorded numbers."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r08_bench_prob_head.jsonl")


def stub(**attrs):
    """A SegPipeline without its constructor, with only these attributes set: every option not given reads its class-level default."""
    from clip_decontamination_amd.pipeline import SegPipeline
    pipe = SegPipeline.__new__(SegPipeline)
    for name, value in attrs.items():
        setattr(pipe, name, value)
    return pipe


def fused(mode, Q):
    from clip_decontamination_amd.pipeline import SegPipeline
    return SegPipeline.fused_prob_head(stub(prob_head=mode, num_queries=Q))


def recorded_rule():
    med = {}
    with open(PROFILE) as f:
        for line in f:
            r = json.loads(line)
            if r.get("case") in ("canvas", "fused"):
                med.setdefault(r["Q"], {})[r["case"]] = r["ms"]["median"]
    return all(med[q]["fused"] <= med[q]["canvas"] for q in (130, 256))


@pytest.mark.parametrize("Q", [1, 16, 64, 65, 130, 256])
def test_explicit_modes(Q):
    assert fused("fused", Q) is True
    assert fused("canvas", Q) is False


@pytest.mark.parametrize("Q", [1, 16, 64])
def test_auto_keeps_the_canvas_up_to_64_queries(Q):
    assert fused("auto", Q) is False


@pytest.mark.parametrize("Q", [65, 130, 256])
def test_auto_beyond_64_queries_follows_the_recorded_measurement(Q):
    from clip_decontamination_amd import pipeline
    assert pipeline.PROB_HEAD_AUTO_FUSED_BEYOND_MAX_Q is recorded_rule()
    assert fused("auto", Q) is recorded_rule()


def test_a_pipeline_without_the_attribute_is_auto():
    from clip_decontamination_amd.pipeline import SegPipeline
    assert SegPipeline.fused_prob_head(stub(num_queries=9)) is False


def test_unknown_mode_is_refused_by_the_pipeline():
    from clip_decontamination_amd.pipeline import SegPipeline
    with pytest.raises(ValueError, match="prob_head"):
        SegPipeline(None, None, None, prob_head="both")
