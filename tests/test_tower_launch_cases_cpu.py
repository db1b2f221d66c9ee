"""The launch-size cases of tests/tower_launch_cases.py, checked without a GPU: every case passes the GEMM dispatcher's rule for the
persistent kernels on 256 compute units (and the size the one-tile / 24-prompt tests run does not), the fixture keys exist, the batch
builder places the probe tile where it says, and the oracle's answer for a probe does not depend on its batch."""
import os

import numpy as np
import pytest
import torch

import tower_launch_cases as TL


def setup_module(_m):
    torch.set_num_threads(min(16, os.cpu_count() or 1))


ALL = {**TL.VISION_CASES, **TL.TEXT_CASES}


@pytest.mark.parametrize("name", list(ALL))
def test_case_matches_the_table_and_passes_the_rule(name):
    case = ALL[name]
    tokens, batch, rows = TL.TABLE[name]
    if name in TL.VISION_CASES:
        assert (case.tokens, case.batch, case.rows) == (tokens, batch, rows)
        assert case.batch >= 16 and case.batch % 8 != 0 and case.cfg.heads % 4 == 0        # 'Experimental': order=images with a ragged last group
    else:
        assert (case.cfg.context_length, case.prompts, case.rows) == (tokens, batch, rows)
    assert case.rows % 256 != 0
    for N in TL.rule_widths(case):
        assert TL.gemm_prefers_persistent(case.rows, N, TL.CU_COUNT_MI355X), (name, N)
        assert not TL.gemm_prefers_persistent(TL.small_rows(case), N, TL.CU_COUNT_MI355X), (name, N)
    assert TL.rule_holds(case, TL.CU_COUNT_MI355X) and not TL.rule_holds(case, TL.CU_COUNT_MI355X, TL.small_rows(case))


def test_rule_restatement_edges():
    assert TL.few_tiles(1370, 1024, 256) and not TL.few_tiles(17425, 512, 256)      # 6 x 4 x 2 = 48; 69 x 2 x 2 = 276 (V2 at N = embed_dim)
    assert TL.cdiv(17425, 256) * 3 * 2 == 414                                        # V2 at N = width
    assert not TL.few_tiles(256 * 64, 512, 256) and TL.few_tiles(256 * 64 - 256, 512, 256)   # the threshold itself: 64 x 2 x 2 = 256
    assert not TL.gemm_prefers_persistent(1023, 4096, 8) and not TL.gemm_prefers_persistent(1 << 20, 256, 8)


@pytest.mark.parametrize("name", ["V1", "V2", "V3"])
def test_fixture_keys(golden, name):
    case = TL.VISION_CASES[name]
    g = golden("real_logits")
    for mt, _ in case.variants:
        lk, ak = TL.fixture_keys(case, mt)
        assert g[lk].shape == (len(TL.POTSDAM_QIDX), case.grid, case.grid) and g[lk].dtype == np.float32
        assert g[ak].shape == (case.grid, case.grid) and g[ak].dtype == np.uint8
        assert np.array_equal(g[lk].argmax(0).astype(np.uint8), g[ak])


@pytest.mark.parametrize("name", list(TL.VISION_CASES))
def test_probe_tile_sits_at_three_indices_and_nowhere_else(name):
    case = TL.VISION_CASES[name]
    batch, probe = TL.vision_batch(case), TL.probe_tile(case)
    assert batch.shape == (case.batch, 3, case.padded, case.padded) and batch.dtype == torch.float32
    at = TL.probe_indices(case.batch)
    assert len(set(at)) == 3 and at[0] == 0 and at[-1] == case.batch - 1
    raw = [batch[i].numpy().tobytes() for i in range(case.batch)]
    for i in range(case.batch):
        assert (raw[i] == probe[0].numpy().tobytes()) == (i in at), i
    assert len(set(raw)) == case.batch - 2                                  # the other tiles are pairwise distinct


def test_padded_probe_tile_shape():
    case = TL.VISION_CASES["V3"]
    assert case.padded == 518 and TL.probe_tile(case).shape == (1, 3, 518, 518)
    assert len({TL.filler_seed(c, i) for c in TL.VISION_CASES.values() for i in range(c.batch)} | {TL.PROBE_SEED}) == \
        sum(c.batch for c in TL.VISION_CASES.values()) + 1


@pytest.mark.parametrize("ign", [True, False])
def test_oracle_probe_does_not_depend_on_its_batch_v4(ign):
    """Tiles are independent in the oracle, so the GPU tests may run it on the probe tile alone.  Up to fp32 summation order (the
    host BLAS blocks a [2 x 257, D] product differently from a [257, D] one): 1e-5 on logits of magnitude <= 1, a hundredth of the bar."""
    case = TL.VISION_CASES["V4"]
    probe = TL.probe_tile(case)
    alone = TL.oracle_logits(case, "Experimental", ign, probe)
    pair = TL.oracle_logits(case, "Experimental", ign, torch.cat([TL._tile(case, TL.filler_seed(case, 1)), probe], 0))
    assert alone.shape == (1, 8, case.grid, case.grid)
    d = (pair[1] - alone[0]).abs().max().item()
    print(f"V4 ignore_residual={ign}: probe alone vs in a pair, max|dlogit| = {d:.2e}")
    assert d < 1e-5
    assert (pair[0] - alone[0]).abs().max().item() > 1e-3                   # the other tile really is another tile


@pytest.mark.parametrize("name", ["T1", "T3"])
def test_oracle_prompts_do_not_depend_on_their_batch(name):
    case = TL.TEXT_CASES[name]
    ids = TL.prompt_ids(case)
    assert ids.shape == (case.prompts, case.cfg.context_length)
    assert len({ids[i].tobytes() for i in range(case.prompts)}) == case.prompts
    probes = list(case.probes)
    alone = TL.oracle_text(case, ids[probes])
    mixed_rows = [7, probes[0], probes[1], 55, probes[2], 200, probes[3], probes[4]]
    mixed = TL.oracle_text(case, ids[mixed_rows])[[1, 2, 4, 6, 7]]
    d = (mixed - alone).abs().max().item()
    scale = alone.abs().max().item()
    print(f"{name}: prompts alone vs mixed, max|d| = {d:.2e} (|feature| max {scale:.2f})")
    assert alone.shape == (5, case.cfg.embed_dim)
    assert d < 1e-5 * max(1.0, scale)                                       # fp32 summation order only: a twentieth of the 2e-4 bar
