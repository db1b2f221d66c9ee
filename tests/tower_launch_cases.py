"""The towers at machine-filling launch sizes: case table, the launch-size rule of the GEMM dispatcher restated, batch builders and
the CPU oracle calls.  Shared by tests/test_tower_launch_cases_cpu.py and tests/test_gpu_tower_launch_shape.py; imports no GPU code.

The rule (clip_decontamination_amd/csrc/gemm_bf16.hip):

    static bool few_tiles(int M, int N) {
      return g_gemm_config != TUNE_NO_SMALL_LAUNCH && (int64_t)cdiv(M, 256) * cdiv(N, 256) * 2 < device_cu_count();
    }
    bool gemm_bf16_prefers_persistent(int M, int N) { return M >= 1024 && N >= 512 && !few_tiles(M, N); }

Below it every linear of a tower runs on the 128 x 128 ring kernels with LayerNorm as a pass; at or above it the linears run on the
persistent kernels and (capi.hip ln_fold_ok(), which needs gemm_bf16_prefers_persistent(R, D)) the vision tower folds ln_1 / ln_2
into its GEMMs.  Every case here is sized to pass the rule on 256 compute units at N = width and N = embed_dim."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F

from clip_decontamination_amd import weights as Wt
from oracle import segment as OS, text as OT, vit as OV          # checker only

CU_COUNT_MI355X = 256
POTSDAM_QIDX = [0, 0, 1, 2, 3, 4, 5, 5]
SIM = dict(similarity_weight=1.0, temperature=1.0, add_self_similarity=True)
OUTLIER = dict(top_k=30)
PROBE_SEED = 1234                                               # the tile test_real_size_parity_f32 and real_logits.npz use


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def few_tiles(M: int, N: int, cu_count: int) -> bool:
    """gemm_bf16.hip few_tiles() with no tuning code set."""
    return cdiv(M, 256) * cdiv(N, 256) * 2 < cu_count


def gemm_prefers_persistent(M: int, N: int, cu_count: int) -> bool:
    """gemm_bf16.hip gemm_bf16_prefers_persistent()."""
    return M >= 1024 and N >= 512 and not few_tiles(M, N, cu_count)


@dataclass(frozen=True)
class VisionCase:
    name: str
    cfg: Wt.VitConfig
    tile: int                                   # S: the tile is S x S pixels before padding to the patch size
    batch: int                                  # B: tiles in the one launch
    reference: str                              # "fixture" (real_logits.npz), "vit" (oracle.vit.vit_forward), "gem" (oracle.vit.gem_forward)
    variants: Tuple[Tuple[str, bool], ...]      # (model_type, ignore_residual) -- for GEM the flag is gem_ignore_residual

    @property
    def padded(self) -> int:
        l, r, _, _ = OS.compute_padsize(self.tile, self.tile, self.cfg.patch)
        return self.tile + l + r

    @property
    def grid(self) -> int:
        return self.padded // self.cfg.patch

    @property
    def tokens(self) -> int:
        return self.grid * self.grid + 1

    @property
    def rows(self) -> int:
        return self.batch * self.tokens

    @property
    def folded_blocks(self) -> int:
        """Blocks that run capi.hip std_block(): all but the last, or for GEM the ones in front of the dual-stream blocks."""
        return self.cfg.layers - 6 if self.reference == "gem" else self.cfg.layers - 1


@dataclass(frozen=True)
class TextCase:
    name: str
    cfg: Wt.TextConfig
    prompts: int = 241                          # 3 classes x 80 templates + 1: ragged against 256 rows and against the template count
    probes: Tuple[int, ...] = (0, 1, 120, 239, 240)

    @property
    def rows(self) -> int:
        return self.prompts * self.cfg.context_length


STD = (("SegEarth", True), ("Experimental", True))
VISION_CASES = {c.name: c for c in (
    VisionCase("V1", Wt.VIT_CONFIGS["ViT-B-16"], 224, 84, "fixture", STD),
    VisionCase("V2", Wt.VIT_CONFIGS["ViT-B-16"], 512, 17, "fixture", STD),
    VisionCase("V3", Wt.VIT_CONFIGS["ViT-L-14"], 512, 17, "fixture", STD),
    # the H/14 width (dh = 80, exact GELU) at four layers: block 0 without a hand-off, the mid-layer similarity tap, the statistics
    # block L-2 and the last block
    VisionCase("V4", Wt.VitConfig("launch-h14-4l", 1280, 4, 16, 14, 1024, quick_gelu=False), 224, 33, "vit",
               (("Experimental", True), ("Experimental", False))),
    # GEM at depth 7 on eight layers: two ordinary blocks, then six dual-stream blocks
    VisionCase("V5", Wt.VitConfig("launch-b16-8l", 768, 8, 12, 16, 512), 224, 84, "gem", (("GEM", True), ("GEM", False))),
)}
TEXT_CASES = {c.name: c for c in (
    TextCase("T1", Wt.TEXT_CONFIGS["ViT-B-16"]),
    TextCase("T2", Wt.TEXT_CONFIGS["ViT-L-14"]),
    TextCase("T3", Wt.TextConfig("launch-h14-2l-text", 1024, 2, 16, 1024, quick_gelu=False)),
)}
# what the case table states, to be checked against the properties above
TABLE = {"V1": (197, 84, 16548), "V2": (1025, 17, 17425), "V3": (1370, 17, 23290), "V4": (257, 33, 8481), "V5": (197, 84, 16548),
         "T1": (77, 241, 18557), "T2": (77, 241, 18557), "T3": (77, 241, 18557)}


def rule_widths(case):
    return (case.cfg.width, case.cfg.embed_dim)


def rule_holds(case, cu_count: int, rows: int | None = None) -> bool:
    """gemm_bf16_prefers_persistent(R, N) for N = width and N = embed_dim."""
    R = case.rows if rows is None else rows
    return all(gemm_prefers_persistent(R, N, cu_count) for N in rule_widths(case))


def small_rows(case) -> int:
    """The launch size the one-tile / 24-prompt tests run the same tower at."""
    return case.tokens if isinstance(case, VisionCase) else 24 * case.cfg.context_length


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def probe_indices(B: int):
    return (0, B // 2, B - 1)


def _tile(case: VisionCase, seed: int) -> torch.Tensor:
    img = torch.from_numpy(Wt.normalize_tiles(Wt.make_tiles_u8(1, case.tile, seed=seed, smooth=True)))
    pad = OS.compute_padsize(case.tile, case.tile, case.cfg.patch)
    return F.pad(img, pad) if any(pad) else img


def probe_tile(case: VisionCase) -> torch.Tensor:
    """[1, 3, S', S'] f32: the tile test_real_size_parity_f32 builds, normalised and padded to the patch size."""
    return _tile(case, PROBE_SEED)


def filler_seed(case: VisionCase, i: int) -> int:
    return 50000 + 1000 * sorted(VISION_CASES).index(case.name) + i


def vision_batch(case: VisionCase) -> torch.Tensor:
    """[B, 3, S', S'] f32: the probe tile at indices 0, B // 2 and B - 1, every other tile from a seed of its own."""
    probe = probe_tile(case)
    at = probe_indices(case.batch)
    return torch.cat([probe if i in at else _tile(case, filler_seed(case, i)) for i in range(case.batch)], 0)


def prompt_ids(case: TextCase) -> np.ndarray:
    return Wt.make_token_ids(case.cfg, case.prompts)


# ---- references -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def vit_weights(cfg: Wt.VitConfig):
    return Wt.make_vit_weights(cfg, seed=0)


@functools.lru_cache(maxsize=2)
def text_weights(cfg: Wt.TextConfig):
    return Wt.make_text_weights(cfg, seed=0)


def text_features(case: VisionCase) -> torch.Tensor:
    return torch.from_numpy(Wt.make_text_features(len(POTSDAM_QIDX), case.cfg.embed_dim))


def fixture_keys(case: VisionCase, model_type: str):
    key = f"{case.cfg.name}.{case.tile}.{model_type}"
    return key + ".logits", key + ".argmax"


def seg_oracle(case: VisionCase, model_type: str, ignore_residual: bool) -> OS.SegOracle:
    """The oracle of one variant, with the knobs real_logits.npz was minted with (oracle/gen_golden.py gen_real); GEM takes no refiner."""
    gem = model_type == "GEM"
    return OS.SegOracle(case.cfg, OV.to_torch(vit_weights(case.cfg)), text_features(case), torch.tensor(POTSDAM_QIDX), model_type=model_type,
                        ignore_residual=ignore_residual, global_debias_factor=0.2, similarity_cfg=None if gem else SIM,
                        outlier_cfg=None if gem else OUTLIER, prob_thd=0.1, bg_idx=5)


def oracle_logits(case: VisionCase, model_type: str, ignore_residual: bool, img: torch.Tensor) -> torch.Tensor:
    """Patch-grid logits [B, Q, g, g] of `img` [B, 3, S', S'] (oracle.vit.vit_forward / gem_forward behind SegOracle.forward_feature)."""
    with torch.no_grad():
        return seg_oracle(case, model_type, ignore_residual).forward_feature(img, (case.grid, case.grid))


def oracle_text(case: TextCase, ids: np.ndarray) -> torch.Tensor:
    with torch.no_grad():
        return OT.encode_text(text_weights(case.cfg), case.cfg, ids)
