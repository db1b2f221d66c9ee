"""The per-element GEMM bound of tests/gemm_reference.py has teeth (CPU only): an f32-accumulated emulation of the kernels' arithmetic
passes it, and each of the small, localised mistakes a tiled GEMM kernel can make fails it -- a dropped or misplaced 8-row x 64-K piece,
a K step counted twice, a tail tile's last row taken from the clamped row, truncation instead of round-to-nearest-even on the output."""
import math

import pytest
import torch

from gemm_reference import (LIPSCHITZ, act_f64, check_within, gemm_bound, gemm_reference, h2_delta, half_ulp, pack_h2,
                            unpack_h2)

# 3 x 2 tiles of 256 x 256; the last row tile holds 8 rows, the last column tile 8 columns; 4 K steps of 64
M, N, K, T, KS = 520, 264, 256, 256, 64


def operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    bias = torch.randn(N, generator=g) * 0.1
    return A, W, bias


def emulate_f32(A, W, bias, act=0):
    """The kernels' arithmetic in f32: per-K-step partial products (exact products, f32 sums) added in REVERSE step order, then bias and
    activation in f32 -- a different summation order from the f64 reference's and from any single matmul."""
    Af, Wf = A.float(), W.float()
    acc = torch.zeros(M, N, dtype=torch.float32)
    for k in reversed(range(0, K, KS)):
        acc = acc + Af[:, k:k + KS] @ Wf[:, k:k + KS].T
    v = acc + bias
    return act_f64(v.double(), act).float()


def piece(A, W, m0, n0, k0, rows=8):
    """The contribution of the 8-row x 64-K piece at (m0, k0) to output tile column n0, in f32."""
    return A[m0:m0 + rows, k0:k0 + KS].float() @ W[n0:n0 + T, k0:k0 + KS].float().T


def bound_for(A, W, bias, act, fmt):
    pre, out = gemm_reference(A, W, bias, None, act)
    return out, gemm_bound(A, W, bias, pre, out, act=act, out_fmt=fmt)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_emulation_passes(act, fmt):
    A, W, bias = operands()
    ref, bound = bound_for(A, W, bias, act, fmt)
    got = emulate_f32(A, W, bias, act)
    got = got if fmt == "f32" else got.bfloat16()
    ratio = check_within(got, ref, bound, "emulation")
    print(f"emulation act={act} {fmt}: max err/bound {ratio:.3g}")
    assert ratio < 1


def _fails(got, ref, bound):
    with pytest.raises(AssertionError, match="outside the bound"):
        check_within(got, ref, bound, "mutant")


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_dropped_piece_fails(fmt):
    A, W, bias = operands(1)
    ref, bound = bound_for(A, W, bias, 0, fmt)
    got = emulate_f32(A, W, bias)
    got[264:272, 256:264] -= piece(A, W, 264, 256, 128)[:, :8]          # tile (1, 1), K step 2, rows 8-15 of the tile
    _fails(got if fmt == "f32" else got.bfloat16(), ref, bound)


def test_piece_from_neighbouring_tile_fails():
    A, W, bias = operands(2)
    ref, bound = bound_for(A, W, bias, 0, "bf16")
    got = emulate_f32(A, W, bias)
    # rows 16-23 of tile (0, 0) take K step 1 of the A rows of tile (1, 0) instead of their own
    got[16:24, 0:256] += piece(A, W, 256 + 16, 0, 64) - piece(A, W, 16, 0, 64)
    _fails(got.bfloat16(), ref, bound)


def test_k_step_counted_twice_fails():
    A, W, bias = operands(3)
    ref, bound = bound_for(A, W, bias, 1, "bf16")
    Af, Wf = A.float(), W.float()
    acc = Af @ Wf.T + Af[:, 192:256] @ Wf[:, 192:256].T                 # the last K step twice, everywhere
    got = act_f64((acc + bias).double(), 1).float().bfloat16()
    _fails(got, ref, bound)


def test_clamped_tail_row_fails():
    A, W, bias = operands(4)
    ref, bound = bound_for(A, W, bias, 0, "f32")
    got = emulate_f32(A, W, bias)
    got[M - 1] = got[M - 2]                                             # the tail tile's last row computed from the row before it
    _fails(got, ref, bound)


def test_truncated_bf16_output_fails():
    A, W, bias = operands(5)
    ref, bound = bound_for(A, W, bias, 0, "bf16")
    v = emulate_f32(A, W, bias)
    trunc = (v.view(torch.int32) & ~0xFFFF).view(torch.float32).bfloat16()   # drop the low 16 bits: round toward zero
    _fails(trunc, ref, bound)
    check_within(v.bfloat16(), ref, bound, "rne")                       # the same values rounded to nearest even pass


def test_lipschitz_constants():
    x = torch.linspace(-30, 30, 2_000_001, dtype=torch.float64)
    for act in (1, 2):
        y = act_f64(x, act)
        slope = ((y[1:] - y[:-1]) / (x[1:] - x[:-1])).abs().max().item()
        assert slope <= LIPSCHITZ[act], (act, slope)
        assert slope > LIPSCHITZ[act] - 0.04                               # and not far above it (the constants are the true peaks)


def test_half_ulp():
    v = torch.tensor([1.0, 1.5, 2.0 ** -14, 2.0 ** -20, 0.0, 3.0e38], dtype=torch.float64)
    assert half_ulp(v, "bf16").tolist()[:2] == [2.0 ** -8, 2.0 ** -8]
    assert half_ulp(v, "f16").tolist()[2:5] == [2.0 ** -25, 2.0 ** -25, 2.0 ** -25]     # the subnormal spacing below 2^-14
    assert half_ulp(v, "f32")[0].item() == 2.0 ** -24
    # every f16 / bf16 / f32 rounding of random data stays within half an ulp at the value
    # (f16 / bf16 from f32 values: torch rounds f64 -> f16 through f32, which can round twice)
    x = torch.randn(100_000, dtype=torch.float64) * torch.exp(torch.randn(100_000, dtype=torch.float64) * 8)
    for fmt, dt in (("f16", torch.float16), ("bf16", torch.bfloat16), ("f32", torch.float32)):
        xs = x.clamp(-60000, 60000).float().double() if fmt == "f16" else x.float().double() if fmt == "bf16" else x
        assert ((xs.to(dt).double() - xs).abs() <= half_ulp(xs.abs(), fmt)).all(), fmt


def test_two_plane_storage_and_small_magnitude_regime():
    """hi + lo of the two-plane storage is within max(2^-22 |x|, 2^-25) of x -- and below |x| = 2^-3 it is the absolute 2^-25 floor that
    holds, not 22 significant bits: at |x| ~ 1e-3 (lo an f16 subnormal) the error is far above 2^-22 |x| for many elements."""
    g = torch.Generator().manual_seed(7)
    for scale in (1.0, 1e-3):
        x = torch.randn(64, 1024, generator=g) * scale
        back = unpack_h2(pack_h2(x))
        err = (back - x.double()).abs()
        assert (err <= h2_delta(x.double())).all()
        rel = err > 2.0 ** -22 * x.double().abs()
        assert not rel[x.abs() >= 2.0 ** -3].any()                          # 22 significant bits from |x| = 2^-3 up
        if scale == 1e-3:
            assert rel.float().mean().item() > 0.5                          # the 2^-25 floor, i.e. ~15 bits at |x| ~ 1e-3
    # storage layout: element 8g + i at f16 index 16g + i (hi) and 16g + 8 + i (lo)
    x = torch.arange(16, dtype=torch.float32) + 1 / 3
    p = pack_h2(x)
    assert torch.equal(p[0:8], x[0:8].half()) and torch.equal(p[16:24], x[8:16].half())
    assert torch.equal(p[8:16], (x[0:8] - x[0:8].half().float()).half())
    assert math.isclose(float(unpack_h2(p)[9]), float(x[9]), rel_tol=2.0 ** -22)
