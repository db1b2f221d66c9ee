"""The tolerant-matching entries at the drop-in boundary, without a GPU: include/segearth_hip.h declares them, the library exports them,
the ctypes table carries them with the header's parameter counts and types, sg_tolerant_accumulate refuses what its contract lists through
the error channel before any device work, the option checks of ops and RelaxedMetric raise before any library call, evaluate keeps its
default signature, and metrics_from_tolerant turns hand-made tables into the scores."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
NEW = {"sg_tolerant_workspace_bytes": 2, "sg_tolerant_accumulate": 15}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name in NEW:
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        out[name] = None if m is None else (m.group(1), [p.strip() for p in m.group(2).split(",")])
    return out


def _ctype(param: str):
    if "*" in param or param.startswith("sg_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}[param.split()[0]]


def test_header_declares_and_library_exports_the_entries():
    from clip_decontamination_amd import _lib
    protos = _prototypes()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in NEW.items():
        assert protos[name] is not None, f"{name} is not declared in the header"
        assert len(protos[name][1]) == n, (name, protos[name])
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    src = open(HEADER).read()
    assert re.search(r"#define\s+SG_TOL_REGION\s+0\b", src) and re.search(r"#define\s+SG_TOL_CONTOUR\s+1\b", src)
    assert (_lib.TOL_REGION, _lib.TOL_CONTOUR) == (0, 1)


def test_ctypes_table_matches_the_header():
    from clip_decontamination_amd import _lib
    protos = _prototypes()
    for name, n in NEW.items():
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype(protos[name][0]) and len(args) == n
        assert args == [_ctype(p) for p in protos[name][1]], (name, protos[name])


def test_entry_refuses_before_any_device_work():
    """Every refusal of the contract, with pointers that are never followed: the checks read only the host arrays."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(1 << 20)                                  # non-null, aligned, never followed
    odd = ctypes.c_void_p((1 << 20) + 4)
    I32, I64 = ctypes.c_int32, ctypes.c_int64

    def acc(labels=one, gt=one, fmt=_lib.GT_U8, hw=(4, 5), off=0, tol=9, N=1, K=3, mode=0, counts=one, ws=one, nbytes=1 << 20, arrays=(1, 1, 1)):
        a = [(I32 * 2)(*hw), (I64 * 1)(off), (I32 * 1)(tol)]
        a = [x if keep else None for x, keep in zip(a, arrays)]
        return lib.sg_tolerant_accumulate(labels, gt, fmt, *a, N, K, mode, 255, 0, counts, ws, nbytes, None)

    cases = [
        (lambda: acc(labels=None), "null pointer"), (lambda: acc(gt=None), "null pointer"), (lambda: acc(counts=None), "null pointer"),
        (lambda: acc(ws=None), "null pointer"), (lambda: acc(arrays=(0, 1, 1)), "null pointer"), (lambda: acc(arrays=(1, 0, 1)), "null pointer"),
        (lambda: acc(arrays=(1, 1, 0)), "null pointer"),
        (lambda: acc(fmt=-1), "format"), (lambda: acc(fmt=2), "format"), (lambda: acc(mode=2), "mode"), (lambda: acc(mode=-1), "mode"),
        (lambda: acc(N=0), "N=0"), (lambda: acc(N=-1), "N=-1"), (lambda: acc(hw=(4, 0)), "non-positive"), (lambda: acc(hw=(-4, 5)), "non-positive"),
        (lambda: acc(hw=(1 << 15, 1 << 16)), "2^31"), (lambda: acc(tol=-1), "tol_sq[0]=-1"), (lambda: acc(tol=254 * 254 + 1), "tol_sq[0]=64517"),
        (lambda: acc(K=0), "K=0"), (lambda: acc(K=128), "K=128"), (lambda: acc(off=3), "offset"), (lambda: acc(off=-1), "offset"),
        (lambda: acc(labels=odd), "aligned"), (lambda: acc(counts=odd), "aligned"), (lambda: acc(gt=odd, fmt=_lib.GT_I64), "aligned"),
        (lambda: acc(nbytes=3 * 256 - 1), "workspace too small"), (lambda: acc(K=9, nbytes=8 * 256 - 1), "workspace too small"),
    ]
    for fn, word in cases:
        rc = fn()
        err = lib.sg_last_error().decode()
        assert rc == -1 and word in err, (word, rc, err)
        assert "sg_tolerant_accumulate" in err, err
    # the workspace: min(K, 8) planes of the call's pixels, each rounded up to 256; 0 for a negative count or a K outside [1, 127]
    W = lib.sg_tolerant_workspace_bytes
    assert (W(20, 1), W(20, 3), W(20, 8), W(20, 9), W(20, 127)) == (256, 3 * 256, 8 * 256, 8 * 256, 8 * 256)
    assert (W(257, 5), W(0, 5)) == (5 * 512, 0)
    assert (W(-1, 5), W(20, 0), W(20, 128), W(20, -3)) == (0, 0, 0, 0)


def test_refused_call_leaves_the_counts_untouched():
    """The counts live in host memory here: a refused call never follows the pointer, so the bytes stay."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    counts = (ctypes.c_int64 * 12)(*range(100, 112))
    one = ctypes.c_void_p(1 << 20)
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    for kw in (dict(tol=-1), dict(K=128), dict(mode=5), dict(N=0), dict(hw=(0, 5)), dict(nbytes=16)):
        a = dict(hw=(4, 5), tol=9, N=1, K=3, mode=0, nbytes=1 << 20)
        a.update(kw)
        rc = lib.sg_tolerant_accumulate(one, one, _lib.GT_U8, (I32 * 2)(*a["hw"]), (I64 * 1)(0), (I32 * 1)(a["tol"]), a["N"], a["K"], a["mode"],
                                        255, 0, ctypes.cast(counts, ctypes.c_void_p), one, a["nbytes"], None)
        assert rc == -1, kw
        assert list(counts) == list(range(100, 112)), kw


def test_images_must_not_overlap():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(1 << 20)
    hw = (ctypes.c_int32 * 4)(4, 5, 2, 3)
    tol = (ctypes.c_int32 * 2)(1, 4)
    for offs in ((0, 10), (0, 19), (0, 21), (6, 0), (0, 0)):
        off = (ctypes.c_int64 * 2)(*offs)
        assert lib.sg_tolerant_accumulate(one, one, _lib.GT_U8, hw, off, tol, 2, 3, 0, 255, 0, one, one, 1 << 20, None) == -1, offs
        assert "offset[" in lib.sg_last_error().decode()
    bad = (ctypes.c_int32 * 2)(1, 254 * 254 + 1)                     # the second image's tolerance
    assert lib.sg_tolerant_accumulate(one, one, _lib.GT_U8, hw, (ctypes.c_int64 * 2)(0, 20), bad, 2, 3, 0, 255, 0, one, one, 1 << 20, None) == -1
    assert "tol_sq[1]" in lib.sg_last_error().decode()


def test_ops_refuse_before_any_library_call(monkeypatch):
    from clip_decontamination_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was loaded before the option checks")

    monkeypatch.setattr(_lib, "load", no_library)
    assert ops.TOLERANT_MAX_SQ == 254 * 254 and ops.TOLERANT_MAX_K == 127
    assert inspect.signature(ops.tolerance_sq).parameters["ratio"].default == 0.0075
    p = inspect.signature(ops.tolerant_accumulate).parameters
    assert (p["ignore_index"].default, p["reduce_zero_label"].default, p["mode"].default) == (255, False, "region")
    assert (ops.tolerance_sq((2048, 4608)), ops.tolerance_sq((512, 512)), ops.tolerance_sq((1, 1))) == (38 * 38, 36, 1)
    assert ops.tolerance_sq((300, 400), 0.0101) == 36
    for ratio in (0, -1.0, float("nan"), float("inf"), "x", True, None):
        with pytest.raises(ValueError, match="tolerance_ratio"):
            ops.tolerance_sq((4, 5), ratio)
    with pytest.raises(ValueError, match="above the limit of 254"):
        ops.tolerance_sq((3000, 4000), 0.051)                       # 255 px
    assert ops.tolerance_sq((3000, 4000), 0.05079) == 254 * 254    # the ceiling of 253.95
    with pytest.raises(ValueError, match="size"):
        ops.tolerance_sq((0, 5))
    lab = torch.zeros(4, 5, dtype=torch.int64)
    flat, counts = lab.view(-1), torch.zeros(4, 3, dtype=torch.int64)
    for t in (-1, 254 * 254 + 1, 1.5, True, None, "2"):
        with pytest.raises(ValueError, match="squared tolerance"):
            ops.tolerant_accumulate(flat, flat, [(4, 5)], t, counts, 3)
    with pytest.raises(ValueError, match="tolerances"):
        ops.tolerant_accumulate(flat, flat, [(4, 5)], [1, 2], counts, 3)
    with pytest.raises(ValueError, match="mode"):
        ops.tolerant_accumulate(flat, flat, [(4, 5)], 4, counts, 3, mode="band")
    for K in (0, 128):
        with pytest.raises(ValueError, match="K="):
            ops.tolerant_accumulate(flat, flat, [(4, 5)], 4, torch.zeros(4, max(K, 1), dtype=torch.int64), K)
    with pytest.raises(ValueError, match="images of sizes"):
        ops.tolerant_accumulate(flat, flat, [(4, 6)], 4, counts, 3)
    with pytest.raises(ValueError, match="positive size"):
        ops.tolerant_accumulate(flat, flat, [(0, 5)], 4, counts, 3)
    with pytest.raises(ValueError, match="positive size"):
        ops.tolerant_accumulate(flat, flat, [], 4, counts, 3)
    with pytest.raises(ValueError, match="counts"):
        ops.tolerant_accumulate(flat, flat, [(4, 5)], 4, torch.zeros(3, 3, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="counts"):
        ops.tolerant_accumulate(flat, flat, [(4, 5)], 4, torch.zeros(4, 3, dtype=torch.int32), 3)
    with pytest.raises(TypeError):
        ops.tolerant_accumulate(flat.to(torch.int32), flat, [(4, 5)], 4, counts, 3)
    with pytest.raises(TypeError):
        ops.tolerant_accumulate(flat, flat.float(), [(4, 5)], 4, counts, 3)
    # with every option in order the next refusal is the missing device: no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tolerant_accumulate(flat, flat, [(4, 5)], 0, counts, 3, mode="contour")


def test_metric_options(monkeypatch):
    from clip_decontamination_amd import _lib, metrics
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    M = metrics.RelaxedMetric
    assert issubclass(M, metrics.IoUMetric)
    sig = inspect.signature(M.__init__).parameters
    assert (sig["mode"].default, sig["tolerance_px"].default, sig["tolerance_ratio"].default) == ("region", None, 0.0075)
    for kw in (dict(tolerance_px=-1), dict(tolerance_px=255), dict(tolerance_px=2.0), dict(tolerance_px=True)):
        with pytest.raises(ValueError, match="tolerance_px"):
            M(num_classes=3, **kw)
    for kw in (dict(tolerance_ratio=0), dict(tolerance_ratio=-1.0), dict(tolerance_ratio=float("nan")), dict(tolerance_ratio="x")):
        with pytest.raises(ValueError, match="tolerance_ratio"):
            M(num_classes=3, **kw)
    with pytest.raises(ValueError, match="mode"):
        M(num_classes=3, mode="band")
    with pytest.raises(ValueError, match="num_classes"):
        M(num_classes=128)
    with pytest.raises(KeyError):
        M(num_classes=3, iou_metrics=["mAP"])                       # IoUMetric's own checks still hold
    m = M(num_classes=3, tolerance_px=3, tolerance_ratio=0.5)
    assert m.tolerance_sq((512, 512)) == 9                          # a fixed tolerance overrides the ratio
    assert M(num_classes=3, tolerance_px=0).tolerance_sq((9, 9)) == 0 and M(num_classes=3, tolerance_px=254).tolerance_sq((9, 9)) == 254 * 254
    m = M(num_classes=3)
    assert (m.tolerance_sq((512, 512)), m.tolerance_sq((2048, 4608)), m.tolerance_sq((1, 1))) == (36, 38 * 38, 1)
    assert tuple(m.tolerant_counts.shape) == (4, 3) and m.tolerant_counts.dtype == torch.int64 and not m.tolerant_counts.any()
    assert tuple(m.confusion.shape) == (4, 4)
    lab = torch.zeros(4, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="add_flat"):
        m.add(lab.view(-1), lab.view(-1))
    with pytest.raises(ValueError, match="differ in size"):
        m.add(lab, torch.zeros(5, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="images of sizes"):
        m.add_flat(lab.view(-1), lab.view(-1), [(4, 6)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(lab, lab)
    t = torch.arange(16, dtype=torch.int64).view(4, 4)
    m.add_confusion(t)                                              # unchanged: the confusion table only
    assert torch.equal(m.confusion, t) and not m.tolerant_counts.any()
    out = m.compute()
    assert set(out) == set(metrics.metrics_from_confusion(t)) | {"RelPrecision", "RelRecall", "RelFscore"}
    assert {"mIoU", "mRelPrecision", "mRelRecall", "mRelFscore"} <= set(out["summary"])
    c = M(num_classes=3, mode="contour")
    c.add_confusion(t)
    out = c.compute()
    assert {"BPrecision", "BRecall", "BFscore"} <= set(out) and {"mIoU", "mBPrecision", "mBRecall", "mBF"} <= set(out["summary"])
    m.reset()
    assert not m.confusion.any() and not m.tolerant_counts.any()


def test_metrics_from_tolerant_on_hand_tables():
    from clip_decontamination_amd.metrics import metrics_from_tolerant
    #                  class 0  class 1  class 2 (never predicted)  class 3 (absent)  class 4 (nothing right, nothing found)
    counts = np.array([[10, 4, 0, 0, 5],
                       [5, 4, 0, 0, 0],
                       [20, 8, 6, 0, 5],
                       [5, 2, 0, 0, 0]], dtype=np.int64)
    out = metrics_from_tolerant(counts, "region")
    assert np.array_equal(out["RelPrecision"], [0.5, 1.0, np.nan, np.nan, 0.0], equal_nan=True)
    assert np.array_equal(out["RelRecall"], [0.25, 0.25, 0.0, np.nan, 0.0], equal_nan=True)
    assert np.allclose(out["RelFscore"][:2], [2 * 0.5 * 0.25 / 0.75, 2 * 0.25 / 1.25], rtol=0, atol=1e-15) and np.isnan(out["RelFscore"][2:]).all()
    assert out["summary"] == {"mRelPrecision": 50.0, "mRelRecall": 12.5, "mRelFscore": float(np.round((1 / 3 + 0.4) / 2 * 100, 2))}
    assert all(v.dtype == np.float64 for k, v in out.items() if k != "summary")
    b = metrics_from_tolerant(torch.from_numpy(counts), "contour")
    assert np.array_equal(b["BFscore"], out["RelFscore"], equal_nan=True) and np.array_equal(b["BPrecision"], out["RelPrecision"], equal_nan=True)
    assert b["summary"] == {"mBPrecision": 50.0, "mBRecall": 12.5, "mBF": out["summary"]["mRelFscore"]}
    z = metrics_from_tolerant(counts, "region", nan_to_num=0)
    assert z["RelPrecision"].tolist() == [0.5, 1.0, 0.0, 0.0, 0.0] and z["summary"]["mRelPrecision"] == 30.0
    empty = metrics_from_tolerant(np.zeros((4, 2), dtype=np.int64), "region")
    assert all(np.isnan(v) for v in empty["summary"].values())
    for bad in (np.zeros((3, 2), dtype=np.int64), np.zeros((4,), dtype=np.int64), np.zeros((4, 0), dtype=np.int64)):
        with pytest.raises(ValueError):
            metrics_from_tolerant(bad)
    with pytest.raises(TypeError):
        metrics_from_tolerant(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="mode"):
        metrics_from_tolerant(counts, "band")


def test_evaluate_keeps_its_defaults():
    import segearth_segmentor
    import segmentor
    for cls in (segmentor.SegmentorEx, segearth_segmentor.Segmentor):
        p = inspect.signature(cls.evaluate).parameters
        assert list(p)[:10] == ["self", "inputs", "gt_maps", "metric", "reduce_zero_label", "ignore_index", "iou_metrics", "at_gt_size",
                                "boundary_ratio", "boundary_px"]
        assert (p["metric"].default, p["reduce_zero_label"].default, p["ignore_index"].default, p["iou_metrics"].default,
                p["at_gt_size"].default) == (None, False, 255, ("mIoU",), False)
        assert p["boundary_ratio"].default is None and p["boundary_px"].default is None
        assert (p["relaxed_px"].default, p["relaxed_ratio"].default, p["relaxed_mode"].default) == (None, None, "region")
