"""The object-match entries at the drop-in boundary, without a GPU: include/segearth_hip.h declares them, the library exports them, the
ctypes table carries them with the header's parameter counts and types, sg_object_match refuses what its contract lists through the error
channel before any device work, the option checks of ops and ObjectMetric raise before any library call, evaluate keeps its default
signature, and metrics_from_objects turns hand-made tables into the scores."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
NEW = {"sg_object_workspace_bytes": 1, "sg_object_match": 20}


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
    from clip_decontamination_amd import build
    assert "objmatch.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "objmatch.hip"))


def test_ctypes_table_matches_the_header():
    from clip_decontamination_amd import _lib
    protos = _prototypes()
    for name, n in NEW.items():
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype(protos[name][0]) and len(args) == n
        assert args == [_ctype(p) for p in protos[name][1]], (name, protos[name])


def _call(lib, labels, gt, fmt, hw, off, N, K, conn, min_area, num, den, counts, mm, ws, nbytes, skip=0, use_skip=0):
    return lib.sg_object_match(labels, gt, fmt, hw, off, N, K, conn, min_area, skip, use_skip, num, den, 255, 0, counts, mm, ws, nbytes, None)


def test_entry_refuses_before_any_device_work():
    """Every refusal of the contract, with pointers that are never followed: the checks read only the host arrays."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(1 << 20)                                  # non-null, aligned, never followed
    odd = ctypes.c_void_p((1 << 20) + 4)
    I32, I64 = ctypes.c_int32, ctypes.c_int64

    def m(labels=one, gt=one, fmt=_lib.GT_U8, hw=(4, 5), off=0, N=1, K=3, conn=4, area=1, iou=(1, 2), counts=one, mm=one, ws=one, nbytes=1 << 20,
          arrays=(1, 1)):
        a = [(I32 * 2)(*hw), (I64 * 1)(off)]
        a = [x if keep else None for x, keep in zip(a, arrays)]
        return _call(lib, labels, gt, fmt, a[0], a[1], N, K, conn, area, iou[0], iou[1], counts, mm, ws, nbytes)

    cases = [
        (lambda: m(labels=None), "null pointer"), (lambda: m(gt=None), "null pointer"), (lambda: m(counts=None), "null pointer"),
        (lambda: m(ws=None), "null pointer"), (lambda: m(arrays=(0, 1)), "null pointer"), (lambda: m(arrays=(1, 0)), "null pointer"),
        (lambda: m(fmt=-1), "format"), (lambda: m(fmt=2), "format"),
        (lambda: m(N=0), "N=0"), (lambda: m(N=-1), "N=-1"), (lambda: m(hw=(4, 0)), "non-positive"), (lambda: m(hw=(-4, 5)), "non-positive"),
        (lambda: m(hw=(1 << 15, 1 << 16)), "2^31"), (lambda: m(off=3), "offset"), (lambda: m(off=-1), "offset"),
        (lambda: m(K=0), "K=0"), (lambda: m(K=128), "K=128"), (lambda: m(conn=6), "connectivity=6"), (lambda: m(conn=0), "connectivity=0"),
        (lambda: m(area=0), "min_area=0"), (lambda: m(area=-3), "min_area=-3"),
        (lambda: m(iou=(0, 1)), "threshold 0 / 1"), (lambda: m(iou=(1, 1)), "threshold 1 / 1"), (lambda: m(iou=(3, 2)), "threshold 3 / 2"),
        (lambda: m(iou=(1 << 20, (1 << 20) + 1)), "2^20"), (lambda: m(iou=(49, 100)), "below 1/2"), (lambda: m(iou=(1, 3)), "below 1/2"),
        (lambda: m(iou=(-1, 2)), "threshold -1 / 2"),
        (lambda: m(labels=odd), "aligned"), (lambda: m(counts=odd), "aligned"), (lambda: m(gt=odd, fmt=_lib.GT_I64), "aligned"),
        (lambda: m(ws=odd), "aligned"),
        (lambda: m(nbytes=36 * 20 + 2 * 256 - 1), "workspace too small"), (lambda: m(nbytes=0), "workspace too small"),
    ]
    for fn, word in cases:
        rc = fn()
        err = lib.sg_last_error().decode()
        assert rc == -1 and word in err, (word, rc, err)
        assert "sg_object_match" in err, err
    # a uint8 truth and a null match_map at odd addresses are fine: the next refusal is the workspace
    assert m(gt=odd, mm=None, nbytes=8) == -1 and "workspace too small" in lib.sg_last_error().decode()
    # the workspace: 36 bytes per pixel and two planes of the call's pixels rounded up to 256; 0 for a negative count
    W = lib.sg_object_workspace_bytes
    assert (W(0), W(1), W(20), W(256), W(257), W(-1), W(-(1 << 40))) == (0, 36 + 512, 36 * 20 + 512, 36 * 256 + 512, 36 * 257 + 1024, 0, 0)
    assert W((1 << 31) - 1) == 36 * ((1 << 31) - 1) + 2 * (1 << 31)


def test_refused_call_leaves_counts_and_map_untouched():
    """Counts and match_map live in host memory here: a refused call never follows the pointers, so the bytes stay."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    counts = (ctypes.c_int64 * 12)(*range(100, 112))
    mm = (ctypes.c_uint8 * 20)(*range(20))
    one = ctypes.c_void_p(1 << 20)
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    for kw in (dict(iou=(1, 3)), dict(K=128), dict(conn=5), dict(N=0), dict(hw=(0, 5)), dict(nbytes=16), dict(area=0), dict(fmt=7), dict(off=1)):
        a = dict(hw=(4, 5), N=1, K=3, conn=4, area=1, iou=(1, 2), nbytes=1 << 20, fmt=_lib.GT_U8, off=0)
        a.update(kw)
        rc = _call(lib, one, one, a["fmt"], (I32 * 2)(*a["hw"]), (I64 * 1)(a["off"]), a["N"], a["K"], a["conn"], a["area"], a["iou"][0], a["iou"][1],
                   ctypes.cast(counts, ctypes.c_void_p), ctypes.cast(mm, ctypes.c_void_p), one, a["nbytes"])
        assert rc == -1, kw
        assert list(counts) == list(range(100, 112)) and list(mm) == list(range(20)), kw


def test_images_must_not_overlap():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(1 << 20)
    hw = (ctypes.c_int32 * 4)(4, 5, 2, 3)
    for offs in ((0, 10), (0, 19), (0, 21), (6, 0), (0, 0)):
        off = (ctypes.c_int64 * 2)(*offs)
        assert _call(lib, one, one, _lib.GT_U8, hw, off, 2, 3, 4, 1, 1, 2, one, None, one, 1 << 20) == -1, offs
        assert "offset[" in lib.sg_last_error().decode()


def test_ops_refuse_before_any_library_call(monkeypatch):
    from clip_decontamination_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was loaded before the option checks")

    monkeypatch.setattr(_lib, "load", no_library)
    assert ops.OBJECT_MAX_K == 127 and ops.OBJECT_MAX_DEN == 1 << 20 and ops.OBJECT_SQ_ONE == 1 << 24
    p = inspect.signature(ops.object_match).parameters
    assert list(p) == ["labels", "gt", "image_hw", "counts", "K", "iou", "connectivity", "min_area", "skip_label", "ignore_index",
                       "reduce_zero_label", "match_map"]
    assert (p["iou"].default, p["connectivity"].default, p["min_area"].default, p["skip_label"].default, p["ignore_index"].default,
            p["reduce_zero_label"].default, p["match_map"].default) == ((1, 2), 4, 1, None, 255, False, None)
    F = ops.object_iou_fraction
    assert (F(0.5), F(0.6), F(0.75), F((3, 4)), F((6, 8)), F([1, 2]), F(0.999999), F((1048575, 1048576))) == \
        ((1, 2), (3, 5), (3, 4), (3, 4), (3, 4), (1, 2), (999999, 1000000), (1048575, 1048576))
    for t in (0.49, 1.0, 0, 1, 2.5, -0.5, (1, 3), (2, 2), (3, 2), (0, 1)):
        with pytest.raises(ValueError, match="outside"):
            F(t)
    for t in (0.9999999, (1048576, 1048577)):
        with pytest.raises(ValueError, match="denominator"):
            F(t)
    for t in (float("nan"), float("inf"), "0.5", None, True, (1, 2, 3), (0.5, 1), (1, 0), (True, 2)):
        with pytest.raises(ValueError, match="object_iou"):
            F(t)
    lab = torch.zeros(4, 5, dtype=torch.int64)
    flat, counts = lab.view(-1), torch.zeros(4, 3, dtype=torch.int64)
    for iou in (0.49, 1.0, (1, 3), "x"):
        with pytest.raises(ValueError, match="object_iou"):
            ops.object_match(flat, flat, [(4, 5)], counts, 3, iou)
    for c in (6, 0, True, None):
        with pytest.raises(ValueError, match="connectivity"):
            ops.object_match(flat, flat, [(4, 5)], counts, 3, connectivity=c)
    for a in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_area"):
            ops.object_match(flat, flat, [(4, 5)], counts, 3, min_area=a)
    for s in (1.0, True, "bg"):
        with pytest.raises(ValueError, match="skip_label"):
            ops.object_match(flat, flat, [(4, 5)], counts, 3, skip_label=s)
    for K in (0, 128, 2.0, True):
        with pytest.raises(ValueError, match="K="):
            ops.object_match(flat, flat, [(4, 5)], torch.zeros(4, 128, dtype=torch.int64), K)
    with pytest.raises(ValueError, match="images of sizes"):
        ops.object_match(flat, flat, [(4, 6)], counts, 3)
    with pytest.raises(ValueError, match="positive size"):
        ops.object_match(flat, flat, [(0, 5)], counts, 3)
    with pytest.raises(ValueError, match="positive size"):
        ops.object_match(flat, flat, [], counts, 3)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.object_match(flat, flat, [(1 << 15, 1 << 16)], counts, 3)
    with pytest.raises(ValueError, match="counts"):
        ops.object_match(flat, flat, [(4, 5)], torch.zeros(3, 3, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="counts"):
        ops.object_match(flat, flat, [(4, 5)], torch.zeros(4, 3, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="match_map"):
        ops.object_match(flat, flat, [(4, 5)], counts, 3, match_map=torch.zeros(19, dtype=torch.uint8))
    with pytest.raises(ValueError, match="match_map"):
        ops.object_match(flat, flat, [(4, 5)], counts, 3, match_map=torch.zeros(20, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.object_match(flat.to(torch.int32), flat, [(4, 5)], counts, 3)
    with pytest.raises(TypeError):
        ops.object_match(flat, flat.float(), [(4, 5)], counts, 3)
    # with every option in order the next refusal is the missing device: no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.object_match(flat, flat, [(4, 5)], counts, 3, 0.75, 8, 2, 0, match_map=torch.zeros(20, dtype=torch.uint8))


def test_metric_options(monkeypatch):
    from clip_decontamination_amd import _lib, metrics
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    M = metrics.ObjectMetric
    assert issubclass(M, metrics.IoUMetric)
    sig = inspect.signature(M.__init__).parameters
    assert (sig["object_iou"].default, sig["min_area"].default, sig["connectivity"].default, sig["skip_label"].default) == (0.5, 1, 4, None)
    for kw in (dict(object_iou=0.49), dict(object_iou=1.0), dict(object_iou=(1, 3)), dict(object_iou="x"), dict(object_iou=None)):
        with pytest.raises(ValueError, match="object_iou"):
            M(num_classes=3, **kw)
    for kw in (dict(min_area=0), dict(min_area=2.0), dict(min_area=True)):
        with pytest.raises(ValueError, match="min_area"):
            M(num_classes=3, **kw)
    with pytest.raises(ValueError, match="connectivity"):
        M(num_classes=3, connectivity=6)
    with pytest.raises(ValueError, match="skip_label"):
        M(num_classes=3, skip_label=0.0)
    with pytest.raises(ValueError, match="num_classes"):
        M(num_classes=128)
    with pytest.raises(KeyError):
        M(num_classes=3, iou_metrics=["mAP"])                       # IoUMetric's own checks still hold
    m = M(num_classes=3, object_iou=0.6, min_area=4, connectivity=8, skip_label=0)
    assert (m.object_iou, m.min_area, m.connectivity, m.skip_label) == ((3, 5), 4, 8, 0)
    m = M(num_classes=3)
    assert m.object_iou == (1, 2)
    assert tuple(m.object_counts.shape) == (4, 3) and m.object_counts.dtype == torch.int64 and not m.object_counts.any()
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
    assert torch.equal(m.confusion, t) and not m.object_counts.any()
    out = m.compute()
    assert set(out) == set(metrics.metrics_from_confusion(t)) | {"ObjPrecision", "ObjRecall", "ObjF1", "SQ", "PQ"}
    assert {"mIoU", "mObjPrecision", "mObjRecall", "mObjF1", "mSQ", "mPQ"} <= set(out["summary"])
    m.reset()
    assert not m.confusion.any() and not m.object_counts.any()


def test_metrics_from_objects_on_hand_tables():
    from clip_decontamination_amd.metrics import metrics_from_objects
    one = 1 << 24
    #                  class 0       class 1   class 2 (never predicted)  class 3 (absent)  class 4 (nothing matched)
    counts = np.array([[2, 4, 0, 0, 0],
                       [4, 4, 0, 0, 5],
                       [2, 8, 6, 0, 5],
                       [3 * one // 2, 4 * one, 0, 0, 0]], dtype=np.int64)
    out = metrics_from_objects(counts)
    assert np.array_equal(out["ObjPrecision"], [0.5, 1.0, np.nan, np.nan, 0.0], equal_nan=True)
    assert np.array_equal(out["ObjRecall"], [1.0, 0.5, 0.0, np.nan, 0.0], equal_nan=True)
    assert np.array_equal(out["ObjF1"], [4 / 6, 8 / 12, 0.0, np.nan, 0.0], equal_nan=True)
    assert np.array_equal(out["SQ"], [0.75, 1.0, np.nan, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(out["PQ"], [0.75 * (4 / 6), 8 / 12, np.nan, np.nan, np.nan], equal_nan=True)
    assert out["summary"] == {"mObjPrecision": 50.0, "mObjRecall": 37.5, "mObjF1": float(np.round((4 / 6 + 8 / 12) / 4 * 100, 2)),
                              "mSQ": 87.5, "mPQ": float(np.round((0.5 + 8 / 12) / 2 * 100, 2))}
    assert all(v.dtype == np.float64 for k, v in out.items() if k != "summary")
    t = metrics_from_objects(torch.from_numpy(counts))
    assert all(np.array_equal(t[k], out[k], equal_nan=True) for k in out if k != "summary") and t["summary"] == out["summary"]
    z = metrics_from_objects(counts, nan_to_num=0)
    assert z["ObjPrecision"].tolist() == [0.5, 1.0, 0.0, 0.0, 0.0] and z["summary"]["mObjPrecision"] == 30.0
    empty = metrics_from_objects(np.zeros((4, 2), dtype=np.int64))
    assert all(np.isnan(v) for v in empty["summary"].values())
    for bad in (np.zeros((3, 2), dtype=np.int64), np.zeros((4,), dtype=np.int64), np.zeros((4, 0), dtype=np.int64)):
        with pytest.raises(ValueError):
            metrics_from_objects(bad)
    with pytest.raises(TypeError):
        metrics_from_objects(np.zeros((4, 2)))


def test_evaluate_keeps_its_defaults():
    import segearth_segmentor
    import segmentor
    for cls in (segmentor.SegmentorEx, segearth_segmentor.Segmentor):
        p = inspect.signature(cls.evaluate).parameters
        assert list(p)[:13] == ["self", "inputs", "gt_maps", "metric", "reduce_zero_label", "ignore_index", "iou_metrics", "at_gt_size",
                                "boundary_ratio", "boundary_px", "relaxed_px", "relaxed_ratio", "relaxed_mode"]
        assert (p["metric"].default, p["reduce_zero_label"].default, p["ignore_index"].default, p["iou_metrics"].default,
                p["at_gt_size"].default) == (None, False, 255, ("mIoU",), False)
        assert p["boundary_ratio"].default is None and p["boundary_px"].default is None
        assert (p["relaxed_px"].default, p["relaxed_ratio"].default, p["relaxed_mode"].default) == (None, None, "region")
        assert (p["object_iou"].default, p["object_min_area"].default, p["object_include_bg"].default) == (None, 1, False)
