"""The Boundary IoU entries at the drop-in boundary, without a GPU: include/segearth_hip.h declares them, the library exports them, the
ctypes table carries them with the header's parameter counts and types, every entry refuses what its contract lists through the error
channel before any device work, the option checks of ops and BoundaryIoUMetric raise before any library call, and evaluate keeps its
default signature."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
NEW = {"sg_boundary_workspace_bytes": 1, "sg_boundary_band": 10, "sg_boundary_accumulate": 14}


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


def test_ctypes_table_matches_the_header():
    from clip_decontamination_amd import _lib
    protos = _prototypes()
    for name, n in NEW.items():
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype(protos[name][0]) and len(args) == n
        assert args == [_ctype(p) for p in protos[name][1]], (name, protos[name])


def test_entries_refuse_before_any_device_work():
    """Every refusal of the contract, with pointers that are never followed: the checks read only the host arrays."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(1 << 20)                                  # non-null, aligned, never followed
    I32, I64 = ctypes.c_int32, ctypes.c_int64

    def band(labels=one, fmt=_lib.GT_I64, hw=(4, 5), off=0, d=2, N=1, out=one, ws=one, nbytes=1 << 20, arrays=True):
        a = ((I32 * 2)(*hw), (I64 * 1)(off), (I32 * 1)(d)) if arrays else (None, None, None)
        return lib.sg_boundary_band(labels, fmt, *a, N, out, ws, nbytes, None)

    def acc(labels=one, gt=one, fmt=_lib.GT_U8, hw=(4, 5), off=0, d=2, N=1, K=3, areas=one, ws=one, nbytes=1 << 20, arrays=True):
        a = ((I32 * 2)(*hw), (I64 * 1)(off), (I32 * 1)(d)) if arrays else (None, None, None)
        return lib.sg_boundary_accumulate(labels, gt, fmt, *a, N, K, 255, 0, areas, ws, nbytes, None)

    cases = [
        (lambda: band(labels=None), "null pointer"), (lambda: band(out=None), "null pointer"), (lambda: band(ws=None), "null pointer"),
        (lambda: band(arrays=False), "null pointer"), (lambda: band(fmt=2), "format"), (lambda: band(N=0), "N=0"),
        (lambda: band(hw=(0, 5)), "non-positive"), (lambda: band(hw=(4, -1)), "non-positive"),
        (lambda: band(hw=(1 << 16, 1 << 15)), "2^31"), (lambda: band(d=0), "d[0]=0"), (lambda: band(d=4096), "d[0]=4096"),
        (lambda: band(off=1), "offset"), (lambda: band(off=-1), "offset"), (lambda: band(nbytes=19), "workspace too small"),
        (lambda: band(labels=ctypes.c_void_p((1 << 20) + 4)), "aligned"),
        (lambda: acc(labels=None), "null pointer"), (lambda: acc(gt=None), "null pointer"), (lambda: acc(areas=None), "null pointer"),
        (lambda: acc(ws=None), "null pointer"), (lambda: acc(arrays=False), "null pointer"), (lambda: acc(fmt=-1), "format"),
        (lambda: acc(N=0), "N=0"), (lambda: acc(hw=(4, 0)), "non-positive"), (lambda: acc(hw=(1 << 15, 1 << 16)), "2^31"),
        (lambda: acc(d=0), "d[0]=0"), (lambda: acc(d=4096), "d[0]=4096"), (lambda: acc(K=0), "K=0"), (lambda: acc(K=128), "K=128"),
        (lambda: acc(off=3), "offset"), (lambda: acc(nbytes=4 * 256 - 1), "workspace too small"),
        (lambda: acc(areas=ctypes.c_void_p((1 << 20) + 4)), "aligned"),
    ]
    for fn, word in cases:
        rc = fn()
        err = lib.sg_last_error().decode()
        assert rc == -1 and word in err, (word, rc, err)
        assert ("sg_boundary_band" in err) or ("sg_boundary_accumulate" in err), err
    assert lib.sg_boundary_workspace_bytes(-1) == 0
    assert lib.sg_boundary_workspace_bytes(20) == 4 * 256 and lib.sg_boundary_workspace_bytes(257) == 4 * 512
    assert lib.sg_boundary_workspace_bytes(0) == 0


def test_ops_refuse_before_any_library_call(monkeypatch):
    from clip_decontamination_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was loaded before the option checks")

    monkeypatch.setattr(_lib, "load", no_library)
    lab = torch.zeros(4, 5, dtype=torch.int64)
    for d in (0, -1, 4096, 1.5, True, None, "2"):
        with pytest.raises(ValueError, match="band width"):
            ops.boundary_band(lab, d)
        with pytest.raises(ValueError, match="band width"):
            ops.boundary_accumulate(lab.view(-1), lab.view(-1), [(4, 5)], d, torch.zeros(3, 3, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="widths"):
        ops.boundary_band([lab, lab], [1, 2, 3])
    with pytest.raises(TypeError):
        ops.boundary_band(lab.to(torch.int32), 2)
    with pytest.raises(TypeError):
        ops.boundary_band([lab, lab.to(torch.uint8)], 2)
    for bad in (lab.view(-1), torch.zeros(2, 4, 5, dtype=torch.int64), torch.zeros(0, 5, dtype=torch.int64), [], "map"):
        with pytest.raises(ValueError):
            ops.boundary_band(bad, 2)
    flat, areas = lab.view(-1), torch.zeros(3, 3, dtype=torch.int64)
    for K in (0, 128):
        with pytest.raises(ValueError, match="K="):
            ops.boundary_accumulate(flat, flat, [(4, 5)], 2, torch.zeros(3, max(K, 1), dtype=torch.int64), K)
    with pytest.raises(ValueError, match="images of sizes"):
        ops.boundary_accumulate(flat, flat, [(4, 6)], 2, areas, 3)
    with pytest.raises(ValueError, match="positive size"):
        ops.boundary_accumulate(flat, flat, [(0, 5)], 2, areas, 3)
    with pytest.raises(ValueError, match="areas"):
        ops.boundary_accumulate(flat, flat, [(4, 5)], 2, torch.zeros(3, 4, dtype=torch.int64), 3)
    with pytest.raises(TypeError):
        ops.boundary_accumulate(flat.to(torch.int32), flat, [(4, 5)], 2, areas, 3)
    with pytest.raises(TypeError):
        ops.boundary_accumulate(flat, flat.float(), [(4, 5)], 2, areas, 3)
    # with every option in order the next refusal is the missing device: no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.boundary_band(lab, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.boundary_accumulate(flat, flat, [(4, 5)], 2, areas, 3)


def test_metric_options(monkeypatch):
    from clip_decontamination_amd import _lib, metrics
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    M = metrics.BoundaryIoUMetric
    assert issubclass(M, metrics.IoUMetric)
    sig = inspect.signature(M.__init__).parameters
    assert sig["boundary_ratio"].default == 0.02 and sig["boundary_px"].default is None
    for kw in (dict(boundary_px=0), dict(boundary_px=4096), dict(boundary_px=2.0), dict(boundary_px=True)):
        with pytest.raises(ValueError, match="boundary_px"):
            M(num_classes=3, **kw)
    for kw in (dict(boundary_ratio=0), dict(boundary_ratio=-1.0), dict(boundary_ratio=float("nan")), dict(boundary_ratio="x")):
        with pytest.raises(ValueError, match="boundary_ratio"):
            M(num_classes=3, **kw)
    with pytest.raises(ValueError, match="num_classes"):
        M(num_classes=128)
    with pytest.raises(KeyError):
        M(num_classes=3, iou_metrics=["mAP"])                       # IoUMetric's own checks still hold
    m = M(num_classes=3, boundary_px=7, boundary_ratio=0.5)
    assert m.width((512, 512)) == 7                                 # a fixed width overrides the ratio
    m = M(num_classes=3)
    assert (m.width((512, 512)), m.width((2048, 4608)), m.width((1, 1))) == (14, 101, 1)
    assert tuple(m.boundary_areas.shape) == (3, 3) and m.boundary_areas.dtype == torch.int64 and not m.boundary_areas.any()
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
    assert torch.equal(m.confusion, t) and not m.boundary_areas.any()
    out = m.compute()
    assert set(out) == set(metrics.metrics_from_confusion(t)) | {"BIoU"} and "mBIoU" in out["summary"] and "mIoU" in out["summary"]
    m.reset()
    assert not m.confusion.any() and not m.boundary_areas.any()


def test_evaluate_keeps_its_defaults():
    import segearth_segmentor
    import segmentor
    for cls in (segmentor.SegmentorEx, segearth_segmentor.Segmentor):
        p = inspect.signature(cls.evaluate).parameters
        assert list(p)[:8] == ["self", "inputs", "gt_maps", "metric", "reduce_zero_label", "ignore_index", "iou_metrics", "at_gt_size"]
        assert (p["metric"].default, p["reduce_zero_label"].default, p["ignore_index"].default, p["iou_metrics"].default,
                p["at_gt_size"].default) == (None, False, 255, ("mIoU",), False)
        assert p["boundary_ratio"].default is None and p["boundary_px"].default is None


def test_images_must_not_overlap():
    """Offsets ascend and the images are disjoint: an overlap, a gap past the end and a descending order are refused."""
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(1 << 20)
    hw = (ctypes.c_int32 * 4)(4, 5, 2, 3)
    d = (ctypes.c_int32 * 2)(1, 1)
    for offs in ((0, 10), (0, 19), (0, 21), (6, 0), (0, 0)):
        off = (ctypes.c_int64 * 2)(*offs)
        assert lib.sg_boundary_band(one, _lib.GT_U8, hw, off, d, 2, one, one, 1 << 20, None) == -1, offs
        assert "offset[" in lib.sg_last_error().decode()
        assert lib.sg_boundary_accumulate(one, one, _lib.GT_U8, hw, off, d, 2, 3, 255, 0, one, one, 1 << 20, None) == -1, offs
        assert "offset[" in lib.sg_last_error().decode()
