"""The min_region entries at the drop-in boundary, without a GPU: include/segearth_hip.h declares them, the library exports them, the
ctypes table carries them, sg_sieve refuses every bad argument through the error channel before any device work, and the Python layer
raises its ValueErrors and refusal constants where construction allows it."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
NEW = ("sg_sieve_workspace_bytes", "sg_sieve")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _ctype(param: str):
    if "*" in param or param.startswith("sg_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}[param.split()[0]]


def test_header_library_and_ctypes_table_agree():
    from clip_decontamination_amd import _lib, ops
    src = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype(m.group(1))
        assert args == [_ctype(p.strip()) for p in m.group(2).split(",")], name
    for word, value in ops.SIEVE_FILLS.items():
        m = re.search(r"#define\s+SG_SIEVE_FILL_" + word.upper() + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == value
    assert callable(ops.sieve) and callable(ops.sieve_flat) and callable(ops.sieve_args)


def test_workspace_bytes_is_monotone_and_holds_the_three_arrays():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    for fill, per_pixel in ((0, 8), (1, 16)):                                  # parent + area, and best for the neighbour fill
        last = -1
        for n in (0, 1, 2, 63, 64, 65, 1000, 2048 * 4608, (1 << 31) - 1, 1 << 33):
            b = lib.sg_sieve_workspace_bytes(n, fill)
            assert b >= last and b >= per_pixel * n
            last = b
    assert lib.sg_sieve_workspace_bytes(-1, 0) == 0 and lib.sg_sieve_workspace_bytes(10, 2) == 0


def test_sg_sieve_refuses_before_any_device_work():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                                   # non-null, aligned, never followed
    big = 1 << 40

    def call(labels=one, out=one, hw=((4, 5),), off=(0,), N=None, min_region=3, conn=4, fill=1, ws=one, ws_bytes=big):
        n = len(hw) if N is None else N
        hw_a = None if hw is None else (ctypes.c_int32 * (2 * len(hw)))(*[v for s in hw for v in s])
        off_a = None if off is None else (ctypes.c_int64 * len(off))(*off)
        return lib.sg_sieve(labels, out, hw_a, off_a, n, min_region, conn, fill, 0, ws, ws_bytes, None)

    cases = [
        (dict(labels=None), "null pointer"), (dict(out=None), "null pointer"), (dict(hw=None, N=1), "null pointer"),
        (dict(off=None), "null pointer"), (dict(ws=None), "null pointer"),
        (dict(min_region=0), "min_region=0"), (dict(min_region=-4), "min_region=-4"),
        (dict(conn=6), "connectivity=6"), (dict(conn=0), "connectivity=0"),
        (dict(fill=2), "unknown fill 2"), (dict(fill=-1), "unknown fill -1"),
        (dict(N=0), "N=0 images"), (dict(N=-2), "N=-2 images"),
        (dict(hw=((0, 5),)), "non-positive size"), (dict(hw=((4, 5), (3, -1)), off=(0, 20)), "image 1 has non-positive size"),
        (dict(hw=((1 << 16, 1 << 15),)), "2^31 or more pixels"), (dict(hw=((46341, 46341),)), "2^31 or more pixels"),
        (dict(off=(-8,)), "negative"),
        (dict(labels=ctypes.c_void_p(12)), "8-byte aligned"), (dict(ws=ctypes.c_void_p(4)), "8-byte aligned"),
        (dict(ws_bytes=16 * 20 - 1), "workspace too small"), (dict(fill=0, ws_bytes=8 * 20 - 1), "workspace too small"),
        (dict(hw=((4, 5), (2, 3)), off=(0, 20), ws_bytes=16 * 26 - 1), "workspace too small"),
    ]
    for kw, word in cases:
        rc = call(**kw)
        err = lib.sg_last_error().decode()
        assert rc == -1 and word in err and err.startswith("sg_sieve:"), (kw, rc, err)


def test_python_checks_raise_value_errors():
    from clip_decontamination_amd import ops
    for bad in (0, -3, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="min_region"):
            ops.sieve_args(bad)
    for bad in (0, 6, "8", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            ops.sieve_args(4, bad)
    for bad in ("background", "nearest", None, 1):
        with pytest.raises(ValueError, match="fill"):
            ops.sieve_args(4, 8, bad)
    assert ops.sieve_args(7, 8, "bg") == (7, 8, "bg") and ops.sieve_args(1) == (1, 4, "neighbour")


def _stub_pipeline(**kw):
    """A SegPipeline built without the constructor's net (the class defaults cover every option), with the options under test set."""
    from clip_decontamination_amd.pipeline import SegPipeline
    pipe = object.__new__(SegPipeline)
    for k, v in kw.items():
        setattr(pipe, k, v)
    return pipe


def test_refusal_constants_without_a_gpu():
    from clip_decontamination_amd import pipeline as P
    assert "min_region" in P.SIEVE_TILE_GROUP and "tile_group" in P.SIEVE_TILE_GROUP and "min_region" in P.SIEVE_TOPK
    off = _stub_pipeline()
    assert off.min_region is None and off.region_connectivity == 4 and off.region_fill == "neighbour"
    off._check_sharding(True)                                                 # nothing to refuse without the option
    pipe = _stub_pipeline(min_region=4, num_classes=5)
    with pytest.raises(ValueError) as e:
        pipe._check_sharding(True)
    assert str(e.value) == P.SIEVE_TILE_GROUP
    pipe._check_sharding(False)
    with pytest.raises(ValueError) as e:
        pipe.topk_k(2)
    assert str(e.value) == P.SIEVE_TOPK
    with pytest.raises(ValueError) as e:
        pipe._wanted("segment_scene", False, 2, False)
    assert str(e.value) == P.SIEVE_TOPK


def test_constructors_refuse_bad_options_before_anything_is_built():
    """The drop-in classes check the min_region options first: no checkpoint, class file or GPU is touched before the ValueError."""
    import torch
    import segearth_segmentor
    import segmentor
    from clip_decontamination_amd import pipeline as P
    for cls in (segmentor.SegmentorEx, segearth_segmentor.Segmentor):
        base = dict(clip_type="CLIP", vit_type="tiny-8", model_type="SegEarth", name_path="/nonexistent/classes.txt", device=torch.device("cpu"))
        for kw, word in ((dict(min_region=0), "min_region"), (dict(min_region=2.0), "min_region"), (dict(min_region=4, region_connectivity=6), "connectivity"),
                         (dict(region_connectivity=5), "connectivity"), (dict(min_region=4, region_fill="nearest"), "fill"), (dict(region_fill="x"), "fill")):
            with pytest.raises(ValueError, match=word):
                cls(**base, **kw)
        with pytest.raises(ValueError) as e:
            cls(**base, min_region=4, tile_group="world")
        assert str(e.value) == P.SIEVE_TILE_GROUP
