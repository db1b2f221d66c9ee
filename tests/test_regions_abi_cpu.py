"""The region-table entries at the drop-in boundary, without a GPU: include/segearth_hip.h declares them, the library exports them, the
ctypes table carries them, sg_regions refuses every bad argument through the error channel before any device work, and the Python
layer raises its ValueErrors and its refusal constant."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
NEW = ("sg_regions_workspace_bytes", "sg_regions")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _ctype(param: str):
    if "*" in param or param.startswith("sg_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}[param.split()[0]]


def _define(src, name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
    assert m, f"{name} is not defined in the header"
    return int(m.group(1))


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
    for word, value in ops.REGION_COLUMNS.items():
        assert _define(src, "SG_REGION_" + word.upper()) == value
    assert sorted(ops.REGION_COLUMNS.values()) == list(range(11))
    assert _define(src, "SG_REGION_FIELDS") == ops.REGION_FIELDS == 12
    assert _define(src, "SG_REGIONS_BLOCK_PIXELS") == ops.REGIONS_BLOCK_PIXELS
    assert _define(src, "SG_REGIONS_SCAN_BLOCKS") == ops.REGIONS_SCAN_BLOCKS
    assert callable(ops.regions) and callable(ops.regions_flat) and callable(ops.regions_args)


def test_workspace_bytes_is_monotone_and_at_least_the_stated_formula():
    from clip_decontamination_amd import _lib, ops
    lib = _lib.load()
    group = _define(_header(), "SG_SIEVE_GROUP")
    last = -1
    for n in (0, 1, 2, 63, 64, 65, 1000, 2047, 2048, 2049, 2048 * 4608, (1 << 31) - 1, 1 << 33):
        b = lib.sg_regions_workspace_bytes(n, 1)
        blocks = -(-n // ops.REGIONS_BLOCK_PIXELS) + group + 1
        assert b >= last and b >= 8 * n + 4 * blocks and b % 8 == 0
        assert b <= 12 * n + 4 * blocks + 7                                     # at or below 12 bytes per pixel plus the scan's block array (rounded up to 8)
        assert b == lib.sg_regions_workspace_bytes(n, 1 << 40)                  # max_regions does not enter it
        last = b
    assert lib.sg_regions_workspace_bytes(-1, 1) == 0 and lib.sg_regions_workspace_bytes(10, 0) == 0


def test_sg_regions_refuses_before_any_device_work():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)                                                   # non-null, aligned, never followed
    big = 1 << 40
    need = lib.sg_regions_workspace_bytes(20, 1)
    need2 = lib.sg_regions_workspace_bytes(26, 1)

    def call(labels=one, conf=None, hw=((4, 5),), off=(0,), N=None, conn=4, min_area=1, max_regions=16, table=one, region_of=None, counts=one,
             ws=one, ws_bytes=big):
        n = len(hw) if N is None else N
        hw_a = None if hw is None else (ctypes.c_int32 * (2 * len(hw)))(*[v for s in hw for v in s])
        off_a = None if off is None else (ctypes.c_int64 * len(off))(*off)
        return lib.sg_regions(labels, conf, hw_a, off_a, n, conn, min_area, 0, 0, max_regions, table, region_of, counts, ws, ws_bytes, None)

    cases = [
        (dict(labels=None), "null pointer"), (dict(hw=None, N=1), "null pointer"), (dict(off=None), "null pointer"),
        (dict(table=None), "null pointer"), (dict(counts=None), "null pointer"), (dict(ws=None), "null pointer"),
        (dict(conn=6), "connectivity=6"), (dict(conn=0), "connectivity=0"),
        (dict(min_area=0), "min_area=0"), (dict(min_area=-4), "min_area=-4"),
        (dict(max_regions=0), "max_regions=0"), (dict(max_regions=-1), "max_regions=-1"),
        (dict(N=0), "N=0 images"), (dict(N=-2), "N=-2 images"),
        (dict(hw=((0, 5),)), "non-positive size"), (dict(hw=((4, 5), (3, -1)), off=(0, 20)), "image 1 has non-positive size"),
        (dict(off=(-8,)), "negative"),
        (dict(hw=((1 << 16, 1 << 15),)), "2^31 or more pixels"), (dict(hw=((46341, 46341),)), "2^31 or more pixels"),
        (dict(hw=((1 << 15, 1 << 15), (1 << 15, 1 << 15)), off=(0, 1 << 30)), "2^31 or more pixels"),      # the total, not one image
        (dict(labels=ctypes.c_void_p(12)), "8-byte aligned"), (dict(table=ctypes.c_void_p(4)), "8-byte aligned"),
        (dict(counts=ctypes.c_void_p(20)), "8-byte aligned"), (dict(ws=ctypes.c_void_p(4)), "8-byte aligned"),
        (dict(conf=ctypes.c_void_p(6)), "4-byte aligned"), (dict(region_of=ctypes.c_void_p(9)), "4-byte aligned"),
        (dict(ws_bytes=need - 1), "workspace too small"), (dict(hw=((4, 5), (2, 3)), off=(0, 20), ws_bytes=need2 - 1), "workspace too small"),
    ]
    for kw, word in cases:
        rc = call(**kw)
        err = lib.sg_last_error().decode()
        assert rc == -1 and word in err and err.startswith("sg_regions:"), (kw, rc, err)


def test_python_checks_raise_value_errors():
    from clip_decontamination_amd import ops
    for bad in (0, 6, "8", None, True):
        with pytest.raises(ValueError, match="connectivity"):
            ops.regions_args(bad)
    for bad in (0, -3, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="min_area"):
            ops.regions_args(4, bad)
    for bad in (2.5, "1", True):
        with pytest.raises(ValueError, match="skip_label"):
            ops.regions_args(4, 1, bad)
    for bad in (0, -1, 2.5, "9", True):
        with pytest.raises(ValueError, match="max_regions"):
            ops.regions_args(4, 1, None, bad)
    assert ops.regions_args() == (4, 1, None, None) and ops.regions_args(8, 5, -2, 10) == (8, 5, -2, 10)
    with pytest.raises(ValueError, match="label map"):
        ops.regions([])
    with pytest.raises(ValueError, match="label map"):
        ops.regions("labels")


def _stub_pipeline(**kw):
    """A SegPipeline built without the constructor's net (the class defaults cover every option), with the options under test set."""
    from clip_decontamination_amd.pipeline import SegPipeline
    pipe = object.__new__(SegPipeline)
    for k, v in kw.items():
        setattr(pipe, k, v)
    return pipe


def test_tile_group_is_refused_with_the_constant():
    import torch
    from clip_decontamination_amd import pipeline as P
    assert "tile_group" in P.REGIONS_TILE_GROUP and "region" in P.REGIONS_TILE_GROUP
    pipe = _stub_pipeline(tile_group="world", bg_idx=0)
    with pytest.raises(ValueError) as e:
        pipe.regions(torch.zeros(4, 5, dtype=torch.int64))
    assert str(e.value) == P.REGIONS_TILE_GROUP
    import segmentor
    seg = object.__new__(segmentor.SegmentorEx)
    seg.__dict__["tile_group"] = "world"
    with pytest.raises(ValueError) as e:
        seg.predict_regions([torch.zeros(3, 8, 8)])
    assert str(e.value) == P.REGIONS_TILE_GROUP
