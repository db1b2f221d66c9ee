"""The area_thd entries at the drop-in boundary, without a GPU: include/segearth_hip.h declares them, the library exports them, the
ctypes table carries them with the header's parameter counts and types, and every entry refuses null pointers, a K beyond
SG_AREA_MAX_K and a bg_idx out of range through the error channel before any device work."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
NEW = ("sg_class_area", "sg_class_area_multi", "sg_area_keep", "sg_area_filter_probs", "sg_area_filter_probs_multi", "sg_area_relabel",
       "sg_area_relabel_multi")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototypes():
    src = _header()
    out = {}
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        out[name] = None if m is None else [p.strip() for p in m.group(1).split(",")]
    return out


def _ctype(param: str):
    if "*" in param or param.startswith("sg_stream"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}[param.split()[0]]


def test_header_declares_and_library_exports_the_entries():
    from clip_decontamination_amd import _lib, ops
    protos = _prototypes()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert protos[name] is not None, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    m = re.search(r"#define\s+SG_AREA_MAX_K\s+(\d+)", _header())
    assert m and int(m.group(1)) == ops.AREA_MAX_K
    assert 2 * 4 * ops.AREA_MAX_K <= 160 * 1024                                    # two workgroups' tables fit a CU's LDS


def test_ctypes_table_matches_the_header():
    from clip_decontamination_amd import _lib
    protos = _prototypes()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert args == [_ctype(p) for p in protos[name]], (name, protos[name])
    # the relabel entries take sg_label_head[_multi]'s arguments plus keep and conf (labels, in/out, stays where it was)
    for a, b in (("sg_area_relabel", "sg_label_head"), ("sg_area_relabel_multi", "sg_label_head_multi")):
        assert len(_lib.SIGNATURES[a][1]) == len(_lib.SIGNATURES[b][1]) + 1


def test_python_layer_exposes_the_ops():
    from clip_decontamination_amd import ops
    for name in ("class_area", "class_area_multi", "area_keep", "area_filter_probs", "area_filter_probs_multi", "area_relabel",
                 "area_relabel_multi", "area_filter"):
        assert callable(getattr(ops, name)), name


def test_entries_refuse_before_any_device_work():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    big = 4097
    one = ctypes.c_void_p(8)                                                        # a non-null, aligned pointer that is never followed
    calls = {
        "null": [
            lambda: lib.sg_class_area(None, 10, 3, None, None),
            lambda: lib.sg_class_area_multi(None, None, None, None, 1, 1, 10, 3, None, None),
            lambda: lib.sg_area_keep(None, 1, 3, 0, 0.1, None, None),
            lambda: lib.sg_area_filter_probs(None, None, None, 3, 2, 2, 0.0, 0, None, None),
            lambda: lib.sg_area_filter_probs_multi(None, None, None, None, None, None, 1, 1, 4, 3, 0.0, 0, None, None),
            lambda: lib.sg_area_relabel(None, None, 1, 3, 2, 2, 4, 4, 0, 0, 4, 4, None, 3, 50.0, 0.0, 0, None, None, None, None),
            lambda: lib.sg_area_relabel_multi(None, None, None, 1, 3, 2, 2, 4, 4, 0, 0, None, None, None, None, 1, 1, 16, None, 3, 50.0, 0.0, 0,
                                              None, None, None, None),
        ],
        "SG_AREA_MAX_K": [
            lambda: lib.sg_class_area(one, 10, big, one, None),
            lambda: lib.sg_class_area_multi(one, one, one, one, 1, 1, 10, big, one, None),
            lambda: lib.sg_area_keep(one, 1, big, 0, 0.1, one, None),
            lambda: lib.sg_area_filter_probs(one, one, one, big, 2, 2, 0.0, 0, one, None),
            lambda: lib.sg_area_filter_probs_multi(one, one, one, one, one, one, 1, 1, 4, big, 0.0, 0, one, None),
            lambda: lib.sg_area_relabel(one, one, 1, big, 2, 2, 4, 4, 0, 0, 4, 4, one, big, 50.0, 0.0, 0, one, one, one, None),
            lambda: lib.sg_area_relabel_multi(one, one, one, 1, big, 2, 2, 4, 4, 0, 0, one, one, one, one, 1, 1, 16, one, big, 50.0, 0.0, 0,
                                              one, one, one, None),
        ],
        "bg_idx": [
            lambda: lib.sg_area_keep(one, 1, 3, 3, 0.1, one, None),
            lambda: lib.sg_area_keep(one, 1, 3, -1, 0.1, one, None),
            lambda: lib.sg_area_filter_probs(one, one, one, 3, 2, 2, 0.0, 3, one, None),
            lambda: lib.sg_area_filter_probs_multi(one, one, one, one, one, one, 1, 1, 4, 3, 0.0, -1, one, None),
            lambda: lib.sg_area_relabel(one, one, 1, 3, 2, 2, 4, 4, 0, 0, 4, 4, one, 3, 50.0, 0.0, 3, one, one, one, None),
            lambda: lib.sg_area_relabel_multi(one, one, one, 1, 3, 2, 2, 4, 4, 0, 0, one, one, one, one, 1, 1, 16, one, 3, 50.0, 0.0, 5,
                                              one, one, one, None),
        ],
    }
    for word, fns in calls.items():
        for fn in fns:
            rc = fn()
            err = lib.sg_last_error().decode()
            assert rc == -1 and word in err, (word, rc, err)
    assert lib.sg_area_keep(one, 1, 3, 0, -0.5, one, None) == -1 and "area_thd" in lib.sg_last_error().decode()
    assert lib.sg_area_keep(one, 1, 3, 0, float("nan"), one, None) == -1
    assert lib.sg_class_area(one, 0, 3, one, None) == 0                            # no pixels: a valid no-op, nothing launched


def test_python_checks_raise_value_errors():
    from clip_decontamination_amd import ops
    for K, bg in ((3, 3), (3, -1), (1, 1)):
        with pytest.raises(ValueError, match="bg_idx"):
            ops.area_args("t", K, bg)
    for thd in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="area_thd"):
            ops.area_args("t", 3, 0, thd)
    assert ops.area_args("t", 3, 2, 1.5) == (3, 2)
