"""The wide upsampler entries at the drop-in boundary, without a GPU: include/segearth_hip.h declares sg_jbu_logits_wide and
sg_jbu_workspace_bytes_wide, the library exports them, the ctypes table carries them with the header's parameter counts, and the wide
entry refuses null arguments through the error channel before any device work, leaving the launch record as it was."""
import ctypes
import os
import re
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "segearth_hip.h")
NEW = ("sg_jbu_logits_wide", "sg_jbu_workspace_bytes_wide")


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        out[name] = None if m is None else [p.strip() for p in m.group(1).split(",")]
    return out


def test_header_declares_and_library_exports_the_wide_entries():
    from clip_decontamination_amd import _lib
    protos = _prototypes()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert protos[name] is not None, f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} declared in the header but not exported"


def test_ctypes_table_matches_the_header():
    from clip_decontamination_amd import _lib
    protos = _prototypes()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(protos[name]), (name, protos[name])
    # the wide logits entry has the signature of sg_jbu_logits; the sizing entry that of sg_jbu_workspace_bytes plus Q
    assert _lib.SIGNATURES["sg_jbu_logits_wide"] == _lib.SIGNATURES["sg_jbu_logits"]
    res, args = _lib.SIGNATURES["sg_jbu_workspace_bytes"]
    assert _lib.SIGNATURES["sg_jbu_workspace_bytes_wide"] == (res, [*args, ctypes.c_int])


def test_wide_entries_refuse_null_arguments_without_a_device():
    from clip_decontamination_amd import _lib
    lib = _lib.load()
    seen = []

    def fresh_thread():                      # a thread of its own: its launch record starts at 'none'
        seen.append(lib.sg_jbu_last_kernels())
        for Q in (1, 32, 33, 130):
            seen.append((lib.sg_jbu_logits_wide(None, None, None, 1, 2, 2, 32, 32, 2, None, Q, None, 0.0, None, None, 0, None), lib.sg_last_error()))
        seen.append(lib.sg_jbu_last_kernels())
        seen.append(lib.sg_jbu_workspace_bytes_wide(None, 1, 2, 2, 130))

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen[0] == b"none" and seen[5] == b"none", seen
    for rc, err in seen[1:5]:
        assert rc != 0 and b"sg_jbu_logits_wide: null argument" in err, (rc, err)
    assert seen[6] == 0
