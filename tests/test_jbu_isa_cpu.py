"""The low-res JBU convolutions stay free of packed f32 arithmetic (no GPU needed).

With its Keff arithmetic SLP-packed into v_pk_fma_f32, jbu_conv_lowres_kernel was not reproducible from run to run (DESIGN.md section 4
'JBU reproducibility'); the only guard is the unit's -fno-slp-vectorize in build.py.  Without that flag the two-plane kernel
jbu_conv_lowres_x2_kernel (the f16x2 upsampler) gets hundreds of v_pk_*_f32 instructions, and no GPU test would notice.  This test
compiles jbu.hip device-only for gfx950 with the real build's flags (imported, not copied) and reads the disassembly."""
import os
import re
import shutil
import subprocess

import pytest

from clip_decontamination_amd import build as B

LLVM = "/opt/rocm/llvm/bin"
PACKED = ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32")
LOWRES = ("jbu_conv_lowres_kernel<5>", "jbu_conv_lowres_kernel<3>", "jbu_conv_lowres_x2_kernel<5>", "jbu_conv_lowres_x2_kernel<3>")


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def _functions(disasm: str):
    """{symbol: body text} from `llvm-objdump -d` output."""
    out, cur, buf = {}, None, []
    for line in disasm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if cur is not None:
                out[cur] = "\n".join(buf)
            cur, buf = m.group(1), []
        elif cur is not None:
            buf.append(line)
    if cur is not None:
        out[cur] = "\n".join(buf)
    return out


@pytest.fixture(scope="module")
def jbu_isa(tmp_path_factory):
    try:
        hipcc = B.hipcc()
    except RuntimeError:
        pytest.skip("hipcc is not installed")
    bundler, objdump = _tool("clang-offload-bundler"), _tool("llvm-objdump")
    if not (bundler and objdump):
        pytest.skip("clang-offload-bundler / llvm-objdump not installed")
    tmp = tmp_path_factory.mktemp("jbu_isa")
    bundle, co = str(tmp / "jbu.bundle.o"), str(tmp / "jbu.co")
    src = os.path.join(B.CSRC, "jbu.hip")
    r = subprocess.run([hipcc, *B.FLAGS, *B.EXTRA_FLAGS.get("jbu.hip", []), "--cuda-device-only", "-c", src, "-o", bundle],
                       capture_output=True, text=True, cwd=str(tmp))
    assert r.returncode == 0, r.stderr
    r = subprocess.run([bundler, "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{B.ARCH}", f"--input={bundle}", f"--output={co}",
                        "--unbundle"], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
        shutil.copyfile(bundle, co)                   # a device-only compile of one arch may already be the bare code object
    r = subprocess.run([objdump, "-d", "--demangle", co], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return _functions(r.stdout)


@pytest.mark.parametrize("kernel", LOWRES)
def test_lowres_conv_has_no_packed_f32(jbu_isa, kernel):
    # demangled symbol: "void sg::jbu_conv_lowres_kernel<5>(unsigned short const*, ...)"
    names = [n for n in jbu_isa if re.match(r"^(void )?sg::" + re.escape(kernel) + r"\(", n)]
    assert len(names) <= 1, names
    body = jbu_isa[names[0]] if names else None
    assert body is not None, f"{kernel} not found in the code object (symbols: {sorted(jbu_isa)[:8]} ...)"
    assert "v_mfma" in body, f"{kernel}: the disassembly does not look like the kernel body"
    counts = {op: len(re.findall(r"\b" + op + r"\b", body)) for op in PACKED}
    assert not any(counts.values()), f"{kernel}: packed f32 arithmetic in a kernel that must stay scalar: {counts}"
