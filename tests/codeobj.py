"""The gfx950 code objects of the built library, read once (host only: ELF
notes of the device code, nothing runs on a GPU).

The library's .hip_fatbin section holds one offload bundle per .hip source
file, one after the other; each is unbundled for gfx950 and its AMDGPU
metadata note parsed.  The ABI tests and tests/test_codeobj.py filter the one
result by mangled kernel name."""
import os
import re
import subprocess
import tempfile

import pytest

from subproc_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count", "sgpr_count")
_CACHE = {}


def kernels(lib_path=None):
    """name -> {private_segment_fixed_size, group_segment_fixed_size,
    vgpr_count, sgpr_count} of every gfx950 kernel of every bundle of the
    library (do not modify: shared by every test of the process).  Skips the
    calling test when the library or the ROCm LLVM tools are absent."""
    lib_path = os.path.abspath(lib_path or _lib.LIB_PATH)
    if lib_path not in _CACHE:
        if not os.path.exists(lib_path):
            pytest.skip("HIP library not built (__graft_entry__.build())")
        if not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler",
                                                                   "llvm-readelf")):
            pytest.skip("ROCm LLVM tools not present")
        _CACHE[lib_path] = _read(lib_path)
    return _CACHE[lib_path]


def named(wanted):
    """name -> resources of the kernels whose name holds one of ``wanted``."""
    return {name: v for name, v in kernels().items() if any(w in name for w in wanted)}


def grouped(wanted, pattern="%s"):
    """want -> [resources of every kernel whose name matches the regex
    ``pattern % want``], for each of ``wanted`` that has a match."""
    found = {}
    for name, v in kernels().items():
        for want in wanted:
            if re.search(pattern % want, name):
                found.setdefault(want, []).append(v)
    return found


def _read(lib_path):
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        fb = os.path.join(tmp, "fb.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, lib_path,
                               os.path.join(tmp, "host.so")])
        blob = open(fb, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)] + [len(blob)]
        for i in range(len(starts) - 1):
            part, co = os.path.join(tmp, f"fb{i}.bin"), os.path.join(tmp, f"co{i}.o")
            with open(part, "wb") as f:
                f.write(blob[starts[i]:starts[i + 1]])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                                   "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.symbol:\s+(\S+)\.kd", block).group(1)
                assert name not in found, f"kernel {name} is in two bundles"
                found[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in FIELDS}
    return found
