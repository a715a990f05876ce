"""The firpfbchr kernels as built (chanr_kernels.hip), read from the gfx950 code object: every instantiation is present
and none uses scratch -- the column kernel keeps its taps and its window in registers, which holds only while every ring
index is a compile-time constant."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
EXPECTED = {
    "firpfbchr_kernel": 2,                       # M a power of two or not
    "firpfbchr_col_kernel": 3 * 4 * 3,           # built branch length 4, 8, 16 x P/gcd(M,P) 1, 3, 5, 7 x M 64, 128, 256
    "firpfbchr_syn_transform_kernel": 2,
    "firpfbchr_syn_combine_kernel": 1,
}


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def test_chanr_kernels_are_all_there_and_use_no_scratch(tmp_path):
    seen = {k: set() for k in EXPECTED}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*\d(" + "|".join(EXPECTED) + r")I?\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            meta = notes[lo: hi if hi > 0 else len(notes)]
            pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
            assert pm and int(pm.group(1)) == 0, (m.group(1), pm and pm.group(1))
            seen[m.group(2)].add(m.group(1))
    assert {k: len(v) for k, v in seen.items()} == EXPECTED
