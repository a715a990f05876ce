"""ConvCode's kernels as built (convcode_kernels.hip), read from the gfx950 code object: the encoder and the four decoders
(1 state per lane with a step's decisions narrower than a ballot or whole ballots, 2 and 4 states per lane) are present
and none uses scratch: the path metrics, branch masks and ballots live in
registers, the decisions and the staged soft bytes in LDS."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
KERNELS = {"conv_encode_kernel": 1, "conv_decode_kernel": 4}


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def test_convcode_kernels_are_present_and_use_no_scratch(tmp_path):
    seen = dict.fromkeys(KERNELS, 0)
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*(conv_encode_kernel|conv_decode_kernel)\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            meta = notes[lo: hi if hi > 0 else len(notes)]
            pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
            assert pm and int(pm.group(1)) == 0, (m.group(1), pm and pm.group(1))
            seen[m.group(2)] += 1
    assert seen == KERNELS, seen
