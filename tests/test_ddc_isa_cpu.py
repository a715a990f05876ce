"""The fused kernels of Ddc and Duc as built (ddc_kernels.hip), read from the gfx950 code object: every instantiation is
present and none uses scratch.  No claim about fused multiply-adds is made here: the FIR sums of the shared bodies use
them by design, and that the mix does not is pinned bit for bit by tests/test_gpu_ddc.py."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
# {crcf, cccf} x {NCO, VCO} x ...
EXPECTED = {
    "ddc_decim_consec_kernel": 2 * 2 * 5,      # (NT, R) in (256, 8), (256, 4), (128, 4), (64, 8), (64, 4)
    "ddc_block_kernel": 2 * 2,                 # the general staged kernel
    "duc_fewbranch_kernel": 2 * 2,
    "duc_all_kernel": 2 * 2 * 2,               # taps in LDS or in global memory
}


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def test_fused_kernels_are_all_there_and_use_no_scratch(tmp_path):
    seen = {k: set() for k in EXPECTED}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*(ddc_decim_consec_kernel|ddc_block_kernel|duc_fewbranch_kernel|duc_all_kernel)\S*)",
                             notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            meta = notes[lo: hi if hi > 0 else len(notes)]
            pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
            assert pm and int(pm.group(1)) == 0, (m.group(1), pm and pm.group(1))
            seen[m.group(2)].add(m.group(1))
    assert {k: len(v) for k, v in seen.items()} == EXPECTED
