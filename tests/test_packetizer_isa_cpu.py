"""Packetizer's kernels as built (packetizer_kernels.hip), read from the gfx950 code object on the pattern of
tests/test_convcode_isa_cpu.py: the encoder and the four decoders (the instantiations of ConvCode's decoder body) are
present and none uses scratch: the CRC register, the field and the path metrics live in registers, the decisions, the
expanded steps and the CRC table in LDS."""
import re
import subprocess

from conftest import ROOT
from test_convcode_isa_cpu import LLVM, _code_objects

KERNELS = {"pkt_encode_kernel": 1, "pkt_decode_kernel": 4}


def test_packetizer_kernels_are_present_and_use_no_scratch(tmp_path):
    assert (ROOT / "yagi_amd" / "csrc" / "packetizer_kernels.hip").exists()
    seen = dict.fromkeys(KERNELS, 0)
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*(pkt_encode_kernel|pkt_decode_kernel)\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            meta = notes[lo: hi if hi > 0 else len(notes)]
            pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
            assert pm and int(pm.group(1)) == 0, (m.group(1), pm and pm.group(1))
            seen[m.group(2)] += 1
    assert seen == KERNELS, seen
