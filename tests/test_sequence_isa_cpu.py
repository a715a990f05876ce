"""The kernels of sequence_kernels.hip as built, read from the gfx950 code object: the expected kernels are there (the
generator once per bits-per-symbol 1 .. 8, the correlator once), none uses scratch, and the LDS of each is what
YAGI_MSEQUENCE_TILE, YAGI_BSEQUENCE_TILE and YAGI_BSEQUENCE_NMAX imply."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")


def _constants():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    return tuple(int(re.search(rf"#define YAGI_{name} (\d+)", hdr).group(1))
                 for name in ("MSEQUENCE_TILE", "BSEQUENCE_TILE", "BSEQUENCE_NMAX"))


def _kernel_metadata(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    found = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950")):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*((?:msequence|bsequence)_\w+_kernel)\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            found[m.group(1)] = notes[lo: hi if hi > 0 else len(notes)]
    return found


def test_sequence_kernels_present_without_scratch_and_with_the_implied_lds(tmp_path):
    mtile, btile, nmax = _constants()
    words = nmax // 32
    lds = {"msequence_gen_kernel": mtile,                           # the tile's bytes
           # the packed words a tile's windows span (8 bits per symbol at most, the window, a word of slack at either
           # end) and the symbol bytes under them (1 bit per symbol at least, alignment slack)
           "bsequence_corr_kernel": (btile * 8 // 32 + words + 2) * 4 + btile + (words + 2) * 32 + 16}
    assert max(lds.values()) <= 64 * 1024
    found = _kernel_metadata(tmp_path)
    names = sorted(found)
    assert sum("bsequence_corr_kernel" in s for s in names) == 1, names
    for bps in range(1, 9):                                         # one instantiation per bits-per-symbol
        assert sum(f"msequence_gen_kernelILi{bps}E" in s for s in names) == 1, (bps, names)
    assert len(names) == 9, names
    for name, meta in found.items():
        pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
        assert pm and int(pm.group(1)) == 0, (name, pm and pm.group(1))
        gm = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
        want = next(v for k, v in lds.items() if k in name)
        assert gm and int(gm.group(1)) == want, (name, gm and gm.group(1), want)
