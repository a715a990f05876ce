"""OrdFilt's kernels as built (ordfilt_kernels.hip), read from the gfx950 code object: the expected kernels are there
(the LDS form, and the register-resident form for every n it serves), none uses scratch, and the LDS of each is what
YAGI_ORDFILT_TILE, YAGI_ORDFILT_NMAX and the workgroup of 256 lanes imply."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
WG = 256


def _constants():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    return tuple(int(re.search(rf"#define YAGI_ORDFILT_{name} (\d+)", hdr).group(1)) for name in ("TILE", "NMAX", "REG_NMAX"))


def _kernel_metadata(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    found = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950")):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*(ordfilt_\w+_kernel)\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            found[m.group(1)] = notes[lo: hi if hi > 0 else len(notes)]
    return found


def test_ordfilt_kernels_present_without_scratch_and_with_the_implied_lds(tmp_path):
    tile, nmax, reg_nmax = _constants()
    stage = tile + nmax - 1                                   # a tile's samples and the halo in front
    lds = {"ordfilt_rank_kernel": stage * 4 + tile * 4 + stage // 8,      # keys, outputs, a "-0.0" bit per sample
           "ordfilt_reg_kernel": (WG + 1) * (tile // WG + 4) * 4}         # rows of 16 samples padded to 20 words, + 1
    assert max(lds.values()) <= 64 * 1024
    found = _kernel_metadata(tmp_path)
    names = sorted(found)
    assert sum("ordfilt_rank_kernel" in s for s in names) == 1, names
    for n in range(2, reg_nmax + 1):                          # one instantiation per window length: ...kernelILi<n>E...
        assert sum(f"ordfilt_reg_kernelILi{n}E" in s for s in names) == 1, (n, names)
    assert len(names) == reg_nmax, names
    for name, meta in found.items():
        pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
        assert pm and int(pm.group(1)) == 0, (name, pm and pm.group(1))
        gm = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
        want = next(v for k, v in lds.items() if k in name)
        assert gm and int(gm.group(1)) == want, (name, gm and gm.group(1), want)
