"""Channel's kernels as built (channel_kernels.hip), read from the gfx950 code object: all four are present (NCO and VCO,
pitched and broadcast), none uses scratch (the tile, the taps and Osc's table live in LDS, the sums in registers) and none
holds an f32 fused multiply-add, since every product and add of the definition keeps its own rounding."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
F32_FMA = re.compile(r"^(v_fma_f32|v_fmac_f32|v_fmaak_f32|v_fmamk_f32|v_pk_fma_f32|v_mad_f32|v_mac_f32|v_fma_mix\w*)")
N_KERNELS = 4      # {NCO, VCO} x {pitched, broadcast}


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def test_channel_kernels_use_no_scratch(tmp_path):
    seen = 0
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*channel_kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            meta = notes[lo: hi if hi > 0 else len(notes)]
            pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
            assert pm and int(pm.group(1)) == 0, (m.group(1), pm and pm.group(1))
            seen += 1
    assert seen == N_KERNELS, seen


def test_channel_kernels_have_no_f32_fma(tmp_path):
    seen = 0
    for co in _code_objects(tmp_path):
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "-s", "-W", str(co)], capture_output=True, text=True).stdout
        names = sorted({l.split()[-1] for l in syms.splitlines() if "channel_kernel" in l and " FUNC " in l})
        for name in names:
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(co)],
                                 capture_output=True, text=True).stdout
            ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
            ops = [o for o in ops if o]
            assert sum(o.startswith("v_mul_f32") or o.startswith("v_pk_mul_f32") for o in ops) >= 1, \
                (name, "not the device listing")
            bad = [o for o in ops if F32_FMA.match(o)]
            assert not bad, (name, bad[:4])
            seen += 1
    assert seen == N_KERNELS, seen
