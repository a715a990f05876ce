"""Autocorr's kernels as built (autocorr_kernels.hip), read from the gfx950 code object: the four expected kernels are
there ({cccf, rrrf} x {with, without energy}), none uses scratch, the LDS of each is what YAGI_AUTOCORR_TILE,
YAGI_AUTOCORR_WMAX and the workgroup of 256 lanes imply, and none holds an f32 fused multiply-add, since every product
and every add of the sums must keep its own rounding."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
F32_FMA = re.compile(r"^(v_fma_f32|v_fmac_f32|v_fmaak_f32|v_fmamk_f32|v_pk_fma_f32|v_mad_f32|v_mac_f32|v_fma_mix\w*)")
WG = 256
# template arguments as mangled: <float, true>, <float, false>, <yagi_cf32, true>, <yagi_cf32, false>
KERNELS = {"autocorr_kernelIfLb1E": ("rrrf", True), "autocorr_kernelIfLb0E": ("rrrf", False),
           "autocorr_kernelI9yagi_cf32Lb1E": ("cccf", True), "autocorr_kernelI9yagi_cf32Lb0E": ("cccf", False)}


def _constants():
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    return tuple(int(re.search(rf"#define YAGI_AUTOCORR_{name} (\d+)", hdr).group(1)) for name in ("TILE", "WMAX"))


def _lds(kind, energy):
    """per staged sample (TILE + WMAX of them, in rows of TILE / 256 padded by 16 bytes) its term of rxx, two floats for
    cccf and one for rrrf; its term of the energy in rows of its own for cccf, beside the first for rrrf"""
    tile, wmax = _constants()
    r = tile // WG
    rows = (tile + wmax) // r
    if kind == "cccf":
        return rows * (r * 8 + 16) + (rows * (r * 4 + 16) if energy else 0)
    return rows * (r * (8 if energy else 4) + 16)


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def test_autocorr_kernels_present_without_scratch_and_with_the_implied_lds(tmp_path):
    found = {}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*autocorr_\w*kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            found[m.group(1)] = notes[lo: hi if hi > 0 else len(notes)]
    assert len(found) == len(KERNELS), sorted(found)
    for key, (kind, energy) in KERNELS.items():
        hits = [name for name in found if key in name]
        assert len(hits) == 1, (key, sorted(found))
        meta = found[hits[0]]
        pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
        assert pm and int(pm.group(1)) == 0, (hits[0], pm and pm.group(1))
        gm = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
        want = _lds(kind, energy)
        assert want <= 65536
        assert gm and int(gm.group(1)) == want, (hits[0], gm and gm.group(1), want)


def test_autocorr_kernels_multiply_and_have_no_f32_fma(tmp_path):
    seen = 0
    for co in _code_objects(tmp_path):
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "-s", "-W", str(co)], capture_output=True, text=True).stdout
        names = sorted({l.split()[-1] for l in syms.splitlines() if "autocorr_" in l and "kernel" in l and " FUNC " in l})
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
    assert seen == len(KERNELS), seen
