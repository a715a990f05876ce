"""SymStream's kernels as built (symstream_kernels.hip), read from the gfx950 code object: the six instantiations of the
fused kernel ({few-branch, taps in LDS, taps global} x {LFSR source, caller's symbols}), the range check and the gain
kernel of the three-launch route are there; none uses scratch; none has static LDS.  The fused kernel's LDS is all
dynamic -- the span of the workgroup's tiles, the taps as firpfb_all_plan(8, 4, k, Ls) places them, the M x 8 byte table
and the jumped state, each part rounded to 16 bytes -- so a fixed group segment of 0 is what keeps the dynamic carve's
base 16-byte aligned, and the sizes the launches ask for stay inside the 64 KiB a workgroup may have for every shape
the tests run fused."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
# template arguments as mangled: <plan kind, LFSR>
FUSED = [f"symstream_kernelILi{plan}ELb{lfsr}EE" for plan in (0, 1, 2) for lfsr in (0, 1)]
KERNELS = FUSED + ["symstream_check_kernel", "symstream_gain_kernel"]


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def _found(tmp_path):
    found = {}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*symstream_\w*kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            found[m.group(1)] = (co, notes[lo: hi if hi > 0 else len(notes)])
    return found


def test_symstream_kernels_present_without_scratch_or_static_lds(tmp_path):
    found = _found(tmp_path)
    assert len(found) == len(KERNELS), sorted(found)
    for key in KERNELS:
        hits = [name for name in found if key in name]
        assert len(hits) == 1, (key, sorted(found))
        meta = found[hits[0]][1]
        pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
        assert pm and int(pm.group(1)) == 0, (hits[0], pm and pm.group(1))
        gm = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
        assert gm and int(gm.group(1)) == 0, (hits[0], gm and gm.group(1))
        wg = re.search(r"\.max_flat_workgroup_size:\s+(\d+)", meta)
        assert wg and int(wg.group(1)) == 256, (hits[0], wg and wg.group(1))


def test_fused_kernels_sum_with_fused_multiply_adds(tmp_path):
    """the bank kernels' mac is fmaf: the sums must not have been split into multiply and add"""
    found = _found(tmp_path)
    for key in FUSED:
        name = [n for n in found if key in n][0]
        dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(found[name][0])],
                             capture_output=True, text=True).stdout
        ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
        assert sum(o.startswith(("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32")) for o in ops) >= 2, name
        assert not [o for o in ops if o.startswith("scratch_")], name


def test_dynamic_lds_of_the_tested_shapes_fits_a_workgroup():
    """one tile per workgroup (a short call): the bank plan's span and taps, each rounded to 16 bytes, the table and the
    16 bytes of the jumped state.  A long call stages more tiles per workgroup, up to a 40 KiB span."""
    import yagi_amd as ya
    for k, m, M, kind in [(2, 1, 16, 0), (16, 31, 16, 0), (5, 17, 256, 0), (17, 3, 64, 1), (64, 100, 8, 2), (12, 12, 4, 0)]:
        p = ya.plan_firpfb_all(8, 4, k, 2 * m + 1)
        assert p.kind == kind, (k, m, p)
        span = ((256 if kind == 0 else 64) + 2 * m) * 8
        taps = k * (2 * m + 1) * 4 if kind == 1 else 0
        assert p.lds == (span if kind == 0 else (span + 15) // 16 * 16 + taps), (k, m, p.lds)
        assert (span + 15) // 16 * 16 + (taps + 15) // 16 * 16 + 8 * M + 16 <= 65536


def test_source_has_one_dynamic_lds_region_and_no_inline_assembly():
    src = (ROOT / "yagi_amd" / "csrc" / "symstream_kernels.hip").read_text()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert code.count("__shared__") == 1 and "extern __shared__ __align__(16)" in code
    assert "asm" not in code
