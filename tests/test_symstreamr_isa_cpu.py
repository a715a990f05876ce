"""SymStreamR's kernel as built (symstreamr_kernels.hip), read from the gfx950 code object as
tests/test_symstream_isa_cpu.py reads SymStream's: symstreamr_kernel is there once, uses no scratch and has no static LDS
(its LDS is all dynamic -- symbols, samples, the M x 8 byte table and the jumped state, each part rounded to 16 bytes --
so a fixed group segment of 0 keeps the dynamic carve's base 16-byte aligned), and its register count is the one the
build shows: 59 VGPRs, inside the 128 that leave four waves per SIMD."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
VGPRS = 59


def _found(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    found = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950")):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*symstreamr_kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            found[m.group(1)] = (co, notes[lo: hi if hi > 0 else len(notes)])
    return found


def _field(meta, name):
    m = re.search(rf"\.{name}:\s+(\d+)", meta)
    assert m, name
    return int(m.group(1))


def test_kernel_present_without_scratch_or_static_lds_at_the_registers_the_build_shows(tmp_path):
    found = _found(tmp_path)
    assert len(found) == 1, sorted(found)
    name, (co, meta) = next(iter(found.items()))
    assert _field(meta, "private_segment_fixed_size") == 0, name
    assert _field(meta, "vgpr_spill_count") == 0, name
    assert _field(meta, "group_segment_fixed_size") == 0, name
    assert _field(meta, "max_flat_workgroup_size") == 256, name
    assert _field(meta, "vgpr_count") == VGPRS <= 128, (name, _field(meta, "vgpr_count"))
    dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(co)],
                         capture_output=True, text=True).stdout
    ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
    assert not [o for o in ops if o.startswith("scratch_")], name
    # both chains are fmaf chains (fir_bodies.hpp): the sums must not have been split into multiply and add
    assert sum(o.startswith(("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32")) for o in ops) >= 4, name


def test_dynamic_lds_of_the_planned_shapes_fits_a_workgroup():
    import yagi_amd as ya
    for bw in (1.0, 0.77, 0.5, 0.4, 0.25, 0.2, 0.03, 0.001):
        for m in (1, 7, 12, 25, 31, 100):
            p = ya.plan_symstreamr(bw, m, 1 << 24)
            assert p.max_wg_tiles >= 1 and 1 <= p.wg_tiles <= p.max_wg_tiles, (bw, m, p)
            assert p.lds <= 64 * 1024, (bw, m, p)


def test_source_has_one_dynamic_lds_region_and_no_inline_assembly():
    src = (ROOT / "yagi_amd" / "csrc" / "symstreamr_kernels.hip").read_text()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert code.count("__shared__") == 1 and "extern __shared__ __align__(16)" in code
    assert "asm" not in code
