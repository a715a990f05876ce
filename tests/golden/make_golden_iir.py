#!/usr/bin/env python3
"""Transcribe the reference's IirFilter golden vectors into tests/golden/iirfilt.npz.

Run ONCE where the reference tree is available (it never travels with the tests):

    python tests/golden/make_golden_iir.py REFERENCE_ROOT

Like make_golden.py it reads only *numeric literals*; no reference source text is kept.  Sources (relative to the
reference root):

  src/filter/iir/test_data.rs            IIRFILT_{RRRF,CRCF,CCCF}_DATA_H{3,5,7}X64_{B,A,X,Y}
  src/filter/iir/iirfiltsos.rs:137-244   iirfiltsos_impulse_n2 / iirfiltsos_step_n2: b, a and expected outputs
  src/filter/iir/iirfilt.rs:644-820      iir_groupdelay_{n3,n8,sos_n8}: b, a, fc and expected group delays
"""
import re
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
CPLX = re.compile(r"Complex32::new\(\s*(%s)\s*,\s*(%s)\s*\)" % (NUM, NUM))


def nums(body):
    body = re.sub(r"//[^\n]*", "", body)
    body = re.sub(r"f32\b", "", body)
    return [float(v) for v in re.findall(NUM, body)]


def const_table(src, name):
    m = re.search(r"(?:pub )?const %s:\s*\[(\w+);\s*\d+\]\s*=\s*\[(.*?)\];" % name, src, re.S)
    if not m:
        raise SystemExit(f"{name} not found")
    if m.group(1) == "Complex32":
        return np.asarray([complex(float(a), float(b)) for a, b in CPLX.findall(m.group(2))], np.complex64)
    return np.asarray(nums(m.group(2)), np.float32)


def let_array(body, name):
    m = re.search(r"let %s\s*=\s*\[(.*?)\];" % name, body, re.S)
    if not m:
        raise SystemExit(f"let {name} not found")
    return np.asarray(nums(m.group(1)), np.float64)


def fn_body(src, fn):
    i = src.index(f"fn {fn}(")
    j = src.find("#[test]", i)
    return src[i: j if j > 0 else len(src)]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    root = Path(sys.argv[1])
    d = root / "src" / "filter" / "iir"
    data = (d / "test_data.rs").read_text()
    out = {}
    for kind in ("RRRF", "CRCF", "CCCF"):
        for h in (3, 5, 7):
            for part in "BAXY":
                out[f"{kind.lower()}_h{h}_{part.lower()}"] = const_table(data, f"IIRFILT_{kind}_DATA_H{h}X64_{part}")
    sos = (d / "iirfiltsos.rs").read_text()
    for t in ("impulse", "step"):
        body = fn_body(sos, f"test_iirfiltsos_{t}_n2")
        out[f"sos_{t}_b"] = let_array(body, "b")
        out[f"sos_{t}_a"] = let_array(body, "a")
        out[f"sos_{t}_y"] = let_array(body, "test")
    filt = (d / "iirfilt.rs").read_text()
    for t in ("n3", "n8", "sos_n8"):
        body = fn_body(filt, f"test_iir_groupdelay_{t}")
        for v in ("b", "a", "fc", "g0"):
            out[f"gd_{t}_{v}"] = let_array(body, v)
    np.savez_compressed(HERE / "iirfilt.npz", **out)
    print(f"wrote {HERE / 'iirfilt.npz'}: {len(out)} arrays")


if __name__ == "__main__":
    main()
