#!/usr/bin/env python3
"""Transcribe the numeric literals of the reference's sequence module into tests/golden/sequence.npz.

Run ONCE where the reference's tree is at hand (it never travels with this repository):

    python tests/golden/make_golden_sequence.py <reference root>

Like make_golden.py it reads only *numeric literals* and keeps no source text.  Sources, relative to the reference root:

  src/sequence/msequence.rs:8-37      the 30 (m, g) pairs of the default generator polynomials     -> genpoly_m, genpoly_g
  src/sequence/bsequence.rs:204-362   the byte vectors of the init / correlate / add / mul / accumulate tests and what
                                      they expect: the 16 index() values after init, correlate = 7, accumulate = 8 and
                                      the 16 expected bits each of the add and mul tests (stored by index, 0 .. 15)
"""
import re
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def test_body(txt, name):
    i0 = txt.index(f"fn {name}(")
    nxt = txt.find("#[test]", i0)
    return txt[i0: nxt if nxt > 0 else len(txt)]


def byte_vector(body, var):
    m = re.search(r"let\s+%s\s*=\s*\[([^\]]*)\]" % var, body)
    return np.array([int(v, 16) for v in re.findall(r"0x([0-9a-fA-F]+)u8", m.group(1))], np.uint8)


def index_bits(body, var):
    bits = np.full(16, 255, np.uint8)
    for i, b in re.findall(r"assert_eq!\(%s\.index\((\d+)\)\.unwrap\(\),\s*(\d+)\)" % var, body):
        bits[int(i)] = int(b)
    assert bits.max() <= 1, bits
    return bits


def main():
    src = Path(sys.argv[1]) / "src" / "sequence"
    ms = (src / "msequence.rs").read_text()
    pairs = [(int(m), int(g, 16)) for m, g in re.findall(r"const\s+MSEQUENCE_GENPOLY_M(\d+)\s*:\s*u32\s*=\s*0x([0-9a-fA-F]+)\s*;", ms)]
    assert [m for m, _ in pairs] == list(range(2, 32)), pairs
    out = {"genpoly_m": np.array([m for m, _ in pairs], np.uint32), "genpoly_g": np.array([g for _, g in pairs], np.uint32)}

    bs = (src / "bsequence.rs").read_text()
    body = test_body(bs, "test_bsequence_init")
    out["init_v"] = byte_vector(body, "v")
    out["init_bits"] = index_bits(body, "q")
    body = test_body(bs, "test_bsequence_correlate")
    out["v0"], out["v1"] = byte_vector(body, "v0"), byte_vector(body, "v1")
    out["correlate"] = np.array([int(re.search(r"correlate\(&q1\)\.unwrap\(\),\s*(\d+)\)", body).group(1))], np.int32)
    for op in ("add", "mul"):
        body = test_body(bs, f"test_bsequence_{op}")
        assert np.array_equal(byte_vector(body, "v0"), out["v0"]) and np.array_equal(byte_vector(body, "v1"), out["v1"])
        out[f"{op}_bits"] = index_bits(body, "r")
    body = test_body(bs, "test_bsequence_accumulate")
    out["accumulate_v"] = byte_vector(body, "v")
    out["accumulate"] = np.array([int(re.search(r"accumulate\(\),\s*(\d+)\)", body).group(1))], np.uint32)
    np.savez_compressed(HERE / "sequence.npz", **out)
    print(f"sequence.npz: {len(out)} arrays, {sum(a.size for a in out.values())} values")


if __name__ == "__main__":
    main()
