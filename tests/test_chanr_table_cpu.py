"""The committed micro-benchmark table of FirPfbChr (profiles/r13_kbench_chanr.txt, the raw output of tools/kb_chanr.py on
an MI355X) against the rule kernel choice auto follows (chanr_ref.auto_takes_column, which tests/test_gpu_chanr.py holds
the library to): in every row the `auto` column is what the rule gives; wherever the rule takes the column kernel it was
faster than the general one, in that row and in the row of the same shape at the other block length; and for the
zero-padded branch lengths, which the rule sends to the column kernel only at P/gcd(M, P) = 1, the column kernel at the
built length beats the general kernel at half that length."""
import math

from chanr_ref import auto_takes_column
from conftest import ROOT


def _rows():
    rows = []
    for line in (ROOT / "profiles" / "r13_kbench_chanr.txt").read_text().splitlines():
        f = line.split()
        if f and f[0] == "ana":
            rows.append(dict(M=int(f[1]), P=int(f[2]), p=int(f[3]), n=int(f[4]), gen=float(f[5]), col=float(f[7]),
                             auto=int(f[11])))
    return rows


def test_the_table_covers_every_served_built_shape_at_both_block_lengths():
    seen = {(r["M"], r["P"], r["p"], r["n"] > (1 << 22)) for r in _rows()}
    want = {(M, a * M // 8, p, big) for M in (64, 128, 256) for a in range(1, 9) for p in (4, 8, 16) for big in (False, True)}
    assert seen == want


def test_auto_in_the_table_is_the_rule_and_the_rule_takes_the_column_kernel_only_where_it_was_faster():
    rows = _rows()
    by_shape = {}
    for r in rows:
        by_shape.setdefault((r["M"], r["P"], r["p"]), []).append(r)
    for r in rows:
        rule = auto_takes_column(r["M"], r["P"], r["p"] // 2, r["n"] // r["P"])
        assert r["auto"] == (2 if rule else 1), r
        if rule:
            assert all(o["col"] < o["gen"] for o in by_shape[(r["M"], r["P"], r["p"])]), r


def test_zero_padded_lengths_at_unit_slide_beat_the_general_kernel_at_half_the_taps():
    rows = {(r["M"], r["P"], r["p"], r["n"]): r for r in _rows()}
    checked = 0
    for (M, P, p, n), r in rows.items():
        if P // math.gcd(M, P) == 1 and p in (8, 16):
            half = rows[(M, P, p // 2, n)]
            assert r["col"] < half["gen"], (r, half)
            checked += 1
    assert checked == 3 * 4 * 2 * 2
