"""tests/gcm_records_cases.py without a device: the generated record lengths reach every boundary of k_gcm_records'
arrangement rule and of gh_tree_groups' row skipping, and no test hands the compiled reference more than it finishes in
a few seconds.

Which live counts matter (read from gh_tree_groups): the level with table H^m, m = 256, 64, 16, 4, skips
k0 = 4 - ceil(lv / m) rows of a group with lv = min(live, 4 m), so its boundaries are the multiples of m up to 4 m; the
last level takes min(live, 4) entries.  The multiples of 4 up to 16, of 16 up to 64, of 64 up to 256 and of 256 up to 1024
are therefore all among the multiples of 4 up to 128 and the multiples of 16 beyond: lengths_for covers the former with
every count up to 130 and the latter, with both neighbours, all the way to the longest record -- which also puts a
record on either side of S in the two-position forms, where the fold by H^S meets records that fit in one position."""
import random

import pytest

from tests import gcm_records_cases as GC

FORMS = [(t, name) for t in GC.TARGETS for name in GC.AAD_FORMS if name == "none" or t in GC.UPPER_TARGETS]


def test_the_rule_has_six_arrangements_and_the_targets_sit_on_their_edges():
    seen = []
    for n in range(0, GC.record_max(0) + 1, 16):
        a = GC.arrangement(0, n)
        if not seen or seen[-1] != a:
            seen.append(a)
    assert tuple(seen) == GC.ARRANGEMENTS
    for t in GC.TARGETS:
        n = GC.max_len_for(t, 0)
        assert GC.positions(0, n) + 1 == t
    for t, a in zip(GC.UPPER_TARGETS, GC.ARRANGEMENTS):
        for aad_len, _ in GC.AAD_FORMS.values():
            n = GC.max_len_for(t, aad_len)
            assert GC.positions(aad_len, n) + 1 == t and GC.arrangement(aad_len, n) == a
            if t < 2047:
                assert GC.arrangement(aad_len, n + 1) != a
    assert GC.max_len_for(2047, 0) == GC.record_max(0) == 16 * 2045
    assert GC.record_max(16 * 2045) == 0 and GC.record_max(16 * 2044) == 16 and GC.record_max(17) == 16 * 2043
    assert GC.record_max(16 * 2045 + 1) == 0 and GC.positions(16 * 2045, 0) == GC.MAXNV
    with pytest.raises(ValueError):
        GC.arrangement(0, GC.record_max(0) + 1)
    assert [GC.groups(S) for S, _ in GC.ARRANGEMENTS] == [16, 16, 4, 4, 1, 1]


@pytest.mark.parametrize("target,form", FORMS)
def test_lengths_reach_every_boundary(target, form):
    aad_len, _ = GC.AAD_FORMS[form]
    max_len = GC.max_len_for(target, aad_len)
    S, steps = GC.arrangement(aad_len, max_len)
    lens = GC.lengths_for(aad_len, max_len, random.Random(target))
    assert lens == GC.lengths_for(aad_len, max_len, random.Random(target)), "seeded: the same list every time"
    live = {GC.positions(aad_len, n) for n in lens}
    lo, hi = GC.positions(aad_len, 0), GC.positions(aad_len, max_len)
    assert hi + 1 == target and hi <= steps * S - 1 and min(live) == lo and max(live) == hi
    marks = set(range(4, 129, 4)) | set(range(16, steps * S, 16)) | {S}
    for k in (4, 16, 64, 256):
        assert set(range(k, min(4 * k, steps * S - 1) + 1, k)) <= marks
    for m in sorted(marks):
        for v in (m - 1, m, m + 1):
            if lo <= v <= hi:
                assert v in live, "no record with %d positions (boundary %d)" % (v, m)
    assert 0 in lens and lens[0] == max_len and lens[-1] == max_len and max(lens) == max_len
    assert any(n % 16 == 0 for n in lens[1:-1]) and any(n % 16 == 15 for n in lens) and any(n % 16 == 1 for n in lens)
    G = GC.groups(S)
    turns = [set(lens[i:i + G]) for i in range(0, len(lens) - G + 1, G)]
    assert G == 1 or sum(len(t) > 1 for t in turns) >= len(turns) - 1, "the groups of a turn hold unlike lengths"
    assert GC.reference_bytes(lens, aad_len) <= GC.REF_CAP


@pytest.mark.parametrize("aad_len", [0, 13, 33])
def test_fixed_lengths(aad_len):
    cases = GC.fixed_lengths(aad_len)
    reached = {GC.positions(aad_len, n) + 1 for n, _ in cases}
    for b in (64, 128, 256, 512, 1024):
        assert {b - 1, b, b + 1} <= reached
    assert set(range(max(2, GC.blocks(aad_len) + 2), 7)) <= reached and 2047 in reached
    assert {GC.arrangement(aad_len, n) for n, _ in cases} == set(GC.ARRANGEMENTS)
    assert all(nrec == GC.groups(GC.arrangement(aad_len, n)[0]) + 1 for n, nrec in cases)
    assert {n % 16 for n, _ in cases} == {0, 1, 15}
    assert sum(GC.reference_bytes([n] * nrec, aad_len) for n, nrec in cases) <= GC.REF_CAP


def test_turn_forms_and_counts():
    forms = GC.turn_forms()
    assert [(S, steps) for S, steps, _ in forms] == [(64, 1), (256, 1), (256, 2), (1024, 1), (1024, 2)]
    assert [n for _, _, n in forms] == [1, 2017, 4065, 8161, 16353]
    for S, steps, n in forms:
        assert n == 1 or GC.arrangement(0, n - 16) != (S, steps)
        G = GC.groups(S)
        for cus in (256, 304):
            counts = GC.turn_counts(cus, G)
            turns = [(c + G - 1) // G for c in counts]
            assert turns == ([cus, cus, cus + 1, 2 * cus + 1] if G > 1 else [cus - 1, cus, cus + 1, 2 * cus])
            assert [c % G for c in counts] == [(G - 1) % G, 0, 1 % G, (G - 1) % G]
            # the reference answers are made once for the largest count and shared by the four
            assert GC.reference_bytes([n] * counts[-1], 0) <= GC.REF_CAP
            lens = GC.turn_lengths(n, counts[-1], S + steps)
            assert lens[0] == 0 and lens[1] == n and max(lens) == n and GC.reference_bytes(lens, 0) <= GC.REF_CAP
