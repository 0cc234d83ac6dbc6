"""tests/xts_cases.py without a device: the spot reference equals the oracle at every block, the case lists of
tests/test_gpu_xts.py hold what they claim (read against k_xts_small, k_xts_tweaks, k_xts_expand, k_xts and k_xts_cts in
csrc/uaes_kernels.hip), and the oracle is handed no more than it finishes in about ten seconds.  The plan and the shape
hook answer here for a 256-CU MI355X, the device the GPU file runs on."""
import random

import micro_aes_amd as uaes
from tests import xts_cases as XC


# ---- the spot reference -----------------------------------------------------------------------------------------------
def test_field_arithmetic_against_plain_doubling():
    cur = 1
    for j in range(1, 3000):
        cur <<= 1
        if cur >> 128:
            cur = (cur & XC.M128) ^ 0x87
        if j < 300 or j % 97 == 0:
            assert XC.alpha_pow(j) == cur, j
    rng = random.Random(5)
    for _ in range(50):
        a, b, c = (rng.getrandbits(128) for _ in range(3))
        assert XC.gf_mul(a, b) == XC.gf_mul(b, a) and XC.gf_mul(a, 1) == a
        assert XC.gf_mul(XC.gf_mul(a, b), c) == XC.gf_mul(a, XC.gf_mul(b, c))
    assert XC.gf_mul(XC.alpha_pow(1 << 20), XC.alpha_pow((1 << 26) + 5)) == XC.alpha_pow((1 << 20) + (1 << 26) + 5)


SPOT_UNITS = list(range(16, 32)) + [32, 33, 47, 4096 - 17, 4096 + 17] + [16400 + r for r in range(16)]


def test_spot_reference_equals_the_oracle_at_every_block_and_the_tail(orc):
    rng = random.Random(38)
    for unit in SPOT_UNITS:
        keys = XC.keys_for(unit)
        tweak = rng.randbytes(16)
        spot = XC.Spot(orc, keys, tweak)
        for decrypt in (False, True):
            data = rng.randbytes(unit)
            rc, want = orc.xts(keys, tweak, data, not decrypt)
            assert rc == 0 and spot.unit(data, decrypt) == want, (unit, decrypt)


def test_spot_reference_equals_the_oracle_over_numbered_units(orc):
    rng = random.Random(39)
    for unit in (16, 17, 31, 33, 47, 4096 - 17, 4096 + 17):
        keys = XC.keys_for(unit)
        for first in (0, XC.SECTOR_CARRY, XC.SECTOR_WRAP):
            for decrypt in (False, True):
                data = rng.randbytes(3 * unit)
                rc, want = orc.xts_sectors(keys, first, unit, data, not decrypt)
                got = b"".join(XC.Spot(orc, keys, first + i).unit(data[i * unit:(i + 1) * unit], decrypt) for i in range(3))
                assert rc == 0 and got == want, (unit, first, decrypt)


# ---- the groups -------------------------------------------------------------------------------------------------------
def test_group_a_walks_every_run_chunk_and_table_edge_of_one_unit():
    cases = XC.group_a()
    assert all(c.n == 1 and c.tweak is not None and XC.shape_of(c).name == ("xts.bulk" if 16 < c.unit < 32 else "xts.small") for c in cases)
    explicit = {c.unit for c in cases if c.tweak == XC.TWEAK}
    null = {c.unit for c in cases if c.tweak == XC.NULL_TWEAK}
    assert explicit == {c.unit for c in cases} and null == {u for u in explicit if u // 16 <= 1025}
    ws = {u // 16 for u in explicit}
    for edge in (64, 256, 512, 1024, 16384, 16384 + 256, 32768):       # a run, a chunk, two, a workgroup, bit 0 of the group, a chunk beyond, bit 1
        assert {edge - 1, edge, edge + 1} <= ws
    assert {1, 2, 49152} <= ws and (49152 // 256 // 64) == 3           # both bits of the group index
    for w in ws:
        assert {u % 16 for u in explicit if u // 16 == w} == ({0, 1, 15} if w < 1024 else {0, 15})
    heads = sorted({c.unit // 16 for c in cases if c.note == "empty head"})
    assert heads == [257, 513, 1025, 16385, 16384 + 257, 32769]
    for c in cases:
        mb, r, cps = XC.geometry(c.unit)
        assert (c.note == "empty head") == (r != 0 and 4 * cps > (mb + 63) // 64 and mb > 0 and mb % 256 == 0)
        assert XC.shape_of(c).cps == cps


def test_group_b_walks_the_run_to_unit_mapping():
    cases = XC.group_b()
    assert all(XC.shape_of(c).name == "xts.small" and c.tweak is None and c.unit % 16 == 0 for c in cases)
    for first in XC.B_FIRST:
        mine = [c for c in cases if c.first == first and not c.note]
        assert {(c.unit // 16, c.n) for c in mine} == {(mb, n) for mb in XC.B_MB for n in XC.B_COUNTS}
    for edge in (64, 128, 256):                                       # 64-block runs: a unit of one run less a block, exactly, and a block more
        assert {edge - 1, edge, edge + 1} <= set(XC.B_MB)
    assert {1, 2, 3, 4, 260} <= set(XC.B_MB) and {2, 3, 17, 64, 65} == set(XC.B_COUNTS)
    # the carry into the second word of the unit number and the wrap to zero happen at unit 2, inside every call but n = 2
    assert XC.SECTOR_CARRY + 2 == 1 << 32 and XC.SECTOR_WRAP + 2 == 1 << 64
    last = {c.unit // 16: c for c in cases if c.note == "last small"}
    assert sorted(last) == [1, 64, 256]
    for mb, c in last.items():
        assert uaes.plan("xts", c.unit, c.n)[0] == "xts.small" and uaes.plan("xts", c.unit, c.n + 1)[0] != "xts.small"
        assert XC.shape_of(c).grid * 16 >= c.n * -(-mb // 64) > (XC.shape_of(c).grid - 1) * 16          # a wave per run


def test_group_c_has_all_63_sizes_and_the_division_steps():
    cases = XC.group_c()
    off = [c for c in cases if c.no_small and c.note != "stepping"]
    assert {c.unit for c in off} == set(range(64, 4033, 64)) and len({c.unit for c in off}) == 63
    for c in cases:
        s = XC.shape_of(c)
        assert s.name == "xts.packed" and s.nmain == s.chunks == -(-c.n * (c.unit // 16) // 256), c
    for unit in XC.C_SIZES:
        mb = unit // 16
        mine = {c.note: c.n * mb for c in off if c.unit == unit}
        assert ("below a chunk" in mine) == (2 * mb < 256) and mine.get("below a chunk", 1) < 256
        exists = any(k * 256 % mb == 0 and k * 256 // mb >= 2 for k in (1, 2, 3, 4))
        assert ("whole chunks" in mine) == exists and mine.get("whole chunks", 256) % 256 == 0 and mine.get("whole chunks", 256) <= 1024
        part = mine["three chunks and a part"]
        assert 768 < part < 1024 and part % 256 != 0                  # lanes of the fourth chunk lie past the last unit
        # the multiplication that stands for the division, for every x a lane can have (the kernel's comment: x < 512)
        magic = ((1 << 24) + mb - 1) // mb
        assert all((x * magic) >> 24 == x // mb for x in range(512))
    real = [c for c in cases if not c.no_small]
    assert {c.unit for c in real} == {64, 2112, 4032}
    for unit in XC.C_REAL:
        ns = sorted(c.n for c in real if c.unit == unit)
        assert len(ns) == 2 and ns[1] == ns[0] + 1 and uaes.plan("xts", unit, ns[0] - 1)[0] == "xts.small"
    step = [c for c in cases if c.note == "stepping"]
    assert len(step) == 1
    s = XC.shape_of(step[0])
    assert s.chunks > XC.waves(s) and (XC.waves(s) * 256) % (step[0].unit // 16) != 0 and step[0].unit * step[0].n <= XC.SHA_ABOVE
    with XC.small_off():
        before = uaes.xts_plan(step[0].unit, step[0].n - 1)
    assert before.chunks <= XC.waves(before)


def test_group_d_has_every_quarter_and_the_empty_chunks():
    cases = XC.group_d()
    got = {(c.unit // 16 - 1, c.unit % 16, c.n) for c in cases}
    assert got >= {(m, r, n) for m in XC.D_M for r in XC.D_R for n in XC.D_COUNTS}
    ms = {m for m, _, _ in got}
    assert ms - set(XC.D_M) == {400} and all((400, r, 3) in got for r in XC.D_R)
    for quarter in range(4):                                          # m % 256 in each quarter of a chunk, below and beyond one chunk
        assert any(m % 256 // 64 == quarter and m < 256 for m in ms) and any(m % 256 // 64 == quarter and m >= 256 for m in ms)
    for edge in (64, 128, 192, 256, 320, 512):
        assert {edge - 1, edge} <= ms
    assert {m % 64 for m in ms} >= {0, 1, 63} and {m // 256 for m in ms} == {0, 1, 2, 3}
    assert max(XC.D_COUNTS) > 64                                      # a second wave of k_xts_cts, a second workgroup of k_xts_tweaks
    for c in cases:
        s, m = XC.shape_of(c), c.unit // 16 - 1
        assert s.name == "xts.bulk" and not s.aligned and s.serial and s.cps == m // 256 + 1
        assert (c.note == "empty chunk") == (m in XC.D_EMPTY) == (m > 0 and m % 256 == 0) == XC.empty_chunk(c.unit)
        if c.note == "empty chunk":
            assert s.chunks > c.n * -(-m // 256)                      # chunks in all exceed nsectors * ceil(mb / 256)
        elif m:
            assert s.chunks == c.n * -(-m // 256)


def test_group_e_sits_on_both_sides_of_every_round_edge():
    for unit in XC.E_UNITS:
        c = XC.body_chunks(unit)
        assert XC.shape_of(XC.case("E", unit, 2, no_small=True)).cps == c == {80: 1, 272: 1, 4112: 2, 9616: 3}[unit]
        for wg16 in ((False, True) if unit in XC.E_UNITS_16 else (False,)):
            mine = [x for x in XC.group_e(unit) if x.note.startswith("16-wave" if wg16 else "4-wave")]
            shapes = {x.n: XC.shape_of(x) for x in mine}
            assert all(s.name == "xts.bulk" and s.threads == (1024 if wg16 else 256) and s.aligned and not s.allfull for s in shapes.values())
            W = max(XC.waves(s) for s in shapes.values())
            assert W == (4096 if wg16 else 1024) and all(XC.waves(s) == W for s in shapes.values())
            chunks = {n * c for n in shapes}
            assert all(s.chunks == n * c for n, s in shapes.items())
            for t in (W - 1, W, W + 1) + ((2 * W + 1,) if wg16 else ()):
                assert any(t - c < k <= t for k in chunks) and any(t <= k < t + c for k in chunks), (unit, wg16, t)
            if not wg16:
                assert all(k <= 2048 for k in chunks) and (c > 1 or 2 * W in chunks)
            q = [x for x in mine if x.note.endswith("quarter side")][0]
            m = [x for x in mine if x.note.endswith("main side")][0]
            assert m.n == q.n + 1 and shapes[q.n].nmain == W < shapes[q.n].chunks and shapes[m.n].nmain == shapes[m.n].chunks
            assert (q.n * c - W) * 100 < W * 80 <= (m.n * c - W) * 100
            for n, s in shapes.items():                                  # which side each count is on
                left = n * c % W
                assert (s.nmain < s.chunks) == (n * c > W and left != 0 and left * 100 < W * 80), (unit, n)
            if wg16:
                assert all(x.no_small == (uaes.plan("xts", unit, x.n)[0] == "xts.small") for x in mine)
                assert any(not x.no_small for x in mine)
    # step_r != 0 needs a wave count that is no multiple of the chunks per unit
    assert 1024 % 3 != 0
    full = [x for x in XC.group_e() if x.note.startswith("all-full")]
    part = [x for x in XC.group_e() if x.note.startswith("aligned, not all-full")]
    assert len(full) == len(part) == 1
    sf, sp = XC.shape_of(full[0]), XC.shape_of(part[0])
    assert sf.allfull and sf.aligned and sf.chunks == XC.waves(sf) + 1 and full[0].unit == 4096
    assert not sp.allfull and sp.aligned and XC.waves(sp) < sp.chunks <= XC.waves(sp) + 2 and part[0].unit == 4096 + 16


def test_group_f_reaches_the_expansion_and_the_big_unit_thirteen_table_entries():
    cases = XC.group_f()
    assert {(XC.geometry(c.unit)[2], c.unit % 16) for c in cases} == {(cps, r) for cps in XC.F_CPS for r in XC.F_R}
    for c in cases:
        s = XC.shape_of(c)
        assert s.name == "xts.bulk" and c.n == 2 and s.cps == XC.geometry(c.unit)[2] and s.serial == (s.cps <= 128)
    serial = {XC.shape_of(c).cps for c in cases if XC.shape_of(c).serial}
    assert serial == {128} and {XC.shape_of(c).cps for c in cases} - serial == {129, 192, 193}
    assert (192 - 1) // 64 == 2 and 192 // 64 == 3                   # chunk 191 ends group 2, chunk 192 opens group 3
    # the big unit
    big = XC.big_case()
    mb, r, cps = XC.geometry(XC.BIG_UNIT)
    s = XC.shape_of(big)
    assert s.name == "xts.bulk" and not s.serial and s.cps == cps == (1 << 18) + 64 and r == 5 and mb == (1 << 26) + 63 * 256
    assert XC.empty_chunk(XC.BIG_UNIT) and s.chunks == cps and s.aligned and s.allfull
    spots = XC.big_unit_spots()
    groups = {blk // 256 // 64 for _, blk in spots}
    assert {1 << i for i in range(13)} <= groups and 4095 in groups and max(groups) == 4096       # entries 0..12, one by one and 0..11 together
    assert all(0 <= blk < mb for _, blk in spots) and {blk % 256 for _, blk in spots} == {0, 255}
    assert len(spots) == 2 * 15 and (mb - 1) in {blk for _, blk in spots}
    assert XC.big_unit_words(3) == (6 * XC.BIG_MUL % (1 << 64)).to_bytes(8, "little") + (7 * XC.BIG_MUL % (1 << 64)).to_bytes(8, "little")


def test_group_g_takes_one_case_of_each_kernel_family():
    cases = XC.group_g()
    assert [c.group for c in cases] == ["A", "B", "C", "D", "E", "E"]
    shapes = [XC.shape_of(c) for c in cases]
    assert [s.name for s in shapes] == ["xts.small", "xts.small", "xts.packed", "xts.bulk", "xts.bulk", "xts.bulk"]
    assert [s.threads for s in shapes[3:]] == [256, 256, 1024] and not shapes[3].aligned
    assert shapes[4].nmain < shapes[4].chunks and shapes[5].nmain < shapes[5].chunks
    assert XC.PLACES == ((False, 0), (True, 0), (True, 1), (True, 3))


# ---- the reference cap, and where spot compares are used ----------------------------------------------------------------
def test_the_oracle_is_handed_at_most_64_mib():
    cases = XC.whole_cases()
    total = XC.reference_bytes(cases)
    print("reference bytes: %d (%.2f MiB) for %d cases" % (total, total / XC.MIB, len(cases)))
    assert XC.REF_CAP == 64 << 20 and total <= XC.REF_CAP
    # nothing is counted twice or forgotten: every numbered case is a prefix of its family's text
    fam = XC.families(cases)
    assert all(c.n <= fam[(c.unit, c.first)] for c in cases if c.tweak is None)
    assert all(c.unit * c.n <= XC.SHA_ABOVE for c in cases)            # every whole compare is bytes against bytes


def test_spot_compares_only_where_the_case_list_says_so():
    assert all(XC.compare_of(c) == "whole" for c in XC.whole_cases())
    big = XC.big_case()
    assert XC.compare_of(big) == "spot" and big.group == "F" and big.unit == (1 << 30) + 63 * 4096 + 16 + 5
    assert big.unit not in {c.unit for c in XC.whole_cases()}
