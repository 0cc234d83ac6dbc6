"""The lists of tests/gcm_stream_cases.py hold what they claim (no device: the planners answer for 256 CUs).

Every coverage claim the GPU tests rely on is checked here on the lists the generator produces: each arrangement as a
stream's first, middle and last piece, each boundary of the piece planner, each first counter, stripe count, tail and
ragged end of the striped piece, each ordered pair of piece kinds under each mask, each rebuild and reuse of the cached
tables, each placement -- and the oracle's budget, the fixed message set, and that the prefix tags are the oracle's."""
import collections

import micro_aes_amd as uaes
from tests import gcm_stream_cases as G

ALL = [c for cs in G.items().values() for c in cs]


def by_group(g):
    return [c for c in ALL if c.group == g]


def test_the_piece_planner_has_the_boundaries_the_cases_are_built_on():
    bs = G.piece_bounds()
    cus = G.cus()
    assert [(below, above) for _b, below, above in bs] == [("d", "c1"), ("c1", "c2"), ("c2", "c4"), ("c4", "t")]
    b16k, b2, b4, btwo = [b for b, _below, _above in bs]
    # one chunk workgroup and the finisher; then as many chunk workgroups as CUs before the positions per thread double
    assert uaes.plan_gcm_piece(b16k) == ("gcm.chunks", 1, 1, 1) and uaes.plan_gcm_piece(b16k - 16)[:2] == ("gcm.levels", 0)
    assert uaes.plan_gcm_piece(b2 - 16) == ("gcm.chunks", 1, cus, 1) and uaes.plan_gcm_piece(b2)[3] == 2
    assert uaes.plan_gcm_piece(b4 - 16) == ("gcm.chunks", 1, cus, 2) and uaes.plan_gcm_piece(b4)[3] == 4
    assert uaes.plan_gcm_piece(btwo - 16) == ("gcm.chunks", 1, cus, 4) and uaes.plan_gcm_piece(btwo)[::3] == ("gcm.twophase", 8)
    assert b16k == 16 * 1024 and b2 == 2 * (b4 - 16) // 4 + 16 and btwo == 2 * (b4 - 16) + 16
    # the longest piece of the parity suite's stream test is far below the striped arrangement's own start
    pieces, mask = G.group_f()[0]
    assert mask == 0 and uaes.plan_gcm_piece(pieces[0] - 16 * G.STRIPE)[0] == "gcm.twophase"
    assert uaes.plan_gcm_piece(pieces[0] - 16 * G.STRIPE + 16)[0] == "gcm.striped"
    for dec in (False, True):
        assert [uaes.plan_gcm_piece(p, sum(pieces[:k]), dec)[0] for k, p in enumerate(pieces)] == \
            ["gcm.striped", "gcm.levels", "gcm.striped", "gcm.levels"]
    # the counter position crosses 2^23 blocks inside the first long piece and 2^24 inside the second
    assert 2 < (1 << 23) < 2 + pieces[0] // 16 and 2 + sum(pieces[:2]) // 16 < (1 << 24) < 2 + sum(pieces[:3]) // 16
    assert sum(pieces) == 2 * (128 * G.MIB + 32 * 1024) + 48


def test_every_case_is_a_splitting_of_a_fixed_message():
    ms = G.messages()
    assert len(ALL) > 150 and len(ms) <= 13
    for c in ALL:
        assert c.msg in ms and c.place in G.PLACES and c.look in (None, 0), c
        assert all(p > 0 and p % 16 == 0 for p in c.pieces[:-1]) and c.pieces[-1] > 0, c
        n = sum(c.pieces)
        assert n <= ms[c.msg].text_len, c
        if G.is_prefix(c):
            assert c.pieces[-1] % 16 and ms[c.msg].oracle, c             # only a ragged last piece needs a prefix
        # the same kinds in both directions (G.simulate is asked for both), and no arrangement the mask switched off
        assert G.kinds(c) == G.kinds(c, True), c
        done = 0
        for p in c.pieces:
            name = G.piece_plan(c.mask, p, done)[0]
            assert name == "gcm.levels" or not c.mask & G.mask_of(name), (c, p)
            done += p
    assert {ms[c.msg].bits for c in ALL} == {128, 192, 256}
    # groups C and D run with AES-128, and so does E but for the second of its two streams side by side
    assert {ms[c.msg].bits for c in ALL if c.group in "CD"} == {128}
    assert sorted(ms[c.msg].bits for c in ALL if c.group == "E" and c.note == "side by side") == [128, 192]
    assert {ms[c.msg].bits for c in ALL if c.group == "E" and c.note != "side by side"} == {128}
    sizes = sorted(m.text_len for m in ms.values() if m.name[0] == "m")
    assert sizes[-1] == G.TOP - 3 and 8.0 * G.MIB < sizes[-2] < 8.3 * G.MIB and 1.0 * G.MIB < sizes[0] < 1.2 * G.MIB


def test_the_oracle_budget():
    """conditions, not measurements: at most ITEM_CAP bytes per test item, FILE_CAP for the file"""
    assert G.ITEM_CAP == 40 * G.MIB and G.FILE_CAP == 110 * G.MIB
    for name, cases in G.items().items():
        assert G.oracle_bytes(cases) <= G.ITEM_CAP, (name, G.oracle_bytes(cases))
    assert G.oracle_bytes(ALL) <= G.FILE_CAP, G.oracle_bytes(ALL)
    # (the two tests of Group E that are no item use the messages of item E and no prefix); Group F's two heads
    assert G.oracle_bytes(ALL) + 2 * G.HEAD <= G.FILE_CAP


def test_prefix_tags_are_the_oracles(orc):
    m = G.Message("t", 192, 21, 5 * 4096 + 7, 5, True)
    r = G.Reference(orc, m, seg=4096)
    # from the front, from the back (out of the tag of the whole message) and from the side the cases take: in and
    # next to the first, a middle and the last segment, on and next to a segment's and a block's edge
    for n in (1, 15, 16, 4095, 4096, 4097, 2 * 4096 + 2048, 3 * 4096 + 33, 4 * 4096 - 16, 4 * 4096, 4 * 4096 + 1, 5 * 4096 - 1,
              5 * 4096, 5 * 4096 + 6, m.text_len):
        want = orc.gcm_encrypt(r.key, r.nonce, r.aad, r.text[:n])
        assert want[:n] == r.ct[:n], n
        assert want[n:] == r.prefix_tag(n) == r.prefix_tag(n, back=False) == r.prefix_tag(n, back=True), n
    assert not G.from_back(m, m.text_len // 2) and G.from_back(m, m.text_len // 2 + 1)
    # a message of whole segments, no associated data; and the passes asked for in the other order
    m0 = G.Message("t0", 128, 0, 3 * 4096, 6, True)
    for ns in ((16, 4096 + 5, 2 * 4096, 2 * 4096 + 17, 3 * 4096 - 1), (3 * 4096 - 1, 2 * 4096 + 17, 2 * 4096, 4096 + 5, 16)):
        r0 = G.Reference(orc, m0, seg=4096)
        for n in ns:
            want = orc.gcm_encrypt(r0.key, r0.nonce, b"", r0.text[:n])[n:]
            assert want == r0.prefix_tag(n, back=False) == r0.prefix_tag(n, back=True), n


def test_prefix_bytes_counts_what_the_reference_hands_over(orc):
    """the budget's count against the bytes Reference really passes to orc.ghash"""
    m = G.Message("t", 256, 21, 9 * 4096 + 7, 5, True)
    prefixes = [15, 4096 + 33, 3 * 4096, 6 * 4096 - 16, 6 * 4096 + 1, 8 * 4096 + 100, 9 * 4096 + 3]

    class Counting:
        def __init__(self):
            self.n = 0

        def __getattr__(self, name):
            return getattr(orc, name)

        def ghash(self, h, aad, data):
            self.n += len(aad) + len(data)
            return orc.ghash(h, aad, data)

    co = Counting()
    r = G.Reference(co, m, seg=4096)
    for n in prefixes:
        r.prefix_tag(n)
    assert 0 < co.n == G.prefix_bytes(m, prefixes, seg=4096)


def test_group_a_takes_every_boundary_as_middle_first_and_last_piece():
    a = by_group("A")
    for b, below, above in G.piece_bounds():
        for look in (None, 0):
            mine = [c for c in a if c.look == look and c.note.startswith("%s->%s" % (below, above))]
            assert {c.pieces[1] for c in mine if c.note.endswith("middle") and G.messages()[c.msg].bits == 128} == {b - 16, b, b + 16}
            assert [c.pieces[0] for c in mine if c.note.endswith("first")].count(b) >= 1
            last = {c.pieces[-1]: c for c in mine if c.note.endswith("last")}
            assert set(last) == {b - 3, b + 1}
            assert G.kinds(last[b - 3])[-1] == above and G.kinds(last[b + 1])[-1] == above
            for c in mine:
                if c.note.endswith("middle"):
                    assert G.kinds(c)[1] == (below if c.pieces[1] < b else above), c
    # the first boundary at all three key sizes, in every form
    b, below, above = G.piece_bounds()[0]
    for bits in (128, 192, 256):
        mine = [c for c in a if c.note.startswith("%s->%s" % (below, above)) and G.messages()[c.msg].bits == bits]
        for look in (None, 0):
            assert {(c.note.split()[-1], c.pieces[0 if c.note.endswith("first") else 1]) for c in mine if c.look == look} == \
                {("middle", b - 16), ("middle", b), ("middle", b + 16), ("first", b), ("last", b - 3), ("last", b + 1)}, bits
    # each arrangement as a stream's first, middle and last piece, somewhere in the file
    seen = collections.defaultdict(set)
    for c in ALL:
        ks = G.kinds(c)
        seen[ks[0]].add("first")
        seen[ks[-1]].add("last")
        for k in ks[1:-1]:
            seen[k].add("middle")
    for kind in ("d", "a14", "c1", "c2", "c4", "t", "s"):
        assert seen[kind] == {"first", "middle", "last"}, (kind, seen[kind])


def _striped_piece(c):
    """(index, done) of the piece a Group B case is about: its longest"""
    k = c.pieces.index(max(c.pieces))
    return k, sum(c.pieces[:k])


def test_group_b_covers_stripes_counters_tails_and_ragged_ends():
    cus = G.cus()
    both = G.mask_of(G.CH, G.TP)
    b = [c for c in by_group("B") if c.mask == both]
    cells, row, full = set(), set(), set()
    for c in b:
        k, done = _striped_piece(c)
        n = c.pieces[k]
        h0, g_lo, n8, h1 = G.geometry_at(done, n)
        c0 = G.c0_at(done)
        assert (h0, g_lo) == ((G.GROUP - c0) % G.GROUP, 1 if c0 else 0)
        assert G.kinds(c)[k] == ("s" if n8 >= cus else "a14"), c
        cells.add((n8, c0, G.messages()[c.msg].bits))
        if G.messages()[c.msg].bits == 128:
            full.add((n8, c0, n // 16 - h1, n % 16))
        if n % 16:
            assert k == len(c.pieces) - 1, c                            # the ragged forms are last pieces
            assert G.is_prefix(c), c
        if n8 == cus:
            row.add((G.messages()[c.msg].bits, c0, n // 16 - h1, n % 16))
        else:
            assert G.messages()[c.msg].bits == 128, c
    assert {(n8, c0) for n8, c0, bits in cells if bits == 128} == {(n8, c0) for n8 in G.n8s() for c0 in G.C0S}
    assert full == {(n8, c0, t, r) for n8 in G.n8s() for c0 in G.C0S for t in G.TAILS for r in G.RAGGED}
    assert G.n8s() == (cus - 1, cus, cus + 1, 2 * cus - 1) and G.C0S == (2, 255, 0, 1)
    assert {(c0, bits) for n8, c0, bits in cells if n8 == cus} == {(c0, bits) for c0 in G.C0S for bits in (128, 192, 256)}
    # the n8 = CUs row whole at all three key sizes: first counter x tail x ragged end ((0, r): no whole tail block at all)
    assert row == {(bits, c0, t, r) for bits in (128, 192, 256) for c0 in G.C0S for t in (0, 1, 2047) for r in (0, 1, 15)}
    assert G.TAILS == (0, 1, G.STRIPE - 1) and G.RAGGED == (0, 1, 15)
    # gcm.twophase alone: a chunk piece (or a direct one), then the first two-phase length striped, no chunk switch between
    alone = [c for c in by_group("B") if c.mask == G.mask_of(G.TP)]
    assert sorted(G.kinds(c)[0] for c in alone) == ["c1", "d"]
    for c in alone:
        assert G.kinds(c)[1] == "s" and "t" not in G.kinds(c) and c.pieces[1] == G.piece_bounds()[3][0], c


def test_group_c_covers_every_pair_and_every_cache_event():
    cs = by_group("C")
    for names in G.C_MASKS:
        mask = G.mask_of(*names)
        got = set()
        for c in cs:
            if c.mask == mask and c.msg == "m17":
                ks = G.kinds(c)
                got |= set(zip(ks, ks[1:]))
        want = set(G.feasible_pairs(mask, G.messages()["m17"].text_len))
        assert want and want <= got, (names, want - got)
        kinds = {k for p in want for k in p}
        assert kinds == {(): {"d", "c1", "c2", "c4", "t"}, (G.CH,): {"d", "a14", "s", "t"}, (G.CH, G.TP): {"d", "a14", "s"},
                         (G.TP,): {"d", "c1", "c2", "c4", "s"}}[names], (names, kinds)
        # every pair that fits the message is there: what is left out does not fit
        first = G.first_lengths(mask, G.messages()["m17"].text_len)
        for x in kinds:
            for y in kinds:
                assert (x, y) in want or first[x] + first[y] > G.messages()["m17"].text_len - 16 * 2 * G.GROUP, (names, x, y)

    def named(seq):
        """the stream that starts with these kinds"""
        return [c for c in cs if G.kinds(c)[:len(seq)] == list(seq)][0]

    valid = True
    c = named(("s", "d", "s"))
    assert G.simulate(c)[0][:4] == [(valid, 0, False, False)] + [(valid, 0, False, True)] * 3
    assert G.simulate(c)[1][:2] == [("striped", "rebuilt"), ("striped", "reused")]
    c = named(("s", "a14", "s"))
    assert G.simulate(c)[0][:4] == [(valid, 0, False, False), (valid, 0, False, True), (valid, 14, False, True), (valid, 14, False, True)]
    assert G.simulate(c)[1][:3] == [("striped", "rebuilt"), ("logA", "rebuilt"), ("striped", "reused")]
    c = named(("a14", "d", "a14"))
    assert c.msg == "m1" and G.simulate(c)[1][:2] == [("logA", "rebuilt"), ("logA", "reused")]
    assert G.simulate(c)[0][:4] == [(valid, 0, False, False)] + [(valid, 14, False, False)] * 3
    # associated data at begin: each length, then a direct piece and a chunk piece
    direct = 16 * G.GH_DIRECT
    aads = {G.messages()[c.msg].aad_len: c for c in cs if c.msg.startswith("aad") and c.msg != "aad32.s"}
    assert sorted(aads) == [0, 1, 16, 17, direct, direct + 1, 64 * direct + 16] and direct == 512 * 1024
    for alen, c in aads.items():
        assert G.kinds(c) == ["d", "c1"] and c.mask == 0
        lg = 0 if alen <= direct else 14 if alen <= 32 * direct else 16
        assert G.simulate(c)[0] == [(valid, lg, lg == 16, False)] * 3, (alen, G.simulate(c))
    c = [c for c in cs if c.msg == "aad32.s"][0]
    assert c.mask == G.mask_of(G.CH, G.TP) and G.kinds(c)[0] == "s"
    assert G.simulate(c)[0][:2] == [(valid, 16, True, False), (valid, 0, False, True)]
    # over the group and Group F: rebuilt and reused for each table
    events = set()
    for c in cs:
        events |= set(G.simulate(c)[1])
    for pieces, mask in G.group_f():
        events |= set(G.simulate_pieces(0, pieces, mask)[1])
    assert events == {(t, e) for t in ("logA", "B", "striped") for e in ("rebuilt", "reused")}
    assert ("B", "reused") in G.simulate_pieces(0, *G.group_f()[1])[1]


def test_group_d_runs_every_boundary_and_smallest_striped_piece_three_ways():
    d = by_group("D")
    shapes = collections.defaultdict(set)
    for c in d:
        shapes[(c.msg, tuple(c.pieces), c.mask)].add(c.place)
    assert all(v == set(G.PLACES) for v in shapes.values())
    bs = [b for b, _below, _above in G.piece_bounds()]
    assert {p[1] for (_m, p, mask) in shapes if mask == 0 and len(p) == 3} == set(bs)
    assert {p[1] for (_m, p, mask) in shapes if mask == 0 and len(p) == 2} == {b + 1 for b in bs}
    b_cus = {(c.msg, tuple(c.pieces), c.mask) for c in by_group("B")
             if G.messages()[c.msg].bits == 128 and c.mask == G.mask_of(G.CH, G.TP)
             and G.geometry_at(_striped_piece(c)[1], c.pieces[_striped_piece(c)[0]])[2] == G.cus()}
    assert len(b_cus) == len(G.C0S) * len(G.TAILS) * len(G.RAGGED) and b_cus <= set(shapes)
    # the three orders that are built around "in may be out", decrypting in place
    inplace = [G.kinds(c, True) for c in d if c.place == "inplace"]
    assert any("s" in ks for ks in inplace) and any("t" in ks for ks in inplace) and any("d" in ks for ks in inplace)


def test_group_e_streams():
    e = G.group_e()
    side = [c for c in e if c.note == "side by side"]
    assert len(side) == 2 and G.key_of(G.messages()[side[0].msg]) != G.key_of(G.messages()[side[1].msg])
    for c in side:
        assert G.kinds(c)[:4] == ["d", "c1", "d", "c2"] and c.mask == 0
    full = [c for c in e if c.note.startswith("leaves")][0]
    last = G.simulate(full)[0][-1]
    assert last[3] and last[1] == 14
    after = [c for c in e if c.note == "on a recycled scratch"]
    assert len(after) == 2 and all(G.kinds(c)[:2] == ["d", "c1"] for c in after)
    assert len({G.key_of(G.messages()[c.msg]) for c in after + [full]} | {G.key_of(G.messages()["m8"])}) == 4
