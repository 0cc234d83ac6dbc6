"""The cases of tests/test_gpu_xts.py, made without a device, and an independent spot reference for XTS.

Every size that depends on what the launcher decides -- where "xts.small" ends, where "xts.packed" begins, how many waves
the chunk kernel's grid has, which chunk counts fall on either side of the 80 % rule -- is found by asking uaes.plan and
uaes.xts_plan (the launcher's own shape function, uaesk_plan_xts_shape); both answer without a device, for a 256-CU
MI355X.  tests/test_xts_cases.py proves that the lists below hold what they claim and that the oracle is handed at most
REF_CAP bytes.

A case is one call: `n` data units of `unit` bytes.  tweak None: the units are numbered from `first` (uaes_xts_sectors);
tweak bytes or NULL_TWEAK: one unit under an explicit 16-byte tweak (uaes_xts_encrypt / _decrypt; NULL_TWEAK passes a
NULL pointer, which the reference API reads as sixteen zero bytes).  no_small: the call runs with "xts.small" switched
off (uaes_debug_plan_disable).  The text of a numbered case is the first n * unit bytes of its FAMILY's stream -- one
stream per (unit, first) -- so the oracle's answer for the family's largest count holds the answer of every smaller
count as a prefix (units are independent) and is computed once."""
import collections
import contextlib

import micro_aes_amd as uaes

MIB = 1 << 20
CHUNK = 256                                  # blocks per chunk: what the hook's chunk counts count
RUN = 64                                     # blocks per run of k_xts_small (one per lane)
REF_CAP = 64 * MIB                           # bytes tests/test_gpu_xts.py may send through orc.xts / orc.xts_sectors
SHA_ABOVE = 20 * MIB                         # a longer text is compared by SHA-256
NULL_TWEAK = "null"
TWEAK = bytes(range(0xE0, 0xF0))
SECTOR_CARRY = (1 << 32) - 2                 # the unit number carries into its second word inside the call
SECTOR_WRAP = (1 << 64) - 2                  # ... and wraps to 0

Case = collections.namedtuple("Case", "group unit n first tweak no_small note")


def case(group, unit, n=1, first=0, tweak=None, no_small=False, note=""):
    return Case(group, unit, n, first, tweak, no_small, note)


# ---- keys and texts ---------------------------------------------------------------------------------------------------
def bits_for(unit):
    """the key size of a unit size: all three take part, and a family has one"""
    return (128, 256, 192)[(unit // 16) % 3]


def keys_for(unit):
    nb = bits_for(unit) // 8
    return bytes((0x31 + 11 * i + unit) & 0xff for i in range(2 * nb))


def seed_for(unit, first):
    return (unit * 1000003 + first) & 0x7fffffff


def text_for(orc, c, n=None):
    """the plaintext of a case (or of the first n units of its family)"""
    return orc.splitmix(seed_for(c.unit, c.first if c.tweak is None else 1), c.unit * (c.n if n is None else n))


# ---- geometry, restated from xts_geometry (csrc/uaes_kernels.hip) to NAME the cases; the counts come from the hook ----
def geometry(unit):
    """(mb, r, cps): blocks before the stealing pair, bytes of the tail, chunks per unit (block m's chunk included)"""
    whole, r = divmod(unit, 16)
    return whole - (1 if r else 0), r, max(1, -(-whole // CHUNK))


def body_chunks(unit):
    """the chunks of a unit that hold blocks of the chunk kernel's"""
    return -(-geometry(unit)[0] // CHUNK)


def empty_chunk(unit):
    """a ragged unit with a multiple of 256 blocks before the stealing pair: its last chunk holds block m's tweak and no
    block of the body (one unit: `heads` exceeds `runs_per_unit` in k_xts_small and a run without blocks writes that
    tweak; many units: chunks_per_sector exceeds the chunks with blocks)"""
    mb, r, cps = geometry(unit)
    return bool(r) and mb > 0 and mb % CHUNK == 0


def waves(shape):
    return shape.grid * (shape.threads // 64)


_SMALL = {}


@contextlib.contextmanager
def small_off(off=True):
    """uaes_debug_plan_disable is process-wide: set inside try / finally and put back to 0"""
    L = uaes.engine()
    if "bit" not in _SMALL:
        _SMALL["bit"] = 1 << uaes.arrangement_id("xts.small")
    try:
        L.uaes_debug_plan_disable(_SMALL["bit"] if off else 0)
        yield
    finally:
        L.uaes_debug_plan_disable(0)


def shape_of(c):
    with small_off(c.no_small):
        return uaes.xts_plan(c.unit, c.n, c.tweak is not None)


def first_count(pred, lo, hi):
    """the smallest n in [lo, hi] with pred(n), pred being false below it and true from it on"""
    assert pred(hi), (lo, hi)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def last_small(unit):
    """the last unit count the plan still calls xts.small"""
    return first_count(lambda n: uaes.plan("xts", unit, n)[0] != "xts.small", 2, 1 << 20) - 1


# ---- A. one unit, one launch ------------------------------------------------------------------------------------------
A_W = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 16383, 16384, 16385,
       16384 + 255, 16384 + 256, 16384 + 257, 32767, 32768, 32769, 49152)


def group_a():
    out = []
    for w in A_W:
        for r in ((0, 1, 15) if w < 1024 else (0, 15)):
            unit = 16 * w + r
            note = "empty head" if empty_chunk(unit) else ""
            out.append(case("A", unit, tweak=TWEAK, note=note))
            if w <= 1025:
                out.append(case("A", unit, tweak=NULL_TWEAK, note=note))
    return out


# ---- B. few units, one launch -----------------------------------------------------------------------------------------
B_MB = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260)
B_COUNTS = (2, 3, 17, 64, 65)
B_FIRST = (0, SECTOR_CARRY, SECTOR_WRAP)
B_LAST = ((1, 0), (64, SECTOR_WRAP), (256, SECTOR_CARRY))        # (mb, first) of the last counts that are still xts.small


def group_b(first=None):
    out = []
    for f in (B_FIRST if first is None else (first,)):
        out += [case("B", 16 * mb, n, f) for mb in B_MB for n in B_COUNTS]
        out += [case("B", 16 * mb, last_small(16 * mb), f, note="last small") for mb, lf in B_LAST if lf == f]
    return out


# ---- C. packed --------------------------------------------------------------------------------------------------------
C_SIZES = tuple(range(64, 4033, 64))
C_REAL = (64, 2112, 4032)
C_FIRST = 7


def packed_counts(unit):
    """[(n, note)] with xts.small off: less than one chunk (the most units that fit; two units of 2 KiB and more are a
    chunk already), a whole number of chunks where one exists within four, three chunks and a partial one"""
    mb = unit // 16
    out = []
    if 2 * mb < CHUNK:
        out.append(((CHUNK - 1) // mb, "below a chunk"))
    whole = [k * CHUNK // mb for k in (1, 2, 3, 4) if k * CHUNK % mb == 0 and k * CHUNK // mb >= 2]
    if whole:
        out.append((whole[0], "whole chunks"))
    out.append((3 * CHUNK // mb + 1, "three chunks and a part"))
    return out


def packed_stepping_count(unit):
    """the first count (xts.small off) whose chunks outnumber the grid's waves: every wave's (unit, block) position is
    stepped by (adv / mb, adv % mb) at least once.  (Found by walking: a larger count can have fewer chunks than waves
    again, where the workgroups grow to 16 waves.)"""
    with small_off():
        for n in range(2, 1 << 16):
            s = uaes.xts_plan(unit, n)
            if s.name == "xts.packed" and s.chunks > waves(s):
                return n
    raise AssertionError("no packed shape with more chunks than waves")


def group_c():
    out = [case("C", unit, n, C_FIRST, no_small=True, note=note) for unit in C_SIZES for n, note in packed_counts(unit)]
    for unit in C_REAL:
        n0 = last_small(unit) + 1
        out += [case("C", unit, n0, C_FIRST, note="first packed"), case("C", unit, n0 + 1, C_FIRST, note="first packed + 1")]
    out.append(case("C", C_REAL[-1], packed_stepping_count(C_REAL[-1]), C_FIRST, no_small=True, note="stepping"))
    return out


# ---- D. stealing across units -----------------------------------------------------------------------------------------
D_M = (0, 1, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 319, 320, 511, 512, 513, 768)
D_R = (1, 8, 15)
D_COUNTS = (2, 3, 65)
D_EMPTY = (256, 512, 768)
D_MORE = ((400, (2, 3)),)                    # a block m beyond one chunk in the third quarter of its chunk: the list above has none


def group_d(r=None):
    return [case("D", 16 * (m + 1) + rr, n, SECTOR_CARRY, note="empty chunk" if m in D_EMPTY else "")
            for rr in (D_R if r is None else (r,)) for m, counts in [(m, D_COUNTS) for m in D_M] + list(D_MORE) for n in counts]


# ---- E. rounds and the quarter tail at small sizes --------------------------------------------------------------------
E_UNITS = (80, 272, 4112, 9616)
E_UNITS_16 = (80, 272)
E_FIRST = SECTOR_WRAP - 1
E_ALLFULL = 4096


def bulk_shape(unit, n):
    with small_off():
        return uaes.xts_plan(unit, n)


def wave_limits(unit):
    """(n4, W4, W16): the last unit count that still runs in 4-wave workgroups, the waves of the grid there, and the waves
    of a full grid of 16-wave workgroups"""
    n4 = first_count(lambda n: bulk_shape(unit, n).threads != 256, 1, 1 << 20) - 1
    return n4, waves(bulk_shape(unit, n4)), waves(bulk_shape(unit, 1 << 20))


def rule_sides(unit, W, lo, hi):
    """the two unit counts on either side of `left * 100 < W * 80` in the round after the first: the last count whose
    remainder goes by quarter chunks (nmain < chunks) and the next one (nmain == chunks), among counts in (lo, hi]"""
    def whole_round(n):
        s = bulk_shape(unit, n)
        return s.nmain == s.chunks
    n = first_count(whole_round, lo + 1, hi)
    return n - 1, n


def rounds_counts(unit, wg16):
    """[(n, note)]: chunk counts W - 1, W, W + 1, 2 W + 1 and the sides of the 80 % rule, as unit counts -- with c chunks
    per unit the counts on either side of a target that is no multiple of c; the note says where the count's chunks lie
    against W.  4-wave workgroups end at twice their grid's waves, so there 2 W + 1 chunks cannot be: for units of one
    chunk the last 4-wave count, 2 W chunks, stands in for it."""
    c = body_chunks(unit)
    n4, W4, W16 = wave_limits(unit)
    W = W16 if wg16 else W4
    ns = []
    for t in (W - 1, W, W + 1) + ((2 * W + 1,) if wg16 else ()):
        ns += [t // c, -(-t // c)]
    if not wg16 and c == 1:
        ns.append(n4)
    out = [(n, "2 W %+d" % (n * c - 2 * W) if n * c >= 2 * W else "W %+d" % (n * c - W)) for n in sorted(set(ns))]
    q, m = rule_sides(unit, W, -(-W // c), 2 * W // c if wg16 else n4)
    return out + [(q, "quarter side"), (m, "main side")]


def group_e(unit=None):
    out = []
    for u in (E_UNITS if unit is None else (unit,) if unit in E_UNITS else ()):
        out += [case("E", u, n, E_FIRST, no_small=True, note="4-wave " + note) for n, note in rounds_counts(u, False)]
        if u in E_UNITS_16:
            # without the switch wherever the plan itself says xts.bulk: the real threshold
            out += [case("E", u, n, E_FIRST, no_small=uaes.plan("xts", u, n)[0] == "xts.small", note="16-wave " + note)
                    for n, note in rounds_counts(u, True)]
    if unit is None or unit == E_ALLFULL:
        W4 = wave_limits(E_ALLFULL)[1]
        out.append(case("E", E_ALLFULL, W4 + 1, SECTOR_CARRY, no_small=True, note="all-full W +1"))
        out.append(case("E", E_ALLFULL + 16, -(-(W4 + 1) // 2), E_FIRST, no_small=True, note="aligned, not all-full W +2"))
    return out


# ---- F. the expansion, and the table on the device --------------------------------------------------------------------
F_CPS = (128, 129, 192, 193)
F_R = (0, 5)
F_FIRST = (1 << 32) - 1
BIG_UNIT = (1 << 30) + 63 * 4096 + 16 + 5
BIG_FIRST = 0x0123456789ABCDEF
BIG_MUL = 0x9E3779B97F4A7C15                 # the big unit's text: 64-bit word k is k * BIG_MUL mod 2^64, little-endian


def group_f():
    """two units of (cps - 1) chunks and two blocks, with and without a tail: cps 128 is the last count one thread of
    k_xts_tweaks walks by itself, from 129 on k_xts_expand multiplies by the table; 192 / 193 are a group of 64 chunks
    further"""
    return [case("F", 16 * ((cps - 1) * CHUNK + 2) + r, 2, F_FIRST, no_small=True, note="cps %d" % cps) for cps in F_CPS for r in F_R]


def big_case():
    """the one case that is compared by spots: no whole-text oracle run, 1 GiB of device memory"""
    return case("F", BIG_UNIT, 1, BIG_FIRST, note="spot")


def compare_of(c):
    """"spot" (the spot reference at chosen blocks) or "whole" (the oracle's whole text, bit for bit)"""
    return "spot" if c.note == "spot" else "whole"


def big_unit_spots():
    """[(what, block index)] of the big unit: the first and last block of chunk 64 * 2^i, i = 0..12 (one table entry
    each), of chunk 64 * 4095 + 63 (entries 0..11 together), of the last chunk with blocks; the stealing pair is block
    m and the tail"""
    mb, r, cps = geometry(BIG_UNIT)
    chunks = [64 << i for i in range(13)] + [64 * 4095 + 63, (mb - 1) // CHUNK]
    out = []
    for c in chunks:
        out.append(("chunk %d first" % c, c * CHUNK))
        out.append(("chunk %d last" % c, min(c * CHUNK + CHUNK, mb) - 1))
    return out


def big_unit_words(block, nblocks=1):
    """the plaintext of blocks [block, block + nblocks) of the big unit"""
    return b"".join(((k * BIG_MUL) & ((1 << 64) - 1)).to_bytes(8, "little") for k in range(2 * block, 2 * (block + nblocks)))


# ---- G. placement -----------------------------------------------------------------------------------------------------
PLACES = ((False, 0), (True, 0), (True, 1), (True, 3))       # (device memory?, offset from a 16-byte boundary)


def group_g():
    """one case of each of A, B, C, D and the two shapes of E"""
    e4 = [c for c in group_e(272) if c.note == "4-wave W +1"][0]
    e16 = [c for c in group_e(80) if c.note == "16-wave W +1"][0]
    return [case("A", 16 * 257 + 15, tweak=TWEAK, note="empty head"), case("B", 16 * 65, 17, SECTOR_CARRY),
            case("C", 2112, packed_counts(2112)[-1][0], C_FIRST, no_small=True), case("D", 16 * 257 + 8, 3, SECTOR_CARRY, note="empty chunk"),
            e4, e16]


# ---- what the oracle is asked for -------------------------------------------------------------------------------------
def whole_cases():
    """every case that is compared whole"""
    return group_a() + group_b() + group_c() + group_d() + group_e() + group_f() + group_g()


def families(cases):
    """{(unit, first): largest count} of the numbered cases"""
    fam = {}
    for c in cases:
        if c.tweak is None:
            fam[(c.unit, c.first)] = max(fam.get((c.unit, c.first), 0), c.n)
    return fam


def reference_bytes(cases):
    """the bytes orc.xts and orc.xts_sectors read for these cases: every one-unit text (a tweak form each) and every
    family's largest text, once"""
    one = {(c.unit, c.tweak) for c in cases if c.tweak is not None}
    return sum(u for u, _ in one) + sum(u * n for (u, _), n in families(cases).items())


# ---- the spot reference -----------------------------------------------------------------------------------------------
# T0 = Enc_key2(tweak); block j of a unit is Enc_key1(P_j ^ T0 alpha^j) ^ T0 alpha^j; the stealing pair as in SP 800-38E.
# alpha^j comes from Python integers modulo x^128 + x^7 + x^2 + x + 1 (bit k of the little-endian block = x^k), by a
# carry-less product and two folds -- no code shared with csrc/uaes_gf.h, the oracle's doubling or tests/test_gf_helpers.py.
M128 = (1 << 128) - 1


def gf_mul(a, b):
    z = 0
    while b:
        low = b & -b
        z ^= a * low
        b ^= low
    while z >> 128:
        hi = z >> 128
        z = (z & M128) ^ hi ^ (hi << 1) ^ (hi << 2) ^ (hi << 7)
    return z


_SQUARES = [2]                               # alpha^(2^i)


def alpha_pow(j):
    z, i = 1, 0
    while j >> i:
        if len(_SQUARES) <= i:
            _SQUARES.append(gf_mul(_SQUARES[-1], _SQUARES[-1]))
        if (j >> i) & 1:
            z = gf_mul(z, _SQUARES[i])
        i += 1
    return z


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


class Spot:
    """one data unit under keys = key1 || key2 and a 16-byte tweak (a unit number: its little-endian 128-bit form)"""

    def __init__(self, orc, keys, tweak):
        if isinstance(tweak, int):
            tweak = (tweak & ((1 << 64) - 1)).to_bytes(16, "little")
        self.orc, self.k1 = orc, keys[:len(keys) // 2]
        self.t0 = int.from_bytes(orc.encrypt_block(keys[len(keys) // 2:], tweak), "little")

    def block(self, j, data, decrypt=False):
        t = gf_mul(self.t0, alpha_pow(j)).to_bytes(16, "little")
        return xor(self.orc.encrypt_block(self.k1, xor(data, t), decrypt), t)

    def pair(self, m, data, decrypt=False):
        """block m and the r-byte tail behind it (16 + r bytes): encrypt block m under T_m, splice, encrypt under
        T_(m+1); decryption swaps the two tweaks"""
        r = len(data) - 16
        ja, jb = (m + 1, m) if decrypt else (m, m + 1)
        cc = self.block(ja, data[:16], decrypt)
        return self.block(jb, data[16:] + cc[r:], decrypt) + cc[:r]

    def unit(self, data, decrypt=False):
        mb, r, _ = geometry(len(data))
        out = b"".join(self.block(j, data[16 * j:16 * j + 16], decrypt) for j in range(mb))
        return out + (self.pair(mb, data[16 * mb:], decrypt) if r else b"")
