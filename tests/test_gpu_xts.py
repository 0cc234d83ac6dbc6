"""The XTS kernels on the GPU (k_xts_small, k_xts_tweaks, k_xts_expand, k_xts in all its forms, k_xts_cts;
csrc/uaes_kernels.hip) at every chunk, run, tail and tweak-power edge, bit for bit against the CPU oracle.

The cases are made by tests/xts_cases.py from uaes.plan and uaes.xts_plan (the launcher's own shape function), and
tests/test_xts_cases.py proves without a device what they reach.  Encryption is compared with the oracle; decryption
decrypts the ORACLE's ciphertext and is compared with the plaintext, so it leans on no encryption of the engine's.  Every
output starts as guard bytes, and what lies in front of and behind the text must stay as it was.  The oracle's answers
are made once per family of cases (xts_cases.py) and shared.  One case is not compared whole: a unit of 1 GiB and a
little, in device memory, checked at chosen blocks by the spot reference.  A failure prints the case that reproduces it."""
import ctypes as C
import hashlib

import pytest

import micro_aes_amd as uaes
from tests import xts_cases as XC
from tests.guarded_mem import GUARD, Mem

pytestmark = pytest.mark.gpu

_cache = {}


def families():
    if "families" not in _cache:
        _cache["families"] = XC.families(XC.whole_cases())
    return _cache["families"]


def expected(orc, c):
    """(plaintext, the oracle's ciphertext) of a case; a numbered case's is a prefix of its family's"""
    if c.tweak is None:
        key = (c.unit, c.first)
        if key not in _cache:
            pt = XC.text_for(orc, c, families()[key])
            rc, ct = orc.xts_sectors(XC.keys_for(c.unit), c.first, c.unit, pt)
            assert rc == 0
            _cache[key] = (pt, ct)
        pt, ct = _cache[key]
        assert c.n * c.unit <= len(pt), c
        return pt[:c.n * c.unit], ct[:c.n * c.unit]
    key = (c.unit, c.tweak)
    if key not in _cache:
        pt = XC.text_for(orc, c)
        rc, ct = orc.xts(XC.keys_for(c.unit), bytes(16) if c.tweak == XC.NULL_TWEAK else c.tweak, pt)
        assert rc == 0
        _cache[key] = (pt, ct)
    return _cache[key]


def call(c, decrypt, src, dst, nbytes=None):
    L = uaes.engine()
    keys, bits = XC.keys_for(c.unit), XC.bits_for(c.unit)
    if c.tweak is None:
        return L.uaes_xts_sectors(bits, keys, c.first, c.unit, c.n, src, dst, 0 if decrypt else 1)
    f = L.uaes_xts_decrypt if decrypt else L.uaes_xts_encrypt
    return f(bits, keys, None if c.tweak == XC.NULL_TWEAK else c.tweak, src, c.unit if nbytes is None else nbytes, dst)


def same(a, b):
    if len(a) > XC.SHA_ABOVE:
        return len(a) == len(b) and hashlib.sha256(a).digest() == hashlib.sha256(b).digest()
    return a == b


def first_difference(c, got, want):
    for i, (x, y) in enumerate(zip(got, want)):
        if x != y:
            return "first wrong byte %d: unit %d, block %d of it" % (i, i // c.unit, i % c.unit // 16)
    return "lengths %d / %d" % (len(got), len(want))


def check(orc, c, place=(False, 0), in_place=False):
    """one case in both directions at one placement"""
    pt, ct = expected(orc, c)
    n = len(pt)
    device, off = place
    with XC.small_off(c.no_small):
        shape = uaes.xts_plan(c.unit, c.n, c.tweak is not None)
        for decrypt, text, want in ((False, pt, ct), (True, ct, pt)):
            src = Mem(text, device, off)
            dst = src if in_place else Mem(b"", device, off, size=n)
            rc = call(c, decrypt, src.ptr, dst.ptr)
            got = dst.get(n)
            why = None
            if rc != 0:
                why = "returned %d (%s)" % (rc, uaes.engine().uaes_last_error().decode())
            elif not same(got, want):
                why = first_difference(c, got, want)
            elif not dst.intact(n):
                why = "bytes around the output changed"
            elif not in_place and not (src.get(n) == text and src.intact(n)):
                why = "the input changed"
            if why:
                raise AssertionError("%s: %r decrypt=%s device=%s offset=%d in_place=%s shape=%r" %
                                     (why, c, decrypt, device, off, in_place, tuple(shape)))
    return shape


# ---- A. one unit, one launch ------------------------------------------------------------------------------------------
def test_a_one_unit_at_every_run_chunk_and_group_edge(orc):
    """k_xts_small, then k_xts_cts: lengths 16 w + r under an explicit tweak and under the NULL tweak.  The "empty head"
    cases have a multiple of 256 blocks before the stealing pair: block m's chunk tweak is written by a run that has no
    blocks."""
    cases = XC.group_a()
    assert sum(c.note == "empty head" for c in cases) >= 6
    for c in cases:
        shape = check(orc, c)
        assert shape.name == ("xts.bulk" if 16 < c.unit < 32 else "xts.small"), c


# ---- B. few units, one launch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", XC.B_FIRST)
def test_b_few_units_in_one_launch(orc, first):
    """k_xts_small<MULTI>: every unit of every call is compared; the unit number carries and wraps inside the call"""
    for c in XC.group_b(first):
        assert check(orc, c).name == "xts.small", c


# ---- C. packed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["every size", "real thresholds"])
def test_c_packed(orc, part):
    """k_xts<PACKED>: all 63 unit sizes with xts.small off (the division by a multiplication for every size); sizes 64, 2112
    and 4032 at the first counts the plan itself calls xts.packed; one shape with more chunks than waves"""
    cases = [c for c in XC.group_c() if (c.no_small and c.note != "stepping") == (part == "every size")]
    assert len({c.unit for c in cases}) == (63 if part == "every size" else 3)
    for c in cases:
        shape = check(orc, c)
        assert shape.name == "xts.packed", c
        if c.note == "stepping":
            assert shape.chunks > XC.waves(shape), (c, shape)


# ---- D. stealing across units -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", XC.D_R)
def test_d_stealing_across_units(orc, r):
    """k_xts_tweaks, the unaligned k_xts and k_xts_cts: block m in every quarter of its chunk and in every chunk of four,
    out of place and in place.  m = 256, 512, 768 leave the unit's last chunk without a block of the body."""
    for c in XC.group_d(r):
        for in_place in (False, True):
            shape = check(orc, c, in_place=in_place)
        assert shape.name == "xts.bulk" and not shape.aligned, c
        body = -(-XC.geometry(c.unit)[0] // XC.CHUNK)                  # ceil(mb / 256)
        if c.note == "empty chunk":
            assert shape.chunks > c.n * body, (c, shape)
        elif body:
            assert shape.chunks == c.n * body, (c, shape)


# ---- E. rounds and the quarter tail at small sizes --------------------------------------------------------------------
@pytest.mark.parametrize("unit", XC.E_UNITS + (XC.E_ALLFULL,))
def test_e_rounds_and_the_quarter_tail(orc, unit):
    """the two-buffer loop of k_xts, its (step_q, step_r) stepping and the 80 % rule at a few hundred KiB: chunk counts
    around one and two rounds of the grid, in 4-wave and in 16-wave workgroups"""
    cases = XC.group_e(unit)
    assert cases
    for c in cases:
        shape = check(orc, c)
        assert shape.name == "xts.bulk" and shape.aligned, c
        assert shape.threads == (1024 if c.note.startswith("16-wave") else 256), (c, shape)
        if c.note.endswith("quarter side"):
            assert shape.nmain < shape.chunks, (c, shape)
        if c.note.endswith("main side"):
            assert shape.nmain == shape.chunks, (c, shape)
        if c.note.startswith("all-full"):
            assert shape.allfull and shape.nmain < shape.chunks, (c, shape)
        if c.note.startswith("aligned, not all-full"):
            assert not shape.allfull and shape.nmain < shape.chunks, (c, shape)


# ---- F. the expansion, and the table on the device --------------------------------------------------------------------
def test_f_chunk_tweaks_walked_and_expanded(orc):
    """two units of 128 (the last serial count), 129, 192 and 193 chunks, with and without a tail, compared whole"""
    for c in XC.group_f():
        shape = check(orc, c)
        assert shape.name == "xts.bulk" and shape.serial == (shape.cps <= 128), (c, shape)


def test_f_one_unit_of_a_gib_uses_thirteen_table_entries(orc):
    """2^30 + 63 * 4096 + 16 + 5 bytes in device memory, encrypted and then decrypted in place: the first and last block
    of chunk 64 * 2^i (i = 0..12, one constant of the power table each), of chunk 64 * 4095 + 63 (twelve together) and of
    the last chunk, and the stealing pair, against the spot reference (xts_cases.Spot: T0 alpha^j from Python integers).
    The text is a pattern made on the device; only the checked blocks come back."""
    import torch
    c = XC.big_case()
    assert XC.compare_of(c) == "spot"
    n = c.unit
    mb, r, cps = XC.geometry(n)
    shape = uaes.xts_plan(n, 1)
    assert shape.name == "xts.bulk" and not shape.serial and shape.cps == cps, shape
    words = (n + 7) // 8 + 8
    buf = torch.arange(words, dtype=torch.int64, device="cuda")
    buf.mul_(XC.BIG_MUL - (1 << 64))                                  # k * BIG_MUL mod 2^64 (two's complement wraps)
    text = buf.view(torch.uint8)
    keys = XC.keys_for(n)
    spot = XC.Spot(orc, keys, c.first)

    def fetch(lo, count):
        return bytes(text[lo:lo + count].cpu().numpy())

    behind = b"".join(((k * XC.BIG_MUL) & ((1 << 64) - 1)).to_bytes(8, "little") for k in range(n // 8, words))[n % 8:]
    pair_plain = XC.big_unit_words(mb, 2)[:16 + r]
    assert fetch(0, 32) == XC.big_unit_words(0, 2) and fetch(16 * mb, 16 + r) == pair_plain and fetch(n, len(behind)) == behind
    spots = XC.big_unit_spots()
    for decrypt in (False, True):
        uaes.xts_sectors_dev(keys, c.first, n, 1, text, text, encrypt=not decrypt)
        torch.cuda.synchronize()
        for what, j in spots:
            plain = XC.big_unit_words(j)
            want = plain if decrypt else spot.block(j, plain)
            assert fetch(16 * j, 16) == want, (what, j, "decrypt" if decrypt else "encrypt", tuple(shape))
        want = pair_plain if decrypt else spot.pair(mb, pair_plain)
        assert fetch(16 * mb, 16 + r) == want, ("stealing pair", mb, r, "decrypt" if decrypt else "encrypt", tuple(shape))
        assert fetch(n, len(behind)) == behind, "bytes behind the unit changed"
    del text, buf
    torch.cuda.empty_cache()


# ---- G. placement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(6))
def test_g_placement(orc, which):
    """host memory, device memory, device memory 1 and 3 bytes behind a 16-byte boundary (the staging path); out of
    place and in place; guards intact, the input unchanged when out of place"""
    c = XC.group_g()[which]
    for place in XC.PLACES:
        for in_place in (False, True):
            check(orc, c, place, in_place)


# ---- H. arguments -----------------------------------------------------------------------------------------------------
def test_h_arguments(orc):
    import torch
    L = uaes.engine()
    keys = XC.keys_for(32)
    for device in (False, True):
        for nbytes in (0, 1, 15):
            for decrypt in (False, True):
                src, dst = Mem(bytes(16), device), Mem(b"", device, size=16)
                c = XC.case("H", nbytes, tweak=XC.TWEAK)
                assert call(c, decrypt, src.ptr, dst.ptr) == 1 and dst.intact(0), ("one short unit", device, nbytes, decrypt)
        src, dst = Mem(bytes(64), device), Mem(b"", device, size=64)
        assert L.uaes_xts_sectors(128, keys, 0, 15, 4, src.ptr, dst.ptr, 1) == 1 and dst.intact(0), ("short units", device)
        assert L.uaes_xts_sectors(128, keys, 0, 32, 0, src.ptr, dst.ptr, 1) == 0 and dst.intact(0), ("no unit", device)
    t = torch.full((96,), GUARD, dtype=torch.uint8, device="cuda")
    for so, do in ((1, 0), (0, 3), (8, 8)):
        with pytest.raises(uaes.EngineError, match="16-byte aligned"):
            uaes.xts_sectors_dev(keys, 0, 32, 2, t[so:], t[do:])
    torch.cuda.synchronize()
    assert set(bytes(t.cpu().numpy())) == {GUARD}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.uaes_xts_sectors_dev(128, keys, 0, 15, 2, C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr()), 1, stream) == 1
    torch.cuda.synchronize()
    assert set(bytes(t.cpu().numpy())) == {GUARD}
