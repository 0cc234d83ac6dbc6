"""The XTS batches on the GPU (k_xts_batch, uaes_xts_batch.hip: uaes_xts_encrypt_batch, uaes_xts_decrypt_batch,
uaes_xts_sector_list) against the CPU oracle's xts(), one call per unit: every short shape, the depth of the walk in and
out of place, the tweak arithmetic at chosen T, unit counts read from the plan, sector lists, the published vectors,
bad lengths, placements, a seeded fuzz with round trips, two threads and the key schedules' wipe.  Every failing case
prints the tuple that reproduces it."""
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests import rsp
from tests.guarded_mem import FILL, Mem, ptr

pytestmark = pytest.mark.gpu

KEYS = {bits: bytes((bits // 8 + 7 * i) & 0xff for i in range(bits // 8)) for bits in (128, 192, 256)}

E_ARG, E_DATALENGTH = -2, 1                     # include/uaes_hip.h
ROW_CH = 16                                     # row_walk's look-ahead in blocks (csrc/uaes_aes.hip.h)
XKEYS = {bits: KEYS[bits] + bytes((b * 5 + 0x3C) & 0xff for b in KEYS[bits]) for bits in (128, 192, 256)}   # key1 || key2


def batch(decrypt, keys, tweaks, nmsg, ml, lens, src, dst):
    """the two entry points; every array bytes, None or Mem"""
    f = uaes.engine().uaes_xts_decrypt_batch if decrypt else uaes.engine().uaes_xts_encrypt_batch
    return f(len(keys) * 4, keys, ptr(tweaks), nmsg, ml, ptr(lens), ptr(src), ptr(dst))


def sector_list(encrypt, keys, sectors, n, sb, src, dst):
    return uaes.engine().uaes_xts_sector_list(len(keys) * 4, keys, ptr(sectors), n, sb, ptr(src), ptr(dst), 1 if encrypt else 0)


def expected(orc, keys, tweaks, texts, decrypt=False):
    """the oracle's answers, one call per unit"""
    out = []
    for tw, t in zip(tweaks, texts):
        rc, o = orc.xts(keys, tw, t, encrypt=not decrypt)
        assert rc == 0
        out.append(o)
    return out


def units(rng, n, ml):
    return [rng.randbytes(16) for _ in range(n)], [rng.randbytes(ml) for _ in range(n)]


def le32(v):
    return b"".join(k.to_bytes(4, "little") for k in v)


def check_both(orc, keys, tweaks, texts, info):
    """both directions through the wrapper (host memory; units of different lengths travel as lens)"""
    for decrypt in (False, True):
        want = expected(orc, keys, tweaks, texts, decrypt)
        rc, got = uaes.xts_batch(keys, tweaks, texts, decrypt=decrypt)
        assert rc == 0, (info, decrypt)
        if got != want:
            bad = [m for m in range(len(texts)) if got[m] != want[m]]
            raise AssertionError("%r decrypt=%r: units %r differ" % (info, decrypt, bad[:8]))


# ---- 1. every short shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(orc, bits):
    """65 units per call: a second 16-wave workgroup's worth.  Every slot size 16..81 -- one block alone, a stealing pair
    alone, one to four blocks and each with every tail length -- and once all of them in one call (lens)"""
    rng = random.Random(bits)
    keys = XKEYS[bits]
    for ml in range(16, 82):
        tweaks, texts = units(rng, 65, ml)
        check_both(orc, keys, tweaks, texts, (bits, ml))
    tweaks, texts = units(rng, 65, 81)
    check_both(orc, keys, tweaks, [t[:16 + m % 66] for m, t in enumerate(texts)], (bits, "ragged"))


# ---- 2. the depth of the walk, in place and out of place --------------------------------------------------------------
@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
@pytest.mark.parametrize("tail", [0, 5])
def test_walk_depth_in_and_out_of_place(orc, tail, decrypt):
    """block counts on both sides of row_walk's look-ahead and of twice it; device memory.  In place is where a unit that
    overwrote the stealing pair before reading it would show"""
    rng = random.Random(tail)
    keys, n = XKEYS[256], 6
    for blocks in (ROW_CH - 1, ROW_CH, ROW_CH + 1, 2 * ROW_CH, 2 * ROW_CH + 1):
        ml = 16 * blocks + tail
        tweaks, texts = units(rng, n, ml)
        want = b"".join(expected(orc, keys, tweaks, texts, decrypt))
        tv = Mem(b"".join(tweaks), True)
        src, dst = Mem(b"".join(texts), True), Mem(b"", True, size=n * ml)
        assert batch(decrypt, keys, tv, n, ml, None, src, dst) == 0, (ml, decrypt)
        assert dst.get() == want and dst.intact(n * ml) and src.get() == b"".join(texts), (ml, decrypt, "out of place")
        io = Mem(b"".join(texts), True)
        assert batch(decrypt, keys, tv, n, ml, None, io, io) == 0, (ml, decrypt)
        assert io.get() == want and io.intact(n * ml), (ml, decrypt, "in place")
        assert tv.get() == b"".join(tweaks) and tv.intact(16 * n)


# ---- 3. the tweak arithmetic at chosen T ------------------------------------------------------------------------------
def one_byte(i, v):
    return bytes(i) + bytes([v]) + bytes(15 - i)


CHOSEN_T = [bytes([0xFF]) * 16, one_byte(15, 0x80), one_byte(3, 0x80), one_byte(7, 0x80), one_byte(11, 0x80),
            one_byte(15, 0xC0), bytes(16),
            # beyond the list of the issue: bit 126 alone (the second fold of alpha^2), two bits across every column
            one_byte(15, 0x40), one_byte(3, 0xC0), one_byte(7, 0xC0), one_byte(11, 0xC0), one_byte(3, 0x40)]


@pytest.mark.parametrize("bits", [128, 256])
def test_tweak_arithmetic_at_chosen_t(orc, bits):
    """T = Enc_key2(tweak) is chosen by deciphering it: all ones, the fold, every column crossing, both fold bits of
    alpha^2, zero.  Five blocks and three bytes: two paired steps, and the stealing pair under T_4 and T_5"""
    keys = XKEYS[bits]
    key2 = keys[bits // 8:]
    tweaks = [orc.encrypt_block(key2, t, decrypt=True) for t in CHOSEN_T]
    assert [orc.encrypt_block(key2, tw) for tw in tweaks] == CHOSEN_T
    rng = random.Random(bits + 3)
    texts = [rng.randbytes(5 * 16 + 3) for _ in CHOSEN_T]
    for decrypt in (False, True):
        want = expected(orc, keys, tweaks, texts, decrypt)
        rc, got = uaes.xts_batch(keys, tweaks, texts, decrypt=decrypt)
        assert rc == 0
        for m, t in enumerate(CHOSEN_T):
            assert got[m] == want[m], (bits, decrypt, "T =", t.hex())
    # nine whole blocks: four paired steps and the odd block under T_8
    texts = [rng.randbytes(9 * 16) for _ in CHOSEN_T]
    check_both(orc, keys, tweaks, texts, (bits, "nine blocks", [t.hex() for t in CHOSEN_T]))


# ---- 4. unit counts from the plan -------------------------------------------------------------------------------------
def shape_change():
    """the last count of the 4-wave workgroups, found by walking the plan"""
    threads = lambda n: uaes.xts_batch_plan(n, 33)[3]                                        # noqa: E731
    lo, hi = 1, 1 << 20
    assert threads(lo) == 256 and threads(hi) == 1024
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if threads(mid) == 256 else (lo, mid)
    return lo


def second_pass():
    """the first count at which the grid-stride loop of the largest launch runs a second time"""
    name, launches, grid, threads = uaes.xts_batch_plan(1 << 20, 33)
    assert name == "xts.batch" and launches == 1 and threads % 16 == 0
    return grid * threads // 16 + 1


@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
@pytest.mark.parametrize("which", ["shape-change", "shape-change+1", "second-pass"])
def test_unit_counts_from_the_plan(orc, which, decrypt):
    nmsg = {"shape-change": shape_change(), "shape-change+1": shape_change() + 1, "second-pass": second_pass()}[which]
    plan = uaes.xts_batch_plan(nmsg, 33)
    assert plan[:2] == ("xts.batch", 1)
    if which == "shape-change":
        assert plan[3] == 256 and uaes.xts_batch_plan(nmsg + 1, 33)[3] == 1024
    if which == "second-pass":
        assert nmsg > plan[2] * plan[3] // 16 >= nmsg - 1                                       # it does run a second time
    rng = random.Random(nmsg)
    keys = XKEYS[128]
    tweaks, texts = units(rng, nmsg, 33)
    want = expected(orc, keys, tweaks, texts, decrypt)
    rc, got = uaes.xts_batch(keys, tweaks, texts, decrypt=decrypt)
    assert rc == 0
    bad = [m for m in range(nmsg) if got[m] != want[m]]                                         # every unit is compared
    assert not bad, (which, nmsg, decrypt, bad[:8])


# ---- 5. sector lists --------------------------------------------------------------------------------------------------
SECTORS = [7, 0, (1 << 64) - 1, 7, 1 << 32, 1, (1 << 63) + 5, 255, 256, (1 << 32) - 1, 0]


@pytest.mark.parametrize("place", ["host", "device", "host+1", "device+1"])
@pytest.mark.parametrize("sb", [512, 520, 4096])
def test_sector_lists(orc, sb, place):
    """any order, repeats, the ends of 64 bits; the tweak is LE128 of the sector number"""
    rng = random.Random(sb)
    keys, n = XKEYS[256 if sb == 520 else 128], len(SECTORS)
    texts = [rng.randbytes(sb) for _ in SECTORS]
    tweaks = [s.to_bytes(16, "little") for s in SECTORS]
    sv = Mem(b"".join(s.to_bytes(8, "little") for s in SECTORS), place.startswith("device"), 1 if "+" in place else 0)
    for encrypt in (True, False):
        want = b"".join(expected(orc, keys, tweaks, texts, not encrypt))
        src, dst = Mem(b"".join(texts), True), Mem(b"", True, size=n * sb)
        assert sector_list(encrypt, keys, sv, n, sb, src, dst) == 0, (sb, place, encrypt)
        got = dst.get()
        bad = [m for m in range(n) if got[m * sb:(m + 1) * sb] != want[m * sb:(m + 1) * sb]]
        assert not bad and dst.intact(n * sb), (sb, place, encrypt, [SECTORS[m] for m in bad])
        assert sv.get() == b"".join(s.to_bytes(8, "little") for s in SECTORS) and sv.intact(8 * n)
    rc, got = uaes.xts_sector_list(keys, SECTORS, sb, b"".join(texts))                         # the wrapper; host memory
    assert rc == 0 and got == b"".join(expected(orc, keys, tweaks, texts)), (sb, "wrapper")


@pytest.mark.parametrize("sb", [512, 520, 4096])
def test_a_contiguous_list_is_the_sectors_call(orc, sb):
    rng = random.Random(sb + 1)
    keys, first = XKEYS[192], (1 << 32) - 4                                                     # the run crosses 2^32
    data = rng.randbytes(9 * sb)
    for encrypt in (True, False):
        rc, want = orc.xts_sectors(keys, first, sb, data, encrypt=encrypt)
        assert rc == 0
        assert uaes.xts_sector_list(keys, [first + i for i in range(9)], sb, data, encrypt=encrypt) == (0, want), (sb, encrypt)


# ---- 6. the vector files ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
def test_the_vector_files(orc, bits):
    """every case as a batch of one, and as unit 3 of 5 among fillers of other lengths (lens), both directions"""
    cases = rsp.xts_cases(bits)
    assert len(cases) >= 600
    rng = random.Random(bits + 6)
    for case in cases:
        keys, tw, pt, ct = case["Key"], case["i"], case["PT"], case["CT"]
        info = (bits, case["section"], case["COUNT"])
        assert len(tw) == 16 and len(keys) == bits // 4, info
        assert uaes.xts_batch(keys, [tw], [pt]) == (0, [ct]), info
        assert uaes.xts_batch(keys, [tw], [ct], decrypt=True) == (0, [pt]), info
        lens = [rng.choice([k for k in range(16, 70) if k != len(pt)]) for _ in range(5)]
        tweaks, fill = [rng.randbytes(16) for _ in range(5)], [rng.randbytes(k) for k in lens]
        tweaks[3] = tw
        for decrypt in (False, True):
            texts = fill[:3] + [ct if decrypt else pt] + fill[4:]
            want = expected(orc, keys, tweaks, texts, decrypt)
            assert want[3] == (pt if decrypt else ct), info
            assert uaes.xts_batch(keys, tweaks, texts, decrypt=decrypt) == (0, want), (info, decrypt, lens)


# ---- 7. bad lengths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
def test_bad_lengths(orc, decrypt, device, lens_on_device):
    """entries 0 and 15 write nothing and make the call return UAES_E_DATALENGTH; 16 is good; one above msg_bytes is
    msg_bytes; every other unit is finished, and what lies behind a unit's end stays the caller's"""
    rng = random.Random(70)
    keys, n, ml = XKEYS[128], 37, 70
    live = uaes.engine().uaes_debug_live_key_schedules()          # (what other tests' key contexts and streams hold)
    lens = [rng.randrange(16, ml + 1) for _ in range(n)]
    lens[3], lens[20], lens[21], lens[36], lens[11] = 0, 15, 16, 17, ml + 7
    eff = [min(k, ml) for k in lens]
    tweaks, slots = units(rng, n, ml)
    good = [m for m in range(n) if eff[m] >= 16]
    want = dict(zip(good, expected(orc, keys, [tweaks[m] for m in good], [slots[m][:eff[m]] for m in good], decrypt)))
    lv = Mem(le32(lens), lens_on_device)
    src, dst, tv = Mem(b"".join(slots), device), Mem(b"", device, size=n * ml), Mem(b"".join(tweaks), device)
    assert batch(decrypt, keys, tv, n, ml, lv, src, dst) == E_DATALENGTH
    out = dst.get()
    for m in range(n):
        info = (decrypt, device, lens_on_device, m, lens[m])
        if m in want:
            assert out[m * ml:m * ml + eff[m]] == want[m], info
            assert set(out[m * ml + eff[m]:(m + 1) * ml]) <= {FILL}, info                       # beyond lens[m]: not written
        else:
            assert set(out[m * ml:(m + 1) * ml]) == {FILL}, info                                # a short unit: its prefill
    assert dst.intact(n * ml) and src.get() == b"".join(slots) and lv.intact(4 * n)
    assert uaes.engine().uaes_debug_live_key_schedules() == live
    # the same lengths without the short ones: the call succeeds
    lens[3], lens[20] = 16, 31
    assert batch(decrypt, keys, tv, n, ml, Mem(le32(lens), lens_on_device), src, dst) == 0


def test_device_lens_must_be_aligned():
    lv = Mem(bytes(4 * 4), True, off=2)
    src, dst, tv = Mem(bytes(64), True), Mem(b"", True, size=64), Mem(bytes(64), True)
    for decrypt in (False, True):
        assert batch(decrypt, XKEYS[128], tv, 4, 16, lv, src, dst) == E_ARG, decrypt
        assert dst.intact(0)


# ---- 8. placement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decrypt", [False, True], ids=["encrypt", "decrypt"])
@pytest.mark.parametrize("place", ["host", "device", "device+1", "device+2", "device+3", "host+1"])
def test_placement(orc, place, decrypt):
    """offsets 1, 2 and 3 with 33-byte units: the byte-wise form (A4 = false); tweaks and lens in host and device memory,
    the tweaks at offset 1, too"""
    device, off = place.startswith("device"), int(place[-1]) if "+" in place else 0
    rng = random.Random(33 + off)
    keys, n = XKEYS[192], 21
    ml = 33 if off else 48
    tweaks, texts = units(rng, n, ml)
    lens = [rng.randrange(16, ml + 1) for _ in range(n)]
    want = b"".join(expected(orc, keys, tweaks, texts, decrypt))
    cut = expected(orc, keys, tweaks, [t[:k] for t, k in zip(texts, lens)], decrypt)
    for tw_device, tw_off in ((True, 0), (True, 1), (False, 0), (False, 1)):
        info = (place, decrypt, tw_device, tw_off)
        tv = Mem(b"".join(tweaks), tw_device, tw_off)
        src, dst = Mem(b"".join(texts), device, off), Mem(b"", device, off, size=n * ml)
        assert batch(decrypt, keys, tv, n, ml, None, src, dst) == 0, info
        assert dst.get() == want and dst.intact(n * ml) and src.get() == b"".join(texts) and src.intact(n * ml), info
        io = Mem(b"".join(texts), device, off)
        assert batch(decrypt, keys, tv, n, ml, None, io, io) == 0, info
        assert io.get() == want and io.intact(n * ml), (info, "in place")
        lv = Mem(le32(lens), not tw_device)                                                     # lens where the tweaks are not
        dst = Mem(b"", device, off, size=n * ml)
        assert batch(decrypt, keys, tv, n, ml, lv, src, dst) == 0, info
        out = dst.get()
        for m in range(n):
            assert out[m * ml:(m + 1) * ml] == cut[m] + bytes([FILL]) * (ml - lens[m]), (info, "lens", m)
        assert dst.intact(n * ml) and tv.get() == b"".join(tweaks) and tv.intact(16 * n) and lv.intact(4 * n), info


# ---- 9. fuzz and round trip -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(orc, seed):
    rng = random.Random(7000 + seed)
    bits = rng.choice((128, 192, 256))
    keys = rng.randbytes(bits // 4)
    decrypt = rng.randrange(2) == 1
    n = rng.randrange(1, 301)
    ml = rng.randrange(16, 701)
    lens = [rng.randrange(16, ml + 9) for _ in range(n)] if rng.randrange(2) else None
    device, off, in_place = rng.randrange(2) == 1, rng.choice((0, 0, 1, 2, 3)), rng.randrange(3) == 0
    info = ("fuzz", seed, bits, decrypt, n, ml, lens is not None, device, off, in_place)
    tweaks, slots = units(rng, n, ml)
    eff = [ml] * n if lens is None else [min(k, ml) for k in lens]
    want = expected(orc, keys, tweaks, [s[:k] for s, k in zip(slots, eff)], decrypt)
    lv = None if lens is None else Mem(le32(lens), rng.randrange(2) == 1)
    tv = Mem(b"".join(tweaks), rng.randrange(2) == 1, rng.randrange(4))
    src = Mem(b"".join(slots), device, off)
    dst = src if in_place else Mem(b"", device, off, size=n * ml)
    assert batch(decrypt, keys, tv, n, ml, lv, src, dst) == 0, info
    out = dst.get()
    for m in range(n):
        rest = slots[m][eff[m]:] if in_place else bytes([FILL]) * (ml - eff[m])
        assert out[m * ml:(m + 1) * ml] == want[m] + rest, (info, m)
    assert dst.intact(n * ml), info
    # the other direction gives the input back
    back = Mem(b"", device, off, size=n * ml)
    assert batch(not decrypt, keys, tv, n, ml, lv, dst, back) == 0, info
    got = back.get()
    for m in range(n):
        assert got[m * ml:m * ml + eff[m]] == slots[m][:eff[m]], (info, m, "round trip")
    assert back.intact(n * ml), info


# ---- 10. threads ------------------------------------------------------------------------------------------------------
def test_two_threads_with_different_keys(orc):
    """the expected values are made first; the threads only call the engine"""
    cases = {}
    for seed in (10, 20):
        rng = random.Random(seed)
        keys = rng.randbytes(32 if seed == 10 else 64)
        cases[seed] = []
        for decrypt in (False, True):
            for n, ml in ((1, 16), (70, 67), (300, 48), (9, 1013)):
                tweaks, texts = units(rng, n, ml)
                cases[seed].append((decrypt, keys, tweaks, texts, expected(orc, keys, tweaks, texts, decrypt)))
    errors = []

    def worker(seed):
        try:
            for _ in range(3):
                for decrypt, keys, tweaks, texts, want in cases[seed]:
                    assert uaes.xts_batch(keys, tweaks, texts, decrypt=decrypt) == (0, want), (seed, decrypt, len(texts), len(texts[0]))
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(s,)) for s in (10, 20)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---- 11. the key schedules are wiped ----------------------------------------------------------------------------------
def test_key_wipe():
    """the count of live key schedules after a call is what it was before: 0 in a process of its own, and whatever the key
    contexts and streams of other tests hold when the whole suite runs"""
    L = uaes.engine()
    keys = XKEYS[256]
    live = L.uaes_debug_live_key_schedules()
    assert uaes.xts_batch(keys, [bytes(16)] * 3, [bytes(40)] * 3)[0] == 0
    assert L.uaes_debug_live_key_schedules() == live
    rc, got = uaes.xts_batch(keys, [bytes(16)] * 3, [bytes(40), bytes(7), bytes(16)])
    assert rc == E_DATALENGTH and got[1] == bytes(7)                                            # (the wrapper's zeros)
    assert L.uaes_debug_live_key_schedules() == live
    assert uaes.xts_sector_list(keys, [5, 4], 520, bytes(1040), encrypt=False)[0] == 0
    assert L.uaes_debug_live_key_schedules() == live
