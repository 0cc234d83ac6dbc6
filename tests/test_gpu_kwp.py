"""AES key wrap with padding (RFC 5649) on the GPU (k_kwp, k_kwp_batch in uaes_kw.hip) against the model of
tests/kwp_ref.py and the recorded vectors: every short length, the LDS / in-place boundary taken from the planner at byte
offsets 0..3, every residue of the chain's length against the look-ahead chunk, the step counter's third byte over a
padded last semiblock, the in-place form, every forgery class per arrangement with the wipe switch, batches with a length
per record (rows of one wave on different trip counts and on the one-block path), forged and refused records at every
row of a wave, guard bytes either side of every output, and a seeded fuzz.  Every failing case prints its tuple."""
import ctypes as C
import functools
import random

import pytest

import micro_aes_amd as uaes
from tests import kwp_ref as R
from tests.guarded_mem import FILL, Mem

pytestmark = pytest.mark.gpu

E_ARG, E_DATALENGTH, E_AUTH = -2, 1, 0x1A
BITS = [128, 192, 256]
CHUNK = 16                                      # KW_CH: the steps kw.global's loads run ahead (uaes_kw.hip)


def words(values, device):
    """a uint32 array in host or (4-byte-aligned) device memory: (pointer, keep-alive)"""
    a = (C.c_uint32 * max(len(values), 1))(*values)
    if not device:
        return C.cast(a, C.c_void_p), a
    m = Mem(bytes(a), True)
    return m.ptr, m


def kbuf(kek):
    return (C.c_uint8 * len(kek)).from_buffer_copy(kek)


def wlen(m):
    return (m + 7) // 8 * 8 + 8


def wrap(kek, secret, device=False, soff=0, doff=0):
    src, dst = Mem(secret, device, soff), Mem(b"", device, doff, size=max(wlen(len(secret)), 8))
    rc = uaes.engine().uaes_kwp_wrap(len(kek) * 8, kbuf(kek), src.ptr, len(secret), dst.ptr)
    assert dst.intact() and src.intact() and src.get() == secret
    return rc, dst.get()


def unwrap(kek, wrapped, device=False, soff=0, doff=0):
    """(code, the len(wrapped) - 8 bytes of the output buffer, *secretLen)"""
    src, dst, ln = Mem(wrapped, device, soff), Mem(b"", device, doff, size=max(len(wrapped) - 8, 0)), C.c_size_t(77)
    rc = uaes.engine().uaes_kwp_unwrap(len(kek) * 8, kbuf(kek), src.ptr, len(wrapped), dst.ptr, C.byref(ln))
    assert dst.intact() and src.intact() and src.get() == wrapped
    return rc, dst.get(), ln.value


def good(secret):
    return 0, secret + bytes(-len(secret) % 8), len(secret)


@functools.lru_cache(None)
def lds_max():
    """the longest secret of kwp.lds, by walking the planner; key wrap's own boundary is the same number"""
    b = [n for n in range(9, 1 << 14) if uaes.kwp_plan(n)[0] != uaes.kwp_plan(n + 1)[0]]
    assert len(b) == 1 and uaes.kwp_plan(b[0])[0] == "kwp.lds" and uaes.kwp_plan(b[0] + 1)[0] == "kwp.global"
    assert b[0] % 8 == 0 and uaes.kw_plan(b[0])[0] == "kw.lds" and uaes.kw_plan(b[0] + 8)[0] == "kw.global"
    return b[0]


@functools.lru_cache(None)
def batch_max():
    top = max(n for n in range(1, 1 << 12) if uaes.kwp_plan(n, 2) is not None)
    assert uaes.kwp_plan(top + 1, 2) is None and uaes.kwp_plan(top, 2, unwrap=True) is not None
    return top


@functools.lru_cache(None)
def case(bits, m, tag=0):
    """a key, a secret of m bytes and the model's wrapped form of it (computed once, shared, never changed)"""
    rng = random.Random(100000 * tag + 1000 * m + bits)
    kek, s = rng.randbytes(bits // 8), rng.randbytes(m)
    return kek, s, R.wrap(kek, s)


def check(bits, m, device=False, soff=0, doff=0, dirs=(0, 1)):
    kek, s, w = case(bits, m)
    info = (bits, m, device, soff, doff)
    if 0 in dirs:
        assert wrap(kek, s, device, soff, doff) == (0, w), info
    if 1 in dirs:
        assert unwrap(kek, w, device, soff, doff) == good(s), info


def test_fixtures(golden_dir):
    for c in R.fixtures(golden_dir):
        for device in (False, True):
            info = (c["source"], len(c["secret"]), device)
            assert wrap(c["kek"], c["secret"], device) == (0, c["wrapped"]), info
            assert unwrap(c["kek"], c["wrapped"], device) == good(c["secret"]), info


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("unwrapping", [0, 1])
def test_every_short_length(bits, unwrapping):
    """1 .. 72 bytes: the one-block case, every count of fill bytes 0 .. 7, n = 1 .. 9; host and device pointers in turn"""
    for m in range(1, 73):
        assert uaes.kwp_plan(m)[0] == ("kwp.block" if m <= 8 else "kwp.lds")
        check(bits, m, device=(m + unwrapping) % 2 == 0, dirs=(unwrapping,))


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("unwrapping", [0, 1])
def test_lds_boundary_at_every_offset(bits, unwrapping):
    """padded length at the boundary (secrets of MAX - 8, MAX - 7, MAX - 1, MAX bytes) and beyond (MAX + 1, + 8, + 9),
    either buffer 0 .. 3 bytes off a 4-byte boundary: both A4 instances of both arrangements"""
    mx = lds_max()
    for m in (mx - 8, mx - 7, mx - 1, mx, mx + 1, mx + 8, mx + 9):
        assert uaes.kwp_plan(m)[0] == ("kwp.lds" if m <= mx else "kwp.global")
        for soff, doff in [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 2), (3, 3)]:
            check(bits, m, True, soff, doff, dirs=(unwrapping,))
        check(bits, m, False, 1, 2, dirs=(unwrapping,))


@pytest.mark.parametrize("unwrapping", [0, 1])
def test_global_chunk_edges(unwrapping):
    """kwp.global's loads run CHUNK steps ahead of the chain and its last chunk is short unless 6 n is a multiple of
    CHUNK.  6 n is even, so the residues 1 and 15 do not exist: the eight n above the boundary give every residue that
    does (0, 2, .. 14; 0, 2 and 14 are asserted to be among them), each with no fill byte and with seven"""
    n0 = lds_max() // 8 + 1
    assert {0, 2, CHUNK - 2} <= {6 * n % CHUNK for n in range(n0, n0 + 8)}
    for k, n in enumerate(range(n0, n0 + 8)):
        for m in (8 * n, 8 * n - 7):
            assert uaes.kwp_plan(m)[0] == "kwp.global"
            check(BITS[k % 3], m, device=k % 2 == 0, dirs=(unwrapping,))


@pytest.mark.parametrize("bits", BITS)
def test_third_counter_byte_over_a_padded_semiblock(bits):
    m = 8 * 10923 - 3
    assert 6 * ((m + 7) // 8) > 0xFFFF and uaes.kwp_plan(m)[0] == "kwp.global"
    check(bits, m, device=True)


@pytest.mark.parametrize("device", [False, True])
def test_in_place(device):
    """secret == wrapped + 8 in kwp.lds and kwp.global, both directions; the wrap writes its fill bytes into `wrapped`.
    kwp.block with separate buffers is test_every_short_length."""
    L = uaes.engine()
    for bits in BITS:
        for m in (9, 20, lds_max() - 1, lds_max() + 1, lds_max() + 8):
            kek, s, w = case(bits, m)
            for off in (0, 3):
                buf = Mem(b"\x11" * 8 + s + b"\x22" * (-m % 8), device, off)
                ln = C.c_size_t(0)
                assert L.uaes_kwp_wrap(bits, kbuf(kek), C.c_void_p(buf.ptr.value + 8), m, buf.ptr) == 0
                assert buf.get() == w and buf.intact(), (bits, m, device, off)
                assert L.uaes_kwp_unwrap(bits, kbuf(kek), buf.ptr, len(w), C.c_void_p(buf.ptr.value + 8), C.byref(ln)) == 0
                assert buf.get()[8:] == s + bytes(-m % 8) and ln.value == m and buf.intact(), (bits, m, device, off)


def forgeries(kek, s, w):
    """[(name, key, wrapped form)] of every class: crafted with wrap_raw, and single flipped bits"""
    return [(name, kek, f) for name, f in R.crafted(kek, s)] + [("flip %d" % i, k2, w2) for i, (k2, w2) in enumerate(R.flipped(kek, w))]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("arrangement", ["kwp.block", "kwp.lds", "kwp.global"])
def test_forgeries_and_the_wipe_switch(bits, arrangement):
    eng = uaes.engine()
    live = eng.uaes_debug_live_key_schedules()                  # (other tests of the process may hold key contexts open)
    for m in {"kwp.block": (5, 8), "kwp.lds": (9, 16, 20), "kwp.global": (lds_max() + 3,)}[arrangement]:
        kek, s, w = case(bits, m)
        assert uaes.kwp_plan(m)[0] == uaes.kwp_plan(len(w) - 8, unwrap=True)[0] == arrangement
        cases = forgeries(kek, s, w)
        assert len(cases) == 6 + 2 * (m % 8 != 0) + 3 + (m > 8)
        for k, (name, k2, w2) in enumerate(cases):
            code, text, n = R.unwrap(k2, w2)
            assert (code, n) == (E_AUTH, 0), (bits, m, name)
            device = k % 2 == 0
            assert unwrap(k2, w2, device, soff=k % 4) == (E_AUTH, text, 0), (bits, m, name)
            eng.uaes_set_wipe_on_auth_failure(1)
            try:
                assert unwrap(k2, w2, not device, doff=k % 4) == (E_AUTH, bytes(len(text)), 0), (bits, m, name)
                assert unwrap(kek, w, device) == good(s)
            finally:
                eng.uaes_set_wipe_on_auth_failure(0)
    assert eng.uaes_debug_live_key_schedules() == live


def test_error_lengths_leave_the_buffer():
    kek = bytes(range(16))
    for device in (False, True):
        assert wrap(kek, b"", device) == (E_DATALENGTH, bytes([FILL]) * 8)
        for n in (8, 12, 20, 33):
            assert unwrap(kek, bytes(n), device) == (E_DATALENGTH, bytes([FILL]) * (n - 8), 77), (device, n)


# ---- batches ---------------------------------------------------------------------------------------------------------
SLOTS = [1, 8, 9, 20, 255, 256]
POOL = 97                                                   # distinct secrets of a batch: record m is number m % POOL


def counts(slot):
    """1, around a wave's four rows, around a workgroup's 64 rows at the largest launch shape, and for the 9-byte slot one
    more than a whole grid's rows, from the planner"""
    out = [1, 3, 4, 5, 63, 64, 65]
    if slot == 9:
        _, _, grid, threads = uaes.kwp_plan(slot, 1 << 22)
        assert threads // 16 == 64
        out.append(grid * 64 + 1)
        assert uaes.kwp_plan(slot, out[-1])[2] * 64 < out[-1]             # the stride loop takes a second turn
    return out


@functools.lru_cache(None)
def pool(bits, slot, mixed):
    """one key and POOL (secret, wrapped) pairs whose lengths cycle through 1, 8, 9 and the slot when `mixed`, so that
    the four rows of a wave differ (the one-block path beside chains of two trip counts)"""
    rng = random.Random(7 * bits + slot + 1000 * mixed)
    kek = rng.randbytes(bits // 8)
    ls = [min(x, slot) for x in (1, 8, 9, slot)]
    secrets = [rng.randbytes(ls[k % 4] if mixed else slot) for k in range(POOL)]
    return kek, secrets, [R.wrap(kek, s) for s in secrets]


def slots(items, slot):
    """the records back to back in slots of `slot` bytes, FILL behind a short one"""
    return b"".join(x + bytes([FILL]) * (slot - len(x)) for x in items)


@pytest.mark.parametrize("slot,bits", list(zip(SLOTS, BITS + BITS)))
def test_wrap_batches(slot, bits):
    L = uaes.engine()
    ws = wlen(slot)
    assert batch_max() == max(SLOTS)
    for ni, nkeys in enumerate(counts(slot)):
        for mixed in (0, 1):
            kek, secrets, wrapped = pool(bits, slot, mixed)
            device = (ni + mixed) % 2 == 0
            off = 0 if nkeys > 100 else (ni + mixed) % 4
            recs = [secrets[m % POOL] for m in range(nkeys)]
            src, dst = Mem(slots(recs, slot), device, off), Mem(b"", device, (off + 1) % 4, size=nkeys * ws)
            lens, keep = words([len(r) for r in recs], device or ni % 3 == 0) if mixed else (None, None)
            info = (slot, bits, nkeys, mixed, device)
            assert L.uaes_kwp_wrap_batch(bits, kbuf(kek), nkeys, slot, lens, src.ptr, dst.ptr) == 0, info
            got = dst.get()
            for m in range(nkeys):
                w = wrapped[m % POOL]
                assert got[m * ws:(m + 1) * ws] == w + bytes([FILL]) * (ws - len(w)), info + (m,)
            assert dst.intact() and src.intact()


@pytest.mark.parametrize("slot,bits", list(zip(SLOTS, BITS + BITS)))
def test_wrap_batch_refuses_a_length(slot, bits):
    """an entry of 0 and one above the slot among valid ones: UAES_E_DATALENGTH, their slots untouched, the others done"""
    L = uaes.engine()
    ws = wlen(slot)
    kek, secrets, wrapped = pool(bits, slot, 1)
    for nkeys, device in ((5, False), (65, True)):
        recs = [secrets[m % POOL] for m in range(nkeys)]
        ls = [len(r) for r in recs]
        refused = {1: 0, nkeys - 2: slot + 1} if nkeys > 5 else {2: 0, 3: slot + 1}
        for m, v in refused.items():
            ls[m] = v
        src, dst = Mem(slots(recs, slot), device), Mem(b"", device, size=nkeys * ws)
        lens, keep = words(ls, device)
        assert L.uaes_kwp_wrap_batch(bits, kbuf(kek), nkeys, slot, lens, src.ptr, dst.ptr) == E_DATALENGTH
        got = dst.get()
        for m in range(nkeys):
            w = b"" if m in refused else wrapped[m % POOL]
            assert got[m * ws:(m + 1) * ws] == w + bytes([FILL]) * (ws - len(w)), (slot, bits, nkeys, m)
        assert dst.intact()


@pytest.mark.parametrize("slot,bits", list(zip(SLOTS, BITS + BITS)))
def test_unwrap_batches_with_forged_and_refused_records(slot, bits):
    L = uaes.engine()
    ws = wlen(slot)
    for ni, nkeys in enumerate(counts(slot)):
        for mixed in (0, 1):
            kek, secrets, wrapped = pool(bits, slot, mixed)
            device = (ni + mixed) % 2 == 1
            off = 0 if nkeys > 100 else (ni + mixed) % 4
            recs = [wrapped[m % POOL] for m in range(nkeys)]
            # forged records first, last, in the middle and in each row of a wave, the classes in turn
            want = {}
            spots = sorted({0, 1, 2, 3, nkeys // 2, nkeys - 2, nkeys - 1} & set(range(nkeys)))
            for k, m in enumerate(spots):
                fs = forgeries(kek, secrets[m % POOL], recs[m])
                name, k2, w2 = fs[(k + ni) % len(fs)]
                if k2 != kek:                                           # one key per batch: the other flips serve
                    name, k2, w2 = fs[0]
                recs[m] = w2
                code, text, n = R.unwrap(kek, w2)
                assert (code, n) == (E_AUTH, 0)
                want[m] = text
            ls = [len(r) for r in recs]
            refused = {}
            if mixed and nkeys >= 63:                                   # lengths the call refuses: the record stays unwritten
                refused = {7: 12, 9: 8, 12: ws + 8}
                for m, v in refused.items():
                    ls[m] = v
            for wipe in (0, 1):
                src, dst = Mem(slots(recs, ws), device, off), Mem(b"", device, (off + 2) % 4, size=nkeys * (ws - 8))
                ver, lo = Mem(b"", device, size=nkeys), Mem(b"", device, size=4 * nkeys)
                wl, keep = words(ls, device or ni % 3 == 0) if mixed else (None, None)
                info = (slot, bits, nkeys, mixed, device, wipe)
                L.uaes_set_wipe_on_auth_failure(wipe)
                try:
                    rc = L.uaes_kwp_unwrap_batch(bits, kbuf(kek), nkeys, ws, wl, src.ptr, dst.ptr, lo.ptr, ver.ptr)
                finally:
                    L.uaes_set_wipe_on_auth_failure(0)
                assert rc == E_AUTH, info
                got, lens_out = dst.get(), list((C.c_uint32 * nkeys).from_buffer_copy(lo.get()))
                failed = set(want) | set(refused)
                assert ver.get() == bytes(0 if m in failed else 1 for m in range(nkeys)), info
                assert lens_out == [0 if m in failed else len(secrets[m % POOL]) for m in range(nkeys)], info
                for m in range(nkeys):
                    s = secrets[m % POOL]
                    text = b"" if m in refused else (bytes(len(want[m])) if wipe else want[m]) if m in want else s + bytes(-len(s) % 8)
                    assert got[m * (ws - 8):(m + 1) * (ws - 8)] == text + bytes([FILL]) * (ws - 8 - len(text)), info + (m,)
                assert dst.intact() and ver.intact() and lo.intact() and src.intact()
    # nothing forged: 0, every verdict 1
    kek, secrets, wrapped = pool(bits, slot, 1)
    nkeys = 65
    recs = [wrapped[m % POOL] for m in range(nkeys)]
    src, dst, ver, lo = Mem(slots(recs, ws), True), Mem(b"", True, size=nkeys * (ws - 8)), Mem(b"", False, size=nkeys), Mem(b"", False, size=4 * nkeys)
    wl, keep = words([len(r) for r in recs], False)
    assert L.uaes_kwp_unwrap_batch(bits, kbuf(kek), nkeys, ws, wl, src.ptr, dst.ptr, lo.ptr, ver.ptr) == 0
    assert ver.get() == b"\x01" * nkeys
    assert list((C.c_uint32 * nkeys).from_buffer_copy(lo.get())) == [len(secrets[m % POOL]) for m in range(nkeys)]


def test_python_mirror_of_the_batches():
    kek, secrets, wrapped = pool(192, 20, 1)
    assert uaes.kwp_batch(kek, secrets[:9]) == (0, wrapped[:9])
    texts = [s + bytes(-len(s) % 8) for s in secrets[:9]]
    assert uaes.kwp_batch(kek, wrapped[:9], unwrap=True) == (0, texts, [len(s) for s in secrets[:9]], [1] * 9)
    bad = list(wrapped[:3])
    bad[1] = R.crafted(kek, secrets[1])[2][1]
    assert uaes.kwp_batch(kek, bad, unwrap=True) == (E_AUTH, [texts[0], R.unwrap(kek, bad[1])[1], texts[2]],
                                                     [len(secrets[0]), 0, len(secrets[2])], [1, 0, 1])
    assert uaes.kwp_wrap(kek, secrets[3]) == (0, wrapped[3]) and uaes.kwp_unwrap(kek, wrapped[3]) == good(secrets[3])


def test_batch_limits():
    L = uaes.engine()
    live = L.uaes_debug_live_key_schedules()
    kek = bytes(range(16))
    top = batch_max()
    src, dst = Mem(bytes(4 * (top + 16)), True), Mem(b"", True, size=4 * (top + 16))
    ver, lo = Mem(b"", True, size=4), Mem(b"", True, size=16)
    for sb in (0, top + 1):
        assert L.uaes_kwp_wrap_batch(128, kbuf(kek), 4, sb, None, src.ptr, dst.ptr) == E_ARG, sb
    assert b"1 .." in L.uaes_last_error()
    for wb in (8, 20, top + 16):
        assert L.uaes_kwp_unwrap_batch(128, kbuf(kek), 4, wb, None, src.ptr, dst.ptr, lo.ptr, ver.ptr) == E_ARG, wb
    assert L.uaes_kwp_wrap_batch(128, kbuf(kek), 0, 32, None, src.ptr, dst.ptr) == 0
    assert L.uaes_kwp_unwrap_batch(128, kbuf(kek), 0, 40, None, src.ptr, dst.ptr, lo.ptr, ver.ptr) == 0
    assert L.uaes_kwp_wrap_batch(128, kbuf(kek), 4, 32, None, None, dst.ptr) == E_ARG
    assert L.uaes_kwp_wrap_batch(128, kbuf(kek), 4, 32, None, src.ptr, None) == E_ARG
    assert L.uaes_kwp_unwrap_batch(128, kbuf(kek), 4, 40, None, src.ptr, dst.ptr, None, ver.ptr) == E_ARG
    assert L.uaes_kwp_unwrap_batch(128, kbuf(kek), 4, 40, None, src.ptr, dst.ptr, lo.ptr, None) == E_ARG
    odd = C.c_void_p(lo.ptr.value + 2)
    assert L.uaes_kwp_wrap_batch(128, kbuf(kek), 2, 32, odd, src.ptr, dst.ptr) == E_ARG
    assert set(dst.get()) == {FILL} and set(ver.get()) == {FILL} and set(lo.get()) == {FILL} and dst.intact()
    assert L.uaes_debug_live_key_schedules() == live


def test_fuzz_round_trips():
    """seeded round trips, lengths 1 .. 8192 (most of them short: the model is a Python loop), mixed placements"""
    rng = random.Random(5649)
    for it in range(200):
        bits = rng.choice(BITS)
        m = rng.randrange(1, 8193) if it % 8 == 0 else rng.randrange(1, 300)
        kek, s = rng.randbytes(bits // 8), rng.randbytes(m)
        device, soff, doff = rng.random() < 0.5, rng.randrange(4), rng.randrange(4)
        info = (it, bits, m, device, soff, doff)
        w = R.wrap(kek, s)
        assert wrap(kek, s, device, soff, doff) == (0, w), info
        assert unwrap(kek, w, device, doff, soff) == good(s), info
