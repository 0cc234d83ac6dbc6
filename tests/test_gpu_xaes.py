"""XAES-256-GCM on the GPU (uaes_xaes256gcm_*; k_xaes_gcm_batch, uaes_xaes.hip) against tests/xaes_ref.py -- the oracle's
encrypt_block and gcm_encrypt composed as the C2SP specification says -- bit for bit: the one-message calls (the
specification's vectors, the lengths around a block, a text on the fused GCM kernels, host and device pointers, the
accumulated stream), and the batches: every short shape, the two halves of the nonce, both branches of CMAC's doubling,
record counts read from the plan, per-record lengths, placements, in place, the counter's carry and the cap, forgeries of
every part of a record, the cross-checks inside the product, two threads and key hygiene.  Every failing case prints the
tuple that reproduces it."""
import ctypes as C
import hashlib
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests import key_wipe_cases as kw
from tests import xaes_ref

pytestmark = pytest.mark.gpu

GUARD = 0xA5
E_ARG = -2                                      # UAES_E_ARG
E_AUTH = 0x1A                                   # UAES_E_AUTHENTICATION
BATCH_MAX = 65535                               # UAES_XAES_GCM_BATCH_MAX
KEY = bytes(range(0x10, 0x30))


class Mem:
    """`data` (then `size - len(data)` guard bytes) in host or device memory, `off` bytes behind an aligned base, with
    guard bytes in front of and behind it"""

    def __init__(self, data=b"", device=False, off=0, size=None, room=64):
        data = bytes(data)
        self.size = max(len(data), size or 0)
        self.off, self.device = off, device
        raw = bytes([GUARD]) * off + data + bytes([GUARD]) * (self.size - len(data) + room)
        if device:
            import torch
            self.t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
            self.ptr = C.c_void_p(self.t.data_ptr() + off)
        else:
            self.h = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
            self.ptr = C.c_void_p(C.addressof(self.h) + off)

    def raw(self):
        if self.device:
            import torch
            torch.cuda.synchronize()
            return bytes(self.t.cpu().numpy())
        return bytes(self.h)

    def get(self, n=None):
        return self.raw()[self.off:self.off + (self.size if n is None else n)]

    def intact(self, n):
        """nothing but the first n bytes was written"""
        r = self.raw()
        return set(r[:self.off]) | set(r[self.off + n:]) <= {GUARD}


def ptr(x):
    return x.ptr if isinstance(x, Mem) else x


def batch(decrypt, key, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts=None):
    """the two entry points; every array bytes, None or Mem"""
    L = uaes.engine()
    if decrypt:
        return L.uaes_xaes256gcm_decrypt_batch(key, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al, ptr(src), ptr(tags),
                                               ptr(dst), ptr(verdicts))
    return L.uaes_xaes256gcm_encrypt_batch(key, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al, ptr(src), ptr(dst), ptr(tags))


def records(rng, n, al, ml):
    """(nonces, aads, texts)"""
    return ([rng.randbytes(24) for _ in range(n)], [rng.randbytes(al) for _ in range(n)], [rng.randbytes(ml) for _ in range(n)])


def expected(key, nonces, aads, texts):
    """the reference's (ciphertexts, tags), one call per record"""
    cts, tags = [], []
    for nonce, aad, pt in zip(nonces, aads, texts):
        ct = xaes_ref.encrypt(key, nonce, aad, pt)
        cts.append(ct[:len(pt)])
        tags.append(ct[len(pt):])
    return cts, tags


def check_against(want, key, nonces, aads, texts, info):
    """encrypt == want per record; decrypt returns 0, all verdicts 1 and the plaintext into a prefilled buffer"""
    got = uaes.xaes256gcm_batch(key, nonces, aads, texts)
    if got != want:
        bad = [m for m in range(len(texts)) if (got[0][m], got[1][m]) != (want[0][m], want[1][m])]
        raise AssertionError("encrypt %r: records %r differ" % (info, bad[:8]))
    rc, pts, verdicts = uaes.xaes256gcm_batch(key, nonces, aads, got[0], decrypt=True, tags=got[1], prefill=0x77)
    assert rc == 0 and verdicts == [1] * len(texts) and pts == texts, ("decrypt", info, rc, verdicts)


def check_both(key, nonces, aads, texts, info):
    check_against(expected(key, nonces, aads, texts), key, nonces, aads, texts, info)


# ---- 1. the one-message calls -----------------------------------------------------------------------------------------
def one(decrypt, key, nonce, aad, data, n, out):
    """uaes_xaes256gcm_encrypt / _decrypt: the AAD bytes, the texts Mem"""
    L = uaes.engine()
    f = L.uaes_xaes256gcm_decrypt if decrypt else L.uaes_xaes256gcm_encrypt
    return f(key, nonce, aad, len(aad), ptr(data), n, ptr(out))


def test_the_vectors():
    for v in xaes_ref.vectors():
        assert uaes.xaes256gcm_derive(v["key"], v["nonce"]) == v["kx"]
        assert uaes.xaes256gcm_encrypt(v["key"], v["nonce"], v["aad"], v["plaintext"]) == v["output"]
        assert uaes.xaes256gcm_decrypt(v["key"], v["nonce"], v["aad"], v["output"]) == (0, v["plaintext"])
        cts, tags = uaes.xaes256gcm_batch(v["key"], [v["nonce"]], [v["aad"]], [v["plaintext"]])
        assert cts[0] + tags[0] == v["output"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_message_lengths(device):
    rng = random.Random(24)
    for n in (0, 1, 15, 16, 17, 4101):
        nonce, aad, pt = rng.randbytes(24), rng.randbytes(n % 19), rng.randbytes(n)
        want = xaes_ref.encrypt(KEY, nonce, aad, pt)
        src, ct = Mem(pt, device), Mem(b"", device, size=n + 16)
        assert one(False, KEY, nonce, aad, src, n, ct) == 0, (device, n)
        assert ct.get() == want and ct.intact(n + 16) and src.get() == pt, (device, n)
        out = Mem(b"", device, size=n)
        assert one(True, KEY, nonce, aad, ct, n, out) == 0, (device, n)
        assert out.get() == pt and out.intact(n), (device, n)
        # a forged tag, a forged first and a forged second half of the nonce: nothing is written
        forged = Mem(xaes_ref.flip(want, 8 * n + 77), device)
        for bad_ct, bad_nonce in ((forged, nonce), (ct, xaes_ref.flip(nonce, 13)), (ct, xaes_ref.flip(nonce, 180))):
            out = Mem(b"", device, size=n)
            assert one(True, KEY, bad_nonce, aad, bad_ct, n, out) == E_AUTH, (device, n)
            assert out.intact(0), (device, n)


def test_a_text_on_the_fused_gcm_kernels():
    """the one-message call IS the one-call GCM path under Kx: with the smaller arrangements switched off, the planner
    answers gcm.striped (k_gcm_fused) for this length, and the call takes it"""
    n = (9 << 20) + 5
    L = uaes.engine()
    nonce, aad = bytes(range(24)), b"fused"
    pt = xaes_ref.oracle().splitmix(24, n)
    src, ct, out = Mem(pt, True), Mem(b"", True, size=n + 16), Mem(b"", True, size=n)
    L.uaes_debug_plan_disable(0x700)                                             # gcm.small, gcm.chunks, gcm.twophase
    try:
        assert uaes.plan("gcm", n, len(aad))[0] == "gcm.striped"
        assert one(False, KEY, nonce, aad, src, n, ct) == 0
        assert one(True, KEY, nonce, aad, ct, n, out) == 0
    finally:
        L.uaes_debug_plan_disable(0)
    assert hashlib.sha256(ct.get()).digest() == hashlib.sha256(xaes_ref.encrypt(KEY, nonce, aad, pt)).digest() and ct.intact(n + 16)
    assert out.get() == pt and out.intact(n)


def test_the_accumulated_stream():
    for i, (key, nonce, pt, aad) in enumerate(xaes_ref.accumulated(256)):
        want = xaes_ref.encrypt(key, nonce, aad, pt)
        assert uaes.xaes256gcm_encrypt(key, nonce, aad, pt) == want, i
        assert uaes.xaes256gcm_decrypt(key, nonce, aad, want) == (0, pt), i


# ---- 2. every short shape ---------------------------------------------------------------------------------------------
AADS = (0, 1, 15, 16, 17, 32)


def short_shapes(key, seed):
    """lengths 0..65 in one launch through lens, for every AAD size; slots of 68 bytes (4-byte aligned texts) or 67 (not):
    (want, nonces, aads, slots, lens)"""
    rng = random.Random(seed)
    cases = []
    for al in AADS:
        ml = 68 if al % 2 == 0 else 67
        lens = list(range(66))
        nonces, aads, slots = records(rng, len(lens), al, ml)
        cases.append((expected(key, nonces, aads, [s[:k] for s, k in zip(slots, lens)]), nonces, aads, slots, lens, (al, ml, seed)))
    return cases


def check_short_shape(key, want, nonces, aads, slots, lens, info):
    cts, tags = uaes.xaes256gcm_batch(key, nonces, aads, slots, lens=lens, prefill=0x3C)
    bad = [m for m, k in enumerate(lens) if (cts[m][:k], tags[m]) != (want[0][m], want[1][m]) or set(cts[m][k:]) - {0x3C}]
    assert not bad, ("encrypt", info, bad[:8])
    rc, pts, verdicts = uaes.xaes256gcm_batch(key, nonces, aads, cts, decrypt=True, tags=tags, lens=lens, prefill=0x77)
    assert rc == 0 and verdicts == [1] * len(lens), ("decrypt", info, rc, verdicts)
    bad = [m for m, k in enumerate(lens) if pts[m][:k] != slots[m][:k] or set(pts[m][k:]) - {0x77}]
    assert not bad, ("decrypt", info, bad[:8])


def test_every_short_shape():
    for case in short_shapes(KEY, 1000):
        check_short_shape(KEY, *case)


# ---- 3. the two halves of the nonce -----------------------------------------------------------------------------------
def test_the_two_nonce_halves():
    """four records are one wave.  first wave: the base record, one that differs only in nonce[0:12] (another key, the
    same J0), one that differs only in nonce[12:24] (the same key, another J0), the base again; second wave: one bit of
    byte 11 (the last byte of the key's half) and one of byte 12 (the first of GCM's)"""
    rng = random.Random(1224)
    base, aad, text = rng.randbytes(24), rng.randbytes(7), rng.randbytes(40)
    first, second = rng.randbytes(12) + base[12:], base[:12] + rng.randbytes(12)
    b11, b12 = xaes_ref.flip(base, 8 * 11 + 7), xaes_ref.flip(base, 8 * 12)
    nonces = [base, first, second, base, base, b11, b12, base]
    kx = [uaes.xaes256gcm_derive(KEY, n) for n in nonces]
    assert kx == [xaes_ref.derive(KEY, n) for n in nonces]
    assert kx[1] != kx[0] and kx[2] == kx[0] and kx[5] != kx[0] and kx[6] == kx[0]
    cts, tags = uaes.xaes256gcm_batch(KEY, nonces, [aad] * 8, [text] * 8)
    for m in (3, 4, 7):
        assert (cts[m], tags[m]) == (cts[0], tags[0]), m
    out = [c + t for c, t in zip(cts, tags)]
    assert len({out[0], out[1], out[2], out[5], out[6]}) == 5
    for m, n in enumerate(nonces):
        assert out[m] == uaes.xaes256gcm_encrypt(KEY, n, aad, text) == xaes_ref.encrypt(KEY, n, aad, text), m
    # the same key, another J0: the same hash key, so the tags differ by Enc(J0) and the keystreams are unrelated; another
    # key, the same J0: nothing in common -- both equal plain GCM under the derived key and the second half
    orc = xaes_ref.oracle()
    for m in (1, 2, 5, 6):
        assert out[m] == orc.gcm_encrypt(kx[m], nonces[m][12:], aad, text), m
    check_both(KEY, nonces, [aad] * 8, [text] * 8, "nonce halves")


# ---- 4. both branches of CMAC's doubling ------------------------------------------------------------------------------
def test_master_keys_with_the_top_bit_of_l_set_and_clear():
    rng = random.Random(87)
    top_set, top_clear = xaes_ref.keys_by_top_bit_of_l()
    assert xaes_ref.big_l(top_set)[0] >> 7 == 1 and xaes_ref.big_l(top_clear)[0] >> 7 == 0
    for key in (top_set, top_clear):
        nonces, aads, texts = records(rng, 5, 11, 33)
        assert [uaes.xaes256gcm_derive(key, n) for n in nonces] == [xaes_ref.derive(key, n) for n in nonces]
        check_both(key, nonces, aads, texts, ("top bit", key.hex()))
        assert uaes.xaes256gcm_encrypt(key, nonces[0], aads[0], texts[0]) == xaes_ref.encrypt(key, nonces[0], aads[0], texts[0])


# ---- 5. record counts from the plan -----------------------------------------------------------------------------------
def second_pass():
    """the first count at which the grid-stride loop of the largest launch runs a second time, + 3"""
    name, launches, grid, threads = uaes.xaes256gcm_batch_plan(16, 1 << 20)
    assert name == "xaes.gcm" and launches == 1 and threads % 16 == 0
    return grid * threads // 16 + 3


@pytest.mark.parametrize("which", range(6), ids=["1", "4", "5", "64", "65", "second-pass"])
def test_record_counts_from_the_plan(which):
    nmsg = (1, 4, 5, 64, 65, second_pass())[which]
    rng = random.Random(nmsg)
    nonces, aads, texts = records(rng, nmsg, 5, 16)
    if which < 5:
        check_both(KEY, nonces, aads, texts, ("count", nmsg))                   # every record is compared
        return
    name, _, grid, threads = uaes.xaes256gcm_batch_plan(16, nmsg)
    assert name == "xaes.gcm" and nmsg > grid * threads // 16                   # it does run a second time
    look = sorted(set(range(70)) | set(range(nmsg - 70, nmsg)) | set(rng.sample(range(nmsg), 200)))
    cts, tags = uaes.xaes256gcm_batch(KEY, nonces, aads, texts)
    pick = lambda a: [a[m] for m in look]                                       # noqa: E731
    want = expected(KEY, pick(nonces), pick(aads), pick(texts))
    bad = [m for k, m in enumerate(look) if (cts[m], tags[m]) != (want[0][k], want[1][k])]
    assert not bad, ("count", nmsg, bad[:8])
    rc, pts, verdicts = uaes.xaes256gcm_batch(KEY, nonces, aads, cts, decrypt=True, tags=tags, prefill=0x77)
    assert rc == 0 and verdicts == [1] * nmsg and pts == texts, ("count", nmsg, rc)


# ---- 6. per-record lengths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_per_record_lengths(device, lens_on_device):
    rng = random.Random(48)
    ml, al = 48, 9
    given = [0, 1, 15, 16, 17, 33, 48, 1000, 48, 0, 31]                         # 1000: taken as msg_bytes
    lens = [min(k, ml) for k in given]
    n = len(given)
    nonces, aads, slots = records(rng, n, al, ml)
    want = expected(KEY, nonces, aads, [s[:k] for s, k in zip(slots, lens)])
    lv = Mem(b"".join(k.to_bytes(4, "little") for k in given), lens_on_device)
    src, dst, tags = Mem(b"".join(slots), device), Mem(b"", device, size=n * ml), Mem(b"", device, size=n * 16)
    mn, ma = Mem(b"".join(nonces), device), Mem(b"".join(aads), device)
    assert batch(False, KEY, n, ml, lv, mn, ma, al, src, dst, tags) == 0
    out, tg = dst.get(), tags.get()
    for m in range(n):
        info = (device, lens_on_device, m, given[m])
        assert out[m * ml:m * ml + lens[m]] == want[0][m] and tg[m * 16:(m + 1) * 16] == want[1][m], info
        assert set(out[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, info            # beyond lens[m]: not written
    assert dst.intact(n * ml) and tags.intact(n * 16) and src.get() == b"".join(slots)
    back, ver = Mem(b"", device, size=n * ml), Mem(b"", device, size=n)
    assert batch(True, KEY, n, ml, lv, mn, ma, al, dst, back, tags, ver) == 0
    got = back.get()
    for m in range(n):
        assert got[m * ml:m * ml + lens[m]] == slots[m][:lens[m]] and set(got[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, m
    assert ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n)


# ---- 7. placements ----------------------------------------------------------------------------------------------------
ARRAYS = ("nonces", "aad", "texts", "tags", "verdicts")
ALL = (1 << len(ARRAYS)) - 1
PLACES = [0, ALL] + [1 << k for k in range(len(ARRAYS))] + [ALL ^ (1 << k) for k in range(len(ARRAYS))]


def place_id(mask):
    return "+".join(a for k, a in enumerate(ARRAYS) if mask >> k & 1) or "host"


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("mask", PLACES, ids=[place_id(p) for p in PLACES])
def test_placements(mask, off):
    """bit k of mask: array k is in device memory.  Offsets 1 and 3 with 33-byte records: the byte-wise paths of the text
    (A4 false) and nonces at odd addresses; offset 0 with 32: the 4-byte-aligned ones"""
    rng = random.Random(33 + off)
    n, al = 21, 17
    ml = 33 if off else 32
    on = {a: bool(mask >> k & 1) for k, a in enumerate(ARRAYS)}
    nonces, aads, texts = records(rng, n, al, ml)
    want = expected(KEY, nonces, aads, texts)
    mn, ma = Mem(b"".join(nonces), on["nonces"], off), Mem(b"".join(aads), on["aad"], off)
    src, dst = Mem(b"".join(texts), on["texts"], off), Mem(b"", on["texts"], off, size=n * ml)
    tags = Mem(b"", on["tags"], off, size=n * 16)
    info = (place_id(mask), off)
    assert batch(False, KEY, n, ml, None, mn, ma, al, src, dst, tags) == 0, info
    assert dst.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]), info
    assert dst.intact(n * ml) and tags.intact(n * 16) and src.get() == b"".join(texts), info
    back, ver = Mem(b"", on["texts"], off, size=n * ml), Mem(b"", on["verdicts"], off, size=n)
    assert batch(True, KEY, n, ml, None, mn, ma, al, dst, back, tags, ver) == 0, info
    assert back.get() == b"".join(texts) and ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n), info
    # crtxt == pntxt
    io = Mem(b"".join(texts), on["texts"], off)
    tags2 = Mem(b"", on["tags"], off, size=n * 16)
    assert batch(False, KEY, n, ml, None, mn, ma, al, io, io, tags2) == 0, info
    assert io.get() == b"".join(want[0]) and tags2.get() == b"".join(want[1]) and io.intact(n * ml) and tags2.intact(n * 16), info
    ver2 = Mem(b"", on["verdicts"], off, size=n)
    assert batch(True, KEY, n, ml, None, mn, ma, al, io, io, tags2, ver2) == 0, info
    assert io.get() == b"".join(texts) and io.intact(n * ml) and ver2.get() == b"\1" * n and ver2.intact(n), info
    assert mn.get() == b"".join(nonces) and ma.get() == b"".join(aads) and mn.intact(n * 24) and ma.intact(n * al), info


@pytest.mark.parametrize("ml", [9 * 16, 17 * 16 + 5], ids=["9 blocks", "17 blocks + 5"])
def test_in_place_with_more_blocks_than_a_chunk(ml):
    """row_walk requests a chunk of blocks ahead (four encrypting, eight on either walk decrypting): records of more
    blocks than that in place, in device memory"""
    rng = random.Random(ml)
    n = 6
    nonces, aads, texts = records(rng, n, 0, ml)
    want = expected(KEY, nonces, aads, texts)
    for off in (0, 2):
        io, tags, ver = Mem(b"".join(texts), True, off), Mem(b"", True, size=n * 16), Mem(b"", True, size=n)
        mn = Mem(b"".join(nonces), True, off)
        assert batch(False, KEY, n, ml, None, mn, None, 0, io, io, tags) == 0
        assert io.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]) and io.intact(n * ml), (ml, off)
        assert batch(True, KEY, n, ml, None, mn, None, 0, io, io, tags, ver) == 0
        assert io.get() == b"".join(texts) and ver.get() == b"\1" * n and io.intact(n * ml), (ml, off)


# ---- 8. the counter's carry and the cap -------------------------------------------------------------------------------
def test_the_counter_carries_into_byte_14():
    """a record of 4112 bytes = 257 blocks: the block counter passes 255 and 256 (J0 + 1 + i with i up to 256), so byte 15
    carries into byte 14"""
    rng = random.Random(4112)
    nonces, aads, texts = records(rng, 1, 3, 4112)
    check_both(KEY, nonces, aads, texts, "carry")


def test_the_cap():
    rng = random.Random(65535)
    nonces, aads, texts = records(rng, 1, 12, BATCH_MAX)
    check_both(KEY, nonces, aads, texts, "a record at the cap")
    nn, big = b"".join(nonces), bytes(BATCH_MAX + 1)
    out, tag, ver = Mem(b"", size=BATCH_MAX + 1), Mem(b"", size=16), Mem(b"", size=1)
    for dec in (False, True):
        assert batch(dec, KEY, 1, BATCH_MAX + 1, None, nn, None, 0, big, out, tag, ver) == E_ARG, dec
        assert batch(dec, KEY, 1, 16, None, nn, big, BATCH_MAX + 1, big, out, tag, ver) == E_ARG, dec
    assert out.intact(0) and tag.intact(0)


# ---- 9. forgeries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["prefilled", "in-place"])
@pytest.mark.parametrize("part", ["text", "tag", "AAD", "nonce[5]", "nonce[17]"])
def test_forgeries(part, in_place):
    """one flipped bit in record 5 among eight (its wave: records 4..7): verdict 0 and an untouched output slot for that
    one, 0x1A for the call, the other seven -- its three wave neighbours among them -- authentic and correct, and all of it
    the same whatever the wipe switch says"""
    rng = random.Random(9)
    n, ml, al, m = 8, 40, 13, 5
    nonces, aads, texts = records(rng, n, al, ml)
    cts, tags = expected(KEY, nonces, aads, texts)
    bit = rng.randrange(8)
    if part == "text":
        cts[m] = xaes_ref.flip(cts[m], rng.randrange(8 * ml))
    elif part == "tag":
        tags[m] = xaes_ref.flip(tags[m], rng.randrange(128))
    elif part == "AAD":
        aads[m] = xaes_ref.flip(aads[m], rng.randrange(8 * al))
    else:
        nonces[m] = xaes_ref.flip(nonces[m], 8 * int(part[6:-1]) + bit)
    assert xaes_ref.decrypt(KEY, nonces[m], aads[m], cts[m] + tags[m])[0] == E_AUTH
    eng = uaes.engine()
    for wipe in (0, 1):
        info = (part, bit, in_place, wipe)
        eng.uaes_set_wipe_on_auth_failure(wipe)
        try:
            if in_place:
                io, ver = Mem(b"".join(cts), True), Mem(b"", True, size=n)
                rc = batch(True, KEY, n, ml, None, b"".join(nonces), b"".join(aads), al, io, io, b"".join(tags), ver)
                out = io.get()
                pts, verdicts = [out[k * ml:(k + 1) * ml] for k in range(n)], list(ver.get())
                left = cts[m]                                                    # it stays ciphertext
                assert io.intact(n * ml), info
            else:
                rc, pts, verdicts = uaes.xaes256gcm_batch(KEY, nonces, aads, cts, decrypt=True, tags=tags, prefill=0x5A)
                left = bytes([0x5A]) * ml                                        # it stays the prefill
        finally:
            eng.uaes_set_wipe_on_auth_failure(0)
        assert rc == E_AUTH and verdicts == [0 if k == m else 1 for k in range(n)], (info, rc, verdicts)
        assert pts[m] == left, info
        assert [pts[k] for k in range(n) if k != m] == [texts[k] for k in range(n) if k != m], info


def test_a_forgery_without_verdicts():
    """verdicts may be NULL: the return code still tells, and the forged record's slot is still untouched"""
    rng = random.Random(10)
    n, ml = 5, 24
    nonces, aads, texts = records(rng, n, 3, ml)
    cts, tags = expected(KEY, nonces, aads, texts)
    out = Mem(b"", True, size=n * ml)
    args = (KEY, n, ml, None, b"".join(nonces), b"".join(aads), 3, Mem(b"".join(cts), True), out)
    assert batch(True, *args, b"".join(tags), None) == 0 and out.get() == b"".join(texts)
    tags[3] = xaes_ref.flip(tags[3], 100)
    out = Mem(b"", True, size=n * ml)
    args = args[:-1] + (out,)
    assert batch(True, *args, b"".join(tags), None) == E_AUTH
    got = out.get()
    assert got[3 * ml:4 * ml] == bytes([GUARD]) * ml and got[:3 * ml] + got[4 * ml:] == b"".join(texts[:3] + texts[4:])


# ---- 10. cross-checks inside the product ------------------------------------------------------------------------------
def test_equals_the_one_message_calls_and_the_multikey_batch():
    rng = random.Random(256)
    for al, ml in ((0, 0), (20, 100), (12, 64), (300, 1000)):
        nonces, aads, texts = records(rng, 8, al, ml)
        cts, tags = uaes.xaes256gcm_batch(KEY, nonces, aads, texts)
        for m in (0, 3, 7):
            info = (al, ml, m)
            assert uaes.xaes256gcm_encrypt(KEY, nonces[m], aads[m], texts[m]) == cts[m] + tags[m], info
            assert uaes.xaes256gcm_decrypt(KEY, nonces[m], aads[m], cts[m] + tags[m]) == (0, texts[m]), info
        kxs = [uaes.xaes256gcm_derive(KEY, n) for n in nonces]
        assert uaes.gcm_multikey_batch(kxs, [n[12:] for n in nonces], aads, texts) == (cts, tags), (al, ml)
        assert uaes.gcm_multikey_batch(kxs, [n[12:] for n in nonces], aads, cts, decrypt=True, tags=tags) == (0, texts, [1] * 8), (al, ml)


# ---- 11. threads and hygiene ------------------------------------------------------------------------------------------
def test_two_threads():
    """each thread runs the loop of test 2 under a master key of its own on its own lane; the expected values are made
    first, the threads only call the engine"""
    keys = {t: bytes([t]) * 32 for t in (1, 2)}
    cases = {t: short_shapes(keys[t], 2000 + t) for t in keys}
    errors = []

    def worker(t):
        try:
            for case in cases[t]:
                check_short_shape(keys[t], *case)
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(t,)) for t in keys]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_no_call_leaves_a_key_schedule_behind(device):
    rng = random.Random(5)
    n, ml = 5, 40
    nonces, aads, texts = records(rng, n, 3, ml)
    cts, tags = expected(KEY, nonces, aads, texts)
    nn, aa = b"".join(nonces), b"".join(aads)
    dst, tg, ver = Mem(b"", device, size=n * ml), Mem(b"", device, size=n * 16), Mem(b"", device, size=n)
    src = Mem(b"".join(texts), device)
    kw.checked("uaes_xaes256gcm_encrypt_batch", (KEY, n, ml, None, nn, aa, 3, src.ptr, dst.ptr, tg.ptr), kw.OK)
    assert dst.get() == b"".join(cts) and tg.get() == b"".join(tags)
    back = Mem(b"", device, size=n * ml)
    kw.checked("uaes_xaes256gcm_decrypt_batch", (KEY, n, ml, None, nn, aa, 3, dst.ptr, tg.ptr, back.ptr, ver.ptr), kw.OK)
    assert back.get() == b"".join(texts)
    forged = Mem(xaes_ref.flip(b"".join(tags), 300), device)
    kw.checked("uaes_xaes256gcm_decrypt_batch", (KEY, n, ml, None, nn, aa, 3, dst.ptr, forged.ptr, back.ptr, ver.ptr), kw.AUTH)
    assert list(ver.get()) == [1, 1, 0, 1, 1]
    for k in (16, 17):
        pt, ct, out = Mem(kw.text(k), device), Mem(b"", device, size=k + 16), Mem(b"", device, size=k)
        kw.checked("uaes_xaes256gcm_encrypt", (KEY, nonces[0], b"hdr", 3, pt.ptr, k, ct.ptr), kw.OK)
        assert ct.get() == xaes_ref.encrypt(KEY, nonces[0], b"hdr", kw.text(k))
        kw.checked("uaes_xaes256gcm_decrypt", (KEY, nonces[0], b"hdr", 3, ct.ptr, k, out.ptr), kw.OK)
        bad = Mem(xaes_ref.flip(ct.get(), 8 * k + 9), device)
        kw.checked("uaes_xaes256gcm_decrypt", (KEY, nonces[0], b"hdr", 3, bad.ptr, k, out.ptr), kw.AUTH)
        assert out.get() == kw.text(k)
