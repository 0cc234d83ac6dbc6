"""The GCM-SIV batches on the GPU (k_gcmsiv_batch, uaes_gcmsiv_batch.hip) against the CPU oracle's gcmsiv_encrypt /
gcmsiv_decrypt, one oracle call per record, bit for bit: every short shape, record counts read from the plan, repeated
nonces, per-record lengths, placements, forgeries of every part of a record, the counter's 32-bit wrap, the published
vectors, the cap, the one-message calls and two threads.  Every failing case prints the tuple that reproduces it."""
import ctypes as C
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests import rsp

pytestmark = pytest.mark.gpu

GUARD = 0xA5
E_AUTH = 0x1A                                   # UAES_E_AUTHENTICATION
BATCH_MAX = 65535                               # UAES_GCMSIV_BATCH_MAX
KEYS = {bits: bytes((bits // 8 + 11 * i) & 0xff for i in range(bits // 8)) for bits in (128, 192, 256)}


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
        return L.uaes_gcmsiv_decrypt_batch(len(key) * 8, key, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al, ptr(src),
                                           ptr(tags), ptr(dst), ptr(verdicts))
    return L.uaes_gcmsiv_encrypt_batch(len(key) * 8, key, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al, ptr(src),
                                       ptr(dst), ptr(tags))


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def records(rng, n, al, ml):
    return [rng.randbytes(12) for _ in range(n)], [rng.randbytes(al) for _ in range(n)], [rng.randbytes(ml) for _ in range(n)]


def expected(orc, key, nonces, aads, texts):
    """the oracle's (ciphertexts, tags), one call per record"""
    cts, tags = [], []
    for nonce, aad, pt in zip(nonces, aads, texts):
        ct = orc.gcmsiv_encrypt(key, nonce, aad, pt)
        cts.append(ct[:len(pt)])
        tags.append(ct[len(pt):])
    return cts, tags


def check_against(want, key, nonces, aads, texts, info):
    """encrypt == want per record; decrypt returns 0, all verdicts 1 and the plaintext into a prefilled buffer"""
    got = uaes.gcmsiv_batch(key, nonces, aads, texts)
    if got != want:
        bad = [m for m in range(len(texts)) if (got[0][m], got[1][m]) != (want[0][m], want[1][m])]
        raise AssertionError("encrypt %r: records %r differ" % (info, bad[:8]))
    rc, pts, verdicts = uaes.gcmsiv_batch(key, nonces, aads, got[0], decrypt=True, tags=got[1], prefill=0x77)
    assert rc == 0 and verdicts == [1] * len(texts) and pts == texts, ("decrypt", info, rc, verdicts)


def check_both(orc, key, nonces, aads, texts, info):
    check_against(expected(orc, key, nonces, aads, texts), key, nonces, aads, texts, info)


# ---- 1. every short shape ---------------------------------------------------------------------------------------------
AADS = (0, 1, 15, 16, 17, 32)


def short_shapes(orc, bits, seed):
    """the cases, with what the oracle gives for them; 5 records per call: one of them lands in a second wave"""
    rng = random.Random(seed)
    key = KEYS[bits]
    cases = []
    for ml in (range(50) if bits == 128 else (0, 15, 16, 17, 49)):
        for al in AADS:
            nonces, aads, texts = records(rng, 5, al, ml)
            cases.append((expected(orc, key, nonces, aads, texts), key, nonces, aads, texts, (bits, al, ml, seed)))
    return cases


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(orc, bits):
    for case in short_shapes(orc, bits, 1000 + bits):
        check_against(*case)


# ---- 2. record counts from the plan -----------------------------------------------------------------------------------
def second_pass():
    """the first count at which the grid-stride loop of the largest launch runs a second time, + 3"""
    name, launches, grid, threads = uaes.gcmsiv_batch_plan(16, 1 << 20)
    assert name == "gcmsiv.batch" and launches == 1 and threads % 16 == 0
    return grid * threads // 16 + 3


@pytest.mark.parametrize("which", range(6), ids=["1", "4", "5", "64", "65", "second-pass"])
def test_record_counts_from_the_plan(orc, which):
    nmsg = (1, 4, 5, 64, 65, second_pass())[which]
    rng = random.Random(nmsg)
    key = KEYS[128]
    nonces, aads, texts = records(rng, nmsg, 5, 16)
    assert len(set(nonces)) == nmsg                                             # every record has its own nonce
    if which < 5:
        check_both(orc, key, nonces, aads, texts, ("count", nmsg))              # every record is compared
        return
    name, _, grid, threads = uaes.gcmsiv_batch_plan(16, nmsg)
    assert name == "gcmsiv.batch" and nmsg > grid * threads // 16               # it does run a second time
    look = sorted(set(range(70)) | set(range(nmsg - 70, nmsg)) | set(rng.sample(range(nmsg), 200)))
    cts, tags = uaes.gcmsiv_batch(key, nonces, aads, texts)
    want = expected(orc, key, [nonces[m] for m in look], [aads[m] for m in look], [texts[m] for m in look])
    bad = [m for k, m in enumerate(look) if (cts[m], tags[m]) != (want[0][k], want[1][k])]
    assert not bad, ("count", nmsg, bad[:8])
    rc, pts, verdicts = uaes.gcmsiv_batch(key, nonces, aads, cts, decrypt=True, tags=tags, prefill=0x77)
    assert rc == 0 and verdicts == [1] * nmsg and pts == texts, ("count", nmsg, rc)


# ---- 3. repeated and distinct nonces in one call ----------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_repeated_and_distinct_nonces(orc, bits):
    """records 0, 2, 5 and 7 are the same record (rows of two waves); 1 and 6 differ from it only in the nonce: a record
    key or a POLYVAL key that leaks from one row to its neighbour shows here"""
    rng = random.Random(bits + 3)
    key = KEYS[bits]
    n0, n1, n6 = rng.randbytes(12), rng.randbytes(12), rng.randbytes(12)
    aad, text = rng.randbytes(7), rng.randbytes(40)
    nonces = [n0, n1, n0, rng.randbytes(12), rng.randbytes(12), n0, n6, n0]
    aads = [aad, aad, aad, rng.randbytes(7), rng.randbytes(7), aad, aad, aad]
    texts = [text, text, text, rng.randbytes(40), rng.randbytes(40), text, text, text]
    cts, tags = uaes.gcmsiv_batch(key, nonces, aads, texts)
    for m in (2, 5, 7):
        assert (cts[m], tags[m]) == (cts[0], tags[0]), (bits, m)
    for m in (1, 6):
        assert tags[m] != tags[0] and cts[m] != cts[0], (bits, m)
    assert tags[1] != tags[6] and cts[1] != cts[6], bits
    check_both(orc, key, nonces, aads, texts, ("nonces", bits))


# ---- 4. per-record lengths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_per_record_lengths(orc, device, lens_on_device):
    rng = random.Random(48)
    key, ml, al = KEYS[128], 48, 9
    given = [0, 1, 15, 16, 17, 33, 48, 1000, 48, 0, 31]                         # 1000: taken as msg_bytes
    lens = [min(k, ml) for k in given]
    n = len(given)
    nonces, aads, slots = records(rng, n, al, ml)
    want = expected(orc, key, nonces, aads, [s[:k] for s, k in zip(slots, lens)])
    lv = Mem(b"".join(k.to_bytes(4, "little") for k in given), lens_on_device)
    src, dst, tags = Mem(b"".join(slots), device), Mem(b"", device, size=n * ml), Mem(b"", device, size=n * 16)
    mn, ma = Mem(b"".join(nonces), device), Mem(b"".join(aads), device)
    assert batch(False, key, n, ml, lv, mn, ma, al, src, dst, tags) == 0
    out, tg = dst.get(), tags.get()
    for m in range(n):
        info = (device, lens_on_device, m, given[m])
        assert out[m * ml:m * ml + lens[m]] == want[0][m] and tg[m * 16:(m + 1) * 16] == want[1][m], info
        assert set(out[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, info            # beyond lens[m]: not written
    assert dst.intact(n * ml) and tags.intact(n * 16) and src.get() == b"".join(slots)
    back, ver = Mem(b"", device, size=n * ml), Mem(b"", device, size=n)
    assert batch(True, key, n, ml, lv, mn, ma, al, dst, back, tags, ver) == 0
    got = back.get()
    for m in range(n):
        assert got[m * ml:m * ml + lens[m]] == slots[m][:lens[m]] and set(got[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, m
    assert ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n)


# ---- 5. placements ----------------------------------------------------------------------------------------------------
ARRAYS = ("nonces", "aad", "texts", "tags", "verdicts")
PLACES = [0b00000, 0b11111] + [1 << k for k in range(5)] + [0b11111 ^ (1 << k) for k in range(5)]


def place_id(mask):
    return "+".join(a for k, a in enumerate(ARRAYS) if mask >> k & 1) or "host"


@pytest.mark.parametrize("off", [0, 1, 7])
@pytest.mark.parametrize("mask", PLACES, ids=[place_id(p) for p in PLACES])
def test_placements(orc, mask, off):
    """bit k of mask: array k is in device memory.  Offsets 1 and 7 with 33-byte records: the byte-wise path; offset 0
    with 32: the 4-byte-aligned one"""
    rng = random.Random(33 + off)
    key, n, al = KEYS[192], 21, 17
    ml = 33 if off else 32
    on = {a: bool(mask >> k & 1) for k, a in enumerate(ARRAYS)}
    nonces, aads, texts = records(rng, n, al, ml)
    want = expected(orc, key, nonces, aads, texts)
    mn, ma = Mem(b"".join(nonces), on["nonces"], off), Mem(b"".join(aads), on["aad"], off)
    src, dst = Mem(b"".join(texts), on["texts"], off), Mem(b"", on["texts"], off, size=n * ml)
    tags = Mem(b"", on["tags"], off, size=n * 16)
    info = (place_id(mask), off)
    assert batch(False, key, n, ml, None, mn, ma, al, src, dst, tags) == 0, info
    assert dst.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]), info
    assert dst.intact(n * ml) and tags.intact(n * 16) and src.get() == b"".join(texts), info
    back, ver = Mem(b"", on["texts"], off, size=n * ml), Mem(b"", on["verdicts"], off, size=n)
    assert batch(True, key, n, ml, None, mn, ma, al, dst, back, tags, ver) == 0, info
    assert back.get() == b"".join(texts) and ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n), info
    # crtxt == pntxt
    io = Mem(b"".join(texts), on["texts"], off)
    tags2 = Mem(b"", on["tags"], off, size=n * 16)
    assert batch(False, key, n, ml, None, mn, ma, al, io, io, tags2) == 0, info
    assert io.get() == b"".join(want[0]) and tags2.get() == b"".join(want[1]) and io.intact(n * ml) and tags2.intact(n * 16), info
    ver2 = Mem(b"", on["verdicts"], off, size=n)
    assert batch(True, key, n, ml, None, mn, ma, al, io, io, tags2, ver2) == 0, info
    assert io.get() == b"".join(texts) and io.intact(n * ml) and ver2.get() == b"\1" * n and ver2.intact(n), info
    assert mn.get() == b"".join(nonces) and ma.get() == b"".join(aads) and mn.intact(n * 12) and ma.intact(n * al), info


def test_in_place_with_more_blocks_than_a_chunk(orc):
    """row_walk requests a chunk of blocks ahead (eight encrypting, four decrypting): records of 21 blocks + 5 bytes in
    place, in device memory"""
    rng = random.Random(341)
    key, n, ml = KEYS[256], 6, 341
    nonces, aads, texts = records(rng, n, 0, ml)
    want = expected(orc, key, nonces, aads, texts)
    for off in (0, 2):
        io, tags, ver = Mem(b"".join(texts), True, off), Mem(b"", True, size=n * 16), Mem(b"", True, size=n)
        mn = Mem(b"".join(nonces), True)
        assert batch(False, key, n, ml, None, mn, None, 0, io, io, tags) == 0
        assert io.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]) and io.intact(n * ml), off
        assert batch(True, key, n, ml, None, mn, None, 0, io, io, tags, ver) == 0
        assert io.get() == b"".join(texts) and ver.get() == b"\1" * n and io.intact(n * ml), off


# ---- 6. forgeries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["tag of 0", "text of 4", "AAD of 8", "nonce of 5"])
def test_forgeries(orc, part):
    rng = random.Random(9)
    key, n, ml, al = KEYS[128], 9, 40, 13
    lens = [40, 33, 17, 40, 25, 16, 40, 1, 39]
    nonces, aads, slots = records(rng, n, al, ml)
    texts = [s[:k] for s, k in zip(slots, lens)]
    cts, tags = expected(orc, key, nonces, aads, texts)
    m = int(part.split()[-1])
    bit = rng.randrange(1 << 16)
    if part.startswith("tag"):
        tags[m] = flip(tags[m], bit)
    elif part.startswith("text"):
        cts[m] = flip(cts[m], bit)
    elif part.startswith("AAD"):
        aads[m] = flip(aads[m], bit)
    else:
        nonces[m] = flip(nonces[m], bit)
    orc_rc, left = orc.gcmsiv_decrypt(key, nonces[m], aads[m], cts[m] + tags[m])
    assert orc_rc == E_AUTH and len(left) == lens[m]
    padded = [c + bytes(ml - len(c)) for c in cts]
    eng = uaes.engine()
    for wipe in (0, 1):
        eng.uaes_set_wipe_on_auth_failure(wipe)
        try:
            rc, pts, verdicts = uaes.gcmsiv_batch(key, nonces, aads, padded, decrypt=True, tags=tags, prefill=0x5A, lens=lens)
        finally:
            eng.uaes_set_wipe_on_auth_failure(0)
        info = (part, bit, wipe)
        assert rc == E_AUTH and verdicts == [0 if k == m else 1 for k in range(n)], (info, rc, verdicts)
        assert pts[m][:lens[m]] == (bytes(lens[m]) if wipe else left), info
        for k in range(n):
            assert set(pts[k][lens[k]:]) <= {0x5A}, (info, k)                       # nothing else moves
            if k != m:
                assert pts[k][:lens[k]] == texts[k], (info, k)


# ---- 7. the counter's 32-bit wrap -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
def test_the_counter_wraps_inside_its_word(orc, bits):
    """received tags that start with LE32 0xFFFFFFFE / 0xFFFFFFFF: the keystream of a 5-block record runs through the wrap,
    which must stay inside bytes 0..3.  The tags are made up, so every verdict is 0 and the released text is the oracle's"""
    rng = random.Random(bits + 7)
    key, ml, al = KEYS[bits], 80, 5
    heads = [0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFD, 0xFFFFFFFC, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE]
    n = len(heads)
    nonces, aads, cts = records(rng, n, al, ml)
    tags = []
    for m, h in enumerate(heads):
        t = bytearray(h.to_bytes(4, "little") + rng.randbytes(12))
        t[15] = (t[15] & 0x7F) | (0x80 if m & 1 else 0)                             # byte 15 with and without bit 7
        tags.append(bytes(t))
    rc, pts, verdicts = uaes.gcmsiv_batch(key, nonces, aads, cts, decrypt=True, tags=tags, prefill=0x33)
    assert rc == E_AUTH and verdicts == [0] * n, (bits, rc, verdicts)
    for m in range(n):
        orc_rc, left = orc.gcmsiv_decrypt(key, nonces[m], aads[m], cts[m] + tags[m])
        assert orc_rc == E_AUTH and pts[m] == left, (bits, m, hex(heads[m]), tags[m].hex())


# ---- 8. published vectors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
def test_published_vectors(bits):
    """every case of SIV_GCM_ACVP.tv at this key size, grouped by (key, AAD length) into batches with per-record lengths.
    The file holds 102 cases, all with 128-bit keys (tests/test_oracle.py says so too), and the counts are asserted so
    that a file with 256-bit cases is noticed: until then 256-bit records are checked against the oracle alone"""
    cases = rsp.gcmsiv_cases(bits)
    assert len(cases) == (102 if bits == 128 else 0)
    groups = {}
    for c in cases:
        groups.setdefault((c["key"], len(c["aad"])), []).append(c)
    total = 0
    for (key, al), grp in groups.items():
        lens = [len(c["pt"]) for c in grp]
        ml = max(lens)
        pad = lambda b: b + bytes(ml - len(b))                                      # noqa: E731
        nonces, aads = [c["iv"] for c in grp], [c["aad"] for c in grp]
        cts, tags = uaes.gcmsiv_batch(key, nonces, aads, [pad(c["pt"]) for c in grp], lens=lens)
        for c, ct, tag, k in zip(grp, cts, tags, lens):
            assert ct[:k] + tag == c["ct"], (bits, c["Count"])
        rc, pts, verdicts = uaes.gcmsiv_batch(key, nonces, aads, [pad(c["ct"][:-16]) for c in grp], decrypt=True,
                                              tags=[c["ct"][-16:] for c in grp], lens=lens)
        assert rc == 0 and verdicts == [1] * len(grp), (bits, key.hex(), al, rc, verdicts)
        assert [p[:k] for p, k in zip(pts, lens)] == [c["pt"] for c in grp], (bits, key.hex(), al)
        total += len(grp)
    assert total == len(cases)


# ---- 9. the cap -------------------------------------------------------------------------------------------------------
def test_the_cap(orc):
    rng = random.Random(65535)
    key = KEYS[256]
    lens = [BATCH_MAX, 4097, 0]
    nonces, aads, slots = records(rng, 3, 3, BATCH_MAX)
    texts = [s[:k] for s, k in zip(slots, lens)]
    want = expected(orc, key, nonces, aads, texts)
    cts, tags = uaes.gcmsiv_batch(key, nonces, aads, slots, lens=lens, prefill=0x44)
    for m in range(3):
        assert cts[m][:lens[m]] == want[0][m] and tags[m] == want[1][m], ("text at the cap", m)
        assert set(cts[m][lens[m]:]) <= {0x44}, ("text at the cap", m)
    rc, pts, verdicts = uaes.gcmsiv_batch(key, nonces, aads, cts, decrypt=True, tags=tags, lens=lens, prefill=0x44)
    assert rc == 0 and verdicts == [1, 1, 1] and [p[:k] for p, k in zip(pts, lens)] == texts
    # 65 535 bytes of AAD, 16-byte texts
    nonces, aads, texts = records(rng, 3, BATCH_MAX, 16)
    check_both(orc, key, nonces, aads, texts, "AAD at the cap")


# ---- 10. one call at a time -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_equals_the_one_message_calls(orc, bits):
    rng = random.Random(bits)
    key = KEYS[bits]
    for al, ml in ((0, 0), (20, 100), (12, 64), (300, 1000)):
        nonces, aads, texts = records(rng, 8, al, ml)
        cts, tags = uaes.gcmsiv_batch(key, nonces, aads, texts)
        for m in range(8):
            one = uaes.GCM_SIV_encrypt(key, nonces[m], aads[m], texts[m])
            assert cts[m] + tags[m] == one, (bits, al, ml, m)
            assert one == orc.gcmsiv_encrypt(key, nonces[m], aads[m], texts[m]), (bits, al, ml, m)
            assert uaes.GCM_SIV_decrypt(key, nonces[m], aads[m], cts[m] + tags[m]) == (0, texts[m]), (bits, al, ml, m)


# ---- 11. threads ------------------------------------------------------------------------------------------------------
def test_two_threads(orc):
    """each thread runs the loop of test 1 for one key size on its own lane; the expected values are made first, the
    threads only call the engine"""
    cases = {bits: short_shapes(orc, bits, 2000 + bits) for bits in (192, 256)}
    errors = []

    def worker(bits):
        try:
            for case in cases[bits]:
                check_against(*case)
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(bits,)) for bits in (192, 256)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
