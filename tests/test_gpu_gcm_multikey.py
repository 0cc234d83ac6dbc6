"""The multi-key GCM batches on the GPU (k_gcm_multikey, uaes_gcm_multikey.hip) against the CPU oracle's gcm_encrypt, one
oracle call per record under that record's key, bit for bit: every short shape, key isolation, record counts read from
the plan, per-record lengths, placements (the keys in device memory included), tag lengths, forgeries of every part of a
record (its key included), the counter's carry and the cap, the NIST vectors as batches, the one-message calls and two
threads.  Every failing case prints the tuple that reproduces it."""
import ctypes as C
import os
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests.rsp import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 0xA5
E_ARG = -2                                      # UAES_E_ARG
E_AUTH = 0x1A                                   # UAES_E_AUTHENTICATION
BATCH_MAX = 65535                               # UAES_GCM_MULTIKEY_BATCH_MAX


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


def batch(decrypt, bits, keys, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts=None):
    """the two entry points; every array bytes, None or Mem"""
    L = uaes.engine()
    if decrypt:
        return L.uaes_gcm_multikey_decrypt_batch(bits, ptr(keys), tl, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al,
                                                 ptr(src), ptr(tags), ptr(dst), ptr(verdicts))
    return L.uaes_gcm_multikey_encrypt_batch(bits, ptr(keys), tl, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al,
                                             ptr(src), ptr(dst), ptr(tags))


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def records(rng, n, bits, al, ml):
    """(keys, nonces, aads, texts): every record with a random key of its own"""
    return ([rng.randbytes(bits // 8) for _ in range(n)], [rng.randbytes(12) for _ in range(n)],
            [rng.randbytes(al) for _ in range(n)], [rng.randbytes(ml) for _ in range(n)])


def expected(orc, keys, nonces, aads, texts, tl=16):
    """the oracle's (ciphertexts, tags), one call per record"""
    cts, tags = [], []
    for key, nonce, aad, pt in zip(keys, nonces, aads, texts):
        ct = orc.gcm_encrypt(key, nonce, aad, pt, tl)
        cts.append(ct[:len(pt)])
        tags.append(ct[len(pt):])
    return cts, tags


def check_against(want, keys, nonces, aads, texts, info, tl=16):
    """encrypt == want per record; decrypt returns 0, all verdicts 1 and the plaintext into a prefilled buffer"""
    got = uaes.gcm_multikey_batch(keys, nonces, aads, texts, tag_len=tl)
    if got != want:
        bad = [m for m in range(len(texts)) if (got[0][m], got[1][m]) != (want[0][m], want[1][m])]
        raise AssertionError("encrypt %r: records %r differ" % (info, bad[:8]))
    rc, pts, verdicts = uaes.gcm_multikey_batch(keys, nonces, aads, got[0], decrypt=True, tags=got[1], tag_len=tl, prefill=0x77)
    assert rc == 0 and verdicts == [1] * len(texts) and pts == texts, ("decrypt", info, rc, verdicts)


def check_both(orc, keys, nonces, aads, texts, info, tl=16):
    check_against(expected(orc, keys, nonces, aads, texts, tl), keys, nonces, aads, texts, info, tl)


# ---- 1. every short shape ---------------------------------------------------------------------------------------------
AADS = (0, 1, 15, 16, 17, 32)


def short_shapes(orc, bits, seed):
    """the cases, with what the oracle gives for them; 5 records per call: one of them lands in a second wave"""
    rng = random.Random(seed)
    cases = []
    for ml in (range(50) if bits == 128 else (0, 15, 16, 17, 49)):
        for al in AADS:
            keys, nonces, aads, texts = records(rng, 5, bits, al, ml)
            cases.append((expected(orc, keys, nonces, aads, texts), keys, nonces, aads, texts, (bits, al, ml, seed)))
    return cases


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(orc, bits):
    for case in short_shapes(orc, bits, 1000 + bits):
        check_against(*case)


# ---- 2. key isolation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_key_isolation(orc, bits):
    """records 0, 2, 5 and 7 are the same record (rows of two waves); 1 and 6 differ from it only in the key: a schedule
    slot or a hash key that leaks from one row to its neighbour shows here"""
    rng = random.Random(bits + 3)
    k0, k1, k6 = (rng.randbytes(bits // 8) for _ in range(3))
    nonce, aad, text = rng.randbytes(12), rng.randbytes(7), rng.randbytes(40)
    other = lambda n: rng.randbytes(n)                                          # noqa: E731
    keys = [k0, k1, k0, other(bits // 8), other(bits // 8), k0, k6, k0]
    nonces = [nonce, nonce, nonce, other(12), other(12), nonce, nonce, nonce]
    aads = [aad, aad, aad, other(7), other(7), aad, aad, aad]
    texts = [text, text, text, other(40), other(40), text, text, text]
    cts, tags = uaes.gcm_multikey_batch(keys, nonces, aads, texts)
    for m in (2, 5, 7):
        assert (cts[m], tags[m]) == (cts[0], tags[0]), (bits, m)
    for m in (1, 6):
        assert tags[m] != tags[0] and cts[m] != cts[0], (bits, m)
    assert tags[1] != tags[6] and cts[1] != cts[6], bits
    check_both(orc, keys, nonces, aads, texts, ("isolation", bits))


# ---- 3. record counts from the plan -----------------------------------------------------------------------------------
def second_pass():
    """the first count at which the grid-stride loop of the largest launch runs a second time, + 3"""
    name, launches, grid, threads = uaes.gcm_multikey_batch_plan(16, 1 << 20)
    assert name == "gcm.multikey" and launches == 1 and threads % 16 == 0
    return grid * threads // 16 + 3


@pytest.mark.parametrize("which", range(6), ids=["1", "4", "5", "64", "65", "second-pass"])
def test_record_counts_from_the_plan(orc, which):
    nmsg = (1, 4, 5, 64, 65, second_pass())[which]
    rng = random.Random(nmsg)
    keys, nonces, aads, texts = records(rng, nmsg, 128, 5, 16)
    assert len(set(keys)) == nmsg                                               # every record has its own key
    if which < 5:
        check_both(orc, keys, nonces, aads, texts, ("count", nmsg))             # every record is compared
        return
    name, _, grid, threads = uaes.gcm_multikey_batch_plan(16, nmsg)
    assert name == "gcm.multikey" and nmsg > grid * threads // 16               # it does run a second time
    look = sorted(set(range(70)) | set(range(nmsg - 70, nmsg)) | set(rng.sample(range(nmsg), 200)))
    cts, tags = uaes.gcm_multikey_batch(keys, nonces, aads, texts)
    pick = lambda a: [a[m] for m in look]                                       # noqa: E731
    want = expected(orc, pick(keys), pick(nonces), pick(aads), pick(texts))
    bad = [m for k, m in enumerate(look) if (cts[m], tags[m]) != (want[0][k], want[1][k])]
    assert not bad, ("count", nmsg, bad[:8])
    rc, pts, verdicts = uaes.gcm_multikey_batch(keys, nonces, aads, cts, decrypt=True, tags=tags, prefill=0x77)
    assert rc == 0 and verdicts == [1] * nmsg and pts == texts, ("count", nmsg, rc)


# ---- 4. per-record lengths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_per_record_lengths(orc, device, lens_on_device):
    rng = random.Random(48)
    bits, ml, al = 128, 48, 9
    given = [0, 1, 15, 16, 17, 33, 48, 1000, 48, 0, 31]                         # 1000: taken as msg_bytes
    lens = [min(k, ml) for k in given]
    n = len(given)
    keys, nonces, aads, slots = records(rng, n, bits, al, ml)
    want = expected(orc, keys, nonces, aads, [s[:k] for s, k in zip(slots, lens)])
    lv = Mem(b"".join(k.to_bytes(4, "little") for k in given), lens_on_device)
    src, dst, tags = Mem(b"".join(slots), device), Mem(b"", device, size=n * ml), Mem(b"", device, size=n * 16)
    mk, mn, ma = Mem(b"".join(keys), device), Mem(b"".join(nonces), device), Mem(b"".join(aads), device)
    assert batch(False, bits, mk, 16, n, ml, lv, mn, ma, al, src, dst, tags) == 0
    out, tg = dst.get(), tags.get()
    for m in range(n):
        info = (device, lens_on_device, m, given[m])
        assert out[m * ml:m * ml + lens[m]] == want[0][m] and tg[m * 16:(m + 1) * 16] == want[1][m], info
        assert set(out[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, info            # beyond lens[m]: not written
    assert dst.intact(n * ml) and tags.intact(n * 16) and src.get() == b"".join(slots)
    back, ver = Mem(b"", device, size=n * ml), Mem(b"", device, size=n)
    assert batch(True, bits, mk, 16, n, ml, lv, mn, ma, al, dst, back, tags, ver) == 0
    got = back.get()
    for m in range(n):
        assert got[m * ml:m * ml + lens[m]] == slots[m][:lens[m]] and set(got[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, m
    assert ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n)


# ---- 5. placements ----------------------------------------------------------------------------------------------------
ARRAYS = ("keys", "nonces", "aad", "texts", "tags", "verdicts")
ALL = (1 << len(ARRAYS)) - 1
PLACES = [0, ALL] + [1 << k for k in range(len(ARRAYS))] + [ALL ^ (1 << k) for k in range(len(ARRAYS))]


def place_id(mask):
    return "+".join(a for k, a in enumerate(ARRAYS) if mask >> k & 1) or "host"


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("mask", PLACES, ids=[place_id(p) for p in PLACES])
def test_placements(orc, mask, off):
    """bit k of mask: array k is in device memory ("keys" alone: the keys on the device and the texts on the host;
    all but "keys": the reverse).  Offsets 1 and 3 with 33-byte records: the byte-wise paths of the text and of the key
    load; offset 0 with 32: the 4-byte-aligned ones"""
    rng = random.Random(33 + off)
    bits, n, al = 192, 21, 17
    ml = 33 if off else 32
    on = {a: bool(mask >> k & 1) for k, a in enumerate(ARRAYS)}
    keys, nonces, aads, texts = records(rng, n, bits, al, ml)
    want = expected(orc, keys, nonces, aads, texts)
    mk = Mem(b"".join(keys), on["keys"], off)
    mn, ma = Mem(b"".join(nonces), on["nonces"], off), Mem(b"".join(aads), on["aad"], off)
    src, dst = Mem(b"".join(texts), on["texts"], off), Mem(b"", on["texts"], off, size=n * ml)
    tags = Mem(b"", on["tags"], off, size=n * 16)
    info = (place_id(mask), off)
    assert batch(False, bits, mk, 16, n, ml, None, mn, ma, al, src, dst, tags) == 0, info
    assert dst.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]), info
    assert dst.intact(n * ml) and tags.intact(n * 16) and src.get() == b"".join(texts), info
    back, ver = Mem(b"", on["texts"], off, size=n * ml), Mem(b"", on["verdicts"], off, size=n)
    assert batch(True, bits, mk, 16, n, ml, None, mn, ma, al, dst, back, tags, ver) == 0, info
    assert back.get() == b"".join(texts) and ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n), info
    # crtxt == pntxt
    io = Mem(b"".join(texts), on["texts"], off)
    tags2 = Mem(b"", on["tags"], off, size=n * 16)
    assert batch(False, bits, mk, 16, n, ml, None, mn, ma, al, io, io, tags2) == 0, info
    assert io.get() == b"".join(want[0]) and tags2.get() == b"".join(want[1]) and io.intact(n * ml) and tags2.intact(n * 16), info
    ver2 = Mem(b"", on["verdicts"], off, size=n)
    assert batch(True, bits, mk, 16, n, ml, None, mn, ma, al, io, io, tags2, ver2) == 0, info
    assert io.get() == b"".join(texts) and io.intact(n * ml) and ver2.get() == b"\1" * n and ver2.intact(n), info
    assert mn.get() == b"".join(nonces) and ma.get() == b"".join(aads) and mn.intact(n * 12) and ma.intact(n * al), info
    assert mk.get() == b"".join(keys) and mk.intact(n * bits // 8), info


def test_in_place_with_more_blocks_than_a_chunk(orc):
    """row_walk requests a chunk of blocks ahead (four encrypting, eight on either walk decrypting): records of 21 blocks
    + 5 bytes in place, in device memory"""
    rng = random.Random(341)
    bits, n, ml = 256, 6, 341
    keys, nonces, aads, texts = records(rng, n, bits, 0, ml)
    want = expected(orc, keys, nonces, aads, texts)
    for off in (0, 2):
        io, tags, ver = Mem(b"".join(texts), True, off), Mem(b"", True, size=n * 16), Mem(b"", True, size=n)
        mk, mn = Mem(b"".join(keys), True, off), Mem(b"".join(nonces), True)
        assert batch(False, bits, mk, 16, n, ml, None, mn, None, 0, io, io, tags) == 0
        assert io.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]) and io.intact(n * ml), off
        assert batch(True, bits, mk, 16, n, ml, None, mn, None, 0, io, io, tags, ver) == 0
        assert io.get() == b"".join(texts) and ver.get() == b"\1" * n and io.intact(n * ml), off


# ---- 6. tag lengths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tl", [1, 4, 8, 12, 13, 16])
def test_tag_lengths(orc, tl):
    """tags are packed at m * tagLen, and the byte after the last tag is not written"""
    rng = random.Random(tl)
    bits, n, ml, al = 128, 7, 37, 11
    keys, nonces, aads, texts = records(rng, n, bits, al, ml)
    want = expected(orc, keys, nonces, aads, texts, tl)
    assert all(len(t) == tl for t in want[1])
    for device in (False, True):
        src, dst, tags = Mem(b"".join(texts), device), Mem(b"", device, size=n * ml), Mem(b"", device, 1, size=n * tl)
        assert batch(False, bits, b"".join(keys), tl, n, ml, None, b"".join(nonces), b"".join(aads), al, src, dst, tags) == 0
        assert dst.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]) and tags.intact(n * tl), (tl, device)
        back, ver = Mem(b"", device, size=n * ml), Mem(b"", device, size=n)
        assert batch(True, bits, b"".join(keys), tl, n, ml, None, b"".join(nonces), b"".join(aads), al, dst, back, tags, ver) == 0
        assert back.get() == b"".join(texts) and ver.get() == b"\1" * n, (tl, device)
    check_against(want, keys, nonces, aads, texts, ("tag length", tl), tl)


# ---- 7. forgeries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["prefilled", "in-place"])
@pytest.mark.parametrize("part", ["text of 4", "tag of 0", "AAD of 7", "nonce of 5", "key of 3"])
def test_forgeries(orc, part, in_place):
    """one flipped bit in one record among eight: verdict 0 and an untouched output slot for that one, 0x1A for the call,
    and the other seven authentic and correct"""
    rng = random.Random(9)
    bits, n, ml, al = 128, 8, 40, 13
    keys, nonces, aads, texts = records(rng, n, bits, al, ml)
    cts, tags = expected(orc, keys, nonces, aads, texts)
    m = int(part.split()[-1])
    bit = rng.randrange(1 << 16)
    what = {"text": cts, "tag": tags, "AAD": aads, "nonce": nonces, "key": keys}[part.split()[0]]
    what[m] = flip(what[m], bit)
    assert orc.gcm_decrypt(keys[m], nonces[m], aads[m], cts[m] + tags[m])[0] == E_AUTH
    info = (part, bit, in_place)
    if in_place:
        io, ver = Mem(b"".join(cts), True), Mem(b"", True, size=n)
        rc = batch(True, bits, b"".join(keys), 16, n, ml, None, b"".join(nonces), b"".join(aads), al, io, io, b"".join(tags), ver)
        out = io.get()
        pts, verdicts = [out[k * ml:(k + 1) * ml] for k in range(n)], list(ver.get())
        left = cts[m]                                                            # it stays ciphertext
        assert io.intact(n * ml), info
    else:
        rc, pts, verdicts = uaes.gcm_multikey_batch(keys, nonces, aads, cts, decrypt=True, tags=tags, prefill=0x5A)
        left = bytes([0x5A]) * ml                                                # it stays the prefill
    assert rc == E_AUTH and verdicts == [0 if k == m else 1 for k in range(n)], (info, rc, verdicts)
    assert pts[m] == left, info
    assert [pts[k] for k in range(n) if k != m] == [texts[k] for k in range(n) if k != m], info


def test_a_forged_record_is_untouched_whatever_the_wipe_switch_says(orc):
    rng = random.Random(77)
    n, ml = 8, 40
    keys, nonces, aads, texts = records(rng, n, 256, 13, ml)
    cts, tags = expected(orc, keys, nonces, aads, texts)
    tags[2] = flip(tags[2], 5)
    eng = uaes.engine()
    for wipe in (0, 1):
        eng.uaes_set_wipe_on_auth_failure(wipe)
        try:
            rc, pts, verdicts = uaes.gcm_multikey_batch(keys, nonces, aads, cts, decrypt=True, tags=tags, prefill=0x5A)
        finally:
            eng.uaes_set_wipe_on_auth_failure(0)
        assert rc == E_AUTH and verdicts == [1, 1, 0, 1, 1, 1, 1, 1], (wipe, rc, verdicts)
        assert pts[2] == bytes([0x5A]) * ml, wipe                                # untouched, not zeroed
        assert pts[:2] + pts[3:] == texts[:2] + texts[3:], wipe


def test_every_byte_of_a_short_tag_is_compared(orc):
    """tagLen 4 in the packed layout: the four bytes of record m are bytes 4 m .. 4 m + 3 of the array and nothing lies
    between two tags, so a flip in byte 3 of record 1's tag (the last one compared) must be caught, in that record only"""
    rng = random.Random(4)
    n, ml, tl = 8, 24, 4
    keys, nonces, aads, texts = records(rng, n, 192, 5, ml)
    cts, tags = expected(orc, keys, nonces, aads, texts, tl)
    packed = bytearray(b"".join(tags))
    assert len(packed) == n * tl
    for byte in range(tl):
        forged = bytearray(packed)
        forged[1 * tl + byte] ^= 0x80
        split = [bytes(forged[k * tl:(k + 1) * tl]) for k in range(n)]
        rc, pts, verdicts = uaes.gcm_multikey_batch(keys, nonces, aads, cts, decrypt=True, tags=split, tag_len=tl, prefill=0x11)
        assert rc == E_AUTH and verdicts == [1, 0] + [1] * 6, (byte, rc, verdicts)
        assert pts[1] == bytes([0x11]) * ml and pts[0] == texts[0] and pts[2:] == texts[2:], byte


# ---- 8. the counter's carry and the cap -------------------------------------------------------------------------------
def test_the_counter_carries_into_byte_14(orc):
    """three records of 4112 bytes = 257 blocks: the block counter passes 255 and 256 (J0 + 1 + i with i up to 256), so
    byte 15 carries into byte 14"""
    rng = random.Random(4112)
    keys, nonces, aads, texts = records(rng, 3, 128, 3, 4112)
    check_both(orc, keys, nonces, aads, texts, "carry")


def test_the_cap(orc):
    rng = random.Random(65535)
    keys, nonces, aads, texts = records(rng, 1, 256, BATCH_MAX, BATCH_MAX)
    check_both(orc, keys, nonces, aads, texts, "text and AAD at the cap")
    k, nn = b"".join(keys), b"".join(nonces)
    big = bytes(BATCH_MAX + 1)
    out, tag, ver = Mem(b"", size=BATCH_MAX + 1), Mem(b"", size=16), Mem(b"", size=1)
    for dec in (False, True):
        assert batch(dec, 256, k, 16, 1, BATCH_MAX + 1, None, nn, None, 0, big, out, tag, ver) == E_ARG, dec
        assert batch(dec, 256, k, 16, 1, 16, None, nn, big, BATCH_MAX + 1, big, out, tag, ver) == E_ARG, dec
    assert out.intact(0) and tag.intact(0)


# ---- 9. the NIST vectors as batches -----------------------------------------------------------------------------------
def nist_groups(bits):
    """the 96-bit-IV stanzas of GcmEncryptExtIV<bits>.rsp, grouped by (PTlen, AADlen, Taglen) in bytes"""
    groups, hdr, cur = {}, {}, None
    with open(os.path.join(GOLDEN, "GcmEncryptExtIV%d.rsp" % bits)) as f:
        for ln in f:
            ln = ln.strip()
            if ln.startswith("["):
                k, v = ln.strip("[]").split("=")
                hdr[k.strip()] = int(v)
            elif "=" in ln:
                k, v = [t.strip() for t in ln.split("=", 1)]
                if k == "Count":
                    cur = {}
                elif cur is not None:
                    cur[k] = bytes.fromhex(v)
                    if k == "Tag":
                        if hdr["Keylen"] == bits and hdr["IVlen"] == 96 and hdr["PTlen"] % 8 == 0 and hdr["AADlen"] % 8 == 0 \
                                and hdr["Taglen"] % 8 == 0:
                            groups.setdefault((hdr["PTlen"] // 8, hdr["AADlen"] // 8, hdr["Taglen"] // 8), []).append(cur)
                        cur = None
    return groups


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_the_nist_vectors_as_batches(bits):
    """every stanza has a key of its own, so a group is one multi-key call"""
    groups = nist_groups(bits)
    assert len(groups) == 25, sorted(groups)            # (the fixture holds the stanzas with 128-bit tags: 25 of 15 cases)
    total = 0
    for (ml, al, tl), grp in sorted(groups.items()):
        assert all(len(c["Key"]) * 8 == bits and len(c["IV"]) == 12 and len(c["PT"]) == ml == len(c["CT"]) and
                   len(c["AAD"]) == al and len(c["Tag"]) == tl for c in grp), (bits, ml, al, tl)
        keys, nonces, aads = [c["Key"] for c in grp], [c["IV"] for c in grp], [c["AAD"] for c in grp]
        cts, tags = uaes.gcm_multikey_batch(keys, nonces, aads, [c["PT"] for c in grp], tag_len=tl)
        bad = [m for m, c in enumerate(grp) if (cts[m], tags[m]) != (c["CT"], c["Tag"])]
        assert not bad, (bits, ml, al, tl, bad)
        rc, pts, verdicts = uaes.gcm_multikey_batch(keys, nonces, aads, [c["CT"] for c in grp], decrypt=True,
                                                    tags=[c["Tag"] for c in grp], tag_len=tl, prefill=0x3C)
        assert rc == 0 and verdicts == [1] * len(grp) and pts == [c["PT"] for c in grp], (bits, ml, al, tl, rc, verdicts)
        total += len(grp)
    assert total == 375                                 # tests/rsp.py: the count is itself a check on the parser


# ---- 10. one call at a time -------------------------------------------------------------------------------------------
def one_message(decrypt, key, nonce, tl, aad, data):
    """uaes_gcm_encrypt_ex / uaes_gcm_decrypt_ex: (code, output)"""
    L = uaes.engine()
    n = len(data) - (tl if decrypt else 0)
    out = (C.c_uint8 * max(n + 16, 1))()
    f = L.uaes_gcm_decrypt_ex if decrypt else L.uaes_gcm_encrypt_ex
    rc = f(len(key) * 8, key, nonce, 12, tl, aad, len(aad), data, n, out)
    return rc, bytes(out)[:n if decrypt else n + tl]


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_equals_the_one_message_calls(orc, bits):
    rng = random.Random(bits)
    for al, ml, tl in ((0, 0, 16), (20, 100, 16), (12, 64, 12), (300, 1000, 8)):
        keys, nonces, aads, texts = records(rng, 8, bits, al, ml)
        cts, tags = uaes.gcm_multikey_batch(keys, nonces, aads, texts, tag_len=tl)
        for m in (0, 3, 7):
            info = (bits, al, ml, tl, m)
            assert one_message(False, keys[m], nonces[m], tl, aads[m], texts[m]) == (0, cts[m] + tags[m]), info
            assert cts[m] + tags[m] == orc.gcm_encrypt(keys[m], nonces[m], aads[m], texts[m], tl), info
            assert one_message(True, keys[m], nonces[m], tl, aads[m], cts[m] + tags[m]) == (0, texts[m]), info


# ---- 11. threads ------------------------------------------------------------------------------------------------------
def test_two_threads(orc):
    """each thread runs the loop of test 1 for one key size on its own lane, with keys of its own; the expected values
    are made first, the threads only call the engine"""
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
