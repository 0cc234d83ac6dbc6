"""The OCB batches on the GPU (k_ocb_batch, uaes_ocb.hip) against the CPU oracle's ocb_encrypt / ocb_decrypt: every short
shape, all 64 values of `bottom`, record counts read from the plan, the offset chain over long records, the cap,
per-record lengths, placements, forgeries of every part of a record, the one-message calls, the published vectors, a
seeded fuzz and two threads.  Every failing case prints the tuple that reproduces it."""
import ctypes as C
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests import rsp

pytestmark = pytest.mark.gpu

GUARD = 0xA5
OCB_BATCH_MAX = 65535                           # UAES_OCB_BATCH_MAX (csrc/uaes_plan.h)
KEYS = {bits: bytes((bits // 8 + 7 * i) & 0xff for i in range(bits // 8)) for bits in (128, 192, 256)}


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


def batch(decrypt, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts=None):
    """the two entry points; every array bytes, None or Mem"""
    L = uaes.engine()
    if decrypt:
        return L.uaes_ocb_decrypt_batch(len(key) * 8, key, nl, tl, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al, ptr(src),
                                        ptr(tags), ptr(dst), ptr(verdicts))
    return L.uaes_ocb_encrypt_batch(len(key) * 8, key, nl, tl, nmsg, ml, ptr(lens), ptr(nonces), ptr(aads), al, ptr(src),
                                    ptr(dst), ptr(tags))


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def records(rng, n, nl, al, ml):
    return [rng.randbytes(nl) for _ in range(n)], [rng.randbytes(al) for _ in range(n)], [rng.randbytes(ml) for _ in range(n)]


def expected(orc, key, nonces, aads, texts, tl):
    """the oracle's (ciphertexts, tags), one call per record"""
    cts, tags = [], []
    for nonce, aad, pt in zip(nonces, aads, texts):
        ct = orc.ocb_encrypt(key, nonce, aad, pt, tag_len=tl)
        cts.append(ct[:len(pt)])
        tags.append(ct[len(pt):])
    return cts, tags


def check_both(orc, key, nonces, aads, texts, tl, info, lens=None):
    """encrypt == the oracle per record; decrypt returns 0, all verdicts 1 and the plaintext over a prefilled output"""
    cut = texts if lens is None else [t[:k] for t, k in zip(texts, lens)]
    want = expected(orc, key, nonces, aads, cut, tl)
    cts, tags = uaes.ocb_batch(key, nonces, aads, texts, tag_len=tl, lens=lens, prefill=0x33)
    got = ([c[:len(t)] for c, t in zip(cts, cut)], tags)
    if got != want:
        bad = [m for m in range(len(texts)) if (got[0][m], got[1][m]) != (want[0][m], want[1][m])]
        raise AssertionError("encrypt %r: records %r differ" % (info, bad[:8]))
    if lens is not None:
        assert all(set(c[k:]) <= {0x33} for c, k in zip(cts, lens)), ("encrypt wrote beyond lens", info)
    rc, pts, verdicts = uaes.ocb_batch(key, nonces, aads, cts, tag_len=tl, decrypt=True, tags=tags, prefill=0x77, lens=lens)
    assert rc == 0 and verdicts == [1] * len(texts), ("decrypt", info, rc, verdicts)
    assert [p[:len(t)] for p, t in zip(pts, cut)] == cut, ("decrypt", info)
    if lens is not None:
        assert all(set(p[k:]) <= {0x77} for p, k in zip(pts, lens)), ("decrypt wrote beyond lens", info)


# ---- 1. every short shape ---------------------------------------------------------------------------------------------
AADS = (0, 1, 15, 16, 17, 32, 33)


@pytest.mark.parametrize("nl", [1, 12, 15])
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(orc, bits, nl):
    """5 records per call: one of them lands in a second wave"""
    rng = random.Random(1000 * bits + nl)
    key = KEYS[bits]
    for ml in (range(50) if bits == 128 else (0, 15, 16, 17, 31, 32, 33, 49)):
        for al in AADS:
            for tl in (1, 8, 16):
                nonces, aads, texts = records(rng, 5, nl, al, ml)
                check_both(orc, key, nonces, aads, texts, tl, (bits, nl, tl, al, ml))


# ---- 2. all 64 values of bottom ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
def test_every_value_of_bottom(orc, bits):
    """the last nonce byte of record m is m: the stretch is shifted by every bit count, word boundaries included"""
    rng = random.Random(64 + bits)
    nonces, aads, texts = records(rng, 64, 12, 7, 33)
    nonces = [nc[:11] + bytes([m]) for m, nc in enumerate(nonces)]
    check_both(orc, KEYS[bits], nonces, aads, texts, 16, ("bottom", bits))


# ---- 3. record counts from the plan -----------------------------------------------------------------------------------
def second_pass():
    """the first count at which the grid-stride loop of the largest launch runs a second time, + 3"""
    name, launches, grid, threads = uaes.ocb_batch_plan(16, 1 << 20)
    assert name == "ocb.batch" and launches == 1 and threads % 16 == 0
    return grid * threads // 16 + 3


@pytest.mark.parametrize("which", range(8), ids=["1", "3", "4", "16", "17", "8192", "8193", "second-pass"])
def test_record_counts_from_the_plan(orc, which):
    nmsg = (1, 3, 4, 16, 17, 8192, 8193, second_pass())[which]
    if which == 7:
        for dec in (False, True):
            name, _, grid, threads = uaes.ocb_batch_plan(16, nmsg, decrypt=dec)
            assert name == "ocb.batch" and nmsg > grid * threads // 16           # it does run a second time
    rng = random.Random(nmsg)
    nonces, aads, texts = records(rng, nmsg, 12, 5, 16)
    check_both(orc, KEYS[128], nonces, aads, texts, 8, ("count", nmsg))         # every record is compared


# ---- 4. the offset chain and the depth of the walk --------------------------------------------------------------------
@pytest.mark.parametrize("ml", [341, 529, 2069])
def test_offset_chain_and_walk_depth(orc, ml):
    """341: 21 blocks + 5 bytes (row_walk looks 16 blocks ahead, an odd count); 529: 33 blocks + 1 byte; 2069: crosses
    block 128 (ntz 7).  In place and out of place, device memory, offsets 0 and 2, both directions."""
    rng = random.Random(ml)
    key, n, nl, al, tl = KEYS[256], 6, 12, 21, 16
    nonces, aads, texts = records(rng, n, nl, al, ml)
    want = expected(orc, key, nonces, aads, texts, tl)
    mn, ma = Mem(b"".join(nonces), True), Mem(b"".join(aads), True)
    for off in (0, 2):
        info = (ml, off)
        # out of place
        src, dst = Mem(b"".join(texts), True, off), Mem(b"", True, off, size=n * ml)
        tags, ver = Mem(b"", True, size=n * tl), Mem(b"", True, size=n)
        assert batch(False, key, nl, tl, n, ml, None, mn, ma, al, src, dst, tags) == 0, info
        assert dst.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]), info
        assert dst.intact(n * ml) and src.get() == b"".join(texts), info
        back = Mem(b"", True, off, size=n * ml)
        assert batch(True, key, nl, tl, n, ml, None, mn, ma, al, dst, back, tags, ver) == 0, info
        assert back.get() == b"".join(texts) and ver.get() == b"\1" * n and back.intact(n * ml), info
        # in place
        io, tags2, ver2 = Mem(b"".join(texts), True, off), Mem(b"", True, size=n * tl), Mem(b"", True, size=n)
        assert batch(False, key, nl, tl, n, ml, None, mn, ma, al, io, io, tags2) == 0, info
        assert io.get() == b"".join(want[0]) and tags2.get() == b"".join(want[1]) and io.intact(n * ml), info
        assert batch(True, key, nl, tl, n, ml, None, mn, ma, al, io, io, tags2, ver2) == 0, info
        assert io.get() == b"".join(texts) and ver2.get() == b"\1" * n and io.intact(n * ml), info


# ---- 5. the cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
def test_the_cap(orc, bits):
    """3 records of 65535 bytes with 65535 bytes of AAD: 4095 blocks and a 15-byte tail, ntz up to 11"""
    rng = random.Random(OCB_BATCH_MAX + bits)
    nonces, aads, texts = records(rng, 3, 12, OCB_BATCH_MAX, OCB_BATCH_MAX)
    check_both(orc, KEYS[bits], nonces, aads, texts, 16, ("cap", bits))


# ---- 6. variable lengths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_variable_lengths(orc, device, lens_on_device):
    rng = random.Random(48)
    key, n, ml, nl, al, tl = KEYS[128], 37, 48, 12, 9, 8
    lens = [rng.randrange(49) for _ in range(n)]
    lens[3], lens[20], lens[36] = 0, 48, 17
    assert min(lens) == 0 and max(lens) == 48
    nonces, aads, slots = records(rng, n, nl, al, ml)
    want = expected(orc, key, nonces, aads, [s[:k] for s, k in zip(slots, lens)], tl)
    lv = Mem(b"".join(k.to_bytes(4, "little") for k in lens), lens_on_device)
    src, dst, tags = Mem(b"".join(slots), device), Mem(b"", device, size=n * ml), Mem(b"", device, size=n * tl)
    mn, ma = Mem(b"".join(nonces), device), Mem(b"".join(aads), device)
    assert batch(False, key, nl, tl, n, ml, lv, mn, ma, al, src, dst, tags) == 0
    out, tg = dst.get(), tags.get()
    for m in range(n):
        info = (device, lens_on_device, m, lens[m])
        assert out[m * ml:m * ml + lens[m]] == want[0][m] and tg[m * tl:(m + 1) * tl] == want[1][m], info
        assert set(out[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, info            # beyond lens[m]: not written
    assert dst.intact(n * ml) and tags.intact(n * tl)
    # decrypt, and an entry above msg_bytes is taken as msg_bytes
    back, ver = Mem(b"", device, size=n * ml), Mem(b"", device, size=n)
    assert batch(True, key, nl, tl, n, ml, lv, mn, ma, al, dst, back, tags, ver) == 0
    got = back.get()
    for m in range(n):
        assert got[m * ml:m * ml + lens[m]] == slots[m][:lens[m]] and set(got[m * ml + lens[m]:(m + 1) * ml]) <= {GUARD}, m
    assert ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n)
    clamp = Mem(b"".join((k if k < 48 else 1000 + k).to_bytes(4, "little") for k in lens), lens_on_device)
    dst2, tags2 = Mem(b"", device, size=n * ml), Mem(b"", device, size=n * tl)
    assert batch(False, key, nl, tl, n, ml, clamp, mn, ma, al, src, dst2, tags2) == 0
    assert dst2.get() == out and tags2.get() == tg and dst2.intact(n * ml)


# ---- 7. placement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_placement(orc, device, off):
    """offsets 1 and 3 with 33-byte records: the byte-wise path; offset 0 with 32: the 4-byte-aligned one"""
    rng = random.Random(33 + off)
    key, n, nl, al, tl = KEYS[192], 21, 13, 17, 10
    ml = 33 if off else 32
    nonces, aads, texts = records(rng, n, nl, al, ml)
    want = expected(orc, key, nonces, aads, texts, tl)
    mn, ma = Mem(b"".join(nonces), device, off), Mem(b"".join(aads), device, off)
    src, dst, tags = Mem(b"".join(texts), device, off), Mem(b"", device, off, size=n * ml), Mem(b"", device, off, size=n * tl)
    info = (device, off)
    assert batch(False, key, nl, tl, n, ml, None, mn, ma, al, src, dst, tags) == 0, info
    assert dst.get() == b"".join(want[0]) and tags.get() == b"".join(want[1]), info
    assert dst.intact(n * ml) and tags.intact(n * tl) and src.get() == b"".join(texts), info
    back, ver = Mem(b"", device, off, size=n * ml), Mem(b"", device, off, size=n)
    assert batch(True, key, nl, tl, n, ml, None, mn, ma, al, dst, back, tags, ver) == 0, info
    assert back.get() == b"".join(texts) and ver.get() == b"\1" * n and back.intact(n * ml) and ver.intact(n), info
    # crtxt == pntxt
    io = Mem(b"".join(texts), device, off)
    tags2 = Mem(b"", device, off, size=n * tl)
    assert batch(False, key, nl, tl, n, ml, None, mn, ma, al, io, io, tags2) == 0, info
    assert io.get() == b"".join(want[0]) and tags2.get() == b"".join(want[1]) and io.intact(n * ml) and tags2.intact(n * tl), info
    ver2 = Mem(b"", device, off, size=n)
    assert batch(True, key, nl, tl, n, ml, None, mn, ma, al, io, io, tags2, ver2) == 0, info
    assert io.get() == b"".join(texts) and io.intact(n * ml) and ver2.get() == b"\1" * n, info


# ---- 8. forgeries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["tag of 0", "text of 4", "AAD of 8", "nonce of 5"])
def test_forgeries(orc, part):
    rng = random.Random(9)
    key, n, ml, nl, al, tl = KEYS[128], 9, 40, 12, 13, 8
    nonces, aads, texts = records(rng, n, nl, al, ml)
    cts, tags = expected(orc, key, nonces, aads, texts, tl)
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
    orc_rc, left = orc.ocb_decrypt(key, nonces[m], aads[m], cts[m] + tags[m], tag_len=tl)
    assert orc_rc == 0x1A and len(left) == ml
    eng = uaes.engine()
    for wipe in (0, 1):
        eng.uaes_set_wipe_on_auth_failure(wipe)
        try:
            rc, pts, verdicts = uaes.ocb_batch(key, nonces, aads, cts, tag_len=tl, decrypt=True, tags=tags, prefill=0x5A)
        finally:
            eng.uaes_set_wipe_on_auth_failure(0)
        info = (part, bit, wipe)
        assert rc == 0x1A and verdicts == [0 if k == m else 1 for k in range(n)], (info, rc, verdicts)
        assert pts[m] == (bytes(ml) if wipe else left), info
        assert [p for k, p in enumerate(pts) if k != m] == [t for k, t in enumerate(texts) if k != m], info


# ---- 9. one call at a time --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_equals_the_one_message_calls(bits):
    rng = random.Random(bits)
    key = KEYS[bits]
    for nl, tl, al, ml in ((1, 1, 0, 0), (12, 16, 20, 100), (15, 8, 13, 64), (12, 10, 300, 1000), (8, 6, 16, 257)):
        nonces, aads, texts = records(rng, 7, nl, al, ml)
        cts, tags = uaes.ocb_batch(key, nonces, aads, texts, tag_len=tl)
        for m in range(7):
            one = uaes.AES_OCB_encrypt(key, nonces[m], aads[m], texts[m], tag_len=tl)
            assert cts[m] + tags[m] == one, (bits, nl, tl, al, ml, m)
            assert uaes.AES_OCB_decrypt(key, nonces[m], aads[m], cts[m] + tags[m], tag_len=tl) == (0, texts[m]), (bits, nl, tl, al, ml, m)


# ---- 10. published vectors --------------------------------------------------------------------------------------------
def test_published_vectors():
    """OCB_AES128.tv: one batch per (key, text length, AAD length) group"""
    cases = rsp.ocb_cases(128)
    groups = {}
    for c in cases:
        groups.setdefault((c["key"], len(c["pt"]), len(c["aad"])), []).append(c)
    total = 0
    for (key, ml, al), g in groups.items():
        nonces, aads, texts = [c["iv"] for c in g], [c["aad"] for c in g], [c["pt"] for c in g]
        cts, tags = uaes.ocb_batch(key, nonces, aads, texts, tag_len=16)
        assert [a + b for a, b in zip(cts, tags)] == [c["ct"] for c in g], (key.hex(), ml, al)
        assert uaes.ocb_batch(key, nonces, aads, cts, tag_len=16, decrypt=True, tags=tags) == (0, texts, [1] * len(g)), (key.hex(), ml, al)
        total += len(g)
    assert total == len(cases) and total != 0


# ---- 11. fuzz ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(orc, seed):
    rng = random.Random(7000 + seed)
    bits = rng.choice((128, 192, 256))
    key = rng.randbytes(bits // 8)
    nl, tl, al, ml, n = rng.randrange(1, 16), rng.randrange(1, 17), rng.randrange(71), rng.randrange(201), rng.randrange(1, 301)
    lens = [rng.randrange(ml + 1) for _ in range(n)] if rng.randrange(2) else None
    nonces, aads, texts = records(rng, n, nl, al, ml)
    check_both(orc, key, nonces, aads, texts, tl, ("fuzz", seed, bits, nl, tl, al, ml, n, lens is not None), lens=lens)


# ---- 12. threads ------------------------------------------------------------------------------------------------------
def test_two_threads_with_different_keys(orc):
    """the expected values are made first; the threads only call the engine"""
    cases = {}
    for seed in (10, 20):
        rng = random.Random(seed)
        key = rng.randbytes(16)
        cases[seed] = []
        for n, ml in ((1, 0), (5, 17), (70, 64), (300, 33), (9, 1000)):
            nonces, aads, texts = records(rng, n, 12, ml % 31, ml)
            cases[seed].append((key, nonces, aads, texts, expected(orc, key, nonces, aads, texts, 8)))
    errors = []

    def worker(seed):
        try:
            for _ in range(3):
                for key, nonces, aads, texts, want in cases[seed]:
                    got = uaes.ocb_batch(key, nonces, aads, texts, tag_len=8)
                    assert got == want, (seed, len(texts), len(texts[0]))
                    back = uaes.ocb_batch(key, nonces, aads, got[0], tag_len=8, decrypt=True, tags=got[1])
                    assert back == (0, texts, [1] * len(texts)), (seed, len(texts), len(texts[0]))
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(s,)) for s in (10, 20)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
