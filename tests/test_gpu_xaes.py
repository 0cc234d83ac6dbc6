"""XAES-256-GCM on the GPU (uaes_xaes256gcm_*; k_xaes_gcm_batch, uaes_xaes.hip) against tests/xaes_ref.py -- the oracle's
encrypt_block and gcm_encrypt composed as the C2SP specification says -- bit for bit.  Its own: the one-message calls (the
specification's vectors, the lengths around a block, a text on the fused GCM kernels, host and device pointers, the
accumulated stream), the two halves of the nonce, both branches of CMAC's doubling, the counter's carry and the cap, a
forgery without verdicts, the multi-key cross-check and key hygiene.  Through the frame of tests/aead_batch_cases.py:
every short shape, record counts read from the plan, per-record lengths, placements, in place, forgeries of every part
of a record, the one-message calls and two threads.  Every failing case prints the tuple that reproduces it."""
import hashlib
import random

import pytest

import micro_aes_amd as uaes
from tests import aead_batch_cases as F
from tests import key_wipe_cases as kw
from tests import xaes_ref
from tests.guarded_mem import FILL, Mem, ptr

pytestmark = pytest.mark.gpu

E_ARG = -2                                      # UAES_E_ARG
E_AUTH = 0x1A                                   # UAES_E_AUTHENTICATION
BATCH_MAX = 65535                               # UAES_XAES_GCM_BATCH_MAX
KEY = bytes(range(0x10, 0x30))
AADS = (0, 1, 15, 16, 17, 32)


def raw(decrypt, bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts):
    L = uaes.engine()
    if decrypt:
        return L.uaes_xaes256gcm_decrypt_batch(key, nmsg, ml, lens, nonces, aads, al, src, tags, dst, verdicts)
    return L.uaes_xaes256gcm_encrypt_batch(key, nmsg, ml, lens, nonces, aads, al, src, dst, tags)


def one_message(decrypt, key, nonce, aad, data, tl):
    return (uaes.xaes256gcm_decrypt if decrypt else uaes.xaes256gcm_encrypt)(key, nonce, aad, data)


def forge(part):
    """record 5 of the forgery case with one bit flipped: `part` is "text", "tag", "AAD" or "nonce[<byte>]" """
    c, rng = F.forgery_case(MODE)
    bit = rng.randrange(8)
    if part.startswith("nonce"):
        what, where = "nonce", lambda b: 8 * int(part[6:-1]) + bit
    else:
        what, where = part, lambda b: rng.randrange(8 * len(b))
    return F.forged(MODE, c, what, 5, lambda b: xaes_ref.flip(b, where(b)))


MODE = F.Mode(
    name="xaes256gcm",
    plan=lambda length, nmsg, decrypt: uaes.xaes256gcm_batch_plan(length, nmsg, decrypt=decrypt),
    arrangement="xaes.gcm",
    wrapper=uaes.xaes256gcm_batch,
    raw=raw,
    key_bits=(256,),
    fixed_keys={256: KEY},
    nonce_lens=(24,),
    tag_lens=None,
    enc=lambda key, nonce, aad, pt, tl: xaes_ref.encrypt(key, nonce, aad, pt),
    dec=lambda key, nonce, aad, ct, tl: xaes_ref.decrypt(key, nonce, aad, ct),
    one=one_message,
    forged=("untouched", "untouched"),
    # lengths 0..65 in one launch through lens, for every AAD size; slots of 68 bytes (4-byte aligned texts) or 67 (not)
    short_shapes=lambda bits: [(66, 16, al, 68 if al % 2 == 0 else 67, list(range(66))) for al in AADS],
    short_nls=(24,),
    short_seed=lambda bits, nl: 1000,
    count_shape=(24, 5, 16, 16),
    count_sampled=True,
    lengths_shape=(24, 16, None),
    placement_shape=(24, 16),
    placement_offsets=(0, 1, 3),
    forgery_shape=(8, 24, 16, None),
    forgery_parts=("text", "tag", "AAD", "nonce[5]", "nonce[17]"),
    forge=forge,
)
COUNTS = (1, 4, 5, 64, 65)
PLACES = F.places(MODE)


def records(rng, n, al, ml):
    """the case of n records under KEY"""
    return F.draw(MODE, rng, 256, n, 24, al, ml)


def batch(decrypt, c, nonces, aads, src, dst, tags, verdicts=None):
    return F.run(MODE, c, decrypt, c.key, None, nonces, aads, src, dst, tags, verdicts)


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
def test_every_short_shape():
    F.check_short_shapes(MODE, 256, 24)


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
    F.check_both(MODE, F.Case(256, KEY, nonces, [aad] * 8, [text] * 8), "nonce halves")


# ---- 4. both branches of CMAC's doubling ------------------------------------------------------------------------------
def test_master_keys_with_the_top_bit_of_l_set_and_clear():
    rng = random.Random(87)
    top_set, top_clear = xaes_ref.keys_by_top_bit_of_l()
    assert xaes_ref.big_l(top_set)[0] >> 7 == 1 and xaes_ref.big_l(top_clear)[0] >> 7 == 0
    for key in (top_set, top_clear):
        c = records(rng, 5, 11, 33)._replace(key=key)
        assert [uaes.xaes256gcm_derive(key, n) for n in c.nonces] == [xaes_ref.derive(key, n) for n in c.nonces]
        F.check_both(MODE, c, ("top bit", key.hex()))
        assert uaes.xaes256gcm_encrypt(key, c.nonces[0], c.aads[0], c.texts[0]) == xaes_ref.encrypt(key, c.nonces[0], c.aads[0], c.texts[0])


# ---- 5. record counts, lengths, placements, in place ------------------------------------------------------------------
@pytest.mark.parametrize("which", range(6), ids=["1", "4", "5", "64", "65", "second-pass"])
def test_record_counts_from_the_plan(which):
    F.check_count(MODE, COUNTS[which] if which < 5 else F.second_pass(MODE), second=which == 5)


@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_per_record_lengths(device, lens_on_device):
    F.check_lengths(MODE, F.lengths_case(MODE), device, lens_on_device)


@pytest.mark.parametrize("off", MODE.placement_offsets)
@pytest.mark.parametrize("mask", PLACES, ids=[F.place_id(MODE, p) for p in PLACES])
def test_placements(mask, off):
    """offsets 1 and 3 also put the nonces at odd addresses"""
    F.check_placement(MODE, F.placement_case(MODE, off), mask, off)


@pytest.mark.parametrize("ml", [9 * 16, 17 * 16 + 5], ids=["9 blocks", "17 blocks + 5"])
def test_in_place_with_more_blocks_than_a_chunk(ml):
    """row_walk requests a chunk of blocks ahead (four encrypting, eight on either walk decrypting)"""
    F.check_in_place(MODE, ml, ml, 24, nonces_at_off=True)


# ---- 6. the counter's carry and the cap -------------------------------------------------------------------------------
def test_the_counter_carries_into_byte_14():
    """a record of 4112 bytes = 257 blocks: the block counter passes 255 and 256 (J0 + 1 + i with i up to 256), so byte 15
    carries into byte 14"""
    F.check_both(MODE, records(random.Random(4112), 1, 3, 4112), "carry")


def test_the_cap():
    c = records(random.Random(65535), 1, 12, BATCH_MAX)
    F.check_both(MODE, c, "a record at the cap")
    nn, big = F.join(c.nonces), bytes(BATCH_MAX + 1)
    out, tag, ver = Mem(b"", size=BATCH_MAX + 1), Mem(b"", size=16), Mem(b"", size=1)
    for dec in (False, True):
        assert raw(dec, 256, KEY, 24, 16, 1, BATCH_MAX + 1, None, nn, None, 0, big, out.ptr, tag.ptr, ver.ptr) == E_ARG, dec
        assert raw(dec, 256, KEY, 24, 16, 1, 16, None, nn, big, BATCH_MAX + 1, big, out.ptr, tag.ptr, ver.ptr) == E_ARG, dec
    assert out.intact(0) and tag.intact(0)


# ---- 7. forgeries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["prefilled", "in-place"])
@pytest.mark.parametrize("part", MODE.forgery_parts)
def test_forgeries(part, in_place):
    """one flipped bit in record 5 among eight (its wave: records 4..7): verdict 0 and an untouched output slot for that
    one, 0x1A for the call, the other seven -- its three wave neighbours among them -- authentic and correct, and all of it
    the same whatever the wipe switch says"""
    F.check_forgery(MODE, F.forgery(MODE, part), in_place)


def test_a_forgery_without_verdicts():
    """verdicts may be NULL: the return code still tells, and the forged record's slot is still untouched"""
    n, ml = 5, 24
    c = records(random.Random(10), n, 3, ml)
    cts, tags = F.expected(MODE, c)
    nonces, aads = F.join(c.nonces), F.join(c.aads)
    src, out = Mem(F.join(cts), True), Mem(b"", True, size=n * ml)
    assert batch(True, c, nonces, aads, src, out, F.join(tags), None) == 0 and out.get() == F.join(c.texts)
    tags[3] = xaes_ref.flip(tags[3], 100)
    out = Mem(b"", True, size=n * ml)
    assert batch(True, c, nonces, aads, src, out, F.join(tags), None) == E_AUTH
    got = out.get()
    assert got[3 * ml:4 * ml] == bytes([FILL]) * ml and got[:3 * ml] + got[4 * ml:] == F.join(c.texts[:3] + c.texts[4:])


# ---- 8. cross-checks inside the product -------------------------------------------------------------------------------
def test_equals_the_one_message_calls_and_the_multikey_batch():
    shapes = ((24, 16, 0, 0), (24, 16, 20, 100), (24, 16, 12, 64), (24, 16, 300, 1000))
    for c, cts, tags in F.check_one_message_calls(MODE, 256, 256, shapes, 8, (0, 3, 7)):
        info = (len(c.aads[0]), len(c.texts[0]))
        kxs, halves = [uaes.xaes256gcm_derive(KEY, n) for n in c.nonces], [n[12:] for n in c.nonces]
        assert uaes.gcm_multikey_batch(kxs, halves, c.aads, c.texts) == (cts, tags), info
        assert uaes.gcm_multikey_batch(kxs, halves, c.aads, cts, decrypt=True, tags=tags) == (0, c.texts, [1] * 8), info


# ---- 9. threads and hygiene -------------------------------------------------------------------------------------------
def test_two_threads():
    """each thread runs the loop of the short shapes under a master key of its own on its own lane"""
    F.check_two_threads(MODE, {t: F.short_cases(MODE, 256, 24, 2000 + t, key=bytes([t]) * 32) for t in (1, 2)})


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_no_call_leaves_a_key_schedule_behind(device):
    n, ml = 5, 40
    c = records(random.Random(5), n, 3, ml)
    cts, tags = F.expected(MODE, c)
    nonces = c.nonces
    nn, aa = F.join(nonces), F.join(c.aads)
    dst, tg, ver = Mem(b"", device, size=n * ml), Mem(b"", device, size=n * 16), Mem(b"", device, size=n)
    src = Mem(F.join(c.texts), device)
    kw.checked("uaes_xaes256gcm_encrypt_batch", (KEY, n, ml, None, nn, aa, 3, src.ptr, dst.ptr, tg.ptr), kw.OK)
    assert dst.get() == F.join(cts) and tg.get() == F.join(tags)
    back = Mem(b"", device, size=n * ml)
    kw.checked("uaes_xaes256gcm_decrypt_batch", (KEY, n, ml, None, nn, aa, 3, dst.ptr, tg.ptr, back.ptr, ver.ptr), kw.OK)
    assert back.get() == F.join(c.texts)
    forged = Mem(xaes_ref.flip(F.join(tags), 300), device)
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
