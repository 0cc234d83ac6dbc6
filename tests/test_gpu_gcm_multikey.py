"""The multi-key GCM batches on the GPU (k_gcm_multikey, uaes_gcm_multikey.hip) against the CPU oracle's gcm_encrypt, one
oracle call per record under that record's key, bit for bit, through the frame of tests/aead_batch_cases.py: every short
shape, record counts read from the plan, per-record lengths, placements (the keys in device memory included), forgeries
of every part of a record (its key included), the one-message calls, two threads -- and, its own, key isolation, tag
lengths, the counter's carry and the cap, and the NIST vectors as batches.  Every failing case prints the tuple that
reproduces it."""
import ctypes as C
import os
import random

import pytest

import micro_aes_amd as uaes
from tests import aead_batch_cases as F
from tests.guarded_mem import Mem
from tests.rsp import GOLDEN

pytestmark = pytest.mark.gpu

E_ARG = -2                                      # UAES_E_ARG
E_AUTH = 0x1A                                   # UAES_E_AUTHENTICATION
BATCH_MAX = 65535                               # UAES_GCM_MULTIKEY_BATCH_MAX
AADS = (0, 1, 15, 16, 17, 32)


def raw(decrypt, bits, keys, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts):
    L = uaes.engine()
    if decrypt:
        return L.uaes_gcm_multikey_decrypt_batch(bits, keys, tl, nmsg, ml, lens, nonces, aads, al, src, tags, dst, verdicts)
    return L.uaes_gcm_multikey_encrypt_batch(bits, keys, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags)


def one(decrypt, key, nonce, aad, data, tl):
    """uaes_gcm_encrypt_ex / uaes_gcm_decrypt_ex: ciphertext || tag, or (code, text)"""
    L = uaes.engine()
    n = len(data) - (tl if decrypt else 0)
    out = (C.c_uint8 * max(n + 16, 1))()
    f = L.uaes_gcm_decrypt_ex if decrypt else L.uaes_gcm_encrypt_ex
    rc = f(len(key) * 8, key, nonce, 12, tl, aad, len(aad), data, n, out)
    return (rc, bytes(out)[:n]) if decrypt else (bytes(out)[:n + tl] if rc == 0 else rc)


MODE = F.Mode(
    name="gcm_multikey",
    plan=lambda length, nmsg, decrypt: uaes.gcm_multikey_batch_plan(length, nmsg, decrypt=decrypt),
    arrangement="gcm.multikey",
    wrapper=uaes.gcm_multikey_batch,
    raw=raw,
    key_bits=(128, 192, 256),
    fixed_keys={},                              # every record has a random key of its own
    nonce_lens=(12,),
    tag_lens=tuple(range(1, 17)),
    enc=lambda key, nonce, aad, pt, tl: F.oracle().gcm_encrypt(key, nonce, aad, pt, tl),
    dec=lambda key, nonce, aad, ct, tl: F.oracle().gcm_decrypt(key, nonce, aad, ct, tag_len=tl),
    one=one,
    forged=("untouched", "untouched"),
    # 5 records per call: one of them lands in a second wave
    short_shapes=lambda bits: [(5, 16, al, ml, None) for ml in (range(50) if bits == 128 else (0, 15, 16, 17, 49)) for al in AADS],
    short_nls=(12,),
    short_seed=lambda bits, nl: 1000 + bits,
    count_shape=(12, 5, 16, 16),
    count_sampled=True,
    lengths_shape=(12, 16, None),
    placement_shape=(12, 16),
    placement_offsets=(0, 1, 3),
    forgery_shape=(8, 12, 16, None),
    forgery_parts=("text of 4", "tag of 0", "AAD of 7", "nonce of 5", "key of 3"),
)
COUNTS = (1, 4, 5, 64, 65)
PLACES = F.places(MODE)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(bits):
    F.check_short_shapes(MODE, bits, 12)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_key_isolation(bits):
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
    F.check_both(MODE, F.Case(bits, keys, nonces, aads, texts), ("isolation", bits))


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
    """"keys" alone: the keys on the device and the texts on the host; all but "keys": the reverse.  Offsets 1 and 3 also
    take the byte-wise path of the key load"""
    F.check_placement(MODE, F.placement_case(MODE, off), mask, off)


def test_in_place_with_more_blocks_than_a_chunk():
    """row_walk requests a chunk of blocks ahead (four encrypting, eight on either walk decrypting): records of 21 blocks
    + 5 bytes"""
    F.check_in_place(MODE, 341, 341, 12)


@pytest.mark.parametrize("tl", [1, 4, 8, 12, 13, 16])
def test_tag_lengths(tl):
    """tags are packed at m * tagLen, and the byte after the last tag is not written"""
    c = F.draw(MODE, random.Random(tl), 128, 7, 12, 11, 37, tl)
    n, ml = 7, 37
    want = F.expected(MODE, c)
    assert all(len(t) == tl for t in want[1])
    keys, nonces, aads = F.join(c.key), F.join(c.nonces), F.join(c.aads)
    for device in (False, True):
        src, dst, tags = Mem(F.join(c.texts), device), Mem(size=n * ml, device=device), Mem(size=n * tl, device=device, off=1)
        assert F.run(MODE, c, False, keys, None, nonces, aads, src, dst, tags) == 0
        assert dst.get() == F.join(want[0]) and tags.get() == F.join(want[1]) and tags.intact(n * tl), (tl, device)
        back, ver = Mem(size=n * ml, device=device), Mem(size=n, device=device)
        assert F.run(MODE, c, True, keys, None, nonces, aads, dst, back, tags, ver) == 0
        assert back.get() == F.join(c.texts) and ver.get() == F.ones(n), (tl, device)
    F.check_against(MODE, want, c, ("tag length", tl))


@pytest.mark.parametrize("in_place", [False, True], ids=["prefilled", "in-place"])
@pytest.mark.parametrize("part", MODE.forgery_parts)
def test_forgeries(part, in_place):
    """one flipped bit in one record among eight: verdict 0 and an untouched output slot for that one, 0x1A for the call,
    and the other seven authentic and correct"""
    F.check_forgery(MODE, F.forgery(MODE, part), in_place)


def test_a_forged_record_is_untouched_whatever_the_wipe_switch_says():
    c = F.draw(MODE, random.Random(77), 256, 8, 12, 13, 40)
    F.check_forgery(MODE, F.forged(MODE, c, "tag", 2, lambda t: F.flip(t, 5)))


def test_every_byte_of_a_short_tag_is_compared():
    """tagLen 4 in the packed layout: the four bytes of record m are bytes 4 m .. 4 m + 3 of the array and nothing lies
    between two tags, so a flip in byte 3 of record 1's tag (the last one compared) must be caught, in that record only"""
    n, ml, tl = 8, 24, 4
    c = F.draw(MODE, random.Random(4), 192, n, 12, 5, ml, tl)
    cts, tags = F.expected(MODE, c)
    packed = bytearray(F.join(tags))
    assert len(packed) == n * tl
    for byte in range(tl):
        forged = bytearray(packed)
        forged[1 * tl + byte] ^= 0x80
        split = [bytes(forged[k * tl:(k + 1) * tl]) for k in range(n)]
        rc, pts, verdicts = uaes.gcm_multikey_batch(c.key, c.nonces, c.aads, cts, decrypt=True, tags=split, tag_len=tl, prefill=0x11)
        assert rc == E_AUTH and verdicts == [1, 0] + [1] * 6, (byte, rc, verdicts)
        assert pts[1] == bytes([0x11]) * ml and pts[0] == c.texts[0] and pts[2:] == c.texts[2:], byte


def test_the_counter_carries_into_byte_14():
    """three records of 4112 bytes = 257 blocks: the block counter passes 255 and 256 (J0 + 1 + i with i up to 256), so
    byte 15 carries into byte 14"""
    F.check_both(MODE, F.draw(MODE, random.Random(4112), 128, 3, 12, 3, 4112), "carry")


def test_the_cap():
    c = F.draw(MODE, random.Random(65535), 256, 1, 12, BATCH_MAX, BATCH_MAX)
    F.check_both(MODE, c, "text and AAD at the cap")
    k, nn = F.join(c.key), F.join(c.nonces)
    big = bytes(BATCH_MAX + 1)
    out, tag, ver = Mem(size=BATCH_MAX + 1), Mem(size=16), Mem(size=1)
    for dec in (False, True):
        assert raw(dec, 256, k, 12, 16, 1, BATCH_MAX + 1, None, nn, None, 0, big, out.ptr, tag.ptr, ver.ptr) == E_ARG, dec
        assert raw(dec, 256, k, 12, 16, 1, 16, None, nn, big, BATCH_MAX + 1, big, out.ptr, tag.ptr, ver.ptr) == E_ARG, dec
    assert out.intact(0) and tag.intact(0)


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


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_equals_the_one_message_calls(bits):
    F.check_one_message_calls(MODE, bits, bits, ((12, 16, 0, 0), (12, 16, 20, 100), (12, 12, 12, 64), (12, 8, 300, 1000)), 8, (0, 3, 7))


def test_two_threads():
    """each thread runs the loop of the short shapes for one key size on its own lane, with keys of its own"""
    F.check_two_threads(MODE, {bits: F.short_cases(MODE, bits, 12, 2000 + bits) for bits in (192, 256)})
