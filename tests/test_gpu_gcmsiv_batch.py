"""The GCM-SIV batches on the GPU (k_gcmsiv_batch, uaes_gcmsiv_batch.hip) against the CPU oracle's gcmsiv_encrypt /
gcmsiv_decrypt, one oracle call per record, bit for bit, through the frame of tests/aead_batch_cases.py: every short
shape, record counts read from the plan, per-record lengths, placements, forgeries of every part of a record, the
one-message calls, two threads -- and, its own, repeated nonces, the counter's 32-bit wrap, the published vectors and the
cap.  Every failing case prints the tuple that reproduces it."""
import random

import pytest

import micro_aes_amd as uaes
from tests import aead_batch_cases as F
from tests import rsp

pytestmark = pytest.mark.gpu

E_AUTH = 0x1A                                   # UAES_E_AUTHENTICATION
BATCH_MAX = 65535                               # UAES_GCMSIV_BATCH_MAX
AADS = (0, 1, 15, 16, 17, 32)


def raw(decrypt, bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts):
    L = uaes.engine()
    if decrypt:
        return L.uaes_gcmsiv_decrypt_batch(bits, key, nmsg, ml, lens, nonces, aads, al, src, tags, dst, verdicts)
    return L.uaes_gcmsiv_encrypt_batch(bits, key, nmsg, ml, lens, nonces, aads, al, src, dst, tags)


def one(decrypt, key, nonce, aad, data, tl):
    return (uaes.GCM_SIV_decrypt if decrypt else uaes.GCM_SIV_encrypt)(key, nonce, aad, data)


MODE = F.Mode(
    name="gcmsiv",
    plan=lambda length, nmsg, decrypt: uaes.gcmsiv_batch_plan(length, nmsg, decrypt=decrypt),
    arrangement="gcmsiv.batch",
    wrapper=uaes.gcmsiv_batch,
    raw=raw,
    key_bits=(128, 192, 256),
    fixed_keys={bits: bytes((bits // 8 + 11 * i) & 0xff for i in range(bits // 8)) for bits in (128, 192, 256)},
    nonce_lens=(12,),
    tag_lens=None,
    enc=lambda key, nonce, aad, pt, tl: F.oracle().gcmsiv_encrypt(key, nonce, aad, pt),
    dec=lambda key, nonce, aad, ct, tl: F.oracle().gcmsiv_decrypt(key, nonce, aad, ct),
    one=one,
    forged=("released", "zeros"),
    # 5 records per call: one of them lands in a second wave
    short_shapes=lambda bits: [(5, 16, al, ml, None) for ml in (range(50) if bits == 128 else (0, 15, 16, 17, 49)) for al in AADS],
    short_nls=(12,),
    short_seed=lambda bits, nl: 1000 + bits,
    count_shape=(12, 5, 16, 16),
    count_sampled=True,
    lengths_shape=(12, 16, None),
    placement_shape=(12, 16),
    placement_offsets=(0, 1, 7),
    forgery_shape=(9, 12, 16, [40, 33, 17, 40, 25, 16, 40, 1, 39]),
    forgery_parts=("tag of 0", "text of 4", "AAD of 8", "nonce of 5"),
)
COUNTS = (1, 4, 5, 64, 65)
PLACES = F.places(MODE)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(bits):
    F.check_short_shapes(MODE, bits, 12)


@pytest.mark.parametrize("which", range(6), ids=["1", "4", "5", "64", "65", "second-pass"])
def test_record_counts_from_the_plan(which):
    F.check_count(MODE, COUNTS[which] if which < 5 else F.second_pass(MODE), second=which == 5)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_repeated_and_distinct_nonces(bits):
    """records 0, 2, 5 and 7 are the same record (rows of two waves); 1 and 6 differ from it only in the nonce: a record
    key or a POLYVAL key that leaks from one row to its neighbour shows here"""
    rng = random.Random(bits + 3)
    key = MODE.fixed_keys[bits]
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
    F.check_both(MODE, F.Case(bits, key, nonces, aads, texts), ("nonces", bits))


@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_per_record_lengths(device, lens_on_device):
    F.check_lengths(MODE, F.lengths_case(MODE), device, lens_on_device)


@pytest.mark.parametrize("off", MODE.placement_offsets)
@pytest.mark.parametrize("mask", PLACES, ids=[F.place_id(MODE, p) for p in PLACES])
def test_placements(mask, off):
    F.check_placement(MODE, F.placement_case(MODE, off), mask, off)


def test_in_place_with_more_blocks_than_a_chunk():
    """row_walk requests a chunk of blocks ahead (eight encrypting, four decrypting): records of 21 blocks + 5 bytes"""
    F.check_in_place(MODE, 341, 341, 12)


@pytest.mark.parametrize("part", MODE.forgery_parts)
def test_forgeries(part):
    F.check_forgery(MODE, F.forgery(MODE, part))


@pytest.mark.parametrize("bits", [128, 256])
def test_the_counter_wraps_inside_its_word(orc, bits):
    """received tags that start with LE32 0xFFFFFFFE / 0xFFFFFFFF: the keystream of a 5-block record runs through the wrap,
    which must stay inside bytes 0..3.  The tags are made up, so every verdict is 0 and the released text is the oracle's"""
    rng = random.Random(bits + 7)
    heads = [0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFD, 0xFFFFFFFC, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE]
    n = len(heads)
    c = F.draw(MODE, rng, bits, n, 12, 5, 80)
    key, nonces, aads, cts = c.key, c.nonces, c.aads, c.texts
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


def test_the_cap():
    rng = random.Random(65535)
    F.check_both(MODE, F.draw(MODE, rng, 256, 3, 12, 3, BATCH_MAX, lens=[BATCH_MAX, 4097, 0]), "text at the cap")
    # 65 535 bytes of AAD, 16-byte texts
    F.check_both(MODE, F.draw(MODE, rng, 256, 3, 12, BATCH_MAX, 16), "AAD at the cap")


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_equals_the_one_message_calls(bits):
    F.check_one_message_calls(MODE, bits, bits, ((12, 16, 0, 0), (12, 16, 20, 100), (12, 16, 12, 64), (12, 16, 300, 1000)), 8)


def test_two_threads():
    """each thread runs the loop of the short shapes for one key size on its own lane"""
    F.check_two_threads(MODE, {bits: F.short_cases(MODE, bits, 12, 2000 + bits) for bits in (192, 256)})
