"""The OCB batches on the GPU (k_ocb_batch, uaes_ocb.hip) against the CPU oracle's ocb_encrypt / ocb_decrypt, through the
frame of tests/aead_batch_cases.py: every short shape, record counts read from the plan, per-record lengths, placements,
forgeries of every part of a record, the one-message calls, two threads -- and, its own, all 64 values of `bottom`, the
offset chain over long records, the cap, the published vectors and a seeded fuzz.  Every failing case prints the tuple
that reproduces it."""
import random

import pytest

import micro_aes_amd as uaes
from tests import aead_batch_cases as F
from tests import rsp
from tests.guarded_mem import Mem

pytestmark = pytest.mark.gpu

OCB_BATCH_MAX = 65535                           # UAES_OCB_BATCH_MAX (csrc/uaes_plan.h)
AADS = (0, 1, 15, 16, 17, 32, 33)


def raw(decrypt, bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts):
    L = uaes.engine()
    if decrypt:
        return L.uaes_ocb_decrypt_batch(bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, tags, dst, verdicts)
    return L.uaes_ocb_encrypt_batch(bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags)


def one(decrypt, key, nonce, aad, data, tl):
    return (uaes.AES_OCB_decrypt if decrypt else uaes.AES_OCB_encrypt)(key, nonce, aad, data, tag_len=tl)


MODE = F.Mode(
    name="ocb",
    plan=lambda length, nmsg, decrypt: uaes.ocb_batch_plan(length, nmsg, decrypt=decrypt),
    arrangement="ocb.batch",
    wrapper=uaes.ocb_batch,
    raw=raw,
    key_bits=(128, 192, 256),
    fixed_keys={bits: bytes((bits // 8 + 7 * i) & 0xff for i in range(bits // 8)) for bits in (128, 192, 256)},
    nonce_lens=tuple(range(1, 16)),
    tag_lens=tuple(range(1, 17)),
    enc=lambda key, nonce, aad, pt, tl: F.oracle().ocb_encrypt(key, nonce, aad, pt, tag_len=tl),
    dec=lambda key, nonce, aad, ct, tl: F.oracle().ocb_decrypt(key, nonce, aad, ct, tag_len=tl),
    one=one,
    forged=("released", "zeros"),
    # 5 records per call: one of them lands in a second wave
    short_shapes=lambda bits: [(5, tl, al, ml, None) for ml in (range(50) if bits == 128 else (0, 15, 16, 17, 31, 32, 33, 49))
                               for al in AADS for tl in (1, 8, 16)],
    short_nls=(1, 12, 15),
    short_seed=lambda bits, nl: 1000 * bits + nl,
    count_shape=(12, 5, 16, 8),
    count_sampled=False,
    lengths_shape=(12, 8, 37),
    placement_shape=(13, 10),
    placement_offsets=(0, 1, 3),
    forgery_shape=(9, 12, 8, None),
    forgery_parts=("tag of 0", "text of 4", "AAD of 8", "nonce of 5"),
)
COUNTS = (1, 3, 4, 16, 17, 8192, 8193)


@pytest.mark.parametrize("nl", MODE.short_nls)
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(bits, nl):
    F.check_short_shapes(MODE, bits, nl)


@pytest.mark.parametrize("bits", [128, 256])
def test_every_value_of_bottom(bits):
    """the last nonce byte of record m is m: the stretch is shifted by every bit count, word boundaries included"""
    c = F.draw(MODE, random.Random(64 + bits), bits, 64, 12, 7, 33)
    F.check_both(MODE, c._replace(nonces=[nc[:11] + bytes([m]) for m, nc in enumerate(c.nonces)]), ("bottom", bits))


@pytest.mark.parametrize("which", range(8), ids=["1", "3", "4", "16", "17", "8192", "8193", "second-pass"])
def test_record_counts_from_the_plan(which):
    F.check_count(MODE, COUNTS[which] if which < 7 else F.second_pass(MODE), second=which == 7)


@pytest.mark.parametrize("ml", [341, 529, 2069])
def test_offset_chain_and_walk_depth(ml):
    """341: 21 blocks + 5 bytes (row_walk looks 16 blocks ahead, an odd count); 529: 33 blocks + 1 byte; 2069: crosses
    block 128 (ntz 7).  In place and out of place, device memory, offsets 0 and 2, both directions."""
    c = F.draw(MODE, random.Random(ml), 256, 6, 12, 21, ml)
    n, tl = 6, 16
    text, (wct, wtag) = F.join(c.texts), map(F.join, F.expected(MODE, c))
    mn, ma = Mem(F.join(c.nonces), True), Mem(F.join(c.aads), True)
    for off in (0, 2):
        info = (ml, off)
        # out of place
        src, dst = Mem(text, True, off), Mem(size=n * ml, device=True, off=off)
        tags, ver = Mem(size=n * tl, device=True), Mem(size=n, device=True)
        assert F.run(MODE, c, False, c.key, None, mn, ma, src, dst, tags) == 0, info
        assert dst.get() == wct and tags.get() == wtag and dst.intact(n * ml) and src.get() == text, info
        back = Mem(size=n * ml, device=True, off=off)
        assert F.run(MODE, c, True, c.key, None, mn, ma, dst, back, tags, ver) == 0, info
        assert back.get() == text and ver.get() == F.ones(n) and back.intact(n * ml), info
        # in place
        io, tags2, ver2 = Mem(text, True, off), Mem(size=n * tl, device=True), Mem(size=n, device=True)
        assert F.run(MODE, c, False, c.key, None, mn, ma, io, io, tags2) == 0, info
        assert io.get() == wct and tags2.get() == wtag and io.intact(n * ml), info
        assert F.run(MODE, c, True, c.key, None, mn, ma, io, io, tags2, ver2) == 0, info
        assert io.get() == text and ver2.get() == F.ones(n) and io.intact(n * ml), info


@pytest.mark.parametrize("bits", [128, 256])
def test_the_cap(bits):
    """3 records of 65535 bytes with 65535 bytes of AAD: 4095 blocks and a 15-byte tail, ntz up to 11"""
    c = F.draw(MODE, random.Random(OCB_BATCH_MAX + bits), bits, 3, 12, OCB_BATCH_MAX, OCB_BATCH_MAX)
    F.check_both(MODE, c, ("cap", bits))


@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_variable_lengths(device, lens_on_device):
    F.check_lengths(MODE, F.lengths_case(MODE), device, lens_on_device)


@pytest.mark.parametrize("off", MODE.placement_offsets)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_placement(device, off):
    """all arrays together, on the host or in device memory"""
    F.check_placement(MODE, F.placement_case(MODE, off), F.places(MODE)[1 if device else 0], off)


@pytest.mark.parametrize("part", MODE.forgery_parts)
def test_forgeries(part):
    F.check_forgery(MODE, F.forgery(MODE, part))


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_equals_the_one_message_calls(bits):
    shapes = ((1, 1, 0, 0), (12, 16, 20, 100), (15, 8, 13, 64), (12, 10, 300, 1000), (8, 6, 16, 257))
    F.check_one_message_calls(MODE, bits, bits, shapes, 7)


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


@pytest.mark.parametrize("seed", range(40))
def test_fuzz(seed):
    rng = random.Random(7000 + seed)
    bits = rng.choice((128, 192, 256))
    key = rng.randbytes(bits // 8)
    nl, tl, al, ml, n = rng.randrange(1, 16), rng.randrange(1, 17), rng.randrange(71), rng.randrange(201), rng.randrange(1, 301)
    lens = [rng.randrange(ml + 1) for _ in range(n)] if rng.randrange(2) else None
    c = F.draw(MODE, rng, bits, n, nl, al, ml, tl, lens, key)
    F.check_both(MODE, c, ("fuzz", seed, bits, nl, tl, al, ml, n, lens is not None))


def test_two_threads_with_different_keys():
    F.check_two_threads(MODE, F.keyed_thread_jobs(MODE, 12), repeats=3)
