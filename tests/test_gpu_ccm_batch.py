"""The CCM batches on the GPU (k_ccm_batch, uaes_mac.hip) against the CPU oracle's ccm_encrypt / ccm_decrypt, through the
frame of tests/aead_batch_cases.py: every short shape, record counts read from the plan, per-record lengths, placements,
forgeries of every part of a record, the one-message calls, two threads -- and, its own, the published vectors.  Every
failing case prints the tuple that reproduces it."""
import pytest

import micro_aes_amd as uaes
from tests import aead_batch_cases as F
from tests import rsp

pytestmark = pytest.mark.gpu

AADS = (0, 1, 13, 14, 15, 30, 31)       # 14 exactly fills the header block, 15 spills one byte, 30 ends on a block


def raw(decrypt, bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts):
    L = uaes.engine()
    if decrypt:
        return L.uaes_ccm_decrypt_batch(bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, tags, dst, verdicts)
    return L.uaes_ccm_encrypt_batch(bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags)


def one(decrypt, key, nonce, aad, data, tl):
    return (uaes.AES_CCM_decrypt if decrypt else uaes.AES_CCM_encrypt)(key, nonce, aad, data, tag_len=tl)


MODE = F.Mode(
    name="ccm",
    plan=lambda length, nmsg, decrypt: uaes.chain_plan("ccm_batch", length, nmsg, decrypt),
    arrangement="ccm.batch",
    wrapper=uaes.ccm_batch,
    raw=raw,
    key_bits=(128, 192, 256),
    fixed_keys={bits: bytes((bits // 8 + 7 * i) & 0xff for i in range(bits // 8)) for bits in (128, 192, 256)},
    nonce_lens=tuple(range(7, 14)),
    tag_lens=(4, 6, 8, 10, 12, 14, 16),
    enc=lambda key, nonce, aad, pt, tl: F.oracle().ccm_encrypt(key, nonce, aad, pt, tag_len=tl),
    dec=lambda key, nonce, aad, ct, tl: F.oracle().ccm_decrypt(key, nonce, aad, ct, tag_len=tl),
    one=one,
    forged=("released", "zeros"),
    # 5 records per call: one of them lands in a second wave
    short_shapes=lambda bits: [(5, tl, al, ml, None) for ml in (range(50) if bits == 128 else (0, 15, 16, 17, 49))
                               for al in AADS for tl in (4, 8, 16)],
    short_nls=(7, 11, 13),
    short_seed=lambda bits, nl: 1000 * bits + nl,
    count_shape=(13, 5, 16, 8),
    count_sampled=False,
    lengths_shape=(12, 8, 37),
    placement_shape=(13, 10),
    placement_offsets=(0, 1, 3),
    forgery_shape=(9, 13, 8, None),
    forgery_parts=("tag of 0", "text of 4", "AAD of 8", "nonce of 5"),
)
COUNTS = (1, 3, 4, 16, 17, 8192, 8193)


@pytest.mark.parametrize("nl", MODE.short_nls)
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_shape(bits, nl):
    F.check_short_shapes(MODE, bits, nl)


@pytest.mark.parametrize("which", range(8), ids=["1", "3", "4", "16", "17", "8192", "8193", "second-pass"])
def test_record_counts_from_the_plan(which):
    F.check_count(MODE, COUNTS[which] if which < 7 else F.second_pass(MODE), second=which == 7)


@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_variable_lengths(device, lens_on_device):
    F.check_lengths(MODE, F.lengths_case(MODE), device, lens_on_device)


@pytest.mark.parametrize("off", MODE.placement_offsets)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_placement(device, off):
    """all arrays together, on the host or in device memory"""
    F.check_placement(MODE, F.placement_case(MODE, off), F.places(MODE)[1 if device else 0], off)


def test_in_place_with_more_blocks_than_a_chunk():
    """row_walk requests sixteen blocks ahead: records of 21 blocks + 5 bytes"""
    F.check_in_place(MODE, 341, 341, 7)


@pytest.mark.parametrize("part", MODE.forgery_parts)
def test_forgeries(part):
    F.check_forgery(MODE, F.forgery(MODE, part))


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_equals_the_one_message_calls(bits):
    shapes = ((7, 4, 0, 0), (11, 16, 20, 100), (13, 8, 13, 64), (12, 10, 300, 1000), (8, 6, 14, 257))
    F.check_one_message_calls(MODE, bits, bits, shapes, 7)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_published_vectors(bits):
    """every [Nlen = n] section of VNT<bits>.rsp: one key, ten records, one batch"""
    total = 0
    for nl in range(7, 14):
        cases = rsp.ccm_cases(bits, nl)
        assert len(cases) == 10 and len({c["Key"] for c in cases}) == 1, (bits, nl, len(cases))
        key = cases[0]["Key"]
        nonces, aads, texts = [c["Nonce"] for c in cases], [c["Adata"] for c in cases], [c["Payload"] for c in cases]
        cts, tags = uaes.ccm_batch(key, nonces, aads, texts, tag_len=16)
        assert [a + b for a, b in zip(cts, tags)] == [c["CT"] for c in cases], (bits, nl)
        assert uaes.ccm_batch(key, nonces, aads, cts, tag_len=16, decrypt=True, tags=tags) == (0, texts, [1] * 10), (bits, nl)
        total += len(cases)
    assert total == 70


def test_two_threads_with_different_keys():
    F.check_two_threads(MODE, F.keyed_thread_jobs(MODE, 13), repeats=3)
