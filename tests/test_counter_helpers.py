"""The counter-solving helpers (tests/counters.py) and the counter-aware plan, without a GPU.

The solvers must reach what they promise against the C oracle -- and, where a matching build travelled, against the
compiled reference -- at every key size: a nonce whose J0 is a chosen counter (GCM), a plaintext whose tag starts a
chosen 32-bit counter word (GCM-SIV).  The library's host data path runs at every named J0 target and at a GCM-SIV
wrap.  uaes.plan(..., counter=...) answers for a 256-CU device here: the striped boundaries of CTR and GCM move with the
first counter's low byte c0 exactly as the formula of gcm_stripes / plan_ctr says, and a text in which counter bits
40..47 move falls out of the striped arrangements.
"""
import random

import pytest

import micro_aes_amd as uaes
from oracle.pyoracle import Reference
from tests import counters as K
from tests.test_gpu_plan import boundaries

MIB = 1 << 20
NONCE_LENS = (16, 17, 32, 60, 4096, 70000)


def _j0(name, v, b8, rnd):
    return K.j0_bytes(rnd.randbytes(8) + bytes([b8]), v)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_gcm_nonce_solver_reaches_every_target(orc, bits):
    """for every named target and nonce length: GHASH(nonce) = J0, and the oracle's GCM under that nonce equals GCM by
    its definition at J0 (gcm_expect) -- the 56-bit counter wraps with byte 8 kept, a carry crosses byte 11"""
    rnd = random.Random(bits)
    key = rnd.randbytes(bits // 8)
    nfull, rem = 300, 5
    pt, aad = orc.splitmix(bits, 16 * nfull + rem), rnd.randbytes(19)
    for k, (name, v, b8) in enumerate(K.gcm_targets(nfull, rem)):
        j0 = _j0(name, v, b8, rnd)
        nlen = NONCE_LENS[k % len(NONCE_LENS)]
        nonce = K.gcm_nonce_for_j0(orc, key, j0, nlen, seed=k)
        assert len(nonce) == nlen
        want = K.gcm_expect(orc, key, j0, aad, pt)
        assert orc.gcm_encrypt(key, nonce, aad, pt) == want, (bits, nlen, j0.hex(), name)
        assert orc.gcm_decrypt(key, nonce, aad, want) == (0, pt), (bits, nlen, j0.hex(), name)
    # the wrap keeps byte 8: the block after 2^56 - 1 is bytes 0..8 || 00..00
    j0 = K.j0_bytes(bytes(8) + b"\xff", K.v_wrap56_at(3))
    ks = orc.ctr_xcrypt_at(key, j0, 1, bytes(16 * 5))
    assert ks[48:64] == orc.encrypt_block(key, bytes(8) + b"\xff" + bytes(7))
    # one target, solved in another block of the nonce
    nonce = K.gcm_nonce_for_j0(orc, key, j0, 60, solve_at=0)
    assert orc.ghash(K.gcm_h(orc, key), b"", nonce) == j0


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_siv_solver_reaches_every_wrap(orc, bits):
    """the tag's low word is what was asked for (oracle), for both fills, with and without AAD and a byte tail"""
    rnd = random.Random(10 + bits)
    key, nonce = rnd.randbytes(bits // 8), rnd.randbytes(12)
    for nblocks, tail, aad, start in ((1, 0, b"", 0xffffffff), (2, 9, b"x" * 17, 0xffffffff), (40, 3, b"", 0xffffffe0),
                                      (1000, 15, rnd.randbytes(33), (1 << 32) - 500), (4096, 0, b"", 5)):
        for fill in ("zero", "random"):
            pt = K.siv_message_for_counter(orc, key, nonce, aad, nblocks, start, tail=tail, fill=fill)
            assert len(pt) == 16 * nblocks + tail
            K.siv_counter_check(orc, key, nonce, aad, pt, start)
            pt = K.siv_message_for_counter(orc, key, nonce, aad, nblocks, start, solve_at=0, tail=tail, fill=fill)
            K.siv_counter_check(orc, key, nonce, aad, pt, start)


def test_solvers_against_the_compiled_reference(orc):
    """one J0 (a 128-byte nonce: the GCM_NONCE_LEN = 128 build) and one GCM-SIV wrap per key size, against the
    reference itself where such a build exists"""
    from tests import refbuilt
    rnd = random.Random(77)
    ran = 0
    if Reference.available(256, gcm_nonce_len=128):
        key = rnd.randbytes(32)
        j0 = K.j0_bytes(rnd.randbytes(8) + b"\xff", K.v_wrap56_at(7))
        nonce = K.gcm_nonce_for_j0(orc, key, j0, 128)
        pt, aad = rnd.randbytes(200), rnd.randbytes(5)
        assert Reference(256, gcm_nonce_len=128).gcm_encrypt(key, nonce, aad, pt) == K.gcm_expect(orc, key, j0, aad, pt)
        ran += 1
    for bits in (128, 192, 256):
        if not Reference.available(bits):
            continue
        key, nonce = rnd.randbytes(bits // 8), rnd.randbytes(12)
        pt = K.siv_message_for_counter(orc, key, nonce, b"hdr", 9, 0xfffffffb, tail=4)
        ct = Reference(bits).gcmsiv_encrypt(key, nonce, b"hdr", pt)
        assert ct == orc.gcmsiv_encrypt(key, nonce, b"hdr", pt) and ct[-16:-12] == bytes([0xfb, 0xff, 0xff, 0xff]), bits
        ran += 1
    if not ran:
        refbuilt.missing("oracle/_ref/libmicroaes_ref_*.so")


def test_host_path_at_every_target(orc):
    """the library's host data path (csrc/uaes_host.c) at every J0 target and at GCM-SIV wraps, against the oracle"""
    rnd = random.Random(88)
    prev = uaes.host_policy(1 << 62, 0, 0)
    try:
        for bits in (128, 192, 256):
            key = rnd.randbytes(bits // 8)
            nfull, rem = 700, 11
            pt, aad = orc.splitmix(bits + 1, 16 * nfull + rem), rnd.randbytes(7)
            for k, (name, v, b8) in enumerate(K.gcm_targets(nfull, rem)):
                j0 = _j0(name, v, b8, rnd)
                nlen = (16, 60)[k % 2]
                nonce = K.gcm_nonce_for_j0(orc, key, j0, nlen)
                want = K.gcm_expect(orc, key, j0, aad, pt)
                what = (bits, nlen, j0.hex(), len(pt), "host", name)
                assert uaes.AES_GCM_encrypt(key, nonce, aad, pt) == want, what
                assert uaes.AES_GCM_decrypt(key, nonce, aad, want) == (0, pt), what
                assert uaes.AES_GCM_decrypt(key, nonce, aad, want[:-4], tag_len=12) == (0, pt), what
            nonce = rnd.randbytes(12)
            for wrap_at in (1, 2, 350, 700):
                sp = K.siv_message_for_counter(orc, key, nonce, aad, nfull, -wrap_at, tail=rem)
                want = orc.gcmsiv_encrypt(key, nonce, aad, sp)
                assert uaes.GCM_SIV_encrypt(key, nonce, aad, sp) == want, (bits, wrap_at)
                assert uaes.GCM_SIV_decrypt(key, nonce, aad, want) == (0, sp), (bits, wrap_at)
    finally:
        uaes.host_policy(*prev)


def _ctr0(c):
    """a CTR counter block whose 56-bit counter (bytes 9..15) is c"""
    return bytes(range(0xA0, 0xA9)) + c.to_bytes(7, "big")


def test_plan_follows_the_first_counter():
    """the smallest striped text is 256 * (2048 + g_lo) - c0 whole blocks (n8 = ((c0 + nfull) / 256 - g_lo) / 8
    stripes >= 256 workgroups) -- CTR with its first counter, GCM with J0 + 1 -- for c0 = 0, 1, 2, 0xff"""
    L = uaes.engine()
    ids = {n: uaes.arrangement_id(n) for n in ("gcm.chunks", "gcm.twophase")}
    try:
        L.uaes_debug_plan_disable((1 << ids["gcm.chunks"]) | (1 << ids["gcm.twophase"]))
        for c0 in (0, 1, 2, 0xff):
            want = 16 * (256 * (2048 + (1 if c0 else 0)) - c0)
            ctr = boundaries(lambda n: uaes.plan("ctr", n, counter=_ctr0(0x1234500 + c0))[0], 4 * MIB, 12 * MIB)
            assert [b for b, _below, above in ctr if above.endswith(".striped")] == [want], (c0, ctr)
            j0 = K.j0_bytes(bytes(9), K.v_for_first(0x777700 + c0))
            for direction in (0, 2):
                gcm = boundaries(lambda n: uaes.plan("gcm", n, 0, direction, counter=j0)[0], 4 * MIB, 12 * MIB)
                assert [b for b, _below, above in gcm if above.endswith(".striped")] == [want], (c0, direction, gcm)
                assert gcm[-1][2] == "gcm.striped", (c0, direction, gcm)
    finally:
        L.uaes_debug_plan_disable(0)
    # a 12-byte IV / nonce: c0 = 1 (CTR_START_VALUE) and 2 (J0 + 1), the default answers
    assert uaes.plan("ctr", 9 * MIB, counter=_ctr0(1)) == uaes.plan("ctr", 9 * MIB)


def test_a_counter_whose_bits_40_47_move_is_not_striped():
    n = 200 * MIB
    assert uaes.plan("gcm", n)[0] == "gcm.striped" and uaes.plan("ctr", n)[:2] == ("ctr.striped", 1)
    for at in (n // 64, n // 64 + 1, n // 32 + 255):            # inside the stripes (not at their first group)
        j0 = K.j0_bytes(bytes(9), K.v_bits40_at(at))
        assert uaes.plan("gcm", n, 0, 0, counter=j0)[0] != "gcm.striped", at
        assert uaes.plan("gcm", n, 0, 2, counter=j0)[0] != "gcm.striped", at
        assert uaes.plan("ctr", n, counter=_ctr0(K.v_bits40_at(at) + 1))[:2] == ("ctr.striped", 2), at
    j0 = K.j0_bytes(bytes(8) + b"\xff", K.v_wrap56_at(n // 64))
    assert uaes.plan("gcm", n, 0, 0, counter=j0)[0] != "gcm.striped"
    # a carry into byte 11 inside the text does not move bits 40..47: still striped
    j0 = K.j0_bytes(bytes(9), K.v_carry32_at(n // 64))
    assert uaes.plan("gcm", n, 0, 0, counter=j0) == uaes.plan("gcm", n)


def test_the_default_counter_gives_the_default_plan():
    """counter = the one a 12-byte IV / nonce gives (CTR: start value 1; GCM: J0 = nonce || 00000001) answers byte for
    byte as counter=None, at every sample size of every direction: the counter-aware planners reduce to the plain ones"""
    from tests.test_gpu_plan import sample_points
    j0 = bytes(range(12)) + b"\0\0\0\1"
    for n in sample_points(0, 1 << 30, 16) + [n + 16 for n in sample_points(16, 1 << 30, 16)]:
        for direction in (0, 1, 2, 3):
            for alen in (0, 37):
                assert uaes.plan("gcm", n, alen, direction, counter=j0) == uaes.plan("gcm", n, alen, direction), (n, direction)
        assert uaes.plan("ctr", n, counter=_ctr0(1)) == uaes.plan("ctr", n), n
        for flags in (0, 4):
            assert uaes.plan("siv", n, 9, 0, flags, counter=j0) == uaes.plan("siv", n, 9, 0, flags)
