"""tests/ocb_ref.py proved before anything leans on it, and OCB's launch shape pinned without a device.

The reference in pieces is what tests/test_gpu_ocb.py holds k_ocb against at the sizes the oracle cannot reach, so it
is checked here against all three things that define it: the OpenSSL / RFC 7253 vectors, the oracle's own OCB, and the
RFC's chained offsets (the pieces compute them from the Gray code instead).  The shape table is the launcher's rule
(csrc/uaes_ocb.hip, ocb_shape) evaluated by hand for 256 CUs -- what every planner assumes when there is no device."""
import random

import numpy as np

import micro_aes_amd as uaes
from tests import ocb_ref as R
from tests.rsp import ocb_cases

MIB = 1 << 20


def test_the_vectors(orc):
    total = 0
    for nlen, tlen, count in ((12, 16, 16), (12, 12, 6), (15, 16, 1)):
        cases = ocb_cases(128, nlen, tlen)
        assert len(cases) == count
        for c in cases:
            o = R.Ocb(orc, c["key"])
            assert o.encrypt(c["iv"], c["aad"], c["pt"], tlen) == c["ct"], (nlen, tlen, c["iv"].hex())
            assert o.decrypt(c["iv"], c["aad"], c["ct"], tlen) == (0, c["pt"]), (nlen, tlen, c["iv"].hex())
            total += 1
    assert total == 23
    # RFC 7253 appendix A's sample with a 96-bit tag
    K, N = bytes.fromhex("0F0E0D0C0B0A09080706050403020100"), bytes.fromhex("BBAA9988776655443322110D")
    A = P = bytes(range(40))
    want = bytes.fromhex("1792A4E31E0755FB03E31B22116E6C2DDF9EFD6E33D536F1A0124B0A55BAE884ED93481529C76B6AD0C515F4D1CDD4FDAC4F02AA")
    assert R.Ocb(orc, K).encrypt(N, A, P, 12) == want
    assert R.Ocb(orc, K).decrypt(N, A, want, 12) == (0, P)


def test_against_the_oracle_at_every_short_length(orc):
    """0 .. 600 bytes and around 256 * 16 * k, the three key sizes in turn, associated data of every residue, nonce and
    tag lengths walking their ranges; a flipped bit must not authenticate"""
    rng = random.Random(7253)
    lens = list(range(601)) + [4096 * k + d for k in (1, 2, 5) for d in (-17, -16, -1, 0, 1, 16, 33)]
    for n in lens:
        key = rng.randbytes((16, 24, 32)[n % 3])
        nlen, tlen = 1 + n % 15, 1 + (n // 3) % 16
        nonce, aad, pt = rng.randbytes(nlen), rng.randbytes((n * 7) % 53), rng.randbytes(n)
        o = R.Ocb(orc, key)
        want = orc.ocb_encrypt(key, nonce, aad, pt, tag_len=tlen)
        assert o.encrypt(nonce, aad, pt, tlen) == want, (n, nlen, tlen)
        assert o.decrypt(nonce, aad, want, tlen) == (0, pt), (n, nlen, tlen)
        if tlen >= 4:
            bad = bytearray(want)
            bad[rng.randrange(len(bad))] ^= 0x10
            assert o.decrypt(nonce, aad, bytes(bad), tlen)[0] == 0x1A == orc.ocb_decrypt(key, nonce, aad, bytes(bad), tag_len=tlen)[0], n


def test_every_bottom_of_the_nonce(orc):
    """the shift of the nonce, 0 .. 63 (and its branch for 0), against the oracle"""
    key = bytes(range(16))
    o = R.Ocb(orc, key)
    for b in range(64):
        nonce = bytes(range(11)) + bytes([0x40 | b])
        assert o.encrypt(nonce, b"a", bytes(40)) == orc.ocb_encrypt(key, nonce, b"a", bytes(40)), b


def test_offsets_by_gray_code_are_the_chained_offsets(orc):
    """every index up to 2^17 from one vectorised call against the RFC's recurrence, in slices that start anywhere"""
    o = R.Ocb(orc, bytes(range(32)))
    off0 = o.offset0(b"nonce", 16)
    n = 1 << 17
    want = np.frombuffer(o.chained(off0, n), dtype=np.int64).reshape(n, 2)
    hi, lo = R.offsets(o, off0, 0, n)
    assert np.array_equal(hi, want[:, 0]) and np.array_equal(lo, want[:, 1])
    for first, count in ((1, 1), (255, 2), (256, 256), (65535, 3), (99999, 1000), (n - 1, 1)):
        hi, lo = R.offsets(o, off0, first, count)
        assert np.array_equal(hi, want[first:first + count, 0]) and np.array_equal(lo, want[first:first + count, 1]), first
    for i in (1, 2, 255, 256, 257, 65536, n):
        assert R.xor(off0, o.delta(i)) == want[i - 1].tobytes(), i


def test_the_recurrence_far_out(orc):
    """Offset_i ^ Offset_{i-1} = L_ntz(i) at random indices up to 2^33, and at the powers of two"""
    o = R.Ocb(orc, bytes(range(16)))
    rng = random.Random(33)
    idx = [1 << j for j in range(1, 34)] + [(1 << j) + 1 for j in range(1, 33)] + [rng.randrange(2, 1 << 33) for _ in range(2000)]
    for i in idx:
        hi, lo = R.offsets(o, R.ZERO, i - 2, 2)
        step = R.unpair(int(hi[0] ^ hi[1]), int(lo[0] ^ lo[1]))
        assert step == o.L(R.ntz(i)), i
        assert R.unpair(int(hi[1]), int(lo[1])) == o.delta(i), i


def test_the_block_wise_text_tag_and_hash_against_the_oracle(orc):
    """1 MiB + 80 bytes of text in slices that are no multiple of a chunk, 300000 bytes of associated data: ciphertext,
    tag and HASH(K, A) put together from text_by_blocks, fold and finish are the oracle's, byte for byte"""
    key, nonce = bytes(range(16, 32)), bytes(range(70, 82))
    o = R.Ocb(orc, key)
    ecb = R.numpy_ecb(o)
    pt, aad = orc.splitmix(5, MIB + 80), orc.splitmix(6, 300000)
    want = orc.ocb_encrypt(key, nonce, aad, pt)
    off0 = o.offset0(nonce)
    src = np.frombuffer(pt, dtype=np.uint8)
    m, step, ck, got = len(pt) // 16, 16 * 20001, R.ZERO, bytearray()
    for lo in range(0, 16 * m, step):
        c, s = R.text_by_blocks(o, off0, lo // 16, src[lo:min(lo + step, 16 * m)], ecb)
        got += c.tobytes()
        ck = R.xor(ck, s)
    a, ma, h = np.frombuffer(aad, dtype=np.uint8), len(aad) // 16, R.ZERO
    for lo in range(0, 16 * ma, 16 * 7001):
        h = R.xor(h, R.text_by_blocks(o, R.ZERO, lo // 16, a[lo:min(lo + 16 * 7001, 16 * ma)], ecb, hash=True)[1])
    h = R.xor(h, o.aad_tail(ma, aad[16 * ma:]))
    assert h == o.hash_aad(aad)
    tail, tag = o.finish(off0, m, ck, pt[16 * m:], h)
    assert bytes(got) + tail + tag == want
    # the same tag as the issue of a call without associated data, XOR the hash
    assert R.xor(orc.ocb_encrypt(key, nonce, b"", pt)[-16:], h) == want[-16:]
    assert o.finish(off0, m, ck, want[16 * m:len(pt)], h, decrypt=True) == (pt[16 * m:], tag)


# ---- the launch shape, no device: 256 CUs -------------------------------------------------------------------------
SHAPES = [
    # len, aad_len, aad_aligned, (run, run_aad, threads per workgroup, workgroups, hash_blocks)
    (16400, 0, True, (1, 1, 256, 2, 0)),
    (MIB, 0, True, (1, 1, 256, 65, 0)),
    (8 * MIB - 16, 0, True, (1, 1, 256, 256, 0)),
    (8 * MIB, 0, True, (1, 1, 1024, 129, 0)),
    (16 * MIB, 0, True, (1, 1, 1024, 256, 0)),
    (268431344, 0, True, (1, 1, 1024, 256, 0)),
    (268431360, 0, True, (2, 1, 1024, 256, 0)),
    (536866816, 0, True, (4, 1, 1024, 256, 0)),
    (1073737728, 0, True, (8, 1, 1024, 256, 0)),
    (2147479536, 0, True, (8, 1, 1024, 256, 0)),
    (2147479552, 0, True, (16, 1, 1024, 256, 0)),
    (0, 131071, True, (1, 1, 256, 1, 0)),
    (0, 131072, True, (1, 1, 256, 9, 8192)),
    (0, 131072, False, (1, 1, 256, 1, 0)),
    (100, 268431365, True, (1, 2, 1024, 256, 16776960)),
    (MIB, 2147479552, True, (1, 16, 1024, 256, 134217472)),
]


def test_the_launch_shape_on_256_cus():
    got = [(n, a, al, want, uaes.plan_ocb(n, a, dec, al)) for n, a, al, want in SHAPES for dec in (False, True)]
    wrong = [g for g in got if g[4] != g[3]]
    assert not wrong, wrong
    # one workgroup's calls have no such shape, and the arrangement's answer is what it was
    for n, a in ((0, 0), (16, 0), (16384 + 15, 65536)):
        assert uaes.plan_ocb(n, a) is None and uaes.plan("ocb", n, a)[0] == "ocb.small", (n, a)
    assert uaes.plan_ocb(16400) is not None and uaes.plan_ocb(0, 65537) is not None
    assert uaes.plan("ocb", 268431360) == ("ocb.runs", 1, 0, 0)
    eng = uaes.engine()
    assert eng.uaes_debug_plan_ocb(2, MIB, 0, 1, None) is None and eng.uaes_debug_plan_ocb(-1, MIB, 0, 1, None) is None
    assert eng.uaes_debug_plan_ocb(0, MIB, 0, 1, None) == b"ocb.runs" and eng.uaes_debug_plan_ocb(1, 16, 0, 1, None) == b"ocb.small"
