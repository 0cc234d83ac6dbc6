"""CPU check of the integer GF(2^128) helpers the GHASH / XTS kernels are built
from (micro-aes_amd/csrc/uaes_gf.h compiles as host C++ too): wave-cooperative
multiply, multiplication tables, the strided-Horner level recursion and the
tweak shifts -- all against the oracle's bit-serial arithmetic."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gfc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gfc") / "libgfc.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tests", "csrc", "gf_check.cpp")], check=True)
    return C.CDLL(out)


def buf(b):
    return (C.c_uint8 * len(b)).from_buffer_copy(bytes(b))


def test_wave_cooperative_multiply(gfc, orc):
    rnd = random.Random(1)
    cases = [(bytes(16), rnd.randbytes(16)), (bytes([0x80] + [0] * 15), rnd.randbytes(16)),
             (bytes([0] * 15 + [1]), bytes([0] * 15 + [1])), (b"\xff" * 16, b"\xff" * 16)]
    cases += [(rnd.randbytes(16), rnd.randbytes(16)) for _ in range(200)]
    for x, y in cases:
        o = (C.c_uint8 * 16)()
        gfc.gfc_wave_mul(buf(x), buf(y), o)
        assert bytes(o) == orc.gf128_mul(x, y)


def test_tables_multiply_by_fixed_element(gfc, orc):
    rnd = random.Random(2)
    for _ in range(3):
        m = rnd.randbytes(16)
        t8, t4 = (C.c_uint8 * 65536)(), (C.c_uint8 * 8192)()
        gfc.gfc_table8(buf(m), t8)
        gfc.gfc_table4(buf(m), t4)
        for _ in range(50):
            a = rnd.randbytes(16)
            z8, z4 = (C.c_uint8 * 16)(), (C.c_uint8 * 16)()
            gfc.gfc_tabmul8(t8, buf(a), z8)
            gfc.gfc_tabmul4(t4, buf(a), z4)
            assert bytes(z8) == bytes(z4) == orc.gf128_mul(a, m)


def gf_pow(orc, h, e):
    r = bytes([0x80] + [0] * 15)
    for _ in range(e):
        r = orc.gf128_mul(r, h)
    return r


@pytest.mark.parametrize("n", [1, 5, 16, 17, 255, 256, 257, 1000])
def test_level_recursion_equals_ghash(gfc, orc, n):
    """strides 64 -> 16 -> 1 (small stand-ins for 2^17 -> 2^12 -> 256 -> 16 -> 1)"""
    rnd = random.Random(n)
    H = rnd.randbytes(16)
    data = rnd.randbytes(16 * n)
    # reference value: GHASH without the length block == orc.ghash minus last step
    acc = bytes(16)
    for k in range(n):
        acc = orc.gf128_mul(bytes(a ^ b for a, b in zip(acc, data[16 * k:16 * k + 16])), H)
    t64, t16, t1 = (C.c_uint8 * 65536)(), (C.c_uint8 * 8192)(), (C.c_uint8 * 8192)()
    gfc.gfc_table8(buf(gf_pow(orc, H, 64)), t64)
    gfc.gfc_table4(buf(gf_pow(orc, H, 16)), t16)
    gfc.gfc_table4(buf(H), t1)
    a64, a16, out = (C.c_uint8 * (64 * 16))(), (C.c_uint8 * (16 * 16))(), (C.c_uint8 * 16)()
    gfc.gfc_level(t64, 0, buf(data), C.c_uint64(n), C.c_uint64(64), a64)
    gfc.gfc_level(t16, 1, a64, C.c_uint64(64), C.c_uint64(16), a16)
    gfc.gfc_last(t1, a16, C.c_uint64(16), out)
    assert bytes(out) == acc


def test_xts_tweak_shifts(gfc, orc):
    """alpha^k by one shift == k doublings, cross-checked through the oracle's
    XTS: block j of a data unit is Enc(P ^ T*alpha^j) ^ T*alpha^j."""
    rnd = random.Random(3)

    def double(t):
        v = int.from_bytes(t, "little") << 1
        if v >> 128:
            v = (v & ((1 << 128) - 1)) ^ 0x87
        return v.to_bytes(16, "little")

    for _ in range(50):
        t = rnd.randbytes(16)
        cur = t
        for k in range(65):
            o = (C.c_uint8 * 16)()
            gfc.gfc_tw_pow(buf(t), k, o)
            assert bytes(o) == cur, k
            cur = double(cur)


def test_xts_chunk_tweak_by_sparse_powers(gfc):
    """tw_mul_a256(t, l) = t * alpha^(256 l) for every lane l = 0..63 (six conditional products by the sparse
    residues of alpha^(256 2^s)) against 256 l doublings"""
    rnd = random.Random(11)

    def double(v):
        v <<= 1
        return (v & ((1 << 128) - 1)) ^ 0x87 if v >> 128 else v

    for _ in range(6):
        t = rnd.randbytes(16)
        cur = int.from_bytes(t, "little")
        for l in range(64):
            o = (C.c_uint8 * 16)()
            gfc.gfc_tw_a256(buf(t), l, o)
            assert int.from_bytes(bytes(o), "little") == cur, l
            for _ in range(256):
                cur = double(cur)


XTS_P = (1 << 128) | 0x87                       # x^128 + x^7 + x^2 + x + 1; bit k of the integer = coefficient of x^k


def xts_mul(a, b):
    """a * b modulo XTS_P on Python integers (the XTS bit order: a block is a 128-bit little-endian integer)"""
    z = 0
    while b:
        if b & 1:
            z ^= a
        a <<= 1
        if a >> 128:
            a ^= XTS_P
        b >>= 1
    return z


def xts_alpha_pow(e):
    """alpha^e by square-and-multiply, alpha = x"""
    z, base = 1, 2
    while e:
        if e & 1:
            z = xts_mul(z, base)
        base = xts_mul(base, base)
        e >>= 1
    return z


def xts_pow_table(gfc, n=40):
    o = (C.c_uint8 * (16 * n))()
    gfc.gfc_tw_pow_table(o, n)
    return [int.from_bytes(bytes(o[16 * i:16 * i + 16]), "little") for i in range(n)]


def test_xts_power_table_all_40_constants(gfc):
    """tw_pow_table (what xts_pow_table() of uaes_kernels.hip hands k_xts_expand and k_xts_small): entry i is
    alpha^(2^(14+i)) for every i < 40 -- no GPU test reaches more than the first twelve (a unit of 2^(14+i) chunks of
    4 KiB is 2^(26+i) bytes).  The reference exponentiation shares no code with the table: square-and-multiply on
    Python integers, itself checked against plain doubling where that is cheap."""
    cur = 1
    for k in range(1, 1025):
        cur <<= 1
        if cur >> 128:
            cur ^= XTS_P
        if k in (1, 127, 128, 129, 1024):
            assert xts_alpha_pow(k) == cur, k
    table = xts_pow_table(gfc)
    assert len(table) == len(set(table)) == 40
    for i, got in enumerate(table):
        assert got == xts_alpha_pow(1 << (14 + i)), "entry %d" % i


def test_xts_wave_wide_product(gfc):
    """wave_tw_mul's arithmetic on 64 simulated lanes with an XOR butterfly: t * e for the 40 constants and for random
    e, all lanes agreeing"""
    rnd = random.Random(40)
    es = xts_pow_table(gfc) + [0, 1, 1 << 63, 1 << 64, 1 << 127, (1 << 128) - 1] + [rnd.getrandbits(128) for _ in range(200)]
    for e in es:
        for t in (rnd.getrandbits(128), 1, (1 << 128) - 1):
            o = (C.c_uint8 * 16)()
            same = gfc.gfc_wave_tw_mul(buf(t.to_bytes(16, "little")), buf(e.to_bytes(16, "little")), o)
            assert same == 1, (hex(t), hex(e))
            assert int.from_bytes(bytes(o), "little") == xts_mul(t, e), (hex(t), hex(e))
