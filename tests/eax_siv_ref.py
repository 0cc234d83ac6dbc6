"""EAX and SIV (RFC 5297) answers of the compiled reference (oracle/_ref, through tests/refbuilt.need()), shared by
tests/test_eax_siv_host.py and tests/test_gpu_eax_siv.py.  The reference is built with EAX_NONCE_LEN = EAX_TAG_LEN
= 16; other lengths are composed from its AES_CMAC (OMAC_t = CMAC([t]_16 || M)) and the CTR of the PRESET_COUNTER
build (the whole counter block given, the 56-bit increment), as AES_EAX_* computes them (micro_aes.c:1560-1648)."""
import ctypes as C

from tests import refbuilt

_libs = {}


def lib(name):
    if name not in _libs:
        _libs[name] = C.CDLL(refbuilt.need(name))
    return _libs[name]


def ref(bits):
    return lib("libmicroaes_ref_%d.so" % bits)


def _buf(b, n=None):
    b = bytes(b)
    n = max(len(b) if n is None else n, 1)
    return (C.c_uint8 * n).from_buffer_copy(b.ljust(n, b"\0"))


def eax_encrypt(bits, key, nonce, aad, pt):
    """the reference's AES_EAX_encrypt: 16-byte nonce, 16-byte tag; returns ct || tag"""
    assert len(nonce) == 16
    o = _buf(b"", len(pt) + 16)
    ref(bits).AES_EAX_encrypt(_buf(key), _buf(nonce), _buf(aad), C.c_size_t(len(aad)), _buf(pt), C.c_size_t(len(pt)), o)
    return bytes(o)[: len(pt) + 16]


def siv_encrypt(bits, keys, aad, pt):
    """the reference's AES_SIV_encrypt: returns (iv, ct)"""
    iv, o = _buf(b"", 16), _buf(b"", len(pt))
    ref(bits).AES_SIV_encrypt(_buf(keys), _buf(aad), C.c_size_t(len(aad)), _buf(pt), C.c_size_t(len(pt)), iv, o)
    return bytes(iv), bytes(o)[: len(pt)]


def siv_decrypt_rc(bits, keys, iv, aad, ct):
    o = _buf(b"", len(ct))
    rc = ref(bits).AES_SIV_decrypt(_buf(keys), _buf(iv), _buf(aad), C.c_size_t(len(aad)), _buf(ct), C.c_size_t(len(ct)), o)
    return rc & 0xff, bytes(o)[: len(ct)]


def cmac(key, data):
    m = _buf(b"", 16)
    lib("libmicroaes_ref_128.so").AES_CMAC(_buf(key), _buf(data), C.c_size_t(len(data)), m)
    return bytes(m)


def ctr_preset(key, ctr0, data):
    o = _buf(b"", len(data))
    lib("libmicroaes_ref_128_presetctr.so").AES_CTR_encrypt(_buf(key), _buf(ctr0), _buf(data), C.c_size_t(len(data)), o)
    return bytes(o)[: len(data)]


def omac(key, t, data):
    return cmac(key, bytes(15) + bytes([t]) + bytes(data))


def eax_composed(key, nonce, aad, pt, tag_len):
    """AES-128 EAX with any nonce and tag length from the reference's primitives: returns ct || tag[:tag_len]"""
    n = omac(key, 0, nonce)
    h = omac(key, 1, aad)
    ct = ctr_preset(key, n, pt)
    c = omac(key, 2, ct)
    return ct + bytes(a ^ b ^ d for a, b, d in zip(n, h, c))[:tag_len]


def aes_decrypt_block(bits, key, block):
    """one AES block decryption (the reference's ECB decrypt of 16 bytes)"""
    o = _buf(b"", 16)
    ref(bits).AES_ECB_decrypt(_buf(key), _buf(block), C.c_size_t(16), o)
    return bytes(o)


def aes_encrypt_block(bits, key, block):
    o = _buf(b"", 16)
    ref(bits).AES_ECB_encrypt(_buf(key), _buf(block), C.c_size_t(16), o)
    return bytes(o)


def dbl(b):
    v = int.from_bytes(b, "big") << 1
    if v >> 128:
        v = (v ^ 0x87) & ((1 << 128) - 1)
    return v.to_bytes(16, "big")


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def eax_nonce_for(bits, key, n_target):
    """a 16-byte nonce whose N = OMAC_0(nonce) = Enc(Enc([0]_16) ^ nonce ^ K1) is n_target"""
    k1 = dbl(aes_encrypt_block(bits, key, bytes(16)))
    e0 = aes_encrypt_block(bits, key, bytes(16))
    return xor(xor(aes_decrypt_block(bits, key, n_target), e0), k1)


def siv_text_for(bits, keys, aad, prefix, v_target):
    """a plaintext prefix || last (len(prefix) % 16 == 0, len >= 16 in total) whose S2V V is v_target:
    V = Enc(m ^ (last ^ Y ^ K1)) with m the CBC-MAC of the prefix (RFC 5297 xorend on a whole last block)"""
    assert len(prefix) % 16 == 0
    kb = bits // 8
    k = keys[:kb]
    k1 = dbl(aes_encrypt_block(bits, k, bytes(16)))
    y = aes_encrypt_block(bits, k, k1)                              # CMAC(0^128)
    if aad:
        y = xor(dbl(y), cmac_any(bits, k, aad))
    m = bytes(16)
    for i in range(0, len(prefix), 16):
        m = aes_encrypt_block(bits, k, xor(m, prefix[i:i + 16]))
    last = xor(xor(xor(aes_decrypt_block(bits, k, v_target), m), y), k1)
    return prefix + last


def cmac_any(bits, key, data):
    m = _buf(b"", 16)
    ref(bits).AES_CMAC(_buf(key), _buf(data), C.c_size_t(len(data)), m)
    return bytes(m)
