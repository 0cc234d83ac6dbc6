"""EAX and SIV (RFC 5297) answers of the compiled reference (oracle/_ref, through tests/refbuilt.need()), shared by
tests/test_eax_siv_host.py, tests/test_gpu_eax_siv.py and the fuzz.  The reference is built with EAX_NONCE_LEN =
EAX_TAG_LEN = 16 and, in three more builds (EAX_LENS, oracle/Makefile's REF_EAXL), with other lengths; the lengths no
build covers are composed from its AES_CMAC (OMAC_t = CMAC([t]_16 || M)) and its AES_ECB_encrypt of the counter
blocks (the 56-bit increment of bytes 9..15), as AES_EAX_* computes them (micro_aes.c:1560-1648)."""
import ctypes as C
import os

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


# (bits, EAX_NONCE_LEN, EAX_TAG_LEN) -> the reference build with these constants (oracle/Makefile, REF_EAXL)
EAX_LENS = {(128, 0, 1): "libmicroaes_ref_128_eaxA.so", (192, 12, 8): "libmicroaes_ref_192_eaxB.so",
            (256, 37, 13): "libmicroaes_ref_256_eaxC.so"}


# the length matrix of tests/test_eax_siv_host.py (host path) and tests/test_gpu_eax_siv.py (kernels)
NONCE_LENS = (0, 1, 5, 12, 15, 16, 17, 31, 32, 37, 1000)
TAG_LENS = (1, 2, 7, 8, 13, 15, 16)
AAD_LENS = (255, 256, 257, 4096 + 3, 65536, (1 << 20) + 7)


def eax_encrypt_lens(bits, nonce_len, tag_len, key, nonce, aad, pt):
    """AES_EAX_encrypt of the reference build with EAX_NONCE_LEN = nonce_len and EAX_TAG_LEN = tag_len (the default
    build for 16 / 16): returns ct || tag"""
    assert len(nonce) == nonce_len and len(key) == bits // 8
    if (nonce_len, tag_len) == (16, 16):
        return eax_encrypt(bits, key, nonce, aad, pt)
    o = _buf(b"", len(pt) + 16)
    lib(EAX_LENS[bits, nonce_len, tag_len]).AES_EAX_encrypt(_buf(key), _buf(nonce), _buf(aad), C.c_size_t(len(aad)),
                                                            _buf(pt), C.c_size_t(len(pt)), o)
    assert bytes(o)[len(pt) + tag_len:] == bytes(16 - tag_len)           # nothing behind the build's own tag length
    return bytes(o)[: len(pt) + tag_len]


def eax_decrypt_lens(bits, nonce_len, tag_len, key, nonce, aad, ct_and_tag, prefill=0):
    """AES_EAX_decrypt of the same builds: (return code, output buffer)"""
    assert len(nonce) == nonce_len and len(key) == bits // 8
    name = "libmicroaes_ref_%d.so" % bits if (nonce_len, tag_len) == (16, 16) else EAX_LENS[bits, nonce_len, tag_len]
    n = len(ct_and_tag) - tag_len
    o = _buf(bytes([prefill]) * n, n)
    rc = lib(name).AES_EAX_decrypt(_buf(key), _buf(nonce), _buf(aad), C.c_size_t(len(aad)), _buf(ct_and_tag),
                                   C.c_size_t(n), o)
    return rc & 0xff, bytes(o)[:n]


def eax_expected(bits, key, nonce, aad, pt, tag_len):
    """ct || tag[:tag_len] from the reference build with exactly these lengths where there is one, else composed"""
    if (len(nonce), tag_len) == (16, 16) or (bits, len(nonce), tag_len) in EAX_LENS:
        return eax_encrypt_lens(bits, len(nonce), tag_len, key, nonce, aad, pt)
    return eax_composed(key, nonce, aad, pt, tag_len, bits)


def siv_encrypt(bits, keys, aad, pt):
    """the reference's AES_SIV_encrypt: returns (iv, ct)"""
    iv, o = _buf(b"", 16), _buf(b"", len(pt))
    ref(bits).AES_SIV_encrypt(_buf(keys), _buf(aad), C.c_size_t(len(aad)), _buf(pt), C.c_size_t(len(pt)), iv, o)
    return bytes(iv), bytes(o)[: len(pt)]


def eax_encrypt_records(bits, key, nonces, aads, texts):
    """AES_EAX_encrypt (16-byte nonces, 16-byte tags) of every record by itself: a list of ct || tag"""
    f, k, al, ml = ref(bits).AES_EAX_encrypt, _buf(key), len(aads[0]), len(texts[0])
    o, out = _buf(b"", ml + 16), []
    for nonce, aad, pt in zip(nonces, aads, texts):
        assert len(nonce) == 16 and len(aad) == al and len(pt) == ml
        f(k, nonce, aad, C.c_size_t(al), pt, C.c_size_t(ml), o)
        out.append(bytes(o)[: ml + 16])
    return out


def siv_encrypt_records(bits, keys, aads, texts):
    """AES_SIV_encrypt of every record by itself: a list of (iv, ct)"""
    f, k, al, ml = ref(bits).AES_SIV_encrypt, _buf(keys), len(aads[0]), len(texts[0])
    iv, o, out = _buf(b"", 16), _buf(b"", ml), []
    for aad, pt in zip(aads, texts):
        assert len(aad) == al and len(pt) == ml
        f(k, aad, C.c_size_t(al), pt, C.c_size_t(ml), iv, o)
        out.append((bytes(iv), bytes(o)[:ml]))
    return out


def eax_vectors(golden_dir):
    """the EAX paper's vectors (tests/golden/EAX_AES128.tv): dicts of KEY, NONCE, HEADER, MSG, CIPHER"""
    cases, cur = [], {}
    with open(os.path.join(golden_dir, "EAX_AES128.tv")) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            name, _, value = line.partition(":")
            cur[name.strip()] = bytes.fromhex(value.strip())
            if name.strip() == "CIPHER":
                cases.append(cur)
                cur = {}
    return cases


RFC5297_A1 = dict(keys=bytes.fromhex("fffefdfcfbfaf9f8f7f6f5f4f3f2f1f0f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff"),
                  ad=bytes.fromhex("101112131415161718191a1b1c1d1e1f2021222324252627"),
                  pt=bytes.fromhex("112233445566778899aabbccddee"),
                  iv=bytes.fromhex("85632d07c6e8f37f950acd320a2ecc93"), ct=bytes.fromhex("40c02b9690c4dc04daef7f6afe5c"))


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


def ctr_blocks(bits, key, ctr0, data):
    """CTR from a whole counter block with the reference's 56-bit increment (incBlock over bytes 9..15,
    micro_aes.c:421-427), the keystream from the reference's AES_ECB_encrypt of the counter blocks: any key size"""
    nb = (len(data) + 15) // 16
    if not nb:
        return b""
    head, c0 = bytes(ctr0[:9]), int.from_bytes(ctr0[9:], "big")
    blocks = b"".join(head + ((c0 + i) & ((1 << 56) - 1)).to_bytes(7, "big") for i in range(nb))
    o = _buf(b"", len(blocks))
    ref(bits).AES_ECB_encrypt(_buf(key), _buf(blocks), C.c_size_t(len(blocks)), o)
    ks = int.from_bytes(bytes(o)[: len(data)], "big")
    return (ks ^ int.from_bytes(data, "big")).to_bytes(len(data), "big")


def omac(key, t, data, bits=128):
    return cmac_any(bits, key, bytes(15) + bytes([t]) + bytes(data))


def eax_composed(key, nonce, aad, pt, tag_len, bits=128):
    """EAX with any nonce and tag length from the reference's primitives: returns ct || tag[:tag_len]"""
    assert len(key) == bits // 8
    n = omac(key, 0, nonce, bits)
    h = omac(key, 1, aad, bits)
    ct = ctr_preset(key, n, pt) if bits == 128 else ctr_blocks(bits, key, n, pt)
    c = omac(key, 2, ct, bits)
    return ct + bytes(a ^ b ^ d for a, b, d in zip(n, h, c))[:tag_len]


def eax_verdict(bits, key, nonce, aad, ct_and_tag, tag_len):
    """what a decryption must answer: 0 when the first tag_len bytes of N ^ H ^ C equal the tag given, else 0x1A (a
    forged text under a short tag is authentic once in 256 ** tag_len)"""
    ct, tag = ct_and_tag[: len(ct_and_tag) - tag_len], ct_and_tag[len(ct_and_tag) - tag_len:]
    t = xor(xor(omac(key, 0, nonce, bits), omac(key, 1, aad, bits)), omac(key, 2, ct, bits))
    return 0 if t[:tag_len] == tag else 0x1A


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
    # the CBC-MAC of the prefix in one call: CMAC(prefix || 0^128) = Enc(m ^ K1)
    m = xor(aes_decrypt_block(bits, k, cmac_any(bits, k, prefix + bytes(16))), k1) if prefix else bytes(16)
    last = xor(xor(xor(aes_decrypt_block(bits, k, v_target), m), y), k1)
    return prefix + last


def cmac_any(bits, key, data):
    m = _buf(b"", 16)
    ref(bits).AES_CMAC(_buf(key), _buf(data), C.c_size_t(len(data)), m)
    return bytes(m)
