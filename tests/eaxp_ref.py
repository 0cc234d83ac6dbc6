"""EAX' (ANSI C12.22 / IEEE 1703) for the tests: the recorded answers of the reference compiled with EAXP 1
(tests/golden/eaxp_vectors.json, written by tests/golden/make_eaxp_fixtures.py) and, for the lengths that file cannot
hold, the mode composed from the block cipher of the compiled reference (oracle/_ref, through tests/refbuilt.need()) as
AES_EAX_* compute it in that build (micro_aes.c:1523-1648):

    L = Enc(0^128), D = dblLE(L), Q = dblLE(D)                  (doubleLblock :449-458)
    CMAC'(start, X): CBC-MAC from `start`, the last block finished with D, or 10* and Q (cMac :576-590)
    N = CMAC'(D, nonce), N' = N with bit 7 of bytes 12 and 14 cleared, C = CTR(N', P) over bytes 9..15 (:421-427)
    C' = CMAC'(Q, C), 0^128 for an empty C (:1535-1539); mac = N[12:16] ^ C'[12:16]
"""
import functools
import json
import os

from tests import eax_siv_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eaxp_vectors.json")


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def entries():
    """(what, bits, key, nonce, pt, ct || mac): main.c's two vectors, then the seeded cases"""
    g = golden()
    text = bytes.fromhex(g["text"])
    for v in g["main_c"]:
        yield (v["what"], v["bits"]) + tuple(bytes.fromhex(v[f]) for f in ("key", "nonce", "pt", "out"))
    for e in g["entries"]:
        yield "seeded", e["bits"], bytes.fromhex(g["keys"][str(e["bits"])]), bytes.fromhex(e["nonce"]), text[:e["n"]], bytes.fromhex(e["out"])


def forged():
    """(what, bits, key, nonce, ct || mac, prefill, the reference's code, what it left in the output)"""
    g = golden()
    for e in g["forged"]:
        yield (e["what"], e["bits"], bytes.fromhex(g["keys"][str(e["bits"])]), bytes.fromhex(e["nonce"]), bytes.fromhex(e["out"]),
               e["prefill"], e["code"], bytes.fromhex(e["left"]))


def dbl_le(b):
    v = int.from_bytes(b, "little") << 1
    if v >> 128:
        v = (v ^ 0x87) & ((1 << 128) - 1)
    return v.to_bytes(16, "little")


def subkeys(bits, key):
    d = dbl_le(R.aes_encrypt_block(bits, key, bytes(16)))
    return d, dbl_le(d)


def cmac_prime(bits, key, start, x):
    d, q = subkeys(bits, key)
    s = (len(x) - 1) % 16 + 1 if x else 0
    m = start
    for i in range(0, len(x) - s, 16):
        m = R.aes_encrypt_block(bits, key, R.xor(m, x[i:i + 16]))
    last = x[len(x) - s:]
    last = R.xor(last, d) if s == 16 else R.xor(last + b"\x80" + bytes(15 - s), q)
    return R.aes_encrypt_block(bits, key, R.xor(m, last))


def clear(n):
    return n[:12] + bytes([n[12] & 0x7F, n[13], n[14] & 0x7F, n[15]])


def encrypt(bits, key, nonce, pt):
    """ct || mac"""
    assert len(key) == bits // 8
    d, q = subkeys(bits, key)
    n = cmac_prime(bits, key, d, nonce)
    ct = R.ctr_blocks(bits, key, clear(n), pt)
    c = cmac_prime(bits, key, q, ct) if ct else bytes(16)
    return ct + R.xor(n[12:], c[12:])


def decrypt(bits, key, nonce, out, prefill=0):
    """(code, text): the mac is checked first and a forgery leaves the prefill"""
    ct, mac = out[:-4], out[-4:]
    d, q = subkeys(bits, key)
    n = cmac_prime(bits, key, d, nonce)
    c = cmac_prime(bits, key, q, ct) if ct else bytes(16)
    if R.xor(n[12:], c[12:]) != mac:
        return 0x1A, bytes([prefill]) * len(ct)
    return 0, R.ctr_blocks(bits, key, clear(n), ct)


def nonce_for(bits, key, n_target):
    """a 16-byte nonce whose N = CMAC'(D, nonce) = Enc(D ^ nonce ^ D) = Enc(nonce) is n_target"""
    return R.aes_decrypt_block(bits, key, n_target)
