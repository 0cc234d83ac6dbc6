"""SIV (RFC 5297) with S2V over a LIST of associated-data components, written from section 2.4 of the RFC on top of three
things the oracle has: cmac, encrypt_block and CTR from a whole counter block (ctr_xcrypt_at, the 56-bit increment the
engine's SIV uses too; it differs from the RFC's only when the counter's low 56 bits wrap, once in 2^40 for a 1 MiB text).

    S2V(K, S1..Sn):  D = CMAC(0^128);  for i < n: D = dbl(D) xor CMAC(Si)
                     len(Sn) >= 16: T = Sn xorend D   else: T = dbl(D) xor pad(Sn)
                     V = CMAC(T)                     (no string at all -- not reachable here, the text always is one)
    encrypt:         V = S2V(K1, AD1..ADk, P);  Q = V with bits 31 and 63 cleared;  C = CTR(K2, Q, P)

An empty component is a component.  The fixtures (tests/golden/siv_v_vectors.json, written by
tests/golden/make_siv_v_fixtures.py) hold RFC 5297's two examples and cases recorded from another implementation.
Shared by tests/test_siv_v_host.py and tests/test_gpu_siv_v.py."""
import functools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "siv_v_vectors.json")


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def dbl(b):
    v = int.from_bytes(b, "big") << 1
    if v >> 128:
        v = (v ^ 0x87) & ((1 << 128) - 1)
    return v.to_bytes(16, "big")


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def cmac(key, data):
    """CMAC of any string; the empty one is Enc(10* xor K2), computed here from the block cipher and checked against the
    oracle's own answer"""
    if data:
        return oracle().cmac(key, data)
    k2 = dbl(dbl(oracle().encrypt_block(key, bytes(16))))
    mac = oracle().encrypt_block(key, xor(b"\x80" + bytes(15), k2))
    assert mac == oracle().cmac(key, b"")
    return mac


def s2v(k1, ads, text):
    d = cmac(k1, bytes(16))
    for s in ads:
        d = xor(dbl(d), cmac(k1, bytes(s)))
    if len(text) >= 16:
        t = text[:-16] + xor(text[-16:], d)
    else:
        t = xor(dbl(d), text + b"\x80" + bytes(15 - len(text)))
    return cmac(k1, t)


def _ctr(k2, v, data):
    q = bytearray(v)
    q[8] &= 0x7F
    q[12] &= 0x7F
    return oracle().ctr_xcrypt_at(k2, bytes(q), 0, data) if data else b""


def siv_encrypt(keys, ads, pt):
    """keys = K1 || K2; returns (iv, ciphertext)"""
    keys, pt = bytes(keys), bytes(pt)
    half = len(keys) // 2
    v = s2v(keys[:half], ads, pt)
    return v, _ctr(keys[half:], v, pt)


def siv_decrypt(keys, iv, ads, ct):
    """(code, text): 0, or 0x1A with the text CTR made (the caller applies the wipe switch)"""
    keys, ct = bytes(keys), bytes(ct)
    half = len(keys) // 2
    pt = _ctr(keys[half:], iv, ct)
    return (0 if s2v(keys[:half], ads, pt) == bytes(iv) else 0x1A), pt


@functools.lru_cache(maxsize=None)
def fixtures():
    """dicts of name, source, keys, ads (a list), pt, iv, ct -- bytes"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    out = []
    for c in doc["cases"]:
        out.append(dict(name=c["name"], source=c["source"], keys=bytes.fromhex(c["keys"]),
                        ads=[bytes.fromhex(a) for a in c["ads"]], pt=bytes.fromhex(c["pt"]),
                        iv=bytes.fromhex(c["iv"]), ct=bytes.fromhex(c["ct"])))
    return out
