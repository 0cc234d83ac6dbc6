"""XAES-256-GCM (C2SP, c2sp.org/XAES-256-GCM) as a composition of two things the oracle has: encrypt_block (the CMAC
subkey and the two derivation blocks; cross-checked against its cmac) and gcm_encrypt / gcm_decrypt at 256 bits.  The
specification's two vectors and its accumulated test are in tests/golden/xaes256gcm_vectors.json
(tests/golden/make_xaes_fixtures.py).  Shared by tests/test_xaes_host.py and tests/test_gpu_xaes.py."""
import functools
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "xaes256gcm_vectors.json")


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def big_l(key):
    """L = AES-256_K(0^128): CMAC's starting point"""
    return oracle().encrypt_block(key, bytes(16))


def k1(key):
    """CMAC's first subkey: L doubled in GF(2^128), big-endian, 0x87 into the last byte when L's top bit was set"""
    l = int.from_bytes(big_l(key), "big")
    v = (l << 1) & ((1 << 128) - 1)
    return (v ^ 0x87 if l >> 127 else v).to_bytes(16, "big")


def derive(key, nonce):
    """Kx = AES_K(M1 ^ K1) || AES_K(M2 ^ K1), Mi = 00 0i 58 00 || nonce[:12]"""
    assert len(key) == 32 and len(nonce) == 24
    sub = k1(key)
    halves = []
    for i in (1, 2):
        m = bytes([0, i, 0x58, 0]) + nonce[:12]
        halves.append(oracle().encrypt_block(key, bytes(a ^ b for a, b in zip(m, sub))))
    return b"".join(halves)


def derive_by_cmac(key, nonce):
    """the same through the oracle's CMAC: each Mi is one whole block"""
    return b"".join(oracle().cmac(key, bytes([0, i, 0x58, 0]) + nonce[:12]) for i in (1, 2))


def encrypt(key, nonce, aad, pt):
    """ciphertext || 16-byte tag"""
    return oracle().gcm_encrypt(derive(key, nonce), nonce[12:], aad, pt)


def decrypt(key, nonce, aad, ct_and_tag, prefill=0xCC):
    """(code, text): 0, or 0x1A with the text left as the prefill"""
    return oracle().gcm_decrypt(derive(key, nonce), nonce[12:], aad, ct_and_tag, prefill=prefill)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def vectors():
    """the specification's two vectors: dicts of key, nonce, aad, plaintext, kx, output (bytes)"""
    return [{k: bytes.fromhex(v) for k, v in vec.items()} for vec in golden()["vectors"]]


@functools.lru_cache(maxsize=None)
def _stream():
    acc = golden()["accumulated"]
    return hashlib.shake_128(b"").digest(acc["stream_bytes"])


def accumulated(count=None):
    """the inputs of the specification's accumulated test, in order: (key, nonce, plaintext, aad); all 10 000 consume
    exactly the fixture's stream_bytes of SHAKE-128 of the empty input"""
    s, pos = _stream(), 0
    n = golden()["accumulated"]["iterations"] if count is None else count

    def take(k):
        nonlocal pos
        pos += k
        return s[pos - k:pos]
    for _ in range(n):
        key, nonce = take(32), take(24)
        pt = take(take(1)[0])
        aad = take(take(1)[0])
        yield key, nonce, pt, aad
    if count is None:
        assert pos == len(s), (pos, len(s))


def accumulated_digest(outputs):
    """what the specification hashes: every ciphertext || tag into a second SHAKE-128, 32 bytes of it"""
    h = hashlib.shake_128()
    for o in outputs:
        h.update(o)
    return h.digest(32).hex()


def keys_by_top_bit_of_l():
    """(a master key whose L has the top bit set, one whose L has it clear): the two branches of the doubling, found by
    walking splitmix seeds"""
    found = {}
    seed = 0
    while len(found) < 2:
        key = oracle().splitmix(0x5841 + seed, 32)
        found.setdefault(big_l(key)[0] >> 7, key)
        seed += 1
        assert seed < 64, "no such key in 64 seeds"
    return found[1], found[0]


def check_vectors_through_the_reference():
    """where oracle/_ref is present: the two vectors through the reference-built 256-bit AES_CMAC and AES_GCM_encrypt.
    Returns False (and checks nothing) where it is not."""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libmicroaes_ref_256.so")):
        return False
    from oracle.pyoracle import Reference
    ref = Reference(256)
    for v in vectors():
        kx = b"".join(ref.cmac(v["key"], bytes([0, i, 0x58, 0]) + v["nonce"][:12]) for i in (1, 2))
        assert kx == v["kx"], kx.hex()
        assert ref.gcm_encrypt(kx, v["nonce"][12:], v["aad"], v["plaintext"]) == v["output"]
    return True


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)
