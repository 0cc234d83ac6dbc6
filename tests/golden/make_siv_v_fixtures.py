#!/usr/bin/env python3
"""Writes tests/golden/siv_v_vectors.json: SIV (RFC 5297) with several components of associated data.

  rfc5297.A1, rfc5297.A2   the RFC's two examples, typed in below (A.2 is nonce-based SIV: two components and the nonce)
  libcrypto.NNN            seeded cases recorded from the system's libcrypto (OpenSSL 3: EVP_CIPHER_fetch "AES-128-SIV" /
                           "AES-192-SIV" / "AES-256-SIV", one AAD update per component) through ctypes: all three key
                           sizes, 1 to 5 components of 1 to 40 bytes, texts of 0 to 80 bytes
  python.NNN               what libcrypto cannot say -- it skips an update of length zero, so a case with an empty
                           component (and an empty text, if it refuses that) comes from tests/siv_v_ref.py alone

Every case carries its `source`.  Before anything is written every recorded case is recomputed with tests/siv_v_ref.py,
and libcrypto must reproduce both RFC examples, so the file holds nothing the two do not agree on.  Run by hand when the
list changes; no test runs it.
Usage: make_siv_v_fixtures.py"""
import ctypes as C
import ctypes.util
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

RFC = [
    dict(name="rfc5297.A1",
         keys="fffefdfcfbfaf9f8f7f6f5f4f3f2f1f0f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff",
         ads=["101112131415161718191a1b1c1d1e1f2021222324252627"],
         pt="112233445566778899aabbccddee",
         iv="85632d07c6e8f37f950acd320a2ecc93", ct="40c02b9690c4dc04daef7f6afe5c"),
    dict(name="rfc5297.A2",
         keys="7f7e7d7c7b7a79787776757473727170404142434445464748494a4b4c4d4e4f",
         ads=["00112233445566778899aabbccddeeffdeaddadadeaddadaffeeddccbbaa99887766554433221100",
              "102030405060708090a0", "09f911029d74e35bd84156c5635688c0"],
         pt="7468697320697320736f6d6520706c61696e7465787420746f20656e6372797074207573696e67205349562d414553",
         iv="7bdb6e3b432667eb06f4d14bff2fbd0f",
         ct="cb900f2fddbe404326601965c889bf17dba77ceb094fa663b7a3f748ba8af829ea64ad544a272e9c485b62a3fd5c0d"),
]

EVP_CTRL_AEAD_GET_TAG = 0x10


class Libcrypto:
    def __init__(self):
        L = self.L = C.CDLL(ctypes.util.find_library("crypto"))
        vp, i = C.c_void_p, C.c_int
        L.EVP_CIPHER_fetch.restype = vp
        L.EVP_CIPHER_fetch.argtypes = [vp, C.c_char_p, C.c_char_p]
        L.EVP_CIPHER_CTX_new.restype = vp
        L.EVP_CIPHER_CTX_free.argtypes = [vp]
        L.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, vp, vp]
        L.EVP_EncryptUpdate.argtypes = [vp, vp, C.POINTER(i), vp, i]
        L.EVP_EncryptFinal_ex.argtypes = [vp, vp, C.POINTER(i)]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, i, i, vp]

    def siv_encrypt(self, keys, ads, pt):
        """(iv, ct), or None where libcrypto refuses the call"""
        L = self.L
        cipher = L.EVP_CIPHER_fetch(None, b"AES-%d-SIV" % (len(keys) * 4), None)
        assert cipher, "libcrypto has no AES-SIV"
        ctx = L.EVP_CIPHER_CTX_new()
        try:
            n = C.c_int(0)
            if L.EVP_EncryptInit_ex(ctx, cipher, None, bytes(keys), None) != 1:
                return None
            for a in ads:
                if L.EVP_EncryptUpdate(ctx, None, C.byref(n), bytes(a), len(a)) != 1:
                    return None
            out = C.create_string_buffer(len(pt) + 16)
            if L.EVP_EncryptUpdate(ctx, out, C.byref(n), bytes(pt), len(pt)) != 1 or n.value != len(pt):
                return None
            if L.EVP_EncryptFinal_ex(ctx, None, C.byref(n)) != 1:
                return None
            tag = C.create_string_buffer(16)
            if L.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_AEAD_GET_TAG, 16, tag) != 1:
                return None
            return tag.raw[:16], out.raw[: len(pt)]
        finally:
            L.EVP_CIPHER_CTX_free(ctx)


def main():
    from tests import siv_v_ref as R
    lib = Libcrypto()
    cases = []
    for v in RFC:
        keys, ads, pt = bytes.fromhex(v["keys"]), [bytes.fromhex(a) for a in v["ads"]], bytes.fromhex(v["pt"])
        want = (bytes.fromhex(v["iv"]), bytes.fromhex(v["ct"]))
        assert lib.siv_encrypt(keys, ads, pt) == want, v["name"]
        assert R.siv_encrypt(keys, ads, pt) == want, v["name"]
        cases.append(dict(v, source="RFC 5297"))
    rng = random.Random(5297)
    refused_empty_text = False
    for k in range(60):
        bits = (128, 192, 256)[k % 3]
        keys = rng.randbytes(bits // 4)
        ads = [rng.randbytes(rng.randrange(1, 41)) for _ in range(1 + k % 5)]
        pt = rng.randbytes(0 if k % 20 == 7 else rng.randrange(0, 81))
        got = lib.siv_encrypt(keys, ads, pt)
        want = R.siv_encrypt(keys, ads, pt)
        if got is None:
            assert not pt, "libcrypto refused a case with a text"
            refused_empty_text = True
            source, name = "tests/siv_v_ref.py (libcrypto refuses an empty text)", "python.%03d" % k
        else:
            assert got == want, (k, got, want)
            source, name = "libcrypto AES-%d-SIV" % bits, "libcrypto.%03d" % k
        cases.append(dict(name=name, source=source, keys=keys.hex(), ads=[a.hex() for a in ads], pt=pt.hex(),
                          iv=want[0].hex(), ct=want[1].hex()))
    for k in range(12):                                    # an empty component, at every position of 1 to 4
        bits = (128, 192, 256)[k % 3]
        keys = rng.randbytes(bits // 4)
        ads = [rng.randbytes(rng.randrange(1, 41)) for _ in range(1 + k % 4)]
        ads[k % len(ads)] = b""
        pt = rng.randbytes(rng.randrange(0, 81))
        iv, ct = R.siv_encrypt(keys, ads, pt)
        cases.append(dict(name="python.%03d" % (100 + k), source="tests/siv_v_ref.py (libcrypto skips an empty update)",
                          keys=keys.hex(), ads=[a.hex() for a in ads], pt=pt.hex(), iv=iv.hex(), ct=ct.hex()))
    path = os.path.join(HERE, "siv_v_vectors.json")
    with open(path, "w") as f:
        json.dump(dict(source="RFC 5297 appendix A; libcrypto through ctypes; tests/siv_v_ref.py", cases=cases), f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(cases), "cases; libcrypto refused an empty text:", refused_empty_text)


if __name__ == "__main__":
    main()
