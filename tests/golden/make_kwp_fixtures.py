#!/usr/bin/env python3
"""Writes tests/golden/kwp_vectors.json: the two vectors of RFC 5649 section 6 and outputs of the OpenSSL command-line
tool (openssl enc -id-aes<bits>-wrap-pad, an implementation that shares nothing with this project) for the three key
sizes at secret lengths 1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 255, 256 and 4097.  The RFC's vectors are reproduced
with the same tool before anything is written.  The tool's cipher filter hands the cipher pieces of 4096 bytes, each of
which it wraps by itself, so the 4097-byte secrets go to the same OpenSSL's library call instead (EVP_EncryptUpdate with
EVP_aes_<bits>_wrap_pad), which every shorter vector is also checked against.  Run by hand when the list changes; no test
runs it.
Usage: make_kwp_fixtures.py"""
import ctypes as C
import ctypes.util
import hashlib
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 255, 256, 4097]
RFC_KEK = "5840df6e29b02af1ab493b705bf16ea1ae8338f4dcc176a8"
RFC = [("c37b7e6492584340bed12207808941155068f738", "138bdeaa9b8fa7fc61f97742e72248ee5ae6ae5360d1ae6a5f54f373fa543b6a"),
       ("466f7250617369", "afbeb0f07dfbf5419200f2ccb50bb24f")]


def stream(tag, n):
    """n bytes that depend on the tag alone (SHA-256 in counter mode)"""
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(("%s/%d" % (tag, i)).encode()).digest()
        i += 1
    return out[:n]


def openssl_wrap(kek, secret):
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(src, "wb") as f:
            f.write(secret)
        subprocess.run(["openssl", "enc", "-id-aes%d-wrap-pad" % (8 * len(kek)), "-e", "-K", kek.hex(), "-iv", "a65959a6",
                        "-in", src, "-out", dst], check=True)
        with open(dst, "rb") as f:
            return f.read()


def libcrypto_wrap(kek, secret):
    lib = C.CDLL(ctypes.util.find_library("crypto"))
    cipher = getattr(lib, "EVP_aes_%d_wrap_pad" % (8 * len(kek)))
    lib.EVP_CIPHER_CTX_new.restype = cipher.restype = C.c_void_p
    lib.EVP_CIPHER_CTX_set_flags.argtypes = [C.c_void_p, C.c_int]
    lib.EVP_CIPHER_CTX_free.argtypes = [C.c_void_p]
    lib.EVP_EncryptInit_ex.argtypes = [C.c_void_p] * 5
    lib.EVP_EncryptUpdate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
    ctx = lib.EVP_CIPHER_CTX_new()
    lib.EVP_CIPHER_CTX_set_flags(ctx, 1)                                    # EVP_CIPHER_CTX_FLAG_WRAP_ALLOW
    out, n = C.create_string_buffer(len(secret) + 16), C.c_int(0)
    assert lib.EVP_EncryptInit_ex(ctx, cipher(), None, kek, None) == 1
    assert lib.EVP_EncryptUpdate(ctx, out, C.byref(n), secret, len(secret)) == 1
    lib.EVP_CIPHER_CTX_free(ctx)
    return out.raw[:n.value]


def main():
    vectors = []
    for secret, wrapped in RFC:
        got = openssl_wrap(bytes.fromhex(RFC_KEK), bytes.fromhex(secret))
        assert got.hex() == wrapped, ("the tool does not reproduce RFC 5649 section 6", secret, got.hex())
        vectors.append(dict(source="RFC 5649 section 6", kek=RFC_KEK, secret=secret, wrapped=wrapped))
    for bits in (128, 192, 256):
        kek = stream("kek %d" % bits, bits // 8)
        for n in LENGTHS:
            secret = stream("secret %d %d" % (bits, n), n)
            wrapped = libcrypto_wrap(kek, secret)
            assert len(wrapped) == (n + 7) // 8 * 8 + 8
            assert n > 4096 or wrapped == openssl_wrap(kek, secret)
            vectors.append(dict(source=("openssl enc -id-aes%d-wrap-pad" if n <= 4096 else "libcrypto EVP_aes_%d_wrap_pad") % bits, kek=kek.hex(), secret=secret.hex(),
                                wrapped=wrapped.hex()))
    version = subprocess.run(["openssl", "version"], check=True, capture_output=True, text=True).stdout.strip()
    path = os.path.join(HERE, "kwp_vectors.json")
    with open(path, "w") as f:
        json.dump(dict(tool=version, vectors=vectors), f, separators=(",", ":"))
        f.write("\n")
    assert os.path.getsize(path) < 64 << 10, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes,", len(vectors), "vectors")


if __name__ == "__main__":
    main()
