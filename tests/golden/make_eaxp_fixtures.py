#!/usr/bin/env python3
"""Records tests/golden/eaxp_vectors.json: what the reference gives for EAX' (ANSI C12.22 / IEEE 1703) when it is compiled
with EAXP 1.

For the build container only (it needs the reference checkout that oracle/Makefile names as REF, or $REF); the tests
read the recorded file and never run this.  The reference is built at 128 / 192 / 256 bits in a temporary directory
outside the repository, from a copy of its header with two lines changed by sed (both checked to have hit) and a link to
micro_aes.c, the way tests/golden/make_ff3_fixtures.py builds its variant; the directory is removed afterwards.  The
recorded file is data only: keys, nonces, texts, return codes.

    python3 tests/golden/make_eaxp_fixtures.py

Contents: the two vectors of the reference's main.c (IEEE 1703 Annex G; Moise, Beroset, Phinney and Burns), seeded cases
over TEXT_LENS x NONCE_LENS x three key sizes (every plaintext is a prefix of "text", every key of a size is "keys"[size]),
and for one flipped bit in each of text, mac and nonce what the reference's decryption returns and leaves in a prefilled
output buffer.
"""
import ctypes as C
import json
import os
import random
import re
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "eaxp_vectors.json")
TEXT_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257)
NONCE_LENS = (0, 1, 15, 16, 17, 33, 50, 65)
FORGED_SHAPES = ((33, 17), (17, 65))            # (text, nonce) lengths of the forged cases
PREFILL = 0x5C

MAIN_C = [  # main.c:322-349
    {"what": "IEEE 1703-2012 Annex G", "bits": 128, "key": "01020304050607080102030405060708",
     "nonce": "A20D060B607C86F7540116007BC175A803020100BE0D280B810984A60C060A607C86F7540116007B040248F3C20403300005",
     "pt": "", "out": "515AE775"},
    {"what": "Moise-Beroset-Phinney-Burns", "bits": 128, "key": "102030405060708090a0b0c0d0e0f000",
     "nonce": "a20e060c6086480186fc2f811caa4e01a806020439a00ebbac0fa20da00ba10980010081044bcee2c3be25282381218"
              "8a60a06082b06010401828563004bcee2c3",
     "pt": "17513030303030303030303030303030303030303030000003300001",
     "out": "9cf32c7ec24c250be7b0749feee71a220d0eee976ec23dbf0caa08ea00543e66"},
]


def reference_checkout():
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        m = re.search(r"^REF\s*\?=\s*(\S+)", f.read(), re.M)
    ref = os.environ.get("REF") or (m.group(1) if m else "")
    if not ref or not os.path.exists(os.path.join(ref, "micro_aes.c")):
        raise SystemExit("no reference checkout (set REF)")
    return ref


def build(ref, tmp, bits):
    d = os.path.join(tmp, str(bits))
    os.mkdir(d)
    with open(os.path.join(d, "micro_aes.h"), "w") as h:
        subprocess.run(["sed", "-e", "s/^#define AES___ .*/#define AES___     %d/" % bits,
                        "-e", "s/^#define EAXP         0 /#define EAXP         1 /",
                        os.path.join(ref, "micro_aes.h")], check=True, stdout=h)
    with open(os.path.join(d, "micro_aes.h")) as h:
        text = h.read()
    assert re.search(r"^#define AES___     %d$" % bits, text, re.M), "the key-size sed did not hit"
    assert re.search(r"^#define EAXP         1 ", text, re.M), "the EAXP sed did not hit"
    assert re.search(r"^#define EAX          1 ", text, re.M), "the reference's EAX switch is off"
    os.symlink(os.path.join(ref, "micro_aes.c"), os.path.join(d, "micro_aes.c"))
    so = os.path.join(d, "libref_eaxp.so")
    subprocess.run(["gcc", "-O2", "-w", "-fPIC", "-shared", "-o", so, os.path.join(d, "micro_aes.c")], check=True)
    lib = C.CDLL(so)
    for n in ("AES_EAX_encrypt", "AES_EAX_decrypt"):            # the EAXP parameter list: nonceLen, no aData
        getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.AES_EAX_encrypt.restype = None
    lib.AES_EAX_decrypt.restype = C.c_char
    return lib


def buf(b, n=None):
    b = bytes(b)
    n = max(len(b) if n is None else n, 1)
    return (C.c_uint8 * n).from_buffer_copy(b.ljust(n, b"\0"))


def encrypt(lib, key, nonce, pt):
    o = buf(bytes([PREFILL]) * (len(pt) + 6))
    lib.AES_EAX_encrypt(buf(key), buf(nonce), len(nonce), buf(pt), len(pt), o)
    assert bytes(o)[len(pt) + 4:] == bytes([PREFILL]) * 2        # four bytes of mac and no more
    return bytes(o)[:len(pt) + 4]


def decrypt(lib, key, nonce, out):
    n = len(out) - 4
    o = buf(bytes([PREFILL]) * (n + 2))
    rc = lib.AES_EAX_decrypt(buf(key), buf(nonce), len(nonce), buf(out), n, o)
    assert bytes(o)[n:] == bytes([PREFILL]) * 2
    return ord(rc), bytes(o)[:n]


def flip(b, i):
    b = bytearray(b)
    b[(i // 8) % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def main():
    ref = reference_checkout()
    tmp = tempfile.mkdtemp(prefix="eaxp_fixtures_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    text = random.Random(1703).randbytes(max(TEXT_LENS))
    keys, entries, forged = {}, [], []
    try:
        for bits in (128, 192, 256):
            lib = build(ref, tmp, bits)
            rng = random.Random(1703 + bits)
            key = keys[str(bits)] = rng.randbytes(bits // 8)
            if bits == 128:
                for v in MAIN_C:
                    k, nonce, pt, out = (bytes.fromhex(v[f]) for f in ("key", "nonce", "pt", "out"))
                    assert encrypt(lib, k, nonce, pt) == out and decrypt(lib, k, nonce, out) == (0, pt), v["what"]
            for nl in NONCE_LENS:
                for n in TEXT_LENS:
                    nonce = rng.randbytes(nl)
                    out = encrypt(lib, key, nonce, text[:n])
                    assert decrypt(lib, key, nonce, out) == (0, text[:n]), (bits, nl, n)
                    entries.append({"bits": bits, "nonce": nonce.hex(), "n": n, "out": out.hex()})
            for n, nl in FORGED_SHAPES:
                nonce = rng.randbytes(nl)
                out = encrypt(lib, key, nonce, text[:n])
                for what, fn, fo in (("text", nonce, flip(out, rng.randrange(8 * n))),
                                     ("mac", nonce, flip(out, 8 * n + rng.randrange(32))),
                                     ("nonce", flip(nonce, rng.randrange(8 * nl)), out)):
                    rc, left = decrypt(lib, key, fn, fo)
                    forged.append({"what": what, "bits": bits, "nonce": fn.hex(), "n": n, "out": fo.hex(), "prefill": PREFILL,
                                   "code": rc, "left": left.hex()})
    finally:
        shutil.rmtree(tmp)
    with open(OUT, "w") as f:
        json.dump({"source": "the reference compiled with EAXP 1 (tests/golden/make_eaxp_fixtures.py)",
                   "main_c": MAIN_C, "text": text.hex(), "keys": {b: k.hex() for b, k in keys.items()},
                   "entries": entries, "forged": forged}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d entries, %d forged -> %s (%d bytes)" % (len(entries), len(forged), OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
