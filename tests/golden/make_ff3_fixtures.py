#!/usr/bin/env python3
"""Records tests/golden/ff3_ref_vectors.json: what the reference gives for FF3-1 when it is compiled with FF_X 3.

For the build container only (it needs the reference checkout that oracle/Makefile names as REF, or $REF); the tests
read the recorded file and never run this.  The reference is built at 128 / 192 / 256 bits in a temporary directory
outside the repository, from a copy of its header with two lines changed by sed (both checked to have hit) and links to
micro_aes.c and micro_fpe.h, the way oracle/Makefile builds its variants; the directory is removed afterwards.  The
recorded file is data only: keys, tweaks, decimal strings, return codes.

    python3 tests/golden/make_ff3_fixtures.py
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
OUT = os.path.join(HERE, "ff3_ref_vectors.json")
FOURTH = [0x0F, 0xF0, 0xFF, 0xA5]
PREFILL = 0x5C


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
                        "-e", "s/^#define FF_X            1 /#define FF_X            3 /",
                        os.path.join(ref, "micro_aes.h")], check=True, stdout=h)
    with open(os.path.join(d, "micro_aes.h")) as h:
        text = h.read()
    assert re.search(r"^#define AES___     %d$" % bits, text, re.M), "the key-size sed did not hit"
    assert re.search(r"^#define FF_X            3 ", text, re.M), "the FF_X sed did not hit"
    for f in ("micro_aes.c", "micro_fpe.h"):
        os.symlink(os.path.join(ref, f), os.path.join(d, f))
    so = os.path.join(d, "libref_ff3.so")
    subprocess.run(["gcc", "-O2", "-w", "-fPIC", "-shared", "-o", so, os.path.join(d, "micro_aes.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    for n in ("AES_FPE_encrypt", "AES_FPE_decrypt"):           # the FF_X 3 parameter list: no tweakLen
        getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        getattr(lib, n).restype = C.c_char
    return lib


def call(lib, name, key, tweak, text, prefill=PREFILL):
    n = len(text) + 2
    o = (C.c_uint8 * n)()
    C.memset(o, prefill, n)
    k = (C.c_uint8 * len(key)).from_buffer_copy(key)
    t = (C.c_uint8 * 7).from_buffer_copy(tweak)
    x = (C.c_uint8 * (len(text) + 1)).from_buffer_copy(text + b"\0")
    rc = getattr(lib, name)(k, t, x, len(text), o)
    return ord(rc), bytes(o)


def main():
    ref = reference_checkout()
    tmp = tempfile.mkdtemp(prefix="ff3_fixtures_")
    assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
    entries, refusals = [], []
    try:
        for bits in (128, 192, 256):
            lib = build(ref, tmp, bits)
            rng = random.Random(3000 + bits)

            def record(what, key, tweak, pt):
                rc, o = call(lib, "AES_FPE_encrypt", key, tweak, pt)
                assert rc == 0 and o[len(pt):] == bytes([0, PREFILL]), (what, rc)
                ct = o[:len(pt)]
                assert call(lib, "AES_FPE_decrypt", key, tweak, ct) == (0, pt + bytes([0, PREFILL])), what
                entries.append({"what": what, "bits": bits, "key": key.hex(), "tweak": tweak.hex(),
                                "pt": pt.decode(), "ct": ct.decode()})

            for n in range(6, 57):
                record("seeded", rng.randbytes(bits // 8), rng.randbytes(7), bytes(rng.choice(b"0123456789") for _ in range(n)))
            for b3 in FOURTH:
                tweak = bytearray(rng.randbytes(7))
                tweak[3] = b3
                for n in (10, 19):
                    record("tweak[3]=%02x" % b3, rng.randbytes(bits // 8), bytes(tweak), bytes(rng.choice(b"0123456789") for _ in range(n)))
            for n in (6, 7, 55, 56):
                for ch in (b"0", b"9"):
                    record("all-" + ch.decode(), rng.randbytes(bits // 8), rng.randbytes(7), ch * n)
            if bits == 128:
                key, tweak = rng.randbytes(16), rng.randbytes(7)
                for what, text in (("length 5", b"12345"), ("length 57", b"123456789" * 6 + b"123"), ("foreign character", b"1234567x90")):
                    e = call(lib, "AES_FPE_encrypt", key, tweak, text)
                    d = call(lib, "AES_FPE_decrypt", key, tweak, text)
                    refusals.append({"what": what, "bits": bits, "key": key.hex(), "tweak": tweak.hex(), "text": text.hex(),
                                     "prefill": PREFILL, "encrypt_code": e[0], "decrypt_code": d[0],
                                     "encrypt_out": e[1].hex(), "decrypt_out": d[1].hex()})
    finally:
        shutil.rmtree(tmp)
    with open(OUT, "w") as f:
        json.dump({"source": "the reference compiled with FF_X 3 (tests/golden/make_ff3_fixtures.py)",
                   "entries": entries, "refusals": refusals}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d entries, %d refusals -> %s (%d bytes)" % (len(entries), len(refusals), OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
