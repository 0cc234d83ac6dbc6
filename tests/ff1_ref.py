"""FF1 (SP 800-38G) answers for tests/test_ff1_host.py and tests/test_gpu_ff1.py, from two independent sources:
the compiled reference (oracle/_ref through tests/refbuilt.need(): the default builds libmicroaes_ref_<bits>.so have
FPE 1, FF_X 1 and the decimal alphabet, micro_aes.c:2267-2347) and a plain-Python FF1 written from the specification,
whose AES is the oracle's ECB and whose b is exact.  The model is the checker for other radices and for the lengths at
which the reference's floating-point b is one too large (v log2(radix) a multiple of 8 at 136 bits or more)."""
import ctypes as C
import os
import random

from tests import refbuilt

VECTOR_FILE = "FPE_FF1&FF3&FF3-1.tv"
DECIMAL = b"0123456789"
_libs = {}


def ref(bits):
    if bits not in _libs:
        lib = C.CDLL(refbuilt.need("libmicroaes_ref_%d.so" % bits))
        for n in ("AES_FPE_encrypt", "AES_FPE_decrypt"):
            getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, n).restype = C.c_char
        _libs[bits] = lib
    return _libs[bits]


def buf(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def fpe_call(lib, name, key, tweak, text, prefill=0, extra=2):
    """char AES_FPE_*(key, tweak, tweakLen, in, len, out) of a library: (code, len(text) + extra bytes of the output
    buffer, which was filled with `prefill`)"""
    n = len(text) + extra
    o = (C.c_uint8 * n)()
    C.memset(o, prefill, n)
    rc = getattr(lib, name)(buf(key), buf(tweak), len(tweak), buf(text), len(text), o)
    return ord(rc), bytes(o)


def ref_encrypt(key, tweak, text):
    """the reference's AES_FPE_encrypt on a decimal string: (code, ciphertext)"""
    rc, o = fpe_call(ref(len(key) * 8), "AES_FPE_encrypt", key, tweak, text)
    return rc, o[:len(text)]


def ref_decrypt(key, tweak, text):
    rc, o = fpe_call(ref(len(key) * 8), "AES_FPE_decrypt", key, tweak, text)
    return rc, o[:len(text)]


def minlen(radix):
    n = 1
    while radix ** n < 1000000:
        n += 1
    return n


def b_exact(radix, v):
    return ((radix ** v - 1).bit_length() + 7) // 8


def b_float(radix, v):
    """the reference's form (micro_aes.c:2283, LOGRDX = log2(radix))"""
    import math
    return int(math.log2(radix) * v + 8 - 1e-14) // 8


def _num(digits, radix):
    x = 0
    for d in digits:
        x = x * radix + d
    return x


def _str(x, radix, m):
    out = [0] * m
    for i in range(m - 1, -1, -1):
        x, out[i] = divmod(x, radix)
    return out


def model(orc, key, tweak, digits, radix, decrypt=False):
    """FF1.Encrypt / FF1.Decrypt of SP 800-38G, algorithms 7 and 8, on a list of digit values"""
    n, t = len(digits), len(tweak)
    u = n // 2
    v = n - u
    a, bb = list(digits[:u]), list(digits[u:])
    b = b_exact(radix, v)
    d = 4 * ((b + 3) // 4) + 4
    p = bytes([1, 2, 1]) + radix.to_bytes(3, "big") + bytes([10, u % 256]) + n.to_bytes(4, "big") + t.to_bytes(4, "big")

    def prf(x):
        y = bytes(16)
        for j in range(0, len(x), 16):
            y = orc.ecb_encrypt(key, bytes(s ^ w for s, w in zip(y, x[j:j + 16])))[:16]
        return y

    def f(i, half):
        q = bytes(tweak) + bytes((-t - b - 1) % 16) + bytes([i]) + _num(half, radix).to_bytes(b, "big")
        r = prf(p + q)
        s = r
        j = 1
        while len(s) < d:
            s += orc.ecb_encrypt(key, bytes(x ^ y for x, y in zip(r, j.to_bytes(16, "big"))))[:16]
            j += 1
        return int.from_bytes(s[:d], "big")

    if not decrypt:
        for i in range(10):
            m = u if i % 2 == 0 else v
            c = (_num(a, radix) + f(i, bb)) % radix ** m
            a, bb = bb, _str(c, radix, m)
    else:
        for i in range(9, -1, -1):
            m = u if i % 2 == 0 else v
            c = (_num(bb, radix) - f(i, a)) % radix ** m
            bb, a = a, _str(c, radix, m)
    return a + bb


def model_text(orc, key, tweak, text, alphabet, decrypt=False):
    """the model on a byte string out of `alphabet` (None: raw digit values; then radix must be given through
    model())"""
    alphabet = bytes(alphabet)
    idx = {c: i for i, c in enumerate(alphabet)}
    out = model(orc, key, tweak, [idx[c] for c in bytes(text)], len(alphabet), decrypt)
    return bytes(alphabet[d] for d in out)


_wave = {}


def wave_cases(orc, batch, top):
    """the one-text shapes that only the wave form takes, at the ends of the radix range: twelve of (radix, key, tweak,
    digits, the model's answer), one key size per case; made once for the GPU test and its host twin"""
    if (batch, top) not in _wave:
        rng = random.Random(64)
        cases = []
        for radix in (2, 255, 256):
            for n in (batch + 1, 1000, top - 1, top):
                key, tweak = rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(rng.choice([0, 3, 16, 21]))
                digits = bytes(rng.randrange(radix) for _ in range(n))
                cases.append((radix, key, tweak, digits, bytes(model(orc, key, tweak, list(digits), radix))))
        _wave[(batch, top)] = tuple(cases)
    return _wave[(batch, top)]


def vectors(golden_dir):
    """the FF1 vectors of the reference's file: dicts of alphabet, key, tweak, pt, ct (bytes)"""
    out, cur = [], {}
    with open(os.path.join(golden_dir, VECTOR_FILE), encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("#") or " = " not in line and not line.endswith(" ="):
                continue
            name, _, value = line.partition(" =")
            cur[name.strip()] = value.strip()
            if name.strip() == "CT":
                if cur.get("Method") == "FF1":
                    out.append({"alphabet": cur["Alphabet"].encode(), "key": bytes.fromhex(cur["Key"]),
                                "tweak": bytes.fromhex(cur["Tweak"]), "pt": cur["PT"].encode(), "ct": cur["CT"].encode()})
                cur = {}
    return out
