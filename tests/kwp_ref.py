"""A model of AES key wrap with padding written from RFC 5649 (sections 3, 4.1, 4.2) on the single-block cipher of the
compiled reference: AES_ECB_encrypt / AES_ECB_decrypt of libmicroaes_ref_<bits>.so (oracle/_ref, through
tests/refbuilt.need()), as tests/kw_ref.py does for RFC 3394.  The reference has no KWP, so the second source of truth
is tests/golden/kwp_vectors.json: the RFC's two vectors and outputs of the OpenSSL command-line tool
(tests/golden/make_kwp_fixtures.py).  Shared by tests/test_kwp_host.py and tests/test_gpu_kwp.py."""
import ctypes as C
import json
import os
import struct

from tests import refbuilt
from tests.kw_ref import flip  # noqa: F401  (the tests use it beside this module's own forgeries)

ICV2 = bytes.fromhex("A65959A6")
AUTH = 0x1A
_libs = {}


def _lib(bits):
    if bits not in _libs:
        lib = C.CDLL(refbuilt.need("libmicroaes_ref_%d.so" % bits))
        lib.AES_ECB_encrypt.argtypes = lib.AES_ECB_decrypt.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.AES_ECB_encrypt.restype = None
        lib.AES_ECB_decrypt.restype = C.c_char
        _libs[bits] = lib
    return _libs[bits]


def _block(kek, block, decrypt):
    assert len(block) == 16
    lib, o = _lib(len(kek) * 8), (C.c_uint8 * 16)()
    k, b = (C.c_uint8 * len(kek)).from_buffer_copy(kek), (C.c_uint8 * 16).from_buffer_copy(block)
    (lib.AES_ECB_decrypt if decrypt else lib.AES_ECB_encrypt)(k, b, 16, o)
    return bytes(o)


def wrap_raw(kek, A, padded):
    """RFC 5649 section 4.1 from its step 2 on with ANY 8-byte A and ANY whole semiblocks `padded`: one block for one
    semiblock, else RFC 3394's W (section 2.2.1) with A as the initial value.  What forgeries are crafted with."""
    assert len(A) == 8 and len(padded) % 8 == 0 and padded
    n = len(padded) // 8
    if n == 1:
        return _block(kek, A + padded, False)
    R = [padded[8 * i:8 * i + 8] for i in range(n)]
    for j in range(6):
        for i in range(n):
            B = _block(kek, A + R[i], False)
            A = bytes(x ^ y for x, y in zip(B[:8], struct.pack(">Q", n * j + i + 1)))
            R[i] = B[8:]
    return A + b"".join(R)


def unwrap_raw(kek, wrapped):
    """the inverse: (A, the whole semiblocks) of a wrapped form of 16 bytes or more"""
    assert len(wrapped) % 8 == 0 and len(wrapped) >= 16
    n = len(wrapped) // 8 - 1
    if n == 1:
        B = _block(kek, wrapped, True)
        return B[:8], B[8:]
    A, R = wrapped[:8], [wrapped[8 * i + 8:8 * i + 16] for i in range(n)]
    for j in range(5, -1, -1):
        for i in range(n - 1, -1, -1):
            B = _block(kek, bytes(x ^ y for x, y in zip(A, struct.pack(">Q", n * j + i + 1))) + R[i], True)
            A, R[i] = B[:8], B[8:]
    return A, b"".join(R)


def wrap(kek, secret):
    """the wrapped form of a secret of 1 .. 2^32 - 1 bytes"""
    assert 1 <= len(secret) < 1 << 32
    return wrap_raw(kek, ICV2 + struct.pack(">I", len(secret)), secret + bytes(-len(secret) % 8))


def unwrap(kek, wrapped):
    """(code, what the chain made -- len(wrapped) - 8 bytes --, length of the secret): code 0 and the MLI, or 0x1A and 0,
    by the three conditions of section 4.2 step 3"""
    A, P = unwrap_raw(kek, wrapped)
    mli = struct.unpack(">I", A[4:])[0]
    ok = A[:4] == ICV2
    ok &= len(P) - 8 < mli <= len(P)
    ok &= ok and not any(P[mli:])
    return (0, P, mli) if ok else (AUTH, P, 0)


def crafted(kek, secret):
    """[(name, wrapped form)]: forgeries of the classes RFC 5649's check has to refuse, made with wrap_raw for a secret
    whose padded form has n semiblocks -- a wrong constant (one bit, and RFC 3394's A6 x 8 over the same semiblocks, a
    valid KW wrapping for n >= 2), a length indicator of 0, 8 (n - 1), 8 n + 1 and 2^32 - 1, and a valid indicator with a
    non-zero byte at the first and at the last position of the zero fill (secret lengths with fewer than 8 n bytes)"""
    padded = secret + bytes(-len(secret) % 8)
    n, m = len(padded) // 8, len(secret)
    mk = lambda icv, mli, p=padded: wrap_raw(kek, icv + struct.pack(">I", mli & 0xFFFFFFFF), p)
    out = [("constant bit", mk(bytes.fromhex("A65959A7"), m)), ("kw constant", wrap_raw(kek, b"\xA6" * 8, padded)),
           ("mli 0", mk(ICV2, 0)), ("mli 8(n-1)", mk(ICV2, 8 * (n - 1))), ("mli 8n+1", mk(ICV2, 8 * n + 1)),
           ("mli 2^32-1", mk(ICV2, 0xFFFFFFFF))]
    if m < 8 * n:
        first, last = bytearray(padded), bytearray(padded)
        first[m], last[-1] = 0x01, 0x80
        out += [("pad first", mk(ICV2, m, bytes(first))), ("pad last", mk(ICV2, m, bytes(last)))]
    return out


def flipped(kek, wrapped):
    """(kek, wrapped) pairs with one bit flipped: in A, in a middle semiblock, in the last semiblock and in the key
    (kw_ref.forgeries' positions; a 16-byte form has no middle semiblock)"""
    n = len(wrapped) // 8 - 1
    out = [(kek, flip(wrapped, 5)), (kek, flip(wrapped, 8 * len(wrapped) - 2)), (flip(kek, 17), wrapped)]
    if n >= 2:
        out.append((kek, flip(wrapped, 64 * (1 + n // 2) + 33)))
    return out


def fixtures(golden_dir):
    """tests/golden/kwp_vectors.json: dicts of source, kek, secret, wrapped"""
    with open(os.path.join(golden_dir, "kwp_vectors.json")) as f:
        return [{k: bytes.fromhex(v) if k in ("kek", "secret", "wrapped") else v for k, v in case.items()}
                for case in json.load(f)["vectors"]]
