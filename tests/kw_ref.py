"""RFC 3394 key wrap answers of the compiled reference (oracle/_ref, through tests/refbuilt.need()): the default builds
libmicroaes_ref_<bits>.so have KWA 1 and export AES_KEY_wrap / AES_KEY_unwrap (micro_aes.c:1829-1894).  Shared by
tests/test_kw_host.py and tests/test_gpu_kw.py."""
import ctypes as C
import json
import os

from tests import refbuilt

_libs = {}


def ref(bits):
    if bits not in _libs:
        lib = C.CDLL(refbuilt.need("libmicroaes_ref_%d.so" % bits))
        for n in ("AES_KEY_wrap", "AES_KEY_unwrap"):
            getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, n).restype = C.c_char
        _libs[bits] = lib
    return _libs[bits]


def _buf(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def _call(fn, kek, data, out_len, prefill):
    o = (C.c_uint8 * max(out_len, 1))()
    C.memset(o, prefill, max(out_len, 1))
    rc = fn(_buf(kek), _buf(data), len(data), o)
    return ord(rc), bytes(o)[:out_len]


def wrap(kek, secret, prefill=0):
    """the reference's AES_KEY_wrap: (return code, the len(secret) + 8 bytes of its output buffer)"""
    return _call(ref(len(kek) * 8).AES_KEY_wrap, kek, secret, len(secret) + 8, prefill)


def unwrap(kek, wrapped, prefill=0):
    """the reference's AES_KEY_unwrap: (return code, the len(wrapped) - 8 bytes of its output buffer)"""
    return _call(ref(len(kek) * 8).AES_KEY_unwrap, kek, wrapped, max(len(wrapped) - 8, 0), prefill)


def rfc3394(golden_dir):
    """the six parameter sets of RFC 3394 section 4 (tests/golden/kw_rfc3394.json): dicts of kek, secret, wrapped"""
    with open(os.path.join(golden_dir, "kw_rfc3394.json")) as f:
        return [{k: bytes.fromhex(v) if isinstance(v, str) else v for k, v in case.items()} for case in json.load(f)]


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def forgeries(kek, wrapped):
    """(kek, wrapped) pairs that must not authenticate: a bit flipped in A, in the first, a middle and the last semiblock,
    and in the key-encryption key"""
    n = len(wrapped) // 8 - 1
    return [(kek, flip(wrapped, 5)), (kek, flip(wrapped, 64 + 9)), (kek, flip(wrapped, 64 * (1 + n // 2) + 33)),
            (kek, flip(wrapped, 8 * len(wrapped) - 2)), (flip(kek, 17), wrapped)]
