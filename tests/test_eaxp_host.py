"""EAX' (ANSI C12.22 / IEEE 1703; uaes_eaxp_*, AES_EAXP_*) without a GPU: the composition of tests/eaxp_ref.py against
every recorded answer of the reference built with EAXP 1, the engine's host path (forced on with uaes.host_policy,
restored after) against the same answers and its recorded forgeries, every argument the calls refuse before a device is
touched, the drop-in header under -DEAX=1 -DEAXP=1, the declarations and the plan rows."""
import ctypes as C
import os
import subprocess

import pytest

import micro_aes_amd as uaes
from tests import eaxp_ref as X
from tests import key_wipe_cases as kw
from tests.test_abi_and_host import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_HIP, AUTH = -2, -1, 0x1A
NAMES = ["uaes_eaxp_encrypt", "uaes_eaxp_decrypt", "uaes_eaxp_encrypt_batch", "uaes_eaxp_decrypt_batch", "uaes_debug_plan_eaxp"]
ENTRIES, FORGED = list(X.entries()), list(X.forged())


@pytest.fixture
def host_forced():
    prev = uaes.host_policy(1 << 62, 1, 1)
    yield
    uaes.host_policy(*prev)


def test_the_fixture_file_holds_what_it_should():
    assert [e[0] for e in ENTRIES[:2]] == ["IEEE 1703-2012 Annex G", "Moise-Beroset-Phinney-Burns"]
    seeded = {(bits, len(nonce), len(pt)) for what, bits, _, nonce, pt, _ in ENTRIES if what == "seeded"}
    assert seeded == {(b, nl, n) for b in (128, 192, 256) for nl in (0, 1, 15, 16, 17, 33, 50, 65)
                      for n in (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257)}
    assert {(what, bits) for what, bits, *_ in FORGED} == {(w, b) for w in ("text", "mac", "nonce") for b in (128, 192, 256)}
    assert all(code == AUTH and set(left) <= {prefill} for *_, prefill, code, left in FORGED)
    assert os.path.getsize(X.GOLDEN) < 128 << 10


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_the_composition_equals_the_reference(bits):
    for what, b, key, nonce, pt, out in ENTRIES:
        if b == bits:
            assert X.encrypt(bits, key, nonce, pt) == out, (what, len(nonce), len(pt))
            assert X.decrypt(bits, key, nonce, out) == (0, pt), (what, len(nonce), len(pt))
    for what, b, key, nonce, out, prefill, code, left in FORGED:
        if b == bits:
            assert X.decrypt(bits, key, nonce, out, prefill) == (code, left), what


def test_nonce_for():
    for bits in (128, 192, 256):
        key, target = bytes(range(bits // 8)), bytes(range(0xF0, 0x100))
        nonce = X.nonce_for(bits, key, target)
        d, _ = X.subkeys(bits, key)
        assert X.cmac_prime(bits, key, d, nonce) == target


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_the_host_path_equals_the_reference(host_forced, bits):
    for what, b, key, nonce, pt, out in ENTRIES:
        if b == bits:
            assert uaes.eaxp_encrypt(key, nonce, pt) == out, (what, len(nonce), len(pt))
            assert uaes.eaxp_decrypt(key, nonce, out, prefill=0x33) == (0, pt), (what, len(nonce), len(pt))


def test_the_host_path_fails_as_recorded_on_forgeries(host_forced):
    eng = uaes.engine()
    for wipe in (0, 1):
        eng.uaes_set_wipe_on_auth_failure(wipe)
        try:
            for what, bits, key, nonce, out, prefill, code, left in FORGED:
                assert uaes.eaxp_decrypt(key, nonce, out, prefill=prefill) == (code, left), (what, bits, wipe)
        finally:
            eng.uaes_set_wipe_on_auth_failure(0)


def test_the_host_path_in_place_and_with_no_nonce_pointer(host_forced):
    L = uaes.engine()
    _, bits, key, nonce, pt, out = next(e for e in ENTRIES if e[0] == "seeded" and len(e[3]) == 0 and len(e[4]) == 33)
    io = (C.c_uint8 * 64).from_buffer_copy(pt.ljust(64, b"\xEE"))
    assert L.uaes_eaxp_encrypt(bits, key, None, 0, io, 33, io) == 0 and bytes(io)[:37] == out and set(bytes(io)[37:]) == {0xEE}
    assert L.uaes_eaxp_decrypt(bits, key, None, 0, io, 33, io) == 0 and bytes(io)[:33] == pt
    # an empty text: nothing is read, four bytes are written; the decryption needs no output
    _, bits, key, nonce, pt, out = next(e for e in ENTRIES if e[0] == "seeded" and len(e[3]) == 17 and len(e[4]) == 0)
    o = (C.c_uint8 * 8)()
    assert L.uaes_eaxp_encrypt(bits, key, nonce, 17, None, 0, o) == 0 and bytes(o) == out + bytes(4)
    assert L.uaes_eaxp_decrypt(bits, key, nonce, 17, out, 0, None) == 0
    assert L.uaes_eaxp_decrypt(bits, key, nonce, 17, bytes(4), 0, None) == AUTH


# ---- arguments ----------------------------------------------------------------------------------------------------------
KEY = bytes(range(1, 33))


def test_refused_single_calls():
    L = uaes.engine()
    B = (C.c_uint8 * 64)()
    for fn in (L.uaes_eaxp_encrypt, L.uaes_eaxp_decrypt):
        assert fn(128, None, B, 16, B, 16, B) == E_ARG                                  # key
        assert fn(100, KEY, B, 16, B, 16, B) == E_ARG                                   # keybits
        assert fn(128, KEY, None, 16, B, 16, B) == E_ARG                                # nonce
        assert fn(128, KEY, B, 16, None, 16, B) == E_ARG                                # input
        assert fn(128, KEY, B, 16, B, 16, None) == E_ARG                                # output
    assert L.uaes_eaxp_encrypt(128, KEY, B, 16, None, 0, None) == E_ARG                 # nowhere to put the mac
    assert L.uaes_eaxp_decrypt(128, KEY, B, 16, None, 0, None) == E_ARG                 # no mac to read
    assert L.uaes_last_error()


def batch_calls(nmsg=2, nonce_bytes=16, nlens=None, msg_bytes=16, lens=None, bits=128, key=KEY, nonces=True, src=True, dst=True,
                macs=True, verdicts=True):
    """(encrypt's code, decrypt's code) for one set of arguments; True = a buffer that is large enough, None = NULL"""
    L = uaes.engine()
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))() if on else None)             # noqa: E731
    small = nmsg if nmsg < 1 << 16 else 1                                        # (a refused call reads nothing)
    room = lambda each: small * each if each < 1 << 20 else 1                   # noqa: E731
    a = (bits, key, nmsg, nonce_bytes, nlens, buf(nonces, room(nonce_bytes)), msg_bytes, lens, buf(src, room(msg_bytes)))
    enc = L.uaes_eaxp_encrypt_batch(*a, buf(dst, room(msg_bytes)), buf(macs, small * 4))
    dec = L.uaes_eaxp_decrypt_batch(*a, buf(macs, small * 4), buf(dst, room(msg_bytes)), buf(verdicts, small))
    return enc, dec


u32 = lambda *v: (C.c_uint32 * len(v))(*v)                                       # noqa: E731
REFUSED = [("text slot too wide", dict(msg_bytes=1 << 32)), ("nonce slot too wide", dict(nonce_bytes=1 << 32)),
           ("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("count overflows", dict(nmsg=(1 << 64) - 1, msg_bytes=0, nonce_bytes=0)),
           ("nonces overflow", dict(nmsg=(1 << 64) // 24 + 1, msg_bytes=0, nonce_bytes=24)),
           ("lengths overflow", dict(nmsg=(1 << 64) // 4, msg_bytes=0, nonce_bytes=0, lens=u32(0, 0))),
           ("NULL key", dict(key=None)), ("bad keybits", dict(bits=129)), ("NULL nonces", dict(nonces=None)),
           ("NULL input", dict(src=None)), ("NULL output", dict(dst=None)), ("NULL macs", dict(macs=None)),
           ("text length above its slot", dict(lens=u32(16, 17))), ("nonce length above its slot", dict(nlens=u32(17, 0))),
           ("nonce length without a slot", dict(nonce_bytes=0, nonces=None, nlens=u32(0, 1)))]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_batches(case):
    assert batch_calls(**case[1]) == (E_ARG, E_ARG), case
    assert uaes.engine().uaes_last_error()


def test_an_empty_batch_and_what_reaches_the_device():
    import torch
    assert batch_calls(nmsg=0) == (0, 0)
    assert batch_calls(nmsg=0, nonces=None, src=None, dst=None, macs=None, verdicts=None, lens=u32(99), nlens=u32(99)) == (0, 0)
    assert batch_calls(nmsg=0, msg_bytes=1 << 32) == (E_ARG, E_ARG) and batch_calls(nmsg=0, key=None) == (E_ARG, E_ARG)
    if not torch.cuda.is_available():
        # accepted arguments get as far as the device (UAES_E_HIP: no usable device): NULL verdicts, no nonce slot, records of
        # no bytes, lengths at their slots; the batches have no host path
        prev = uaes.host_policy(1 << 62, 1, 1)
        try:
            for ok in (dict(), dict(verdicts=None), dict(nonce_bytes=0, nonces=None), dict(msg_bytes=0, src=None, dst=None),
                       dict(lens=u32(16, 0), nlens=u32(0, 16)), dict(nonce_bytes=0, nonces=None, nlens=u32(0, 0))):
                assert batch_calls(**ok) == (E_HIP, E_HIP), ok
        finally:
            uaes.host_policy(*prev)


def test_no_refused_call_leaves_a_key_schedule_behind(host_forced):
    B = kw.buf()
    for name in ("uaes_eaxp_encrypt", "uaes_eaxp_decrypt"):
        kw.checked(name, (128, KEY, None, 16, B, 16, B), kw.ARG)                        # behind the key's expansion
        kw.checked(name, (192, KEY, B, 16, B, 16, None), kw.ARG)
    kw.checked("uaes_eaxp_encrypt_batch", (128, KEY, 1, 16, None, B, 16, None, None, B, B), kw.ARG)
    kw.checked("uaes_eaxp_decrypt_batch", (128, KEY, 1, 16, None, B, 16, None, None, B, B, B), kw.ARG)
    kw.checked("uaes_eaxp_encrypt_batch", (128, KEY, 2, 16, None, B, 16, u32(3, 17), B, B, B), kw.ARG)
    kw.checked("uaes_eaxp_encrypt_batch", (256, KEY, 0, 16, None, None, 16, None, None, None, None), kw.OK)
    pt, ct, out = kw.text(17), kw.buf(21), kw.buf(21)
    kw.checked("uaes_eaxp_encrypt", (256, KEY, b"header", 6, pt, 17, ct), kw.OK)
    assert bytes(ct) == X.encrypt(256, KEY, b"header", pt)
    kw.checked("uaes_eaxp_decrypt", (256, KEY, b"header", 6, ct, 17, out), kw.OK)
    ct[20] ^= 1
    kw.checked("uaes_eaxp_decrypt", (256, KEY, b"header", 6, ct, 17, out), kw.AUTH)


# ---- declarations, wrappers, plan -----------------------------------------------------------------------------------------
def test_declared_and_mirrored():
    names = declared_functions("uaes_hip.h")
    L = uaes.engine()
    for n in NAMES:
        assert n in names and n in uaes.EXPORTS and getattr(L, n), n
    assert uaes.eaxp_encrypt_batch(KEY, [], []) == ([], [])
    assert uaes.eaxp_decrypt_batch(KEY, [], [], []) == (0, [], [])
    with pytest.raises(ValueError):
        uaes.eaxp_encrypt_batch(KEY, [bytes(16)], [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.eaxp_encrypt_batch(KEY, [bytes(16), bytes(15)], [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.eaxp_decrypt_batch(KEY, [bytes(16)], [b"x"], [b"123"])
    with pytest.raises(ValueError):
        uaes.eaxp_decrypt(KEY, b"", b"123")


def test_the_plan_without_a_device():
    small = uaes.eaxp_plan(0)[3]
    assert small == uaes.eax_siv_plan(False, 0)[3] == 16384
    for dec in (False, True):
        assert uaes.eaxp_plan(small, decrypt=dec)[:2] == ("eaxp.small", 1)
        assert uaes.eaxp_plan(small + 1, decrypt=dec)[:2] == ("eaxp.long", 2 if dec else 3)
        assert uaes.eaxp_plan(64, 1 << 20, decrypt=dec)[:3] == ("eaxp.batch", 1, uaes.eax_siv_plan(False, 64, 1 << 20)[2])
    assert uaes.engine().uaes_debug_plan_eaxp(2, 16, 1, None) is None
    assert uaes.eax_siv_plan(False, 16)[0] == "eax.small"                               # the rows before it keep their ids


def test_drop_in_header_switches(tmp_path):
    """a C89 caller built with -DEAX=1 -DEAXP=1 sees the reference's EAX' parameter lists and links to AES_EAXP_*"""
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "e.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "micro_aes.h"\n'
                   "#if EAX != 1 || EAXP != 1\n#error switch\n#endif\n"
                   "#ifdef EAX_NONCE_LEN\n#error the EAX lengths are compiled out\n#endif\n"
                   "void (*volatile ee)(const uint8_t *, const uint8_t *, const size_t, const void *, const size_t, void *)"
                   " = AES_EAX_encrypt;\n"
                   "char (*volatile ed)(const uint8_t *, const uint8_t *, const size_t, const void *, const size_t, void *)"
                   " = AES_EAX_decrypt;\n"
                   "int main(void) { return ee == 0 || ed == 0; }\n")
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-DEAX=1", "-DEAXP=1", "-I", inc, "-c", str(src), "-o",
                    str(tmp_path / "e.o")], check=True)
    libdir = os.path.dirname(uaes.lib_path())
    for bits in (128, 192, 256):
        exe = tmp_path / ("e%d" % bits)
        subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-DEAX=1", "-DEAXP=1", "-DAES___=%d" % bits, "-I", inc,
                        str(src), "-o", str(exe), "-L", libdir, "-lmicro_aes_hip_%d" % bits, "-Wl,-rpath," + libdir], check=True)
        out = subprocess.run(["nm", "-u", str(exe)], check=True, capture_output=True, text=True).stdout
        assert "AES_EAXP_encrypt" in out and "AES_EAXP_decrypt" in out and "AES_EAX_encrypt" not in out
        lib = C.CDLL(uaes.lib_path("libmicro_aes_hip_%d.so" % bits))
        for name in ("AES_EAXP_encrypt", "AES_EAXP_decrypt", "AES_EAX_encrypt", "AES_EAX_decrypt"):
            assert getattr(lib, name) is not None
    # EAXP without EAX declares nothing, as in the reference (micro_aes.h:359)
    alone = tmp_path / "a.c"
    alone.write_text('#include "micro_aes.h"\n#if EAX != 0 || EAXP != 1\n#error switch\n#endif\n'
                     "int AES_EAX_encrypt = 1, AES_EAXP_encrypt = 2;\nint main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-DEAXP=1", "-I", inc, "-c", str(alone), "-o",
                    str(tmp_path / "a.o")], check=True)


def test_the_drop_in_library_on_the_host_path(host_forced):
    for what, bits, key, nonce, pt, out in ENTRIES[:2] + [e for e in ENTRIES if (len(e[3]), len(e[4])) == (33, 257)]:
        lib = C.CDLL(uaes.lib_path("libmicro_aes_hip_%d.so" % bits))
        lib.AES_EAXP_encrypt.argtypes = lib.AES_EAXP_decrypt.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.AES_EAXP_encrypt.restype, lib.AES_EAXP_decrypt.restype = None, C.c_char
        o, back = (C.c_uint8 * (len(pt) + 4))(), (C.c_uint8 * max(len(pt), 1))()
        lib.AES_EAXP_encrypt(key, nonce, len(nonce), pt, len(pt), o)
        assert bytes(o) == out, (what, bits)
        assert ord(lib.AES_EAXP_decrypt(key, nonce, len(nonce), out, len(pt), back)) == 0 and bytes(back)[:len(pt)] == pt
        bad = bytes([out[0] ^ 1]) + out[1:]                                              # a bit of the text, or of a lone mac
        assert ord(lib.AES_EAXP_decrypt(key, nonce, len(nonce), bad, len(pt), back)) == AUTH
