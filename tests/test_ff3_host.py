"""FF3-1 (SP 800-38G revision 1) without a GPU: the specification model of tests/ff3_ref.py against the FF3-1 stanzas of
the reference's vector file and against what the reference compiled with FF_X 3 gave (tests/golden/ff3_ref_vectors.json),
then the engine's host path (forced on with uaes.host_policy, restored after) and the compat libraries against the
same and against the model at other radices; uaes_ff3_maxlen, the planner without a device, the drop-in header's
AES_FF3_* declarations, and the refusals with the output checked against a prefill."""
import ctypes as C
import os
import random
import subprocess

import pytest

import micro_aes_amd as uaes
from tests import ff3_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DATALENGTH, E_DECRYPTION, E_ENCRYPTION = -2, 1, 0x1D, 0x1E


@pytest.fixture
def host_forced():
    prev = uaes.host_policy(max_bytes=1 << 30, chains=1)
    yield
    uaes.host_policy(*prev)


def buf(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def compat(name, key, tweak, text, alphabet=None, prefill=0, extra=2):
    """AES_FF3_<name> of libmicro_aes_hip_<bits>.so, or its _alpha form when an alphabet is given: (code, the
    len(text) + extra bytes of the output buffer)"""
    lib = uaes.compat(len(key) * 8)
    n = len(text) + extra
    o = (C.c_uint8 * n)()
    C.memset(o, prefill, n)
    if alphabet is None:
        rc = getattr(lib, "AES_FF3_" + name)(buf(key), buf(tweak), buf(text), len(text), o)
    else:
        rc = getattr(lib, "AES_FF3_%s_alpha" % name)(bytes(alphabet), len(alphabet), buf(key), buf(tweak), buf(text), len(text), o)
    return ord(rc), bytes(o)


def test_model_reproduces_the_vector_file(orc, golden_dir):
    vs = R.vectors(golden_dir)
    assert len(vs) == 22 and sorted(set(len(v["alphabet"]) for v in vs)) == [10, 26, 36, 64]
    assert sorted(set(len(v["pt"]) for v in vs)) == [10, 19, 28, 29, 40, 56] and sorted(set(len(v["key"]) for v in vs)) == [16, 24, 32]
    assert any((v["pt"], v["ct"]) == (b"3992520240", b"8901801106") for v in vs)
    for v in vs:
        assert R.model_text(orc, v["key"], v["tweak"], v["pt"], v["alphabet"]) == v["ct"], v
        assert R.model_text(orc, v["key"], v["tweak"], v["ct"], v["alphabet"], decrypt=True) == v["pt"], v


def test_model_reproduces_the_recorded_reference(orc, golden_dir):
    entries, refusals = R.fixtures(golden_dir)
    for bits in (128, 192, 256):
        mine = [e for e in entries if len(e["key"]) * 8 == bits]
        assert [len(e["pt"]) for e in mine if e["what"] == "seeded"] == list(range(6, 57))
        assert sorted(set(e["tweak"][3] for e in mine if e["what"].startswith("tweak"))) == [0x0F, 0xA5, 0xF0, 0xFF]
        for ch in b"09":
            assert sorted(len(e["pt"]) for e in mine if e["what"].startswith("all-") and set(e["pt"]) == {ch}) == [6, 7, 55, 56]
    for e in entries:
        assert R.model_text(orc, e["key"], e["tweak"], e["pt"], R.DECIMAL) == e["ct"], e
        assert R.model_text(orc, e["key"], e["tweak"], e["ct"], R.DECIMAL, decrypt=True) == e["pt"], e
    assert sorted(len(r["text"]) for r in refusals) == [5, 10, 57]
    for r in refusals:
        fill = bytes([r["prefill"]]) * (len(r["text"]) + 2)
        assert (r["encrypt_code"], r["encrypt_out"], r["decrypt_code"], r["decrypt_out"]) == (E_ENCRYPTION, fill, E_DECRYPTION, fill)


def test_vector_file_engine_and_compat(host_forced, golden_dir):
    for v in R.vectors(golden_dir):
        key, tweak, a = v["key"], v["tweak"], v["alphabet"]
        assert uaes.AES_FF3_encrypt(key, tweak, v["pt"], a) == (0, v["ct"]), v
        assert uaes.AES_FF3_decrypt(key, tweak, v["ct"], a) == (0, v["pt"]), v
        assert compat("encrypt", key, tweak, v["pt"], a, prefill=7) == (0, v["ct"] + b"\0\x07"), v
        assert compat("decrypt", key, tweak, v["ct"], a, prefill=7) == (0, v["pt"] + b"\0\x07"), v
        if a == R.DECIMAL:
            assert compat("encrypt", key, tweak, v["pt"], prefill=7) == (0, v["ct"] + b"\0\x07"), v
            assert compat("decrypt", key, tweak, v["ct"], prefill=7) == (0, v["pt"] + b"\0\x07"), v


def test_recorded_reference_engine_and_compat(host_forced, golden_dir):
    entries, refusals = R.fixtures(golden_dir)
    for e in entries:
        assert uaes.AES_FF3_encrypt(e["key"], e["tweak"], e["pt"]) == (0, e["ct"]), e
        assert uaes.AES_FF3_decrypt(e["key"], e["tweak"], e["ct"]) == (0, e["pt"]), e
        assert compat("encrypt", e["key"], e["tweak"], e["pt"], prefill=0x5C) == (0, e["ct"] + b"\0\x5C"), e
    for r in refusals:                                         # the compat layer gives the reference's code and buffer
        assert compat("encrypt", r["key"], r["tweak"], r["text"], prefill=r["prefill"]) == (r["encrypt_code"], r["encrypt_out"]), r
        assert compat("decrypt", r["key"], r["tweak"], r["text"], prefill=r["prefill"]) == (r["decrypt_code"], r["decrypt_out"]), r


@pytest.mark.parametrize("radix", [2, 3, 16, 95, 255, 256])
def test_radices_against_the_model(host_forced, orc, radix):
    rng = random.Random(radix)
    alphabet = bytes(rng.sample(range(256), radix))
    for n in range(R.minlen(radix), R.maxlen(radix) + 1):
        key, tweak = rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(7)
        digits = [rng.randrange(radix) for _ in range(n)]
        want = R.model(orc, key, tweak, digits, radix)
        case = (radix, n, key.hex(), tweak.hex())
        assert uaes.AES_FF3_encrypt(key, tweak, bytes(digits), None, radix) == (0, bytes(want)), case
        assert uaes.AES_FF3_decrypt(key, tweak, bytes(want), None, radix) == (0, bytes(digits)), case
        text, ct = bytes(alphabet[d] for d in digits), bytes(alphabet[d] for d in want)
        assert uaes.AES_FF3_encrypt(key, tweak, text, alphabet) == (0, ct), case
        assert uaes.AES_FF3_decrypt(key, tweak, ct, alphabet) == (0, text), case


def test_maxlen_is_exact():
    for radix in range(2, 257):
        assert uaes.ff3_maxlen(radix) == R.maxlen(radix), radix
        k = R.maxlen(radix) // 2
        assert radix ** k <= 1 << 96 < radix ** (k + 1), radix
    assert [uaes.ff3_maxlen(r) for r in (2, 10, 26, 36, 62, 64, 85, 95, 255, 256)] == [192, 56, 40, 36, 32, 32, 28, 28, 24, 24]
    assert [uaes.ff3_maxlen(r) for r in (0, 1, 257)] == [0, 0, 0]


def test_planner_without_a_device():
    eng = uaes.engine()
    for radix in range(2, 257):
        lo, hi = R.minlen(radix), R.maxlen(radix)
        for dec in (False, True):
            assert uaes.ff3_plan(lo, radix=radix, decrypt=dec) == ("ff3.batch", 1, 1, 64), radix
            assert uaes.ff3_plan(hi, radix=radix, decrypt=dec) == ("ff3.batch", 1, 1, 64), radix
            assert uaes.ff3_plan(lo - 1, radix=radix, decrypt=dec) is None and uaes.ff3_plan(hi + 1, radix=radix, decrypt=dec) is None, radix
            assert uaes.ff3_plan(lo - 1, 5, radix, dec) is None and uaes.ff3_plan(hi + 1, 5, radix, dec) is None, radix
            assert uaes.ff3_plan(hi, 5, radix, dec) == ("ff3.batch", 1, 1, 256), radix
    for args in ((2, 10, 16, 0), (-1, 10, 16, 0), (0, 1, 31, 0), (0, 0, 31, 0), (0, 257, 16, 0), (0, 257, 16, 9)):
        assert eng.uaes_debug_plan_ff3(*args, None) is None, args
    assert eng.uaes_debug_plan_ff3(0, 2, 192, 0, None) == b"ff3.batch" and eng.uaes_debug_plan_ff3(1, 256, 3, 5, None) == b"ff3.batch"
    for n in (1, 64, 65, 1 << 20):                             # the row batches' one launch shape
        assert uaes.ff3_plan(16, n)[2:] == uaes.ff1_plan(16, n)[2:], n
    assert uaes.ff3_plan(16, 1 << 20) == ("ff3.batch", 1, 256, 1024)          # a 256-CU part without a device


def gcc(tmp_path, name, text, *flags, ok=True):
    src = tmp_path / (name + ".c")
    src.write_text(text)
    r = subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                        "-I", str(tmp_path), "-c", str(src), "-o", str(tmp_path / (name + ".o"))], capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stderr


BIND = ('#include "micro_aes.h"\n'
        "char (*fe)(const uint8_t *, const uint8_t *, const void *, const size_t, void *) = AES_FF3_encrypt;\n"
        "char (*fd)(const uint8_t *, const uint8_t *, const void *, const size_t, void *) = AES_FF3_decrypt;\n"
        "char (*ae)(const char *, const size_t, const uint8_t *, const uint8_t *, const void *, const size_t, void *) = AES_FF3_encrypt_alpha;\n"
        "char (*ad)(const char *, const size_t, const uint8_t *, const uint8_t *, const void *, const size_t, void *) = AES_FF3_decrypt_alpha;\n"
        "int main(void) { return fe == 0 || fd == 0 || ae == 0 || ad == 0 || FF3_TWEAK_LEN != 7; }\n")


def test_drop_in_header_declares_ff3(tmp_path):
    gcc(tmp_path, "d", '#include "micro_aes.h"\nint AES_FF3_encrypt(int hidden) { return hidden; }\n'
        "int main(void) { return AES_FF3_encrypt(0); }\n")                     # FPE 0: the names are the caller's
    gcc(tmp_path, "k", BIND, "-DFPE=1")
    err = gcc(tmp_path, "x", BIND, "-DFPE=1", "-DFF_X=3", ok=False)           # the switch itself still stops the build
    assert "FF1" in err and "AES_FF3_" in err
    for bits in (128, 192, 256):
        lib = C.CDLL(uaes.lib_path("libmicro_aes_hip_%d.so" % bits))
        for n in ("AES_FF3_encrypt", "AES_FF3_decrypt", "AES_FF3_encrypt_alpha", "AES_FF3_decrypt_alpha"):
            assert getattr(lib, n) is not None


def test_drop_in_program_runs(tmp_path):
    """a C89 caller built with -DFPE=1 and linked to libmicro_aes_hip_128.so: the stanza 3992520240 -> 8901801106
    through AES_FF3_encrypt and back, on the host path"""
    (tmp_path / "m.c").write_text('#include <stdio.h>\n#include "micro_aes.h"\nint main(void) {\n'
                                  "  static const uint8_t key[16] = { 0x2D, 0xE7, 0x9D, 0x23, 0x2D, 0xF5, 0x58, 0x5D, 0x68, 0xCE, 0x47, 0x88,"
                                  " 0x2A, 0xE2, 0x56, 0xD6 };\n"
                                  "  static const uint8_t tweak[FF3_TWEAK_LEN] = { 0xCB, 0xD0, 0x92, 0x80, 0x97, 0x95, 0x64 };\n"
                                  "  char out[16], back[16], a, b;\n"
                                  '  a = AES_FF3_encrypt(key, tweak, "3992520240", 10, out);\n'
                                  "  b = AES_FF3_decrypt(key, tweak, out, 10, back);\n"
                                  '  printf("%d %d %s %s\\n", a, b, out, back);\n  return 0;\n}\n')
    libdir = os.path.dirname(uaes.lib_path())
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-O2", "-DFPE=1", "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), str(tmp_path / "m.c"), "-L", libdir, "-lmicro_aes_hip_128", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = dict(os.environ, UAES_HOST_POLICY="recommended")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, env=env, timeout=60).stdout
    assert out.split() == ["0", "0", "8901801106", "3992520240"], out


def test_refusals_leave_the_output_alone(host_forced):
    rng = random.Random(9)
    key, tweak = rng.randbytes(16), rng.randbytes(7)
    fill = bytes([0x5C])
    for name, fn, code in (("encrypt", uaes.AES_FF3_encrypt, E_ENCRYPTION), ("decrypt", uaes.AES_FF3_decrypt, E_DECRYPTION)):
        for n in (5, 57):                                      # too short, too long
            text = bytes(rng.choice(R.DECIMAL) for _ in range(n))
            assert fn(key, tweak, text, prefill=0x5C) == (E_DATALENGTH, fill * n), (name, n)
            assert compat(name, key, tweak, text, prefill=0x5C) == (code, fill * (n + 2)), (name, n)
        for radix in (2, 64, 256):
            for n in (R.minlen(radix) - 1, R.maxlen(radix) + 1):
                assert fn(key, tweak, bytes(n), None, radix, prefill=0x5C) == (E_DATALENGTH, fill * n), (name, radix, n)
        text = bytes(rng.choice(R.DECIMAL) for _ in range(31))
        for pos in (0, 15, 16, 30):                            # a foreign byte
            bad = text[:pos] + b"x" + text[pos + 1:]
            assert fn(key, tweak, bad, prefill=0x5C) == (code, fill * 31), (name, pos)
            assert compat(name, key, tweak, bad, prefill=0x5C) == (code, fill * 33), (name, pos)
            assert fn(key, tweak, bytes(c - 48 for c in text[:pos]) + b"\x0a" + bytes(30 - pos), None, 10,
                      prefill=0x5C) == (code, fill * 31), (name, pos)
        for radix in (1, 257, 0):
            assert fn(key, tweak, bytes(31), None, radix, prefill=0x5C) == (E_ARG, fill * 31), (name, radix)
        assert fn(key, tweak, text, b"0123456780", prefill=0x5C) == (E_ARG, fill * 31)     # a repeated alphabet byte
        assert compat(name, key, tweak, text, b"0123456780", prefill=0x5C) == (code, fill * 33)
        assert compat(name, key, tweak, text, b"0", prefill=0x5C) == (code, fill * 33)
    with pytest.raises(ValueError):
        uaes.AES_FF3_encrypt(key, bytes(8), b"1234567")        # the withdrawn 64-bit tweak is not taken


def test_in_place(host_forced, orc):
    rng = random.Random(6)
    L = uaes.engine()
    for n in (6, 7, 16, 19, 56):
        key, tweak = rng.randbytes(16), rng.randbytes(7)
        pt = bytes(rng.choice(R.DECIMAL) for _ in range(n))
        ct = R.model_text(orc, key, tweak, pt, R.DECIMAL)
        m = buf(pt)
        assert L.uaes_ff3_encrypt(128, buf(key), 10, R.DECIMAL, buf(tweak), m, n, m) == 0 and bytes(m) == ct, n
        assert L.uaes_ff3_decrypt(128, buf(key), 10, R.DECIMAL, buf(tweak), m, n, m) == 0 and bytes(m) == pt, n
