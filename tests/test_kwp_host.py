"""AES key wrap with padding (RFC 5649) without a GPU: the model of tests/kwp_ref.py against the recorded vectors
(tests/golden/kwp_vectors.json: the RFC's two and OpenSSL's), the engine's host path (forced on with uaes.host_policy,
restored after) against both at every length 1 .. 40, every crafted forgery class, the argument and length errors with
the buffers untouched, the wipe switch, *secretLen, the in-place form, uaes_kwp_wrapped_len, the planner without a
device and the key schedules a call leaves behind (the count of live schedules is level across a test: zero when nothing
else in the process holds a key context open)."""
import ctypes as C
import os
import random
import subprocess

import pytest

import micro_aes_amd as uaes
from tests import kwp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DATALENGTH, E_AUTH = -2, 1, 0x1A
LDS_MAX, BATCH_MAX = 4096, 256                              # UAES_KW_LDS_MAX, UAES_KW_BATCH_MAX (csrc/uaes_plan.h)


@pytest.fixture
def host_forced():
    prev = uaes.host_policy(max_bytes=1 << 30, chains=1)
    yield
    uaes.host_policy(*prev)


def buf(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def test_model_reproduces_every_fixture(golden_dir):
    cases = R.fixtures(golden_dir)
    assert len(cases) == 2 + 3 * 14 and os.path.getsize(os.path.join(golden_dir, "kwp_vectors.json")) < 64 << 10
    assert cases[0]["wrapped"].hex() == "138bdeaa9b8fa7fc61f97742e72248ee5ae6ae5360d1ae6a5f54f373fa543b6a"
    assert cases[1]["secret"].hex() == "466f7250617369" and cases[1]["wrapped"].hex() == "afbeb0f07dfbf5419200f2ccb50bb24f"
    assert sorted({len(c["secret"]) for c in cases[2:]}) == [1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 255, 256, 4097]
    assert sorted({len(c["kek"]) for c in cases[2:]}) == [16, 24, 32]
    for c in cases:
        assert R.wrap(c["kek"], c["secret"]) == c["wrapped"], (c["source"], len(c["secret"]))
        code, text, n = R.unwrap(c["kek"], c["wrapped"])
        assert (code, text[:n], n) == (0, c["secret"], len(c["secret"])) and not any(text[n:])


def test_fixtures_on_the_host_path(host_forced, golden_dir):
    for c in R.fixtures(golden_dir):
        info = (c["source"], len(c["secret"]))
        assert uaes.kwp_wrap(c["kek"], c["secret"], prefill=0x5C) == (0, c["wrapped"]), info
        pad = bytes(-len(c["secret"]) % 8)
        assert uaes.kwp_unwrap(c["kek"], c["wrapped"], prefill=0x5C) == (0, c["secret"] + pad, len(c["secret"])), info


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_length_to_40(host_forced, bits):
    rng = random.Random(bits)
    for m in range(1, 41):
        kek, s = rng.randbytes(bits // 8), rng.randbytes(m)
        w = R.wrap(kek, s)
        assert len(w) == uaes.kwp_wrapped_len(m)
        assert uaes.kwp_wrap(kek, s, prefill=0x5C) == (0, w), (bits, m)
        assert uaes.kwp_unwrap(kek, w, prefill=0x5C) == (0, s + bytes(-m % 8), m), (bits, m)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_forgeries_and_the_wipe_switch(host_forced, bits):
    rng = random.Random(40 + bits)
    eng = uaes.engine()
    live = eng.uaes_debug_live_key_schedules()
    for m in (1, 7, 8, 9, 16, 20, 33, 250, 4097):
        kek, s = rng.randbytes(bits // 8), rng.randbytes(m)
        w = R.wrap(kek, s)
        forged = [(name, kek, f) for name, f in R.crafted(kek, s)] + [("flip", k2, w2) for k2, w2 in R.flipped(kek, w)]
        assert len(forged) == 6 + 2 * (m % 8 != 0) + 3 + (m > 8)
        for name, k2, w2 in forged:
            code, text, n = R.unwrap(k2, w2)
            assert (code, n) == (E_AUTH, 0), (bits, m, name)
            assert uaes.kwp_unwrap(k2, w2, prefill=0x5C) == (E_AUTH, text, 0), (bits, m, name)
            eng.uaes_set_wipe_on_auth_failure(1)
            try:
                assert uaes.kwp_unwrap(k2, w2, prefill=0x5C) == (E_AUTH, bytes(len(w2) - 8), 0), (bits, m, name)
                assert uaes.kwp_unwrap(kek, w, prefill=0x5C) == (0, s + bytes(-m % 8), m)
            finally:
                eng.uaes_set_wipe_on_auth_failure(0)
    assert eng.uaes_debug_live_key_schedules() == live


def test_a_valid_kw_wrapping_is_no_kwp_wrapping(host_forced):
    kek, s = bytes(range(16)), bytes(range(100, 124))
    rc, w = uaes.AES_KEY_wrap(kek, s)
    assert rc == 0 and uaes.kwp_unwrap(kek, w)[0::2] == (E_AUTH, 0)
    assert uaes.AES_KEY_unwrap(kek, R.wrap(kek, s))[0] == E_AUTH


def test_errors_leave_the_buffers(host_forced):
    eng = uaes.engine()
    live = eng.uaes_debug_live_key_schedules()
    kek = bytes(range(32))
    for bits in (128, 192, 256):
        k = kek[:bits // 8]
        assert uaes.kwp_wrap(k, b"", prefill=0x5C) == (E_DATALENGTH, b"\x5c" * 8)
        for n in (0, 8, 12, 20, 33):
            assert uaes.kwp_unwrap(k, bytes(n), prefill=0x5C) == (E_DATALENGTH, b"\x5c" * max(n - 8, 0), 0), (bits, n)
    out, ln = (C.c_uint8 * 64)(), C.c_size_t(77)
    C.memset(out, 0x5C, 64)
    # the key first, then the lengths, then the pointers
    assert eng.uaes_kwp_wrap(100, buf(kek), buf(b"x"), 0, out) == E_ARG
    assert eng.uaes_kwp_wrap(128, None, buf(b"x"), 1, out) == E_ARG
    assert eng.uaes_kwp_wrap(128, buf(kek), None, 0, None) == E_DATALENGTH
    assert eng.uaes_kwp_wrap(128, buf(kek), buf(b"x"), 1 << 32, out) == E_DATALENGTH
    assert eng.uaes_kwp_wrap(128, buf(kek), None, 5, out) == E_ARG
    assert eng.uaes_kwp_wrap(128, buf(kek), buf(b"x"), 1, None) == E_ARG
    assert eng.uaes_kwp_unwrap(100, buf(kek), buf(bytes(16)), 12, out, C.byref(ln)) == E_ARG
    assert eng.uaes_kwp_unwrap(128, buf(kek), None, 12, None, None) == E_DATALENGTH
    assert eng.uaes_kwp_unwrap(128, buf(kek), buf(bytes(16)), (1 << 32) + 16, out, C.byref(ln)) == E_DATALENGTH
    assert eng.uaes_kwp_unwrap(128, buf(kek), None, 16, out, C.byref(ln)) == E_ARG
    assert eng.uaes_kwp_unwrap(128, buf(kek), buf(bytes(16)), 16, None, C.byref(ln)) == E_ARG
    assert eng.uaes_kwp_unwrap(128, buf(kek), buf(bytes(16)), 16, out, None) == E_ARG
    assert set(bytes(out)) == {0x5C} and ln.value == 77
    assert eng.uaes_debug_live_key_schedules() == live


def test_in_place(host_forced):
    """secret == wrapped + 8 in both directions; a wrap writes its zero fill into `wrapped`"""
    rng = random.Random(5)
    L = uaes.engine()
    for bits in (128, 192, 256):
        for m in (1, 8, 9, 20, 41, 4097):
            kek, s = rng.randbytes(bits // 8), rng.randbytes(m)
            w = R.wrap(kek, s)
            both = (C.c_uint8 * len(w)).from_buffer_copy(b"\x5c" * 8 + s + b"\x5c" * (len(w) - 8 - m))
            base, ln = C.addressof(both), C.c_size_t(0)
            assert L.uaes_kwp_wrap(bits, buf(kek), C.c_void_p(base + 8), m, C.c_void_p(base)) == 0
            assert bytes(both) == w, (bits, m)
            assert L.uaes_kwp_unwrap(bits, buf(kek), C.c_void_p(base), len(w), C.c_void_p(base + 8), C.byref(ln)) == 0
            assert bytes(both)[8:] == s + bytes(-m % 8) and ln.value == m, (bits, m)


def test_wrapped_len(tmp_path):
    assert [uaes.kwp_wrapped_len(n) for n in (0, 1, 8, 9, (1 << 32) - 1, 1 << 32)] == [0, 16, 16, 24, (1 << 32) + 8, 0]
    src = tmp_path / "w.c"
    src.write_text('#include <stdio.h>\n#include "uaes_hip.h"\n'
                   "int main(void) { size_t n[5] = { 0, 1, 8, 9, 4294967295u }; int i;\n"
                   '  for (i = 0; i < 5; ++i) printf("%lu ", (unsigned long)uaes_kwp_wrapped_len(n[i]));\n  return 0; }\n')
    exe = tmp_path / "w"
    for std in ("-std=c89", "-std=c11"):
        subprocess.run(["gcc", std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
        assert out.split() == ["0", "16", "16", "24", "4294967304"], (std, out)


def test_planner_without_a_device():
    for dec in (False, True):
        up = lambda n: (n + 7) // 8 * 8 if dec else n        # an unwrap is asked by its padded length
        for n in range(1, 9):
            assert uaes.kwp_plan(up(n), unwrap=dec) == ("kwp.block", 1, 1, 64)
        assert uaes.kwp_plan(up(9), unwrap=dec) == ("kwp.lds", 1, 1, 64)
        for n in range(LDS_MAX - 8 + 1, LDS_MAX + 1):
            assert uaes.kwp_plan(up(n), unwrap=dec) == ("kwp.lds", 1, 1, 64), n
        assert uaes.kwp_plan(up(LDS_MAX + 1), unwrap=dec) == ("kwp.global", 1, 1, 64)
        assert uaes.kwp_plan(up((1 << 32) - 1), unwrap=dec) == ("kwp.global", 1, 1, 64)
        assert uaes.kwp_plan(0, unwrap=dec) is None and uaes.kwp_plan(0, 4, unwrap=dec) is None
        assert uaes.kwp_plan(8, 1, unwrap=dec) == ("kwp.batch", 1, 1, 256)
        assert uaes.kwp_plan(BATCH_MAX, 17, unwrap=dec) == ("kwp.batch", 1, 2, 256)
        assert uaes.kwp_plan(BATCH_MAX + (8 if dec else 1), 17, unwrap=dec) is None
        assert uaes.kwp_plan(32, 65536, unwrap=dec) == ("kwp.batch", 1, 256, 1024)       # a 256-CU part without a device
    # the one boundary of the one-secret calls is KW's, by the padded length
    walk = [n for n in range(9, 1 << 14) if uaes.kwp_plan(n)[0] != uaes.kwp_plan(n + 1)[0]]
    assert walk == [LDS_MAX] and uaes.kw_plan(LDS_MAX)[0] == "kw.lds" and uaes.kw_plan(LDS_MAX + 8)[0] == "kw.global"
    assert uaes.kwp_plan(1 << 32) is None and uaes.kwp_plan(1 << 32, unwrap=True) == ("kwp.global", 1, 1, 64)
    assert uaes.kwp_plan((1 << 32) + 8, unwrap=True) is None and uaes.kwp_plan(20, unwrap=True) is None
    assert uaes.kwp_plan(20, 3) == ("kwp.batch", 1, 1, 256) and uaes.kwp_plan(20, 3, unwrap=True) is None
    eng = uaes.engine()
    assert eng.uaes_debug_plan_kwp(2, 16, 0, None) is None and eng.uaes_debug_plan_kwp(-1, 16, 0, None) is None
    assert eng.uaes_debug_plan_kwp(0, 7, 0, None) == b"kwp.block"


def test_batch_argument_errors_come_before_the_device():
    L = uaes.engine()
    live = L.uaes_debug_live_key_schedules()
    kek, b = buf(bytes(16)), buf(bytes(4096))
    for sb in (0, BATCH_MAX + 1):
        assert L.uaes_kwp_wrap_batch(128, kek, 4, sb, None, b, b) == E_ARG, sb
    for wb in (8, 20, BATCH_MAX + 16):
        assert L.uaes_kwp_unwrap_batch(128, kek, 4, wb, None, b, b, b, b) == E_ARG, wb
    assert L.uaes_kwp_wrap_batch(100, kek, 4, 20, None, b, b) == E_ARG
    assert L.uaes_kwp_wrap_batch(128, kek, 0, 20, None, None, None) == 0
    assert L.uaes_kwp_unwrap_batch(128, kek, 0, 24, None, None, None, None, None) == 0
    assert L.uaes_kwp_wrap_batch(128, kek, 4, 20, None, None, b) == E_ARG
    assert L.uaes_kwp_wrap_batch(128, kek, 4, 20, None, b, None) == E_ARG
    assert L.uaes_kwp_unwrap_batch(128, kek, 4, 24, None, b, b, None, b) == E_ARG
    assert L.uaes_kwp_unwrap_batch(128, kek, 4, 24, None, b, b, b, None) == E_ARG
    assert uaes.kwp_batch(bytes(16), []) == (0, []) and uaes.kwp_batch(bytes(16), [], unwrap=True) == (0, [], [], [])
    assert L.uaes_debug_live_key_schedules() == live
