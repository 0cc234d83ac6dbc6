"""AES key wrap (RFC 3394) without a GPU: the engine's host path (forced on with uaes.host_policy, restored after)
against the compiled reference at every short length and at the lengths where the step counter grows a byte, the RFC's
six parameter sets (tests/golden/kw_rfc3394.json) through uaes_kw_* and through the three compat libraries, error
lengths, forgeries and the wipe switch, the in-place form, the planner without a device, the drop-in header's KWA switch
and the reference's own main.c linked against the compat libraries."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import micro_aes_amd as uaes
from tests import kw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def host_forced():
    prev = uaes.host_policy(max_bytes=1 << 30, chains=1)
    yield
    uaes.host_policy(*prev)


def buf(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def compat_call(name, kek, data, out_len, prefill=0):
    o = (C.c_uint8 * max(out_len, 1))()
    C.memset(o, prefill, max(out_len, 1))
    rc = getattr(uaes.compat(len(kek) * 8), name)(buf(kek), buf(data), len(data), o)
    return ord(rc), bytes(o)[:out_len]


def test_rfc3394_vectors(host_forced, golden_dir):
    cases = R.rfc3394(golden_dir)
    assert [(c["kek_bits"], c["data_bits"]) for c in cases] == [(128, 128), (192, 128), (256, 128), (192, 192), (256, 192),
                                                                (256, 256)]
    assert cases[0]["wrapped"].hex().upper() == "1FA68B0A8112B447AEF34BD8FB5A7B829D3E862371D2CFE5"
    for c in cases:
        kek, s, w = c["kek"], c["secret"], c["wrapped"]
        assert len(kek) * 8 == c["kek_bits"] and len(s) * 8 == c["data_bits"]
        assert R.wrap(kek, s) == (0, w) and R.unwrap(kek, w) == (0, s)
        assert uaes.AES_KEY_wrap(kek, s) == (0, w)
        assert uaes.AES_KEY_unwrap(kek, w) == (0, s)
        assert compat_call("AES_KEY_wrap", kek, s, len(w)) == (0, w)
        assert compat_call("AES_KEY_unwrap", kek, w, len(s)) == (0, s)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_length_and_the_counter_bytes(host_forced, bits):
    """n = 2 .. 48 semiblocks (6 n passes 255 between 42 and 43) and 10922 / 10923 (6 n passes 65535)"""
    rng = random.Random(bits)
    for n in list(range(2, 49)) + [10922, 10923]:
        kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
        rc, w = uaes.AES_KEY_wrap(kek, s)
        assert (rc, w) == R.wrap(kek, s), (bits, n)
        assert uaes.AES_KEY_unwrap(kek, w) == (0, s) == R.unwrap(kek, w), (bits, n)


def test_the_fourth_counter_byte(host_forced):
    """6 n > 2^24 (n = 2796203, 22 MB): the only place where the step counter has four bytes.  The reference needs
    some tens of seconds for its two passes here; the engine's host path a few."""
    n = 2796203
    assert 6 * n > 1 << 24
    rng = random.Random(24)
    kek, s = rng.randbytes(16), rng.randbytes(8 * n)
    rc, w = uaes.AES_KEY_wrap(kek, s)
    assert rc == 0 and (rc, w) == R.wrap(kek, s)
    assert uaes.AES_KEY_unwrap(kek, w) == (0, s)
    assert R.unwrap(kek, w) == (0, s)


def test_error_lengths_leave_the_buffer(host_forced):
    rng = random.Random(3)
    for bits in (128, 192, 256):
        kek = rng.randbytes(bits // 8)
        for n in (0, 8, 12, 20):
            want = (1, b"\x5c" * (n + 8))
            assert uaes.AES_KEY_wrap(kek, rng.randbytes(n), prefill=0x5C) == want, (bits, n)
            assert compat_call("AES_KEY_wrap", kek, rng.randbytes(n), n + 8, 0x5C) == want, (bits, n)
            assert R.wrap(kek, rng.randbytes(n), 0x5C) == want
        for n in (8, 16, 20):
            want = (1, b"\x5c" * (n - 8))
            assert uaes.AES_KEY_unwrap(kek, rng.randbytes(n), prefill=0x5C) == want, (bits, n)
            assert compat_call("AES_KEY_unwrap", kek, rng.randbytes(n), n - 8, 0x5C) == want, (bits, n)
            assert R.unwrap(kek, rng.randbytes(n), 0x5C) == want


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_forgeries(host_forced, bits):
    rng = random.Random(40 + bits)
    eng = uaes.engine()
    for n in (2, 3, 7, 32, 600):
        kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
        w = R.wrap(kek, s)[1]
        for k2, w2 in R.forgeries(kek, w):
            rc, text = R.unwrap(k2, w2, 0x5C)
            assert rc == 0x1A
            assert uaes.AES_KEY_unwrap(k2, w2, prefill=0x5C) == (0x1A, text), (bits, n)
            assert compat_call("AES_KEY_unwrap", k2, w2, 8 * n, 0x5C) == (0x1A, text), (bits, n)
            eng.uaes_set_wipe_on_auth_failure(1)
            try:
                assert uaes.AES_KEY_unwrap(k2, w2, prefill=0x5C) == (0x1A, bytes(8 * n)), (bits, n)
                assert uaes.AES_KEY_unwrap(kek, w, prefill=0x5C) == (0, s)
            finally:
                eng.uaes_set_wipe_on_auth_failure(0)


def test_in_place(host_forced):
    """secret == wrapped + 8, the reference's own in-place form, in both directions"""
    rng = random.Random(5)
    L = uaes.engine()
    for bits in (128, 192, 256):
        for n in (2, 5, 48, 1000):
            kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
            w = R.wrap(kek, s)[1]
            both = (C.c_uint8 * (8 * n + 8)).from_buffer_copy(b"\x5c" * 8 + s)
            base = C.addressof(both)
            assert L.uaes_kw_wrap(bits, buf(kek), C.c_void_p(base + 8), 8 * n, C.c_void_p(base)) == 0
            assert bytes(both) == w, (bits, n)
            assert L.uaes_kw_unwrap(bits, buf(kek), C.c_void_p(base), 8 * n + 8, C.c_void_p(base + 8)) == 0
            assert bytes(both)[8:] == s, (bits, n)


def test_planner_without_a_device():
    walk = [n for n in range(16, 1 << 16, 8) if uaes.kw_plan(n)[0] != uaes.kw_plan(n + 8)[0]]
    assert walk == [4096]                                   # UAES_KW_LDS_MAX: the one boundary of the one-secret calls
    for dec in (False, True):
        assert uaes.kw_plan(16, unwrap=dec) == ("kw.lds", 1, 1, 64)
        assert uaes.kw_plan(walk[0], unwrap=dec) == ("kw.lds", 1, 1, 64)
        assert uaes.kw_plan(walk[0] + 8, unwrap=dec) == ("kw.global", 1, 1, 64)
        assert uaes.kw_plan(1 << 30, unwrap=dec) == ("kw.global", 1, 1, 64)
        top = max(n for n in range(16, 4096, 8) if uaes.kw_plan(n, 1000, unwrap=dec) is not None)
        assert top == 256 and top >= 64                     # UAES_KW_BATCH_MAX
        assert uaes.kw_plan(top + 8, 1000, unwrap=dec) is None
        assert uaes.kw_plan(32, 1, unwrap=dec) == ("kw.batch", 1, 1, 256)
        assert uaes.kw_plan(32, 17, unwrap=dec) == ("kw.batch", 1, 2, 256)
        name, launches, grid, threads = uaes.kw_plan(32, 65536, unwrap=dec)          # a 256-CU part without a device
        assert (name, launches, grid, threads) == ("kw.batch", 1, 256, 1024)
    eng = uaes.engine()
    for args in ((0, 0, 0), (0, 8, 0), (0, 20, 0), (1, 12, 0), (2, 16, 0), (-1, 16, 0), (0, 20, 4), (0, 8, 4)):
        assert eng.uaes_debug_plan_kw(*args, None) is None, args
    assert eng.uaes_debug_plan_kw(0, 16, 0, None) == b"kw.lds"


def test_drop_in_header_switch(tmp_path):
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "k.c"
    src.write_text('#include "micro_aes.h"\n'
                   "#if KWA != 1\n#error switch\n#endif\n"
                   "char (*kw)(const uint8_t *, const void *, const size_t, void *) = AES_KEY_wrap;\n"
                   "char (*ku)(const uint8_t *, const void *, const size_t, void *) = AES_KEY_unwrap;\n"
                   "int main(void) { return kw == 0 || ku == 0; }\n")
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-DKWA=1", "-I", inc, "-c", str(src), "-o",
                    str(tmp_path / "k.o")], check=True)
    dflt = tmp_path / "d.c"
    dflt.write_text('#include "micro_aes.h"\n#if KWA != 0\n#error default\n#endif\n'
                    "int AES_KEY_wrap(int hidden) { return hidden; }\nint main(void) { return AES_KEY_wrap(0); }\n")
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(dflt), "-o",
                    str(tmp_path / "d.o")], check=True)
    for bits in (128, 192, 256):
        lib = C.CDLL(uaes.lib_path("libmicro_aes_hip_%d.so" % bits))
        assert lib.AES_KEY_wrap is not None and lib.AES_KEY_unwrap is not None


def reference_checkout():
    """the reference checkout oracle/Makefile builds from (its REF, or $REF), or None when it is not there"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        m = re.search(r"^REF\s*\?=\s*(\S+)", f.read(), re.M)
    ref = os.environ.get("REF") or (m.group(1) if m else "")
    return ref if ref and os.path.exists(os.path.join(ref, "main.c")) else None


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_reference_main_with_kwa(tmp_path, bits):
    """the reference's unchanged main.c against include/micro_aes.h with -DKWA=1, linked to libmicro_aes_hip_<bits>.so
    and run on the host path: its key wrap and unwrap checks pass like their neighbours"""
    ref = reference_checkout()
    if ref is None:
        pytest.skip("no reference checkout here")
    libdir = os.path.dirname(uaes.lib_path())
    with open(os.path.join(ROOT, "include", "micro_aes.h")) as f:
        header = re.sub(r"^#define AES___ 128 .*$", "#define AES___ %d" % bits, f.read(), count=1, flags=re.M)
    (tmp_path / "micro_aes.h").write_text(header)
    os.symlink(os.path.join(ref, "main.c"), tmp_path / "main.c")
    exe = tmp_path / "main_kw"
    subprocess.run(["gcc", "-O2", "-w", "-DKWA=1", "-o", str(exe), str(tmp_path / "main.c"), "-L", libdir,
                    "-lmicro_aes_hip_%d" % bits, "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = dict(os.environ, UAES_HOST_POLICY="recommended")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, env=env, timeout=120).stdout
    assert "AES-%d KW- (key wrap): PASSED!" % bits in out, out
    assert "AES-%d key unwrapping: PASSED!" % bits in out, out
    assert "FAILED" not in out, out
