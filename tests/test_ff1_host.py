"""FF1 (SP 800-38G) without a GPU: the specification model of tests/ff1_ref.py against the reference's vector file and
the compiled reference, then the engine's host path (forced on with uaes.host_policy, restored after) and the three
compat libraries against the vectors, the compiled reference (decimal) and the model (other radices, and the lengths at
which the reference's floating-point b is one too large); errors, the NUL behind a compat output, the in-place form,
the planner without a device, the drop-in header's FPE / CUSTOM_ALPHABET / FF_X switches, and the reference's own
main.c and vector harness linked against the compat libraries."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import micro_aes_amd as uaes
from tests import ff1_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DATALENGTH, E_DECRYPTION, E_ENCRYPTION = -2, 1, 0x1D, 0x1E
TWEAK_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 100]
RADICES = [2, 26, 36, 64, 95, 255, 256]


@pytest.fixture
def host_forced():
    prev = uaes.host_policy(max_bytes=1 << 30, chains=1)
    yield
    uaes.host_policy(*prev)


def decimal(rng, n):
    return bytes(rng.choice(R.DECIMAL) for _ in range(n))


def compat(name, key, tweak, text, alphabet=None, prefill=0, extra=2):
    """AES_FPE_<name> of libmicro_aes_hip_<bits>.so, or its _alpha form when an alphabet is given: (code, the
    len(text) + extra bytes of the output buffer)"""
    lib = uaes.compat(len(key) * 8)
    n = len(text) + extra
    o = (C.c_uint8 * n)()
    C.memset(o, prefill, n)
    if alphabet is None:
        rc = getattr(lib, "AES_FPE_" + name)(R.buf(key), R.buf(tweak), len(tweak), R.buf(text), len(text), o)
    else:
        rc = getattr(lib, "AES_FPE_%s_alpha" % name)(bytes(alphabet), len(alphabet), R.buf(key), R.buf(tweak), len(tweak),
                                                     R.buf(text), len(text), o)
    return ord(rc), bytes(o)


def test_model_reproduces_the_vector_file(orc, golden_dir):
    vs = R.vectors(golden_dir)
    assert len(vs) == 20 and sorted(set(len(v["key"]) for v in vs)) == [16, 24, 32]
    assert sorted(set(len(v["alphabet"]) for v in vs)) == [2, 10, 26, 36, 62, 72] and max(len(v["pt"]) for v in vs) == 1804
    assert (vs[0]["pt"], vs[0]["ct"]) == (b"0123456789", b"2433477484")           # SP 800-38G FF1 sample 1
    for v in vs:
        assert R.model_text(orc, v["key"], v["tweak"], v["pt"], v["alphabet"]) == v["ct"], v
        assert R.model_text(orc, v["key"], v["tweak"], v["ct"], v["alphabet"], decrypt=True) == v["pt"], v


def test_model_equals_the_compiled_reference(orc):
    rng = random.Random(1)
    for n in range(6, 81):
        key, tweak, pt = rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(rng.choice([0, 3, 16, 21])), decimal(rng, n)
        rc, ct = R.ref_encrypt(key, tweak, pt)
        assert rc == 0 and R.model_text(orc, key, tweak, pt, R.DECIMAL) == ct, (n, key.hex(), tweak.hex())
        assert R.ref_decrypt(key, tweak, ct) == (0, pt)


def test_vector_file_engine_and_compat(host_forced, golden_dir):
    for v in R.vectors(golden_dir):
        key, tweak, a, n = v["key"], v["tweak"], v["alphabet"], len(v["pt"])
        assert uaes.AES_FPE_encrypt(key, tweak, v["pt"], a) == (0, v["ct"]), v
        assert uaes.AES_FPE_decrypt(key, tweak, v["ct"], a) == (0, v["pt"]), v
        assert compat("encrypt", key, tweak, v["pt"], a, prefill=7) == (0, v["ct"] + b"\0\x07"), v
        assert compat("decrypt", key, tweak, v["ct"], a, prefill=7) == (0, v["pt"] + b"\0\x07"), v
        if a == R.DECIMAL:
            assert compat("encrypt", key, tweak, v["pt"]) == (0, v["ct"] + b"\0\0"), v
            assert compat("decrypt", key, tweak, v["ct"]) == (0, v["pt"] + b"\0\0"), v


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_decimal_against_the_compiled_reference(host_forced, bits):
    rng = random.Random(bits)
    lengths = list(range(6, 131)) + [255, 256, 257, 1804, 4095, 4096]
    for k, n in enumerate(lengths):
        key, tweak, pt = rng.randbytes(bits // 8), rng.randbytes(TWEAK_LENS[k % len(TWEAK_LENS)]), decimal(rng, n)
        want = R.ref_encrypt(key, tweak, pt)
        case = (bits, n, key.hex(), tweak.hex())
        assert want[0] == 0 and uaes.AES_FPE_encrypt(key, tweak, pt) == want, case
        assert uaes.AES_FPE_decrypt(key, tweak, want[1]) == (0, pt), case
    key, pt = rng.randbytes(bits // 8), decimal(rng, 57)
    for t in TWEAK_LENS:                                       # every tweak length at one length, too
        tweak = rng.randbytes(t)
        want = R.ref_encrypt(key, tweak, pt)
        assert uaes.AES_FPE_encrypt(key, tweak, pt) == want and uaes.AES_FPE_decrypt(key, tweak, want[1]) == (0, pt), t
        assert compat("encrypt", key, tweak, pt)[1][:57] == want[1], t


@pytest.mark.parametrize("radix", RADICES)
def test_radices_against_the_model(host_forced, orc, radix):
    rng = random.Random(radix)
    extra = {2: [255, 256, 257], 256: [31, 32, 33]}.get(radix, [])
    assert all(R.b_float(radix, n - n // 2) == R.b_exact(radix, n - n // 2) + 1 for n in extra if n % 2 == 0)
    alphabet = bytes(rng.sample(range(256), radix))
    for n in list(range(R.minlen(radix), 71)) + extra:
        key, tweak = rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(rng.choice([0, 3, 16, 21]))
        digits = [rng.randrange(radix) for _ in range(n)]
        want = R.model(orc, key, tweak, digits, radix)
        case = (radix, n, key.hex(), tweak.hex())
        assert uaes.AES_FPE_encrypt(key, tweak, bytes(digits), None, radix) == (0, bytes(want)), case
        assert uaes.AES_FPE_decrypt(key, tweak, bytes(want), None, radix) == (0, bytes(digits)), case
        text, ct = bytes(alphabet[d] for d in digits), bytes(alphabet[d] for d in want)
        assert uaes.AES_FPE_encrypt(key, tweak, text, alphabet) == (0, ct), case
        assert uaes.AES_FPE_decrypt(key, tweak, ct, alphabet) == (0, text), case


def test_wave_shapes_at_the_ends_of_the_radix_range(host_forced, orc):
    """the twelve cases of tests/test_gpu_ff1.py's wave-form test through the host path, which shares no code with the
    kernel: the model's answers are confirmed here"""
    lens = [n for n in range(6, 8200) if uaes.ff1_plan(n) is not None]
    batch, top = max(n for n in lens if uaes.ff1_plan(n)[0] == "ff1.batch"), lens[-1]
    cases = R.wave_cases(orc, batch, top)
    assert len(cases) == 12 and sorted(set(len(c[3]) for c in cases)) == [batch + 1, 1000, top - 1, top]
    for radix, key, tweak, digits, want in cases:
        case = (radix, len(digits), key.hex(), tweak.hex())
        assert uaes.AES_FPE_encrypt(key, tweak, digits, None, radix) == (0, want), case
        assert uaes.AES_FPE_decrypt(key, tweak, want, None, radix) == (0, digits), case


def test_minimum_lengths_are_the_references():
    """radix^minlen >= 1 000 000, exact; equal to micro_fpe.h's MINLEN = 1 + (int)(19.931561 / log2(radix))"""
    import math
    for radix in range(2, 257):
        n = R.minlen(radix)
        assert n == 1 + int(19.931561 / math.log2(radix)), radix
        assert uaes.ff1_plan(n, radix=radix) is not None and uaes.ff1_plan(n - 1, radix=radix) is None, radix


def test_errors_leave_the_output_alone(host_forced):
    rng = random.Random(9)
    key = rng.randbytes(16)
    fill = bytes([0x5C])
    for name, fn, code in (("encrypt", uaes.AES_FPE_encrypt, E_ENCRYPTION), ("decrypt", uaes.AES_FPE_decrypt, E_DECRYPTION)):
        for n in (5, 4097):
            text = decimal(rng, n)
            assert fn(key, b"tw", text, prefill=0x5C) == (E_DATALENGTH, fill * n), (name, n)
            assert compat(name, key, b"tw", text, prefill=0x5C) == (code, fill * (n + 2)), (name, n)
        # the compiled reference gives the same code and buffer for the short text (it has no upper limit)
        assert R.fpe_call(R.ref(128), "AES_FPE_" + name, key, b"tw", b"12345", prefill=0x5C) == (code, fill * 7)
        assert fn(key, b"", bytes(range(7)), None, 2, prefill=0x5C)[0] == E_DATALENGTH       # radix 2 wants 20 numerals
        text = decimal(rng, 31)
        for pos in (0, 15, 30):
            bad = text[:pos] + b"x" + text[pos + 1:]
            assert fn(key, b"tw", bad, prefill=0x5C) == (code, fill * 31), (name, pos)
            got = compat(name, key, b"tw", bad, prefill=0x5C)
            assert got == (code, fill * 33) and got == R.fpe_call(R.ref(128), "AES_FPE_" + name, key, b"tw", bad, prefill=0x5C)
            assert fn(key, b"tw", bytes(c - 48 for c in text[:pos]) + b"\x0a" + bytes(30 - pos), None, 10,
                      prefill=0x5C) == (code, fill * 31), (name, pos)
        for radix in (1, 257, 0):
            assert fn(key, b"", bytes(31), None, radix, prefill=0x5C) == (E_ARG, fill * 31), (name, radix)
        assert fn(key, b"", text, b"0123456780", prefill=0x5C) == (E_ARG, fill * 31)
        assert compat(name, key, b"", text, b"0123456780", prefill=0x5C) == (code, fill * 33)
        assert compat(name, key, b"", text, b"0", prefill=0x5C) == (code, fill * 33)


def test_compat_writes_the_nul_and_nothing_behind_it(host_forced):
    rng = random.Random(4)
    for bits in (128, 192, 256):
        key, tweak, pt = rng.randbytes(bits // 8), rng.randbytes(5), decimal(rng, 16)
        rc, ct = R.ref_encrypt(key, tweak, pt)
        assert compat("encrypt", key, tweak, pt, prefill=0xEE, extra=3) == (0, ct + b"\0\xEE\xEE")
        assert compat("decrypt", key, tweak, ct, prefill=0xEE, extra=3) == (0, pt + b"\0\xEE\xEE")
        assert R.fpe_call(R.ref(bits), "AES_FPE_encrypt", key, tweak, pt, prefill=0xEE, extra=3) == (0, ct + b"\0\xEE\xEE")
        # the engine's own calls append nothing
        o = (C.c_uint8 * 18)()
        C.memset(o, 0xEE, 18)
        assert uaes.engine().uaes_ff1_encrypt(bits, R.buf(key), 10, R.DECIMAL, R.buf(tweak), 5, R.buf(pt), 16, o) == 0
        assert bytes(o) == ct + b"\xEE\xEE"


def test_in_place(host_forced):
    rng = random.Random(6)
    L = uaes.engine()
    for n in (6, 16, 19, 130, 1000):
        key, tweak, pt = rng.randbytes(16), rng.randbytes(9), decimal(rng, n)
        rc, ct = R.ref_encrypt(key, tweak, pt)
        m = R.buf(pt)
        assert L.uaes_ff1_encrypt(128, R.buf(key), 10, R.DECIMAL, R.buf(tweak), 9, m, n, m) == 0 and bytes(m) == ct, n
        assert L.uaes_ff1_decrypt(128, R.buf(key), 10, R.DECIMAL, R.buf(tweak), 9, m, n, m) == 0 and bytes(m) == pt, n
        m = (C.c_uint8 * (n + 1)).from_buffer_copy(pt + b"\xEE")
        assert ord(uaes.compat(128).AES_FPE_encrypt(R.buf(key), R.buf(tweak), 9, m, n, m)) == 0 and bytes(m) == ct + b"\0"


def test_planner_without_a_device():
    walk = [n for n in range(6, 4096) if uaes.ff1_plan(n)[0] != uaes.ff1_plan(n + 1)[0]]
    assert walk == [128]                                    # UAES_FF1_BATCH_MAX: the one boundary of the one-text calls
    top = max(n for n in range(6, 8200) if uaes.ff1_plan(n) is not None)
    assert top == 4096 and walk[0] >= 64                    # UAES_FF1_MAX
    for dec in (False, True):
        assert uaes.ff1_plan(6, decrypt=dec) == ("ff1.batch", 1, 1, 64)
        assert uaes.ff1_plan(walk[0], decrypt=dec) == ("ff1.batch", 1, 1, 64)
        assert uaes.ff1_plan(walk[0] + 1, decrypt=dec) == ("ff1.wave", 1, 1, 64)
        assert uaes.ff1_plan(top, decrypt=dec) == ("ff1.wave", 1, 1, 64)
        assert uaes.ff1_plan(top + 1, decrypt=dec) is None and uaes.ff1_plan(5, decrypt=dec) is None
        assert max(n for n in range(6, 4097) if uaes.ff1_plan(n, 1000, decrypt=dec) is not None) == walk[0]
        assert uaes.ff1_plan(16, 1, decrypt=dec) == ("ff1.batch", 1, 1, 256)
        assert uaes.ff1_plan(16, 17, decrypt=dec) == ("ff1.batch", 1, 2, 256)
        assert uaes.ff1_plan(16, 1 << 20, decrypt=dec) == ("ff1.batch", 1, 256, 1024)     # a 256-CU part without a device
    eng = uaes.engine()
    for args in ((0, 1, 31, 0), (0, 257, 31, 0), (2, 10, 16, 0), (-1, 10, 16, 0), (0, 10, 5, 0), (0, 2, 19, 0), (0, 10, 129, 3)):
        assert eng.uaes_debug_plan_ff1(*args, None) is None, args
    assert eng.uaes_debug_plan_ff1(0, 2, 20, 0, None) == b"ff1.batch" and eng.uaes_debug_plan_ff1(1, 256, 3, 5, None) == b"ff1.batch"


def gcc(tmp_path, name, text, *flags, ok=True):
    src = tmp_path / (name + ".c")
    src.write_text(text)
    r = subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                        "-I", str(tmp_path), "-c", str(src), "-o", str(tmp_path / (name + ".o"))], capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stderr


BIND = ('#include "micro_aes.h"\n#if FPE != 1 || FF_X != 1\n#error switch\n#endif\n'
        "char (*fe)(const uint8_t *, const uint8_t *, const size_t, const void *, const size_t, void *) = AES_FPE_encrypt;\n"
        "char (*fd)(const uint8_t *, const uint8_t *, const size_t, const void *, const size_t, void *) = AES_FPE_decrypt;\n"
        "int main(void) { return fe == 0 || fd == 0 || CUSTOM_ALPHABET > 9; }\n")


def test_drop_in_header_switch(tmp_path):
    gcc(tmp_path, "d", '#include "micro_aes.h"\n#if FPE != 0\n#error default\n#endif\n'
        "int AES_FPE_encrypt(int hidden) { return hidden; }\nint main(void) { return AES_FPE_encrypt(0); }\n")
    gcc(tmp_path, "k", BIND, "-DFPE=1")
    assert "FF1" in gcc(tmp_path, "x", BIND, "-DFPE=1", "-DFF_X=3", ok=False)
    assert "wide" in gcc(tmp_path, "w", BIND, "-DFPE=1", "-DCUSTOM_ALPHABET=10", ok=False)
    # a caller's own micro_fpe.h, as the reference's micro_aes.c includes it
    (tmp_path / "micro_fpe.h").write_text('#if CUSTOM_ALPHABET == 2\n#define ALPHABET "zyxwvutsrq"\n#define RADIX 10\n#endif\n')
    gcc(tmp_path, "a", BIND, "-DFPE=1", "-DCUSTOM_ALPHABET=2")
    for bits in (128, 192, 256):
        lib = C.CDLL(uaes.lib_path("libmicro_aes_hip_%d.so" % bits))
        for n in ("AES_FPE_encrypt", "AES_FPE_decrypt", "AES_FPE_encrypt_alpha", "AES_FPE_decrypt_alpha"):
            assert getattr(lib, n) is not None


def test_custom_alphabet_binding_runs(tmp_path):
    """a caller built with -DFPE=1 -DCUSTOM_ALPHABET=2 and its own micro_fpe.h gets that alphabet (host path)"""
    (tmp_path / "micro_fpe.h").write_text('#define ALPHABET "zyxwvutsrq"\n#define RADIX 10\n')
    (tmp_path / "m.c").write_text('#include <stdio.h>\n#include "micro_aes.h"\nint main(void) {\n'
                                  "  static const uint8_t key[16] = { 0x2B, 0x7E, 0x15, 0x16, 0x28, 0xAE, 0xD2, 0xA6, 0xAB, 0xF7, 0x15, 0x88,"
                                  " 0x09, 0xCF, 0x4F, 0x3C };\n  char out[16], back[16];\n"
                                  '  char a = AES_FPE_encrypt(key, 0, 0, "zyxwvutsrq", 10, out);\n'
                                  "  char b = AES_FPE_decrypt(key, 0, 0, out, 10, back);\n"
                                  '  printf("%d %d %s %s\\n", a, b, out, back);\n  return 0;\n}\n')
    libdir = os.path.dirname(uaes.lib_path())
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-O2", "-DFPE=1", "-DCUSTOM_ALPHABET=2", "-I", os.path.join(ROOT, "include"), "-I", str(tmp_path),
                    "-o", str(exe), str(tmp_path / "m.c"), "-L", libdir, "-lmicro_aes_hip_128", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = dict(os.environ, UAES_HOST_POLICY="recommended")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, env=env, timeout=60).stdout
    # SP 800-38G FF1 sample 1 (0123456789 -> 2433477484) through the substitution 0..9 -> z..q
    assert out.split() == ["0", "0", "xvwwvssvrv", "zyxwvutsrq"], out


def reference_checkout():
    """the reference checkout oracle/Makefile builds from (its REF, or $REF), or None when it is not there"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        m = re.search(r"^REF\s*\?=\s*(\S+)", f.read(), re.M)
    ref = os.environ.get("REF") or (m.group(1) if m else "")
    return ref if ref and os.path.exists(os.path.join(ref, "main.c")) else None


def test_reference_main_with_fpe(tmp_path):
    """the reference's unchanged main.c against include/micro_aes.h with -DFPE=1, linked to libmicro_aes_hip_128.so and
    run on the host path: its FF1 lines pass like their neighbours (main.c checks FPE for AES-128 only)"""
    ref = reference_checkout()
    if ref is None:
        pytest.skip("no reference checkout here")
    libdir = os.path.dirname(uaes.lib_path())
    with open(os.path.join(ROOT, "include", "micro_aes.h")) as f:
        (tmp_path / "micro_aes.h").write_text(f.read())
    os.symlink(os.path.join(ref, "main.c"), tmp_path / "main.c")
    exe = tmp_path / "main_fpe"
    subprocess.run(["gcc", "-O2", "-w", "-DFPE=1", "-o", str(exe), str(tmp_path / "main.c"), "-L", libdir,
                    "-lmicro_aes_hip_128", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    env = dict(os.environ, UAES_HOST_POLICY="recommended")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, env=env, timeout=120).stdout
    assert "AES-128 FF1 encryption: PASSED!" in out, out
    assert "AES-128 FPE decryption: PASSED!" in out, out
    assert "FAILED" not in out, out


def fpe_summary(out):
    """what the harness prints for its FPE file: from its headline to the end of that block"""
    m = re.search(r"Verifying vectors: AES128-FPE\n(.*?)(?:\n\n|\Z)", out, re.S)
    assert m, out
    return m.group(1).strip()


@pytest.mark.parametrize("flags", [("-DFPE=1",), ("-DFPE=1", "-DCUSTOM_ALPHABET=4")])
def test_reference_harness_with_fpe(tmp_path, flags):
    """the reference's unchanged vector harness, built once against its own micro_aes.c and once against
    include/micro_aes.h and libmicro_aes_hip_128.so (host path): the same FPE summary, no failure"""
    ref = reference_checkout()
    if ref is None:
        pytest.skip("no reference checkout here")
    libdir = os.path.dirname(uaes.lib_path())
    outs = []
    for ours in (False, True):
        d = tmp_path / ("ours" if ours else "theirs")
        (d / "testvectors").mkdir(parents=True)
        for f in os.listdir(os.path.join(ref, "testvectors")):
            os.symlink(os.path.join(ref, "testvectors", f), d / "testvectors" / f)
        os.symlink(os.path.join(ref, "micro_fpe.h"), d / "micro_fpe.h")
        exe = d / "harness"
        if ours:
            with open(os.path.join(ROOT, "include", "micro_aes.h")) as f:
                (d / "micro_aes.h").write_text(f.read())
            cmd = ["gcc", "-O2", "-w", *flags, "-o", str(exe), str(d / "testvectors" / "aes_testvectors.c"), "-L", libdir,
                   "-lmicro_aes_hip_128", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"]
        else:
            # the reference's header sets FPE, CUSTOM_ALPHABET and the other switches itself: a copy with the one line
            # changed that the flag stands for (only in the temporary directory)
            with open(os.path.join(ref, "micro_aes.h")) as f:
                h = f.read()
            if "-DCUSTOM_ALPHABET=4" in flags:
                h, k = re.subn(r"^#define CUSTOM_ALPHABET 0", "#define CUSTOM_ALPHABET 4", h, count=1, flags=re.M)
                assert k == 1
            (d / "micro_aes.h").write_text(h)
            os.symlink(os.path.join(ref, "micro_aes.c"), d / "micro_aes.c")
            cmd = ["gcc", "-O2", "-w", "-o", str(exe), str(d / "testvectors" / "aes_testvectors.c"), str(d / "micro_aes.c"), "-lm"]
        subprocess.run(cmd, check=True)
        env = dict(os.environ, UAES_HOST_POLICY="recommended")
        out = subprocess.run([str(exe)], cwd=str(d / "testvectors"), capture_output=True, text=True, env=env, timeout=300).stdout
        outs.append(fpe_summary(out))
    assert outs[0] == outs[1], outs
    assert re.fullmatch(r"Nmber of tests:\s+[1-9]\d*, All Passed!", outs[1]), outs
