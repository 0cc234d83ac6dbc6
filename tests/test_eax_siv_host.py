"""EAX and SIV (RFC 5297) without a GPU: the engine's host path (forced on with uaes.host_policy, restored after)
against the EAX paper's vectors (tests/golden/EAX_AES128.tv), RFC 5297 A.1 and the compiled reference; the drop-in
header's EAX / SIV switches and the planner of uaes_eax_siv.hip."""
import ctypes as C
import os
import random
import subprocess

import pytest

import micro_aes_amd as uaes
from tests import eax_siv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


eax_vectors = R.eax_vectors


@pytest.fixture
def host_forced():
    prev = uaes.host_policy(max_bytes=1 << 30, chains=1)
    yield
    uaes.host_policy(*prev)


def test_eax_paper_vectors(host_forced, golden_dir):
    cases = eax_vectors(golden_dir)
    assert len(cases) == 10
    for c in cases:
        ct = uaes.AES_EAX_encrypt(c["KEY"], c["NONCE"], c["HEADER"], c["MSG"])
        assert ct == c["CIPHER"]
        assert uaes.AES_EAX_decrypt(c["KEY"], c["NONCE"], c["HEADER"], ct) == (0, c["MSG"])


def test_siv_rfc5297_a1(host_forced):
    keys = bytes.fromhex("fffefdfcfbfaf9f8f7f6f5f4f3f2f1f0f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
    ad = bytes.fromhex("101112131415161718191a1b1c1d1e1f2021222324252627")
    pt = bytes.fromhex("112233445566778899aabbccddee")
    iv, ct = uaes.AES_SIV_encrypt(keys, ad, pt)
    assert iv.hex() == "85632d07c6e8f37f950acd320a2ecc93"
    assert ct.hex() == "40c02b9690c4dc04daef7f6afe5c"
    assert uaes.AES_SIV_decrypt(keys, iv, ad, ct) == (0, pt)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_against_the_compiled_reference(host_forced, bits):
    rng = random.Random(bits)
    kb = bits // 8
    for _ in range(40):
        key, keys = rng.randbytes(kb), rng.randbytes(2 * kb)
        aad, pt, nonce = rng.randbytes(rng.randrange(81)), rng.randbytes(rng.randrange(601)), rng.randbytes(16)
        ct = uaes.AES_EAX_encrypt(key, nonce, aad, pt)
        assert ct == R.eax_encrypt(bits, key, nonce, aad, pt)
        assert uaes.AES_EAX_decrypt(key, nonce, aad, ct) == (0, pt)
        iv, sct = uaes.AES_SIV_encrypt(keys, aad, pt)
        assert (iv, sct) == R.siv_encrypt(bits, keys, aad, pt)
        assert uaes.AES_SIV_decrypt(keys, iv, aad, sct) == (0, pt)


def test_eax_other_nonce_and_tag_lengths(host_forced):
    rng = random.Random(7)
    key = rng.randbytes(16)
    for nl in (0, 1, 15, 17, 64):
        for tl in (1, 4, 12, 16):
            aad, pt, nonce = rng.randbytes(rng.randrange(40)), rng.randbytes(rng.randrange(100)), rng.randbytes(nl)
            ct = uaes.AES_EAX_encrypt(key, nonce, aad, pt, tag_len=tl)
            assert ct == R.eax_composed(key, nonce, aad, pt, tl)
            assert uaes.AES_EAX_decrypt(key, nonce, aad, ct, tag_len=tl) == (0, pt)


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def test_reference_builds_with_other_eax_lengths():
    """the three EAX_NONCE_LEN / EAX_TAG_LEN builds agree with the composition from the reference's CMAC and block
    cipher (which stands in for them at every other length), and their decryption accepts their own output"""
    rng = random.Random(21)
    for (bits, nl, tl) in R.EAX_LENS:
        for n in (0, 1, 16, 17, 300, 20000):
            key, nonce, aad, pt = rng.randbytes(bits // 8), rng.randbytes(nl), rng.randbytes(n % 41), rng.randbytes(n)
            ct = R.eax_encrypt_lens(bits, nl, tl, key, nonce, aad, pt)
            assert len(ct) == n + tl and ct == R.eax_composed(key, nonce, aad, pt, tl, bits), (bits, nl, tl, n)
            assert R.eax_decrypt_lens(bits, nl, tl, key, nonce, aad, ct) == (0, pt), (bits, nl, tl, n)
            assert R.eax_decrypt_lens(bits, nl, tl, key, nonce, aad, flip(ct, 8 * n + 3), 0x5C) == (0x1A, b"\x5c" * n)
    key, nonce, aad, pt = rng.randbytes(16), rng.randbytes(16), rng.randbytes(9), rng.randbytes(100)
    for bits in (128, 192, 256):                               # the composition at 16 / 16 against the default builds
        key = rng.randbytes(bits // 8)
        assert R.eax_composed(key, nonce, aad, pt, 16, bits) == R.eax_encrypt(bits, key, nonce, aad, pt)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_eax_length_matrix(host_forced, bits):
    """every nonce length x tag length of the matrix x texts on both sides of the small / long boundary: the pair
    this key size has a reference build for against that build, the rest against the composition; a truncated tag is
    accepted, a flip of each of its bytes rejected with the output untouched"""
    rng = random.Random(1000 + bits)
    small = uaes.eax_siv_plan(False, 0)[3]
    for nl in R.NONCE_LENS:
        for tl in R.TAG_LENS:
            key, nonce = rng.randbytes(bits // 8), rng.randbytes(nl)
            for n in (0, 1, 16, 17, 300 + nl % 16, small, small + 1):
                aad, pt = rng.randbytes((n + tl) % 50), rng.randbytes(n)
                info = (bits, nl, tl, n)
                want = R.eax_expected(bits, key, nonce, aad, pt, tl)
                assert uaes.AES_EAX_encrypt(key, nonce, aad, pt, tag_len=tl) == want, info
                assert uaes.AES_EAX_decrypt(key, nonce, aad, want, tag_len=tl) == (0, pt), info
                for i in range(tl if n in (0, 17, small + 1) else 0):
                    bad = bytearray(want)
                    bad[n + i] ^= 1 << rng.randrange(8)
                    assert uaes.AES_EAX_decrypt(key, nonce, aad, bytes(bad), prefill=0x5C, tag_len=tl) == \
                        (0x1A, b"\x5c" * n), info + (i,)
    done = [k for k in R.EAX_LENS if k[0] == bits]
    assert len(done) == 1 and done[0][1] in R.NONCE_LENS and done[0][2] in R.TAG_LENS     # the build's pair was in the loop


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_long_associated_data(host_forced, bits):
    rng = random.Random(2000 + bits)
    small = uaes.eax_siv_plan(False, 0)[3]
    (nl, tl), = [k[1:] for k in R.EAX_LENS if k[0] == bits]
    key, keys = rng.randbytes(bits // 8), rng.randbytes(bits // 4)
    for alen in R.AAD_LENS:
        aad = rng.randbytes(alen)
        for n in (0, 5, small, small + 1, alen):
            pt = rng.randbytes(n)
            for nlen, tlen in ((nl, tl), (16, 16)):
                nonce = rng.randbytes(nlen)
                want = R.eax_encrypt_lens(bits, nlen, tlen, key, nonce, aad, pt)
                assert uaes.AES_EAX_encrypt(key, nonce, aad, pt, tag_len=tlen) == want, (bits, alen, n, nlen)
                assert uaes.AES_EAX_decrypt(key, nonce, aad, want, tag_len=tlen) == (0, pt), (bits, alen, n, nlen)
                other = flip(aad, 8 * alen - 1)
                rc = R.eax_verdict(bits, key, nonce, other, want, tlen)            # (a one-byte tag can match by chance)
                assert rc == 0x1A or tlen < 3
                assert uaes.AES_EAX_decrypt(key, nonce, other, want, prefill=0x5C, tag_len=tlen) == \
                    (rc, b"\x5c" * n if rc else pt), (bits, alen, n, nlen)
            iv, sct = uaes.AES_SIV_encrypt(keys, aad, pt)
            assert (iv, sct) == R.siv_encrypt(bits, keys, aad, pt), (bits, alen, n)
            assert uaes.AES_SIV_decrypt(keys, iv, aad, sct) == (0, pt), (bits, alen, n)
            assert uaes.AES_SIV_decrypt(keys, iv, flip(aad, 8 * alen - 1), sct)[0] == 0x1A, (bits, alen, n)


def test_forgeries(host_forced):
    rng = random.Random(11)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    aad, pt, nonce = rng.randbytes(20), rng.randbytes(70), rng.randbytes(16)
    ct = uaes.AES_EAX_encrypt(key, nonce, aad, pt)
    for args in ((nonce, aad, flip(ct, len(pt) * 8 + 3)), (nonce, aad, flip(ct, 5)), (nonce, flip(aad, 9), ct),
                 (flip(nonce, 1), aad, ct)):
        assert uaes.AES_EAX_decrypt(key, *args, prefill=0x5C) == (0x1A, b"\x5c" * len(pt))
    iv, sct = uaes.AES_SIV_encrypt(keys, aad, pt)
    for args in ((flip(iv, 2), aad, sct), (iv, aad, flip(sct, 30)), (iv, flip(aad, 4), sct)):
        rc, text = uaes.AES_SIV_decrypt(keys, *args, prefill=0x5C)
        assert rc == 0x1A
        assert text == R.siv_decrypt_rc(128, keys, args[0], args[1], args[2])[1]
    eng = uaes.engine()
    eng.uaes_set_wipe_on_auth_failure(1)
    try:
        assert uaes.AES_SIV_decrypt(keys, iv, aad, flip(sct, 3), prefill=0x5C) == (0x1A, bytes(len(pt)))
    finally:
        eng.uaes_set_wipe_on_auth_failure(0)


def test_drop_in_header_switches(tmp_path):
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "e.c"
    src.write_text('#include "micro_aes.h"\n'
                   "#if EAX != 1 || SIV != 1\n#error switch\n#endif\n"
                   "void (*ee)(const uint8_t *, const uint8_t *, const void *, const size_t, const void *, const size_t,"
                   " void *) = AES_EAX_encrypt;\n"
                   "char (*ed)(const uint8_t *, const uint8_t *, const void *, const size_t, const void *, const size_t,"
                   " void *) = AES_EAX_decrypt;\n"
                   "void (*se)(const uint8_t *, const void *, const size_t, const void *, const size_t, uint8_t *,"
                   " void *) = AES_SIV_encrypt;\n"
                   "char (*sd)(const uint8_t *, const uint8_t *, const void *, const size_t, const void *, const size_t,"
                   " void *) = AES_SIV_decrypt;\n"
                   "int nl(void) { return EAX_NONCE_LEN * 100 + EAX_TAG_LEN; }\n"
                   "int main(void) { return ee == 0 || ed == 0 || se == 0 || sd == 0; }\n")
    for extra in ([], ["-DEAX_NONCE_LEN=12", "-DEAX_TAG_LEN=8"]):
        subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-DEAX=1", "-DSIV=1"] + extra + ["-I", inc,
                        "-c", str(src), "-o", str(tmp_path / "e.o")], check=True)
    # the _lens builds bind to the general entry points; the default one to AES_EAX_encrypt itself
    probe = tmp_path / "p.c"
    probe.write_text('#include <stdio.h>\n#include "micro_aes.h"\n'
                     "void (*volatile f)(const uint8_t *, const uint8_t *, const void *, const size_t, const void *,"
                     " const size_t, void *) = AES_EAX_encrypt;\n"
                     "int main(void) { printf(\"%d %d\\n\", (int)EAX_NONCE_LEN, (int)EAX_TAG_LEN); return f == 0; }\n")
    for extra, want in (([], "16 16"), (["-DEAX_NONCE_LEN=12", "-DEAX_TAG_LEN=8"], "12 8")):
        exe = tmp_path / "p"
        subprocess.run(["gcc", "-DEAX=1", "-DAES___=128"] + extra + ["-I", inc, str(probe), "-o", str(exe),
                        "-L", os.path.dirname(uaes.lib_path()), "-lmicro_aes_hip_128",
                        "-Wl,-rpath," + os.path.dirname(uaes.lib_path())], check=True)
        out = subprocess.run(["nm", "-u", str(exe)], check=True, capture_output=True, text=True).stdout
        assert ("AES_EAX_encrypt_lens" in out) == bool(extra)
        assert ("AES_EAX_encrypt\n" in out) == (not extra)
        assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == want.split()
    dflt = tmp_path / "d.c"
    dflt.write_text('#include "micro_aes.h"\n#if EAX != 0 || SIV != 0 || KWA != 0 || FPE != 0 || EAXP != 0\n'
                    "#error default\n#endif\nint main(void) { return 0; }\n")
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I", inc, "-c", str(dflt), "-o",
                    str(tmp_path / "d.o")], check=True)
    for bits in (128, 192, 256):
        lib = C.CDLL(uaes.lib_path("libmicro_aes_hip_%d.so" % bits))
        for name in ("AES_EAX_encrypt", "AES_EAX_decrypt", "AES_EAX_encrypt_lens", "AES_EAX_decrypt_lens",
                     "AES_SIV_encrypt", "AES_SIV_decrypt"):
            assert getattr(lib, name) is not None


def test_planner_without_a_device():
    small = uaes.eax_siv_plan(False, 0)[3]
    assert small == 16384
    for siv in (False, True):
        pre = "s2v" if siv else "eax"
        for dec in (False, True):
            assert uaes.eax_siv_plan(siv, small, decrypt=dec)[:2] == (pre + ".small", 1)
            name, launches, _, _ = uaes.eax_siv_plan(siv, small + 1, decrypt=dec)
            assert name == pre + ".long" and launches == (3 if not siv and not dec else 2)
        assert uaes.eax_siv_plan(siv, 4096, nmsg=4096)[:2] == (pre + ".batch", 1)
    assert uaes.engine().uaes_debug_plan_eax_siv(2, 0, 16, 1, None) is None
