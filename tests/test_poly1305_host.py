"""Poly1305-AES without a GPU: the arithmetic restated in Python big integers (checked against the reference's short
vectors, its main.c known answers and the compiled reference up to 64 KiB), the library's host path against that
restatement, the drop-in header's POLY1305 switch and the planner of uaes_poly1305.hip.  tests/test_gpu_poly1305.py reuses the
restatement for the kernels."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import micro_aes_amd as uaes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 130) - 5
CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF


def clamp(r16):
    return int.from_bytes(r16, "little") & CLAMP


def block(chunk):
    """c_i = the chunk as a little-endian integer + 2^(8 len)"""
    return int.from_bytes(chunk, "little") + (1 << (8 * len(chunk)))


def poly_h(r, msg, h=0):
    """Horner over the message: h = (h + c_i) r mod p (h = sum c_i r^(q-i+1))"""
    for i in range(0, len(msg), 16):
        h = (h + block(msg[i:i + 16])) * r % P
    return h


def tag(h, s):
    return ((h + s) % (1 << 128)).to_bytes(16, "little")


def aes_s(orc, keys, nonce):
    return int.from_bytes(orc.encrypt_block(keys[:-16], nonce), "little")


def poly1305_aes(orc, keys, nonce, msg):
    """micro_aes.c:1955-1997 restated: keys = k || r, mac = (h + AES_k(nonce)) mod 2^128"""
    return tag(poly_h(clamp(keys[-16:]), msg), aes_s(orc, keys, nonce))


def tv_vectors(golden):
    """the reference's Poly1305AES128.tv vectors kept in tests/golden/poly1305_vectors.json: (keys, nonce, msg, mac)"""
    d = json.load(open(os.path.join(golden, "poly1305_vectors.json")))
    return [tuple(bytes.fromhex(v[f]) for f in ("keys", "nonce", "msg", "mac")) for v in d["vectors"]]


def kats(golden):
    d = json.load(open(os.path.join(golden, "poly1305_kats.json")))
    return [tuple(bytes.fromhex(k[f]) for f in ("keys", "nonce", "msg", "mac")) for k in d["kats"]]


def test_restatement_matches_the_vector_file_and_the_papers_kats(orc, golden_dir):
    vs = tv_vectors(golden_dir)
    assert len(vs) == 80 and sorted(set(len(v[2]) for v in vs)) == [0, 16, 32, 33, 37]
    for keys, nonce, msg, mac in vs + kats(golden_dir):
        assert poly1305_aes(orc, keys, nonce, msg) == mac


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_restatement_matches_the_compiled_reference(orc, bits):
    from oracle.pyoracle import Reference
    from tests.refbuilt import missing
    if not Reference.available(bits):
        missing("oracle/_ref/libmicroaes_ref_%d.so" % bits)
    L = Reference(bits).L
    L.AES_Poly1305.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.AES_Poly1305.restype = None
    rng = random.Random(bits)
    for n in [0, 1, 15, 16, 17, 300, 4097, 65536, 65536 + 5] + [rng.randrange(301) for _ in range(60)]:
        keys = bytes(rng.randrange(256) for _ in range(bits // 8 + 16))
        if n % 3 == 0:
            keys = keys[:-16] + b"\xff" * 16                      # the largest clamped r
        nonce = bytes(rng.randrange(256) for _ in range(16))
        msg = b"\xff" * n if n % 2 else bytes(rng.randrange(256) for _ in range(n))
        out = (C.c_uint8 * 16)()
        L.AES_Poly1305(keys, nonce, msg, n, out)
        assert bytes(out) == poly1305_aes(orc, keys, nonce, msg), (bits, n)


@pytest.fixture()
def host_forced():
    prev = uaes.host_policy(1 << 62, 1, 1)
    yield
    uaes.host_policy(*prev)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_host_path_matches_the_restatement(host_forced, orc, golden_dir, bits):
    rng = random.Random(7 + bits)
    cases = [(k, n, m) for k, n, m, _ in tv_vectors(golden_dir)[::7]] if bits == 128 else []
    for n in list(range(0, 70)) + [255, 256, 257, 4095, 4096, 4097, 65536 + 5]:
        keys = bytes(rng.randrange(256) for _ in range(bits // 8 + 16))
        if n % 4 == 1:
            keys = keys[:-16] + b"\xff" * 16
        msg = b"\xff" * n if n % 3 == 0 else bytes(rng.randrange(256) for _ in range(n))
        cases.append((keys, bytes(rng.randrange(256) for _ in range(16)), msg))
    for keys, nonce, msg in cases:
        assert uaes.AES_Poly1305(keys, nonce, msg) == poly1305_aes(orc, keys, nonce, msg), (bits, len(msg))


def test_host_path_follows_the_policy_limit(orc):
    """max_bytes decides which calls the host takes; without a device the rest fail loudly (GPU-less box) or run on
    the GPU -- either way the host never answers for a longer message than it was given"""
    import torch
    keys, nonce = bytes(range(48)), bytes(16)
    prev = uaes.host_policy(64, 0, 0)
    try:
        assert uaes.AES_Poly1305(keys, nonce, b"a" * 64) == poly1305_aes(orc, keys, nonce, b"a" * 64)
        if not torch.cuda.is_available():
            with pytest.raises(uaes.EngineError, match="no usable HIP device"):
                uaes.AES_Poly1305(keys, nonce, b"a" * 65)
    finally:
        uaes.host_policy(*prev)


def test_bad_arguments_fail_before_any_device_work():
    L = uaes.engine()
    mac = (C.c_uint8 * 16)()
    assert L.uaes_poly1305(100, bytes(48), bytes(16), b"x", 1, mac) == -2          # UAES_E_ARG
    assert L.uaes_poly1305(128, bytes(32), bytes(16), None, 5, mac) == -2
    assert L.uaes_poly1305_dev(100, bytes(48), bytes(16), None, 0, None, None) == -2
    assert L.uaes_poly1305_batch(128, bytes(32), None, 3, 16, None, mac) == -2
    with pytest.raises(ValueError):
        uaes.AES_Poly1305(bytes(33), bytes(16), b"")


def test_drop_in_header_switch(tmp_path):
    """-DPOLY1305=1 declares AES_Poly1305 with the reference's signature (a c89 caller); the default build sees 0"""
    src = tmp_path / "p.c"
    src.write_text('#include "micro_aes.h"\n'
                   "#if POLY1305 != 1\n#error switch\n#endif\n"
                   "void (*f)(const uint8_t *, const uint8_t *, const void *, const size_t, uint8_t *) = AES_Poly1305;\n"
                   "int main(void) { return f == 0; }\n")
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-DPOLY1305=1", "-I", os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "p.o")], check=True)
    dflt = tmp_path / "d.c"
    dflt.write_text('#include "micro_aes.h"\n#if POLY1305 != 0\n#error default\n#endif\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-c", str(dflt), "-o", str(tmp_path / "d.o")], check=True)
    for bits in (128, 192, 256):
        assert C.CDLL(uaes.lib_path("libmicro_aes_hip_%d.so" % bits)).AES_Poly1305 is not None


def test_planner_without_a_device():
    seen, order = [], ["poly.small", "poly.chunks"]
    last = 0
    for n in [0, 1, 16, 1024, 65536, 1 << 17, (1 << 17) + 16, 1 << 20, 1 << 26, 1 << 30, (4 << 30) + 5]:
        name, launches, grid, steps = uaes.poly1305_plan(n)
        assert order.index(name) >= last, n                  # a longer message never goes back to a smaller row
        last = order.index(name)
        seen.append(name)
        assert launches == (1 if name == "poly.small" else 2)
        assert grid * 256 * steps * 16 >= n and grid >= 1
    assert set(seen) == set(order)
    name, launches, grid, steps = uaes.poly1305_plan(1024, 81919)
    assert (name, launches, steps) == ("poly.batch", 1, 1) and grid >= 1
    assert uaes.poly1305_plan(0, 7)[0] == "poly.batch"


def test_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.kernels() if k["name"].startswith("void k_poly_")]
    assert len(ks) == 17
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] <= 128, (k["name"][:60], k)
