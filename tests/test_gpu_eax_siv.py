"""EAX and SIV (RFC 5297) on the GPU (uaes_eax_siv.hip) against the compiled reference: every short length, the
small / long boundary read from the plan, long texts, in-place and device-pointer calls, two threads, chosen counter
blocks (the 56-bit wrap, SIV's carry across the cleared bit 31) and batches with forged records."""
import ctypes as C
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests import eax_siv_ref as R

pytestmark = pytest.mark.gpu


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def check_eax(bits, key, nonce, aad, pt):
    want = R.eax_encrypt(bits, key, nonce, aad, pt)
    ct = uaes.AES_EAX_encrypt(key, nonce, aad, pt)
    assert ct == want, (len(aad), len(pt))
    assert uaes.AES_EAX_decrypt(key, nonce, aad, ct) == (0, pt)
    assert uaes.AES_EAX_decrypt(key, nonce, aad, flip(ct, 8 * len(ct) - 5), prefill=0x3C) == (0x1A, b"\x3c" * len(pt))


def check_siv(bits, keys, aad, pt):
    want = R.siv_encrypt(bits, keys, aad, pt)
    got = uaes.AES_SIV_encrypt(keys, aad, pt)
    assert got == want, (len(aad), len(pt))
    assert uaes.AES_SIV_decrypt(keys, got[0], aad, got[1]) == (0, pt)
    rc, text = uaes.AES_SIV_decrypt(keys, flip(got[0], 77), aad, got[1])
    assert rc == 0x1A and text == R.siv_decrypt_rc(bits, keys, flip(got[0], 77), aad, got[1])[1]


def test_every_short_length():
    rng = random.Random(1)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    for n in range(301):
        aad, pt, nonce = rng.randbytes(n % 49), rng.randbytes(n), rng.randbytes(16)
        check_eax(128, key, nonce, aad, pt)
        check_siv(128, keys, aad, pt)


@pytest.mark.parametrize("bits", [192, 256])
def test_key_sizes(bits):
    rng = random.Random(bits)
    kb = bits // 8
    for n in (0, 15, 16, 33, 300, 20000):
        check_eax(bits, rng.randbytes(kb), rng.randbytes(16), rng.randbytes(n % 37), rng.randbytes(n))
        check_siv(bits, rng.randbytes(2 * kb), rng.randbytes(n % 37), rng.randbytes(n))


def test_small_long_boundary_from_the_plan():
    rng = random.Random(2)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    small = uaes.eax_siv_plan(False, 0)[3]
    assert uaes.eax_siv_plan(False, small)[0] == "eax.small" and uaes.eax_siv_plan(False, small + 1)[0] == "eax.long"
    assert uaes.eax_siv_plan(True, small)[0] == "s2v.small" and uaes.eax_siv_plan(True, small + 1)[0] == "s2v.long"
    for n in (small - 16, small - 1, small, small + 1, small + 16):
        aad = rng.randbytes(n % 29)
        check_eax(128, key, rng.randbytes(16), aad, rng.randbytes(n))
        check_siv(128, keys, aad, rng.randbytes(n))


@pytest.mark.parametrize("n", [1 << 20, (16 << 20) + 5])
def test_long_texts(n):
    rng = random.Random(n)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    pt, aad, nonce = rng.randbytes(n), rng.randbytes(100), rng.randbytes(16)
    ct = uaes.AES_EAX_encrypt(key, nonce, aad, pt)
    assert ct == R.eax_encrypt(128, key, nonce, aad, pt)
    assert uaes.AES_EAX_decrypt(key, nonce, aad, ct) == (0, pt)
    iv, sct = uaes.AES_SIV_encrypt(keys, aad, pt)
    assert (iv, sct) == R.siv_encrypt(128, keys, aad, pt)
    assert uaes.AES_SIV_decrypt(keys, iv, aad, sct) == (0, pt)


def test_in_place_and_device_pointers():
    import torch
    L = uaes.engine()
    rng = random.Random(3)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    for n in (0, 5, 100, 4096, 40000):
        pt, aad, nonce = rng.randbytes(n), rng.randbytes(21), rng.randbytes(16)
        want = R.eax_encrypt(128, key, nonce, aad, pt)
        buf = (C.c_uint8 * (n + 16)).from_buffer_copy(pt + bytes(16))                 # host, in place
        assert L.uaes_eax_encrypt(128, key, nonce, 16, 16, aad, len(aad), buf, n, buf) == 0
        assert bytes(buf) == want
        assert L.uaes_eax_decrypt(128, key, nonce, 16, 16, aad, len(aad), buf, n, buf) == 0
        assert bytes(buf)[:n] == pt
        iv, sct = R.siv_encrypt(128, keys, aad, pt)
        sbuf = (C.c_uint8 * max(n, 1)).from_buffer_copy(pt or b"\0")
        ivb = (C.c_uint8 * 16)()
        assert L.uaes_siv_encrypt(128, keys, aad, len(aad), sbuf, n, ivb, sbuf) == 0
        assert bytes(ivb) == iv and bytes(sbuf)[:n] == sct
        assert L.uaes_siv_decrypt(128, keys, ivb, aad, len(aad), sbuf, n, sbuf) == 0
        assert bytes(sbuf)[:n] == pt
        # device memory: text, AAD, nonce and IV as torch tensors
        d = torch.tensor(list(pt + bytes(16)), dtype=torch.uint8, device="cuda")
        da = torch.tensor(list(aad), dtype=torch.uint8, device="cuda")
        dn = torch.tensor(list(nonce), dtype=torch.uint8, device="cuda")
        div = torch.zeros(16, dtype=torch.uint8, device="cuda")
        p = C.c_void_p(d.data_ptr())
        assert L.uaes_eax_encrypt(128, key, C.c_void_p(dn.data_ptr()), 16, 16, C.c_void_p(da.data_ptr()), len(aad), p, n, p) == 0
        assert bytes(d.cpu().numpy()) == want
        assert L.uaes_eax_decrypt(128, key, C.c_void_p(dn.data_ptr()), 16, 16, C.c_void_p(da.data_ptr()), len(aad), p, n, p) == 0
        assert bytes(d.cpu().numpy())[:n] == pt
        assert L.uaes_siv_encrypt(128, keys, C.c_void_p(da.data_ptr()), len(aad), p, n, C.c_void_p(div.data_ptr()), p) == 0
        assert bytes(div.cpu().numpy()) == iv and bytes(d.cpu().numpy())[:n] == sct
        assert L.uaes_siv_decrypt(128, keys, C.c_void_p(div.data_ptr()), C.c_void_p(da.data_ptr()), len(aad), p, n, p) == 0
        assert bytes(d.cpu().numpy())[:n] == pt


def test_two_threads_with_different_keys():
    """the reference keeps its round keys in a global: its answers are made here, the threads only call the engine"""
    cases = {}
    for seed in (10, 20):
        rng = random.Random(seed)
        key, keys = rng.randbytes(16), rng.randbytes(32)
        cases[seed] = []
        for n in (0, 17, 1000, 17000, 100, 40000):
            aad, pt, nonce = rng.randbytes(n % 31), rng.randbytes(n), rng.randbytes(16)
            cases[seed].append((key, keys, nonce, aad, pt, R.eax_encrypt(128, key, nonce, aad, pt),
                                R.siv_encrypt(128, keys, aad, pt)))
    errors = []

    def worker(seed):
        try:
            for _ in range(3):
                for key, keys, nonce, aad, pt, ect, sv in cases[seed]:
                    assert uaes.AES_EAX_encrypt(key, nonce, aad, pt) == ect, len(pt)
                    assert uaes.AES_EAX_decrypt(key, nonce, aad, ect) == (0, pt), len(pt)
                    assert uaes.AES_SIV_encrypt(keys, aad, pt) == sv, len(pt)
                    assert uaes.AES_SIV_decrypt(keys, sv[0], aad, sv[1]) == (0, pt), len(pt)
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(s,)) for s in (10, 20)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


CTRS = []
for low in (0x00, 0x01, 0x80, 0xFF):
    CTRS.append(bytes(9) + bytes(6) + bytes([low]))                                      # plain
CTRS.append(bytes(9) + b"\xff" * 6 + b"\xf0")                                           # the 56-bit wrap
CTRS.append(bytes(9) + b"\x12\x34" + b"\x7f" + b"\xff\xff\xff" + b"\xf0")              # carry into byte 11


@pytest.mark.parametrize("n", [300, 40000])
def test_chosen_counters(n):
    rng = random.Random(n)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    for target in CTRS:
        nonce = R.eax_nonce_for(128, key, target)
        assert R.omac(key, 0, nonce) == target
        check_eax(128, key, nonce, b"hdr", rng.randbytes(n))
    for target in CTRS:
        v = bytearray(target)
        v[8] |= 0x80                       # cleared by the mask: the counter is the same
        v[12] |= 0x80                      # bit 31 cleared: byte 12's low bits still carry into byte 11
        for vt in (bytes(target), bytes(v)):
            pt = R.siv_text_for(128, keys, b"aad", rng.randbytes(n - n % 16 - 16), vt)
            iv, _ = R.siv_encrypt(128, keys, b"aad", pt)
            assert iv == vt
            check_siv(128, keys, b"aad", pt)


@pytest.mark.parametrize("nmsg", [1, 63, 64, 65, 4096])
@pytest.mark.parametrize("msg_bytes", [0, 1, 16, 17, 4096])
@pytest.mark.parametrize("aad_bytes", [0, 13])
def test_batches(nmsg, msg_bytes, aad_bytes):
    rng = random.Random(nmsg * 7919 + msg_bytes * 31 + aad_bytes)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    texts = [rng.randbytes(msg_bytes) for _ in range(nmsg)]
    aads = [rng.randbytes(aad_bytes) for _ in range(nmsg)]
    nonces = [rng.randbytes(16) for _ in range(nmsg)]
    check = range(nmsg) if nmsg <= 65 else rng.sample(range(nmsg), 40)
    cts, tags = uaes.eax_batch(key, nonces, aads, texts)
    for m in check:
        assert cts[m] + tags[m] == R.eax_encrypt(128, key, nonces[m], aads[m], texts[m]), m
    ivs, scts = uaes.siv_batch(keys, aads, texts)
    for m in check:
        assert (ivs[m], scts[m]) == R.siv_encrypt(128, keys, aads[m], texts[m]), m
    bad = set(rng.sample(range(nmsg), min(3, nmsg)))
    ftags = [flip(t, 5) if m in bad else t for m, t in enumerate(tags)]
    rc, pts, verdicts = uaes.eax_batch(key, nonces, aads, cts, decrypt=True, tags=ftags, prefill=0x77)
    assert rc == 0x1A and verdicts == [0 if m in bad else 1 for m in range(nmsg)]
    for m in range(nmsg):
        assert pts[m] == (b"\x77" * msg_bytes if m in bad else texts[m]), m
    fivs = [flip(v, 9) if m in bad else v for m, v in enumerate(ivs)]
    rc, pts, verdicts = uaes.siv_batch(keys, aads, scts, decrypt=True, ivs=fivs)
    assert rc == 0x1A and verdicts == [0 if m in bad else 1 for m in range(nmsg)]
    for m in range(nmsg):
        if m not in bad:
            assert pts[m] == texts[m], m
    assert uaes.eax_batch(key, nonces, aads, cts, decrypt=True, tags=tags)[:2] == (0, texts)
    assert uaes.siv_batch(keys, aads, scts, decrypt=True, ivs=ivs)[:2] == (0, texts)


def test_siv_batch_wipe_switch():
    rng = random.Random(5)
    keys = rng.randbytes(32)
    texts = [rng.randbytes(40) for _ in range(8)]
    ivs, scts = uaes.siv_batch(keys, None, texts)
    fivs = [flip(v, 3) if m == 2 else v for m, v in enumerate(ivs)]
    eng = uaes.engine()
    eng.uaes_set_wipe_on_auth_failure(1)
    try:
        rc, pts, verdicts = uaes.siv_batch(keys, None, scts, decrypt=True, ivs=fivs, prefill=0x55)
    finally:
        eng.uaes_set_wipe_on_auth_failure(0)
    assert rc == 0x1A and verdicts == [1, 1, 0, 1, 1, 1, 1, 1]
    assert pts[2] == bytes(40) and [p for m, p in enumerate(pts) if m != 2] == [t for m, t in enumerate(texts) if m != 2]
