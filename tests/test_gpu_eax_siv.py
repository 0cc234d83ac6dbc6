"""EAX and SIV (RFC 5297) on the GPU (uaes_eax_siv.hip) against the compiled reference: every short length, the
small / long boundary read from the plan, long texts, in-place and device-pointer calls, two threads, chosen counter
blocks (the 56-bit wrap, SIV's carry across the cleared bit 31, the striped CTR size) and batches with forged records;
the nonce x tag length matrix (tests/eax_siv_ref.py: three pairs against reference builds with those lengths, the
rest against the composition from the reference's CMAC and block cipher), forgeries of every part of a message, long
associated data and the lane scratch it shares with the GCM key cache, batch shapes derived from the device's CU
count with every record compared, batches in device memory / in place / at odd addresses with guard bytes, and the
published vectors through the kernels.  Every failing case prints the tuple that reproduces it."""
import ctypes as C
import itertools
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests import eax_siv_ref as R
from tests.guarded_mem import Mem, ptr

pytestmark = pytest.mark.gpu


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def eax(decrypt, bits, key, nonce, nl, tl, aad, al, src, n, dst):
    """uaes_eax_encrypt / uaes_eax_decrypt; nonce, aad: bytes or Mem, src / dst: Mem"""
    L = uaes.engine()
    return (L.uaes_eax_decrypt if decrypt else L.uaes_eax_encrypt)(bits, key, ptr(nonce), nl, tl, ptr(aad), al, ptr(src), n, ptr(dst))


def siv(decrypt, bits, keys, iv, aad, al, src, n, dst):
    L = uaes.engine()
    if decrypt:
        return L.uaes_siv_decrypt(bits, keys, ptr(iv), ptr(aad), al, ptr(src), n, ptr(dst))
    return L.uaes_siv_encrypt(bits, keys, ptr(aad), al, ptr(src), n, ptr(iv), ptr(dst))


def batch(is_siv, decrypt, bits, key, nmsg, ml, nonces, nl, aads, al, src, dst, tags, verdicts=None):
    """the four batch entry points; every array bytes or Mem (tags = the EAX tags or the SIV IVs)"""
    L = uaes.engine()
    if is_siv and decrypt:
        return L.uaes_siv_decrypt_batch(bits, key, nmsg, ml, ptr(aads), al, ptr(tags), ptr(src), ptr(dst), ptr(verdicts))
    if is_siv:
        return L.uaes_siv_encrypt_batch(bits, key, nmsg, ml, ptr(aads), al, ptr(src), ptr(tags), ptr(dst))
    if decrypt:
        return L.uaes_eax_decrypt_batch(bits, key, nmsg, ml, ptr(nonces), nl, ptr(aads), al, ptr(src), ptr(tags), ptr(dst),
                                        ptr(verdicts))
    return L.uaes_eax_encrypt_batch(bits, key, nmsg, ml, ptr(nonces), nl, ptr(aads), al, ptr(src), ptr(dst), ptr(tags))


def change(b, i):
    b = bytearray(b)
    b[i] ^= 0x40
    return bytes(b)


def small_max():
    return uaes.eax_siv_plan(False, 0)[3]


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
    cts, tags = uaes.eax_batch(key, nonces, aads, texts)
    for m, want in enumerate(R.eax_encrypt_records(128, key, nonces, aads, texts)):
        assert cts[m] + tags[m] == want, m
    ivs, scts = uaes.siv_batch(keys, aads, texts)
    for m, want in enumerate(R.siv_encrypt_records(128, keys, aads, texts)):
        assert (ivs[m], scts[m]) == want, m
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


# ---- the length matrix ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [128, 192, 256])
def test_eax_length_matrix(bits):
    """every nonce length x tag length of the matrix x texts in both arrangements: ciphertext and tag equal the
    reference's (the pair this key size has a reference build for against that build), nothing is written behind a
    truncated tag, decryption accepts the tag with garbage behind it in the caller's buffer and rejects a flip of EACH
    of its bytes with the output untouched"""
    rng = random.Random(3000 + bits)
    small = small_max()
    for nl in R.NONCE_LENS:
        for tl in R.TAG_LENS:
            key, nonce = rng.randbytes(bits // 8), rng.randbytes(nl)
            dnonce = Mem(nonce, True, off=1)                  # the same nonce in device memory at an odd address
            for n in (0, 1, 16, 17, 300 + nl % 16, small, small + 1):
                aad, pt = rng.randbytes((n + tl) % 50), rng.randbytes(n)
                info = (bits, nl, tl, n, len(aad))
                want = R.eax_expected(bits, key, nonce, aad, pt, tl)
                for nn in (nonce, dnonce):                    # a 16-byte aligned device output is written in place by
                    dst = Mem(size=n + tl, device=nn is dnonce, off=16)        # the kernels: a store behind the tag shows
                    assert eax(False, bits, key, nn, nl, tl, aad, len(aad), Mem(pt), n, dst) == 0, info + (nn is dnonce,)
                    assert dst.get() == want and dst.intact(n + tl), info + (nn is dnonce,)
                src, dst = Mem(want + rng.randbytes(16)), Mem(size=n)
                assert eax(True, bits, key, dnonce, nl, tl, aad, len(aad), src, n, dst) == 0, info
                assert dst.get() == pt and dst.intact(n), info
                for i in range(tl):
                    src, dst = Mem(change(want, n + i) + rng.randbytes(16)), Mem(size=n)
                    assert eax(True, bits, key, nonce, nl, tl, aad, len(aad), src, n, dst) == 0x1A, info + (i,)
                    assert dst.intact(0), info + (i,)


def test_eax_lengths_with_long_texts():
    """a few hundred KiB (eax.long: k_eax_macs modes 0, 1 and 2) at the three pairs with a reference build and a handful
    of others"""
    rng = random.Random(31)
    n = (300 << 10) + 5
    assert uaes.eax_siv_plan(False, n)[0] == "eax.long"
    for bits, nl, tl in list(R.EAX_LENS) + [(128, 1, 15), (192, 17, 2), (256, 1000, 7), (128, 31, 13), (256, 0, 16),
                                            (192, 5, 1)]:
        key, nonce, aad, pt = rng.randbytes(bits // 8), rng.randbytes(nl), rng.randbytes(77), rng.randbytes(n)
        info = (bits, nl, tl)
        want = R.eax_expected(bits, key, nonce, aad, pt, tl)
        for device in (False, True):                         # (16-byte aligned device memory is written by the kernels themselves)
            dst = Mem(size=n + tl, device=device, off=16)
            assert eax(False, bits, key, nonce, nl, tl, aad, len(aad), Mem(pt, device), n, dst) == 0, info
            assert dst.get() == want and dst.intact(n + tl), info + (device,)
        src, dst = Mem(want + rng.randbytes(16), True, off=16), Mem(size=n, device=True, off=32)
        assert eax(True, bits, key, nonce, nl, tl, aad, len(aad), src, n, dst) == 0, info
        assert dst.get() == pt and dst.intact(n), info
        for i in range(tl):
            src, dst = Mem(change(want, n + i) + rng.randbytes(16), i % 2 == 1, off=16 * (i % 3)), Mem(size=n, device=i % 4 > 1)
            assert eax(True, bits, key, nonce, nl, tl, aad, len(aad), src, n, dst) == 0x1A, info + (i,)
            assert dst.intact(0), info + (i,)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_forgeries_of_every_part(device):
    """one changed byte in the text's first block, last whole block and ragged tail, in the AAD, in the nonce (EAX) or
    the IV (SIV), in both arrangements: EAX leaves the output untouched, SIV leaves what the reference leaves and zeros
    under uaes_set_wipe_on_auth_failure(1)"""
    rng = random.Random(41)
    eng = uaes.engine()
    small = small_max()
    for bits, n in itertools.product((128, 256), (16 * 19 + 9, small + 16 * 3 + 9)):
        key, keys = rng.randbytes(bits // 8), rng.randbytes(bits // 4)
        nonce, aad, pt = rng.randbytes(16), rng.randbytes(45), rng.randbytes(n)
        spots = (3, n - n % 16 - 5, n - 2)
        ct = R.eax_encrypt(bits, key, nonce, aad, pt)
        for nn, aa, cc in [(nonce, aad, change(ct, i)) for i in spots] + [(nonce, change(aad, 44), ct), (change(nonce, 11), aad, ct)]:
            info = ("eax", bits, n, device, nn != nonce, aa != aad, cc != ct)
            dst = Mem(b"\x3c" * n, device, off=5)
            rc = eax(True, bits, key, Mem(nn, device, off=1), 16, 16, Mem(aa, device, off=3), len(aa), Mem(cc, device, off=1), n, dst)
            assert rc == 0x1A and dst.get() == b"\x3c" * n and dst.intact(n), info
        iv, sct = R.siv_encrypt(bits, keys, aad, pt)
        for wipe in (0, 1):
            for vv, aa, cc in [(iv, aad, change(sct, i)) for i in spots] + [(iv, change(aad, 44), sct), (change(iv, 6), aad, sct)]:
                info = ("siv", bits, n, device, wipe, vv != iv, aa != aad, cc != sct)
                left = R.siv_decrypt_rc(bits, keys, vv, aa, cc)
                assert left[0] == 0x1A
                dst = Mem(b"\x3c" * n, device, off=5)
                eng.uaes_set_wipe_on_auth_failure(wipe)
                try:
                    rc = siv(True, bits, keys, Mem(vv, device, off=1), Mem(aa, device, off=3), len(aa), Mem(cc, device, off=1), n, dst)
                finally:
                    eng.uaes_set_wipe_on_auth_failure(0)
                assert rc == 0x1A and dst.get() == (bytes(n) if wipe else left[1]) and dst.intact(n), info


def test_published_vectors_on_the_gpu(golden_dir):
    """the EAX paper's vectors and RFC 5297 A.1 through the kernels (the default policy: nothing runs on the host)"""
    cases = R.eax_vectors(golden_dir)
    assert len(cases) == 10
    for c in cases:
        ct = uaes.AES_EAX_encrypt(c["KEY"], c["NONCE"], c["HEADER"], c["MSG"])
        assert ct == c["CIPHER"]
        assert uaes.AES_EAX_decrypt(c["KEY"], c["NONCE"], c["HEADER"], ct) == (0, c["MSG"])
        assert uaes.AES_EAX_decrypt(c["KEY"], c["NONCE"], c["HEADER"], change(ct, 0), prefill=0x3C) == (0x1A, b"\x3c" * len(c["MSG"]))
        cts, tags = uaes.eax_batch(c["KEY"], [c["NONCE"]] * 3, [c["HEADER"]] * 3, [c["MSG"]] * 3)
        assert [a + b for a, b in zip(cts, tags)] == [c["CIPHER"]] * 3
    v = R.RFC5297_A1
    assert uaes.AES_SIV_encrypt(v["keys"], v["ad"], v["pt"]) == (v["iv"], v["ct"])
    assert uaes.AES_SIV_decrypt(v["keys"], v["iv"], v["ad"], v["ct"]) == (0, v["pt"])
    assert uaes.siv_batch(v["keys"], [v["ad"]] * 3, [v["pt"]] * 3) == ([v["iv"]] * 3, [v["ct"]] * 3)


# ---- long associated data ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [128, 192, 256])
def test_long_associated_data(bits):
    """AAD up to 1 MiB + 7 (whole row_walk chunks on the AAD wave, an AAD chain that outlasts the text's, a growing lane
    scratch), in host memory and in device memory at an odd address, with texts in both arrangements and one as long
    as the AAD; EAX with 16 / 16 and with this key size's reference-build lengths, SIV; both directions"""
    rng = random.Random(5000 + bits)
    small = small_max()
    (bnl, btl), = [k[1:] for k in R.EAX_LENS if k[0] == bits]
    key, keys = rng.randbytes(bits // 8), rng.randbytes(bits // 4)
    for alen in R.AAD_LENS:
        aad = rng.randbytes(alen)
        daad = Mem(aad, True, off=1)
        assert daad.ptr.value % 2 == 1
        for k, n in enumerate((0, 5, small, small + 1, alen)):
            pt = rng.randbytes(n)
            nl, tl = ((16, 16), (bnl, btl))[k % 2]
            nonce = rng.randbytes(nl)
            want = R.eax_encrypt_lens(bits, nl, tl, key, nonce, aad, pt)
            iv, sct = R.siv_encrypt(bits, keys, aad, pt)
            for a in (aad, daad):
                info = (bits, alen, n, nl, tl, a is daad)
                dst = Mem(size=n + tl)
                assert eax(False, bits, key, nonce, nl, tl, a, alen, Mem(pt), n, dst) == 0, info
                assert dst.get() == want and dst.intact(n + tl), info
                dst = Mem(size=n)
                assert eax(True, bits, key, nonce, nl, tl, a, alen, Mem(want), n, dst) == 0, info
                assert dst.get() == pt and dst.intact(n), info
                dst, div = Mem(size=n), Mem(size=16)
                assert siv(False, bits, keys, div, a, alen, Mem(pt), n, dst) == 0, info
                assert (div.get(), dst.get()) == (iv, sct) and dst.intact(n) and div.intact(16), info
                dst = Mem(size=n)
                assert siv(True, bits, keys, iv, a, alen, Mem(sct), n, dst) == 0, info
                assert dst.get() == pt and dst.intact(n), info
            # the last byte of the AAD counts
            other = change(aad, alen - 1)
            dst = Mem(size=n)
            rc = eax(True, bits, key, nonce, nl, tl, other, alen, Mem(want), n, dst)
            assert rc == R.eax_verdict(bits, key, nonce, other, want, tl) and (rc == 0x1A or tl < 3) and dst.intact(0 if rc else n)
            assert siv(True, bits, keys, iv, other, alen, Mem(sct), n, Mem(size=n)) == 0x1A


def test_lane_scratch_shared_with_the_gcm_key_cache():
    """The lane scratch that carries a host nonce and AAD to the device is where the thread's cached GCM key tables
    live, and its tail holds the counter word of the one-launch GCM forms.  One thread, one GCM key: GCM calls beyond
    gcm.small until the tables are cached, an EAX call whose AAD fits the scratch as it is, GCM again; an EAX call with
    1 MiB of AAD (the scratch grows), GCM again, a GCM-SIV call beyond siv.small, EAX and SIV once more, GCM again --
    every answer equals the compiled reference's."""
    from oracle.pyoracle import Reference
    ref = Reference(128)
    rng = random.Random(51)
    kg, ke, ks = rng.randbytes(16), rng.randbytes(16), rng.randbytes(32)
    ng = next(n for n in (1 << k for k in range(8, 26)) if uaes.plan("gcm", n)[0] != "gcm.small") + 5
    nsv = next(n for n in (1 << k for k in range(8, 26)) if uaes.plan("siv", n)[0] != "siv.small") + 5

    def gcm(n=ng):
        nonce, aad, data = rng.randbytes(12), rng.randbytes(33), rng.randbytes(n)
        want = ref.gcm_encrypt(kg, nonce, aad, data)
        assert uaes.AES_GCM_encrypt(kg, nonce, aad, data) == want, n
        assert uaes.AES_GCM_decrypt(kg, nonce, aad, want) == (0, data), n
        assert uaes.AES_GCM_decrypt(kg, nonce, aad, change(want, len(want) - 1))[0] == 0x1A

    def eax_call(alen, n):
        nonce, aad, pt = rng.randbytes(16), rng.randbytes(alen), rng.randbytes(n)
        want = R.eax_encrypt(128, ke, nonce, aad, pt)
        assert uaes.AES_EAX_encrypt(ke, nonce, aad, pt) == want, (alen, n)
        assert uaes.AES_EAX_decrypt(ke, nonce, aad, want) == (0, pt), (alen, n)

    def siv_call(alen, n):
        aad, pt = rng.randbytes(alen), rng.randbytes(n)
        want = R.siv_encrypt(128, ks, aad, pt)
        assert uaes.AES_SIV_encrypt(ks, aad, pt) == want, (alen, n)
        assert uaes.AES_SIV_decrypt(ks, want[0], aad, want[1]) == (0, pt), (alen, n)

    def gcmsiv():
        nonce, aad, data = rng.randbytes(12), rng.randbytes(20), rng.randbytes(nsv)
        assert uaes.GCM_SIV_encrypt(kg, nonce, aad, data) == ref.gcmsiv_encrypt(kg, nonce, aad, data)

    for _ in range(6):                                         # calls in a row under kg: its tables get built and cached
        gcm()
    for step in (lambda: eax_call(200, 1000), lambda: eax_call((1 << 20) + 7, 1000), gcmsiv,
                 lambda: eax_call(200, 40000), lambda: siv_call(200, 1000), lambda: siv_call((2 << 20) + 3, 40000),
                 lambda: eax_call((1 << 20) + 7, 40000)):
        step()
        gcm()
        gcm(100)
        for _ in range(5):                                     # ... and are cached again
            gcm()


# ---- batches ----------------------------------------------------------------------------------------------------------

def predicted_shape(nmsg, cus):
    """uaes_launch.hip.h's uaesk_row_shape: 256-thread workgroups (16 records each) while ceil(nmsg / 64) * 2 <= CUs, else
    1024-thread ones (64 records); as many workgroups as there are records to fill, at most one per CU"""
    wg = 256 if (nmsg + 63) // 64 * 2 <= cus else 1024
    rows = wg // 16
    grid = min((nmsg + rows - 1) // rows, cus)
    return wg, grid, (nmsg + grid * rows - 1) // (grid * rows)


def spread(rng, nmsg, rows_per_pass):
    """records in the first, last and middle rows of a batch, and on both sides of the first pass's end"""
    picks = {0, 1, 15, 16, 63, 64, nmsg // 2, nmsg - 1, nmsg - 2, rows_per_pass - 1, rows_per_pass, nmsg - rows_per_pass}
    picks |= set(rng.sample(range(nmsg), 6))
    return {m for m in picks if 0 <= m < nmsg}


SHAPE_COUNTS = ("16C", "16C+1", "32C", "32C+1", "64C", "64C+1", "192C+5")


@pytest.mark.parametrize("which", range(7), ids=SHAPE_COUNTS)
@pytest.mark.parametrize("ml", [0, 1, 48])
def test_batch_shapes_from_the_device(which, ml):
    """record counts on both sides of the first second pass of a 256-thread grid, of the switch to 1024-thread
    workgroups and of the first second pass of those; the plan must report the workgroup count this reading of
    uaesk_row_shape predicts; EVERY record against the reference, forged records in first, last and middle rows"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counts = (16 * cus, 16 * cus + 1, 32 * cus, 32 * cus + 1, 64 * cus, 64 * cus + 1, 3 * 64 * cus + 5)
    assert [predicted_shape(n, cus) for n in counts] == [(256, cus, 1), (256, cus, 2), (256, cus, 2), (1024, cus // 2 + 1, 1),
                                                         (1024, cus, 1), (1024, cus, 2), (1024, cus, 4)], cus
    nmsg = counts[which]
    wg, grid, _ = predicted_shape(nmsg, cus)
    for is_siv in (False, True):
        assert uaes.eax_siv_plan(is_siv, ml, nmsg)[::2] == ("s2v.batch" if is_siv else "eax.batch", grid)
        assert uaes.eax_siv_plan(is_siv, ml, nmsg, decrypt=True)[2] == grid
    rng = random.Random(which * 100 + ml)
    key, keys = rng.randbytes(16), rng.randbytes(32)
    blob = rng.randbytes(nmsg * (ml + 16 + 7))
    texts = [blob[m * ml:(m + 1) * ml] for m in range(nmsg)]
    nonces = [blob[nmsg * ml + 16 * m: nmsg * ml + 16 * m + 16] for m in range(nmsg)]
    aads = [blob[nmsg * (ml + 16) + 7 * m: nmsg * (ml + 16) + 7 * m + 7] for m in range(nmsg)]
    bad = spread(rng, nmsg, grid * (wg // 16))
    info = (SHAPE_COUNTS[which], nmsg, ml)
    cts, tags = uaes.eax_batch(key, nonces, aads, texts)
    for m, want in enumerate(R.eax_encrypt_records(128, key, nonces, aads, texts)):
        assert cts[m] + tags[m] == want, info + (m,)
    ftags = [change(t, m % 16) if m in bad else t for m, t in enumerate(tags)]
    rc, pts, verdicts = uaes.eax_batch(key, nonces, aads, cts, decrypt=True, tags=ftags, prefill=0x77)
    assert rc == 0x1A and verdicts == [0 if m in bad else 1 for m in range(nmsg)], info
    assert pts == [b"\x77" * ml if m in bad else texts[m] for m in range(nmsg)], info
    assert uaes.eax_batch(key, nonces, aads, cts, decrypt=True, tags=tags) == (0, texts, [1] * nmsg), info
    ivs, scts = uaes.siv_batch(keys, aads, texts)
    for m, want in enumerate(R.siv_encrypt_records(128, keys, aads, texts)):
        assert (ivs[m], scts[m]) == want, info + (m,)
    fivs = [change(v, m % 16) if m in bad else v for m, v in enumerate(ivs)]
    rc, pts, verdicts = uaes.siv_batch(keys, aads, scts, decrypt=True, ivs=fivs)
    assert rc == 0x1A and verdicts == [0 if m in bad else 1 for m in range(nmsg)], info
    for m in range(nmsg):
        assert pts[m] == (R.siv_decrypt_rc(128, keys, fivs[m], aads[m], scts[m])[1] if m in bad else texts[m]), info + (m,)
    assert uaes.siv_batch(keys, aads, scts, decrypt=True, ivs=ivs) == (0, texts, [1] * nmsg), info


def expected_records(is_siv, bits, key, nonces, aads, texts):
    """[(ct, tag or iv)] of every record by itself from the reference (EAX nonces of 16 bytes: its AES_EAX_encrypt;
    other lengths: the composition)"""
    if is_siv:
        return [(c, v) for v, c in R.siv_encrypt_records(bits, key, aads, texts)]
    if len(nonces[0]) == 16:
        return [(r[:-16], r[-16:]) for r in R.eax_encrypt_records(bits, key, nonces, aads, texts)]
    out = []
    for nonce, aad, pt in zip(nonces, aads, texts):
        r = R.eax_composed(key, nonce, aad, pt, 16, bits)
        out.append((r[:-16], r[-16:]))
    return out


BATCH_MSG = (15, 255, 256, 257, 272, 4099)
BATCH_NONCE = (0, 7, 12, 16, 33)
BATCH_AAD = (0, 1, 16, 300)
BATCH_COUNT = (1, 65, 1000)
_expected = {}


@pytest.mark.parametrize("place", ["host", "device", "device-in-place", "device-odd"])
def test_batch_lengths_key_sizes_and_placements(place):
    """batches under every key size, with nonce lengths whose odd strides put every second nonce at an odd address,
    AAD and record lengths beyond one row_walk chunk and ragged, in host memory / device memory / in place / with the
    text at an address that is 1 mod 4 (the A4 = false kernels even where msg_bytes % 4 == 0); guard bytes around the
    ciphertext, the tags / IVs and the verdicts; every record against the reference, three records forged.
    include/uaes_hip.h documents no constraint on a placement ("every array host or device memory")."""
    device = place != "host"
    toff = 1 if place == "device-odd" else 0
    seen = set()
    for i, (ml, nl, al) in enumerate(itertools.product(BATCH_MSG, BATCH_NONCE, BATCH_AAD)):
        nmsg = BATCH_COUNT[i % 3]                             # (every AAD length meets every count: 4 and 3 are coprime)
        bits = (192, 256, 128)[(i + i // 4) % 3]
        seen |= {(ml, nmsg), (nl, bits), (al, nmsg), (ml, bits)}
        rng = random.Random(7000 + i)
        key, keys = rng.randbytes(bits // 8), rng.randbytes(bits // 4)
        texts = [rng.randbytes(ml) for _ in range(nmsg)]
        nonces = [rng.randbytes(nl) for _ in range(nmsg)]
        aads = [rng.randbytes(al) for _ in range(nmsg)]
        bad = sorted({0, nmsg // 2, nmsg - 1})
        for is_siv in (False, True):
            info = (place, "siv" if is_siv else "eax", bits, nmsg, ml, nl, al)
            k = keys if is_siv else key
            if (i, is_siv) not in _expected:                  # (the same for every placement)
                _expected[i, is_siv] = expected_records(is_siv, bits, k, nonces, aads, texts)
            want = _expected[i, is_siv]
            dn, da = Mem(b"".join(nonces), device, off=toff), Mem(b"".join(aads), device, off=toff)
            src = Mem(b"".join(texts), device, off=toff)
            dst = src if place == "device-in-place" else Mem(size=nmsg * ml, device=device, off=toff)
            dt = Mem(size=16 * nmsg, device=device, off=toff)
            if toff:
                assert src.ptr.value % 4 == 1 and dst.ptr.value % 4 == 1
            assert batch(is_siv, False, bits, k, nmsg, ml, dn, nl, da, al, src, dst, dt) == 0, info
            got, gt = dst.get(nmsg * ml), dt.get()
            for m in range(nmsg):
                assert (got[m * ml:(m + 1) * ml], gt[16 * m:16 * m + 16]) == want[m], info + (m,)
            assert dst.intact(nmsg * ml) and dt.intact(16 * nmsg), info
            # decrypt, three records forged: a changed tag / IV byte, or a changed ciphertext byte
            ct = bytearray(b"".join(c for c, _ in want))
            tg = bytearray(b"".join(t for _, t in want))
            for j, m in enumerate(bad):
                if j % 2 and ml:
                    ct[m * ml + ml - 1] ^= 0x40
                else:
                    tg[16 * m + 5 + j] ^= 0x40
            src = Mem(ct, device, off=toff)
            dst = src if place == "device-in-place" else Mem(b"\x77" * (nmsg * ml), device, off=toff)
            dv = Mem(size=nmsg, device=device, off=toff)
            rc = batch(is_siv, True, bits, k, nmsg, ml, dn, nl, da, al, src, dst, Mem(tg, device, off=toff), dv)
            assert rc == 0x1A and dv.get() == bytes(0 if m in bad else 1 for m in range(nmsg)) and dv.intact(nmsg), info
            got = dst.get(nmsg * ml)
            for m in range(nmsg):
                if m not in bad:
                    exp = texts[m]
                elif is_siv:
                    exp = R.siv_decrypt_rc(bits, k, bytes(tg[16 * m:16 * m + 16]), aads[m], bytes(ct[m * ml:(m + 1) * ml]))[1]
                else:
                    exp = bytes(ct[m * ml:(m + 1) * ml]) if dst is src else b"\x77" * ml
                assert got[m * ml:(m + 1) * ml] == exp, info + (m,)
            assert dst.intact(nmsg * ml), info
    assert len(seen) == 3 * (len(BATCH_MSG) + len(BATCH_AAD)) + 3 * (len(BATCH_NONCE) + len(BATCH_MSG))


# ---- chosen counters where the CTR pass takes the striped kernel -----------------------------------------------------

def striped_from(counter):
    """the smallest text length at which a CTR call from this counter block takes ctr.striped"""
    lo, hi = 0, 1 << 28
    assert uaes.plan("ctr", hi, counter=counter)[0] == "ctr.striped"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if uaes.plan("ctr", mid, counter=counter)[0] == "ctr.striped":
            hi = mid
        else:
            lo = mid
    return hi


AT = 100003                                                                  # blocks into the text (inside the stripes)
WRAP56 = bytes(9) + ((1 << 56) - AT).to_bytes(7, "big")                      # the 56-bit wrap at block AT
CARRY40 = bytes(9) + ((0x1235 << 40) - AT).to_bytes(7, "big")                # counter bits 40..47 move at block AT


@pytest.mark.parametrize("bits", [128, 256])
def test_chosen_counters_at_the_striped_size(bits):
    """eax.long / s2v.long hand N or V' to uaesk_ctr_xcrypt: a text long enough for ctr.striped whose counter wraps at
    56 bits, or carries into bits 40..47 (the plan then reports two launches), inside the text"""
    rng = random.Random(bits + 6)
    key, keys = rng.randbytes(bits // 8), rng.randbytes(bits // 4)
    for target in (WRAP56, CARRY40):
        n = striped_from(target) + 16 * 20 + 3
        name, launches = uaes.plan("ctr", n, counter=target)[:2]
        assert name == "ctr.striped" and uaes.eax_siv_plan(False, n)[0] == "eax.long"
        if target is CARRY40:
            assert launches == 2, "the carry into counter bits 40..47 is not inside the text"
        nonce = R.eax_nonce_for(bits, key, target)
        assert R.omac(key, 0, nonce, bits) == target
        check_eax(bits, key, nonce, b"hdr", rng.randbytes(n))
    for target, set_bits in ((CTRS[-2], False), (CTRS[-1], True)):
        v = bytearray(target)
        if set_bits:
            v[8] |= 0x80                   # cleared by the mask: the counter is the same
            v[12] |= 0x80                  # bit 31 cleared: byte 12's low bits still carry into byte 11
        masked = bytearray(v)
        masked[8] &= 0x7F
        masked[12] &= 0x7F
        n = striped_from(bytes(masked)) + 16 * 20
        assert uaes.plan("ctr", n, counter=bytes(masked))[0] == "ctr.striped" and uaes.eax_siv_plan(True, n)[0] == "s2v.long"
        pt = R.siv_text_for(bits, keys, b"aad", rng.randbytes(n - 16), bytes(v))
        assert R.siv_encrypt(bits, keys, b"aad", pt)[0] == bytes(v)
        check_siv(bits, keys, b"aad", pt)
