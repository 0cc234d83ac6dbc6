"""EAX' (ANSI C12.22 / IEEE 1703) on the GPU (k_eaxp_small, k_eaxp_macs, k_eaxp_batch: uaes_eax_siv.hip) against the
recorded answers of the reference built with EAXP 1 and the composition of tests/eaxp_ref.py: the length matrix on both
sides of the small / long boundary read from the plan, host, device, odd-offset and in-place pointers, chosen counter
blocks (the two cleared bits, the carry into byte 14, the 56-bit counter), forgeries of every part with the wipe switch
off and on, and batches -- record counts from the launch shape, a length per nonce and per text, forged records among
authentic ones, every array between guard bytes.  After every test the count of live key schedules is what it was."""
import ctypes as C
import random

import pytest

import micro_aes_amd as uaes
from tests import eaxp_ref as X
from tests import key_wipe_cases as kw
from tests.aead_batch_cases import flip, join, le32, ones
from tests.guarded_mem import FILL, Mem, ptr

pytestmark = pytest.mark.gpu

AUTH, E_ARG = 0x1A, -2
BITS = (128, 192, 256)
KEYS = {bits: random.Random(bits).randbytes(bits // 8) for bits in BITS}


@pytest.fixture(autouse=True)
def no_key_schedule_left_behind():
    before = kw.live()
    yield
    assert kw.live() == before


def small_max():
    return uaes.eaxp_plan(0)[3]


def one(decrypt, bits, key, nonce, nl, src, n, dst):
    """uaes_eaxp_encrypt / uaes_eaxp_decrypt; nonce: bytes, None or Mem, src / dst: Mem"""
    L = uaes.engine()
    return (L.uaes_eaxp_decrypt if decrypt else L.uaes_eaxp_encrypt)(bits, key, ptr(nonce), nl, ptr(src), n, ptr(dst))


def batch(decrypt, bits, key, n, nb, nlens, nonces, mb, lens, src, dst, macs, verdicts=None):
    """the two batch entry points; every array bytes, None or Mem"""
    L = uaes.engine()
    a = (bits, key, n, nb, ptr(nlens), ptr(nonces), mb, ptr(lens), ptr(src))
    if decrypt:
        return L.uaes_eaxp_decrypt_batch(*a, ptr(macs), ptr(dst), ptr(verdicts))
    return L.uaes_eaxp_encrypt_batch(*a, ptr(dst), ptr(macs))


# ---- single calls -------------------------------------------------------------------------------------------------------
def test_every_recorded_answer():
    for what, bits, key, nonce, pt, out in X.entries():
        assert uaes.eaxp_encrypt(key, nonce, pt) == out, (what, bits, len(nonce), len(pt))
        assert uaes.eaxp_decrypt(key, nonce, out, prefill=0x33) == (0, pt), (what, bits, len(nonce), len(pt))


def text_lens():
    s = small_max()
    assert uaes.eaxp_plan(s)[0] == "eaxp.small" and uaes.eaxp_plan(s + 1)[0] == "eaxp.long"
    return (0, 1, 15, 16, 17, 33, 255, 256, 257, s - 1, s, s + 1, s + 17)


@pytest.mark.parametrize("bits", BITS)
def test_length_matrix(bits):
    rng = random.Random(1703 + bits)
    key = KEYS[bits]
    for nl in (0, 1, 15, 16, 17, 65, 1000):
        for n in text_lens():
            nonce, pt = rng.randbytes(nl), rng.randbytes(n)
            want = X.encrypt(bits, key, nonce, pt)
            assert uaes.eaxp_encrypt(key, nonce, pt) == want, (bits, nl, n)
            assert uaes.eaxp_decrypt(key, nonce, want, prefill=0x44) == (0, pt), (bits, nl, n)


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("off", [0, 1, 3])
def test_pointers(device, off):
    """text and nonce `off` bytes behind an aligned address, in host or device memory, out of place and in place; only the
    output is written, and that inside its bounds"""
    rng = random.Random(17 + off)
    bits = 192
    key = KEYS[bits]
    for n in (0, 33, 256, small_max() + 17):
        nonce, pt = rng.randbytes(50), rng.randbytes(n)
        want, info = X.encrypt(bits, key, nonce, pt), (device, off, n)
        mn, src, dst = Mem(nonce, device, off), Mem(pt, device, off, size=n + 1), Mem(size=n + 4, device=device, off=off)
        assert one(False, bits, key, mn, 50, src, n, dst) == 0, info
        assert dst.get() == want and dst.intact(n + 4) and src.get(n) == pt and mn.get() == nonce, info
        back = Mem(size=n + 1, device=device, off=off)
        assert one(True, bits, key, mn, 50, dst, n, back) == 0, info
        assert back.get(n) == pt and back.intact(n) and dst.get() == want, info
        io = Mem(pt, device, off, size=n + 4)
        assert one(False, bits, key, mn, 50, io, n, io) == 0 and io.get() == want and io.intact(n + 4), info
        assert one(True, bits, key, mn, 50, io, n, io) == 0 and io.get(n) == pt and io.get()[n:] == want[n:] and io.intact(n + 4), info
    # no nonce at all: a NULL pointer with length 0
    pt = rng.randbytes(40)
    dst = Mem(size=44, device=device, off=off)
    assert one(False, bits, key, None, 0, Mem(pt, device, off), 40, dst) == 0 and dst.get() == X.encrypt(bits, key, b"", pt)


# ---- chosen counter blocks ------------------------------------------------------------------------------------------------
COUNTERS = {
    "bytes 12 and 14 all ones": bytes(range(12)) + b"\xff\x5a\xff\x00",
    "carry into byte 14": bytes(range(0x20, 0x2e)) + b"\xff\xf0",
    "56-bit counter about to wrap": bytes(range(0x40, 0x49)) + b"\xff\xff\xff\xff\xff\xff\xf0",
}


@pytest.mark.parametrize("long", [False, True], ids=["small", "long"])
@pytest.mark.parametrize("which", sorted(COUNTERS))
def test_counter_blocks(which, long):
    target = COUNTERS[which]
    n = small_max() + 17 if long else 33 * 16
    for bits in BITS:
        key = KEYS[bits]
        nonce = X.nonce_for(bits, key, target)
        d, _ = X.subkeys(bits, key)
        assert X.cmac_prime(bits, key, d, nonce) == target                       # N is the chosen block
        pt = random.Random(n + bits).randbytes(n)
        want = X.encrypt(bits, key, nonce, pt)
        # the keystream starts at N' = N with the two bits cleared, not at N
        assert want[:16] == X.R.xor(pt[:16], X.R.aes_encrypt_block(bits, key, X.clear(target))) and X.clear(target) != target
        assert uaes.eaxp_encrypt(key, nonce, pt) == want, (which, bits, n)
        assert uaes.eaxp_decrypt(key, nonce, want) == (0, pt), (which, bits, n)
    # the same N in a batch: four records of 33 blocks, one of them with that nonce
    if not long:
        key = KEYS[128]
        nonces = [bytes(16), X.nonce_for(128, key, target), bytes(range(16)), b"\xff" * 16]
        texts = [random.Random(m).randbytes(n) for m in range(4)]
        cts, macs = uaes.eaxp_encrypt_batch(key, nonces, texts)
        assert [c + t for c, t in zip(cts, macs)] == [X.encrypt(128, key, a, b) for a, b in zip(nonces, texts)], which


# ---- forgeries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("long", [False, True], ids=["small", "long"])
def test_forgeries_leave_the_output_untouched(long, device):
    rng = random.Random(77 + long)
    n, bits = (small_max() + 17 if long else 70), 256
    key, nonce, pt = KEYS[bits], rng.randbytes(33), rng.randbytes(n)
    out = X.encrypt(bits, key, nonce, pt)
    # (flip(b, i) flips bit i % 8 of byte i % len(b))
    forged = [("text", nonce, flip(out[:n], rng.randrange(n)) + out[n:]),
              ("last text byte", nonce, out[:n - 1] + bytes([out[n - 1] ^ 0x80]) + out[n:]),
              ("mac", nonce, out[:n] + flip(out[n:], rng.randrange(4))), ("nonce", flip(nonce, rng.randrange(33)), out)]
    for what, fn, fo in forged:
        assert (fn, fo) != (nonce, out) and X.decrypt(bits, key, fn, fo, 0x5C)[0] == AUTH, what
    for wipe in (0, 1):
        uaes.engine().uaes_set_wipe_on_auth_failure(wipe)
        try:
            for what, fn, fo in forged:
                src, dst = Mem(fo, device), Mem(size=n, device=device)
                assert one(True, bits, key, fn, 33, src, n, dst) == AUTH, (what, wipe)
                assert dst.get() == bytes([FILL]) * n and dst.intact(n) and src.get() == fo, (what, wipe)
                io = Mem(fo, device)                                                  # in place: the ciphertext stays
                assert one(True, bits, key, fn, 33, io, n, io) == AUTH and io.get() == fo and io.intact(n + 4), (what, wipe)
        finally:
            uaes.engine().uaes_set_wipe_on_auth_failure(0)


def test_an_empty_text():
    """C' is 0^128 for an empty ciphertext: the mac is N's last four bytes"""
    for bits in BITS:
        key, nonce = KEYS[bits], bytes(range(40))
        d, _ = X.subkeys(bits, key)
        mac = X.cmac_prime(bits, key, d, nonce)[12:]
        assert uaes.eaxp_encrypt(key, nonce, b"") == mac == X.encrypt(bits, key, nonce, b"")
        assert uaes.eaxp_decrypt(key, nonce, mac) == (0, b"") and uaes.eaxp_decrypt(key, nonce, flip(mac, 9))[0] == AUTH
        assert uaes.eaxp_encrypt_batch(key, [nonce] * 3, [b""] * 3) == ([b""] * 3, [mac] * 3)
        assert uaes.eaxp_decrypt_batch(key, [nonce] * 3, [b""] * 3, [mac, flip(mac, 1), mac]) == (AUTH, [b""] * 3, [1, 0, 1])


# ---- batches --------------------------------------------------------------------------------------------------------------
def cut(items, lens, slot):
    return list(items) if lens is None else [x[:min(k, slot)] for x, k in zip(items, lens)]


def expected(bits, key, nonces, nlens, texts, lens, only=None):
    """the composition's (ciphertexts, macs), one record at a time"""
    ns, ts = cut(nonces, nlens, len(nonces[0])), cut(texts, lens, len(texts[0]))
    outs = [X.encrypt(bits, key, ns[m], ts[m]) for m in (range(len(ts)) if only is None else only)]
    return [o[:-4] for o in outs], [o[-4:] for o in outs]


def threads_of(nmsg):
    """threads per workgroup of a row batch of nmsg records (every row batch has the launch shape of ccm.batch)"""
    return uaes.chain_plan("ccm_batch", 16, nmsg)[3]


def record_counts():
    rows = threads_of(1) // 16
    assert rows == threads_of(rows + 1) // 16 and uaes.eaxp_plan(16, rows + 1)[2] == 2           # a second workgroup
    return [1, 2, rows - 1, rows, rows + 1]


@pytest.mark.parametrize("nmsg", record_counts())
def test_record_counts(nmsg):
    rng = random.Random(nmsg)
    key = KEYS[128]
    nonces, texts = [rng.randbytes(32) for _ in range(nmsg)], [rng.randbytes(16) for _ in range(nmsg)]
    wct, wmac = expected(128, key, nonces, None, texts, None)
    assert uaes.eaxp_encrypt_batch(key, nonces, texts) == (wct, wmac)
    assert uaes.eaxp_decrypt_batch(key, nonces, wct, wmac, prefill=0x77) == (0, texts, [1] * nmsg)
    for m in range(nmsg):                                                        # bit for bit the single call's answer
        assert uaes.eaxp_encrypt(key, nonces[m], texts[m]) == wct[m] + wmac[m], m


def test_a_row_takes_a_second_record():
    name, launches, grid, _ = uaes.eaxp_plan(16, 1 << 20)
    nmsg = grid * threads_of(1 << 20) // 16 + 3
    assert name == "eaxp.batch" and launches == 1 and uaes.eaxp_plan(16, nmsg)[2] == grid      # it does run a second time
    rng = random.Random(nmsg)
    key = KEYS[128]
    nonces, texts = [rng.randbytes(16) for _ in range(nmsg)], [rng.randbytes(16) for _ in range(nmsg)]
    look = sorted(set(range(70)) | set(range(nmsg - 70, nmsg)) | set(rng.sample(range(nmsg), 200)))
    cts, macs = uaes.eaxp_encrypt_batch(key, nonces, texts)
    wct, wmac = expected(128, key, nonces, None, texts, None, look)
    assert [(cts[m], macs[m]) for m in look] == list(zip(wct, wmac))
    macs[nmsg - 2] = flip(macs[nmsg - 2], 3)
    rc, pts, verdicts = uaes.eaxp_decrypt_batch(key, nonces, cts, macs, prefill=0x77)
    assert rc == AUTH and verdicts == [0 if m == nmsg - 2 else 1 for m in range(nmsg)]
    assert pts == [b"\x77" * 16 if m == nmsg - 2 else texts[m] for m in range(nmsg)]


MB, NB = 48, 40                                  # the slots of the length cases
LENS = [0, 1, 15, 16, 17, 33, 48, 48, 0, 31, 47, 32, 48, 5, 0, 48, 16, 33, 1, 48, 20]
NLENS = [0, 40, 1, 15, 16, 17, 33, 0, 40, 40, 39, 0, 8, 40, 0, 32, 17, 16, 40, 1, 25]
LENGTHS = {"none": (None, None), "all zero": ([0] * 21, [0] * 21), "mixed": (NLENS, LENS), "nonces only": (NLENS, None),
           "texts only": (None, LENS)}


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("which", sorted(LENGTHS))
def test_lengths_per_record(which, device):
    """over raw pointers with every array between guard bytes: record m is lens[m] bytes under nlens[m] bytes of nonce,
    the rest of its slot is not written, and every record is the single call's answer"""
    nlens, lens = LENGTHS[which]
    rng = random.Random(48)
    n, bits = 21, 192
    key = KEYS[bits]
    nonces, texts = [rng.randbytes(NB) for _ in range(n)], [rng.randbytes(MB) for _ in range(n)]
    wct, wmac = expected(bits, key, nonces, nlens, texts, lens)
    ln = [MB] * n if lens is None else lens
    for off in (0, 1):
        mn, src = Mem(join(nonces), device, off), Mem(join(texts), device, off)
        mnl = None if nlens is None else Mem(le32(nlens), device)
        mln = None if lens is None else Mem(le32(lens), device)
        dst, macs = Mem(size=n * MB, device=device, off=off), Mem(size=n * 4, device=device, off=off)
        info = (which, device, off)
        assert batch(False, bits, key, n, NB, mnl, mn, MB, mln, src, dst, macs) == 0, info
        out, tg = dst.get(), macs.get()
        for m in range(n):
            assert out[m * MB:m * MB + ln[m]] == wct[m] and tg[4 * m:4 * m + 4] == wmac[m], (info, m)
            assert set(out[m * MB + ln[m]:(m + 1) * MB]) <= {FILL}, (info, m)                   # beyond lens[m]: not written
            single = Mem(size=ln[m] + 4, device=device)
            assert one(False, bits, key, cut(nonces, nlens, NB)[m], len(cut(nonces, nlens, NB)[m]),
                       Mem(texts[m], device), ln[m], single) == 0 and single.get() == wct[m] + wmac[m], (info, m)
        assert dst.intact(n * MB) and macs.intact(n * 4) and src.get() == join(texts) and mn.get() == join(nonces), info
        back, ver = Mem(size=n * MB, device=device, off=off), Mem(size=n, device=device, off=off)
        assert batch(True, bits, key, n, NB, mnl, mn, MB, mln, dst, back, macs, ver) == 0, info
        got = back.get()
        for m in range(n):
            assert got[m * MB:m * MB + ln[m]] == texts[m][:ln[m]] and set(got[m * MB + ln[m]:(m + 1) * MB]) <= {FILL}, (info, m)
        assert ver.get() == ones(n) and back.intact(n * MB) and ver.intact(n), info
        # crtxt == pntxt, and no verdicts
        io = Mem(join(texts), device, off)
        macs2 = Mem(size=n * 4, device=device, off=off)
        assert batch(False, bits, key, n, NB, mnl, mn, MB, mln, io, io, macs2) == 0 and macs2.get() == tg, info
        assert all(io.get()[m * MB:m * MB + ln[m]] == wct[m] and io.get()[m * MB + ln[m]:(m + 1) * MB] == texts[m][ln[m]:]
                   for m in range(n)), info
        assert batch(True, bits, key, n, NB, mnl, mn, MB, mln, io, io, macs2, None) == 0 and io.get() == join(texts), info
        assert io.intact(n * MB) and macs2.intact(n * 4), info
        for given in (mnl, mln):
            assert given is None or given.intact(4 * n), info


def test_a_length_above_its_slot():
    """in host memory it is refused before anything runs; in device memory the kernel alone reads it and takes the slot"""
    rng = random.Random(5)
    n, key = 4, KEYS[128]
    nonces, texts = [rng.randbytes(NB) for _ in range(n)], [rng.randbytes(MB) for _ in range(n)]
    for nlens, lens in (([NB + 1, 0, 0, 0], [MB] * n), ([NB] * n, [0, 0, 1000, 0])):
        dst, macs = Mem(size=n * MB), Mem(size=n * 4)
        assert batch(False, 128, key, n, NB, le32(nlens), join(nonces), MB, le32(lens), join(texts), dst, macs) == E_ARG
        assert dst.get() == bytes([FILL]) * (n * MB) and macs.get() == bytes([FILL]) * (n * 4)
        dst, macs = Mem(size=n * MB, device=True), Mem(size=n * 4, device=True)
        assert batch(False, 128, key, n, NB, Mem(le32(nlens), True), join(nonces), MB, Mem(le32(lens), True), join(texts), dst, macs) == 0
        wct, wmac = expected(128, key, nonces, nlens, texts, lens)
        assert macs.get() == join(wmac) and dst.intact(n * MB) and macs.intact(n * 4)
        assert all(dst.get()[m * MB:m * MB + len(wct[m])] == wct[m] for m in range(n))
    # a device array of lengths at an odd address is refused
    odd = Mem(le32([MB] * n), True, 1)
    assert batch(False, 128, key, n, NB, None, join(nonces), MB, odd, join(texts), Mem(size=n * MB), Mem(size=n * 4)) == E_ARG


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in place"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
def test_forged_records_among_authentic_ones(device, in_place):
    rng = random.Random(9)
    n, bits = 21, 128
    key = KEYS[bits]
    nonces, texts = [rng.randbytes(NB) for _ in range(n)], [rng.randbytes(MB) for _ in range(n)]
    cts, macs = expected(bits, key, nonces, NLENS, texts, LENS)
    bad = {5: "text", 9: "mac", 10: "nonce", 20: "mac"}                          # (record 5 has 33 bytes, record 10 a 39-byte nonce)
    padded = [c + texts[m][len(c):] for m, c in enumerate(cts)]
    fn, fm = list(nonces), list(macs)
    padded[5] = flip(padded[5], 32)                                               # (flip(b, i): bit i % 8 of byte i % len(b))
    fm[9], fm[20], fn[10] = flip(macs[9], 3), flip(macs[20], 0), flip(nonces[10], 38)
    for m, what in bad.items():
        assert X.decrypt(bits, key, fn[m][:NLENS[m]], padded[m][:LENS[m]] + fm[m])[0] == AUTH, what
    want_ver = bytes(0 if m in bad else 1 for m in range(n))
    for wipe in (0, 1):
        uaes.engine().uaes_set_wipe_on_auth_failure(wipe)
        try:
            for verdicts in (True, False):
                src = Mem(join(padded), device)
                dst = src if in_place else Mem(size=n * MB, device=device)
                ver = Mem(size=n, device=device) if verdicts else None
                info = (device, in_place, wipe, verdicts)
                assert batch(True, bits, key, n, NB, Mem(le32(NLENS), device), Mem(join(fn), device), MB, Mem(le32(LENS), device), src,
                             dst, Mem(join(fm), device), ver) == AUTH, info
                got = dst.get()
                for m in range(n):
                    before = padded[m] if in_place else bytes([FILL]) * MB
                    slot = got[m * MB:(m + 1) * MB]
                    assert slot == (before if m in bad else texts[m][:LENS[m]] + before[LENS[m]:]), (info, m)
                assert dst.intact(n * MB) and (ver is None or (ver.get() == want_ver and ver.intact(n))), info
        finally:
            uaes.engine().uaes_set_wipe_on_auth_failure(0)


def test_long_records_in_place():
    """row_walk requests a chunk of blocks ahead: six records of more blocks than that, in place in device memory, at
    offsets 0 and 2, with lengths on either side of a chunk"""
    rng = random.Random(600)
    n, mb, bits = 6, 600, 256
    key = KEYS[bits]
    lens = [600, 599, 272, 256, 257, 0]
    nonces, texts = [rng.randbytes(20) for _ in range(n)], [rng.randbytes(mb) for _ in range(n)]
    wct, wmac = expected(bits, key, nonces, None, texts, lens)
    for off in (0, 2):
        io, macs, ver = Mem(join(texts), True, off), Mem(size=n * 4, device=True, off=off), Mem(size=n, device=True)
        assert batch(False, bits, key, n, 20, None, join(nonces), mb, le32(lens), io, io, macs) == 0
        assert macs.get() == join(wmac) and io.intact(n * mb), off
        assert all(io.get()[m * mb:(m + 1) * mb] == wct[m] + texts[m][lens[m]:] for m in range(n)), off
        assert batch(True, bits, key, n, 20, None, join(nonces), mb, le32(lens), io, io, macs, ver) == 0
        assert io.get() == join(texts) and ver.get() == ones(n) and io.intact(n * mb), off


def test_error_exits_leave_no_key_schedule():
    B = (C.c_uint8 * 64)()
    L = uaes.engine()
    before = kw.live()
    assert L.uaes_eaxp_encrypt(128, KEYS[128], None, 5, B, 16, B) == E_ARG
    assert L.uaes_eaxp_decrypt(128, KEYS[128], B, 5, B, 16, None) == E_ARG
    assert L.uaes_eaxp_encrypt_batch(128, KEYS[128], 2, 16, None, B, 16, le32([16, 17]), B, B, B) == E_ARG
    assert L.uaes_eaxp_decrypt_batch(128, KEYS[128], 2, 16, None, B, 16, None, B, None, B, B) == E_ARG
    assert L.uaes_eaxp_decrypt(128, KEYS[128], B, 5, B, 16, B) == AUTH
    assert L.uaes_eaxp_decrypt_batch(128, KEYS[128], 2, 16, None, B, 16, None, B, B, B, None) == AUTH
    assert kw.live() == before
