"""FF1 (SP 800-38G) on the GPU (uaes_ff1.hip): the reference's vector file, decimal texts against the compiled reference
at every length up to the batch limit and at the batch / wave boundary and the maximum (both found by walking the
planner), the tweak lengths around the block size, other radices against the specification model (with the lengths at
which the reference's floating-point b differs), batches whose counts come from the planner (shared and per-record
tweaks, host and device arrays, an odd base address), batches with bytes that are no numerals, the limits, and a seeded
fuzz of round trips.  Every failing case prints the tuple that reproduces it."""
import ctypes as C
import functools
import random

import pytest

import micro_aes_amd as uaes
from tests import ff1_ref as R
from tests.guarded_mem import Mem

pytestmark = pytest.mark.gpu

E_DATALENGTH, E_DECRYPTION, E_ENCRYPTION = 1, 0x1D, 0x1E
TWEAK_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 100]
RADICES = [2, 26, 36, 64, 95, 255, 256]


def kbuf(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def decimal(rng, n):
    return bytes(rng.choice(R.DECIMAL) for _ in range(n))


@functools.lru_cache(maxsize=None)
def plan_limits():
    """(the longest text that runs as ff1.batch, the longest text at all), by walking the planner"""
    names = [(n, uaes.ff1_plan(n)) for n in range(6, 8200)]
    batch = max(n for n, p in names if p and p[0] == "ff1.batch")
    top = max(n for n, p in names if p)
    assert uaes.ff1_plan(batch + 1)[0] == "ff1.wave" and uaes.ff1_plan(top)[0] == "ff1.wave"
    assert all(p is not None for n, p in names if n <= top)
    assert uaes.ff1_plan(batch, 2) is not None and uaes.ff1_plan(batch + 1, 2) is None
    return batch, top


def check_decimal(key, tweak, pt):
    want = R.ref_encrypt(key, tweak, pt)
    assert want[0] == 0
    case = (key.hex(), tweak.hex(), len(pt))
    assert uaes.AES_FPE_encrypt(key, tweak, pt) == want, case
    assert uaes.AES_FPE_decrypt(key, tweak, want[1]) == (0, pt), case


def test_vector_file(golden_dir):
    vs = R.vectors(golden_dir)
    assert len(vs) == 20 and sorted(set(len(v["alphabet"]) for v in vs)) == [2, 10, 26, 36, 62, 72]
    assert max(len(v["pt"]) for v in vs) == 1804
    for v in vs:
        assert uaes.AES_FPE_encrypt(v["key"], v["tweak"], v["pt"], v["alphabet"]) == (0, v["ct"]), v
        assert uaes.AES_FPE_decrypt(v["key"], v["tweak"], v["ct"], v["alphabet"]) == (0, v["pt"]), v


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_decimal_every_length_to_the_batch_limit(bits):
    batch, _ = plan_limits()
    rng = random.Random(bits)
    for n in range(6, batch + 3):
        check_decimal(rng.randbytes(bits // 8), rng.randbytes(rng.choice([0, 3, 16, 21])), decimal(rng, n))


def test_boundary_and_maximum():
    batch, top = plan_limits()
    rng = random.Random(7)
    for n in (batch - 1, batch, batch + 1, batch + 2, 255, 256, 257, 1804, top - 1, top):
        for bits in (128, 192, 256):
            check_decimal(rng.randbytes(bits // 8), rng.randbytes(7), decimal(rng, n))
    key, pt = rng.randbytes(16), decimal(rng, top + 1)
    assert uaes.AES_FPE_encrypt(key, b"", pt, prefill=0x5C) == (E_DATALENGTH, bytes([0x5C]) * len(pt))
    assert uaes.AES_FPE_decrypt(key, b"", pt[:5], prefill=0x5C) == (E_DATALENGTH, bytes([0x5C]) * 5)


def test_tweak_lengths():
    batch, _ = plan_limits()
    rng = random.Random(11)
    for t in TWEAK_LENS:
        for n in (6, 16, 19, 57, batch, batch + 72):
            check_decimal(rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(t), decimal(rng, n))


@pytest.mark.parametrize("radix", RADICES)
def test_radices_against_the_model(orc, radix):
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


def test_wave_form_at_the_ends_of_the_radix_range(orc):
    """k_ff1<NR,64>: 64 lanes and digit runs of up to 32 a lane, which the vector file reaches up to radix 72 only"""
    batch, top = plan_limits()
    cases = R.wave_cases(orc, batch, top)
    assert len(cases) == 12
    for radix, key, tweak, digits, want in cases:
        case = (radix, len(digits), key.hex(), tweak.hex())
        assert uaes.ff1_plan(len(digits), radix=radix)[0] == "ff1.wave", case
        assert uaes.AES_FPE_encrypt(key, tweak, digits, None, radix) == (0, want), case
        assert uaes.AES_FPE_decrypt(key, tweak, want, None, radix) == (0, digits), case


# ---- batches ----------------------------------------------------------------------------------------------------------
BATCH_KEY = bytes(range(0x40, 0x50))
SHARED_TWEAK = bytes(range(11))
PER_TWEAK = 9


@functools.lru_cache(maxsize=None)
def grid_counts():
    """(a count that fills the planner's grid exactly, one more: the kernel strides)"""
    _, _, grid, threads = uaes.ff1_plan(16, 1 << 24)          # far more records than the grid holds: the cap
    fill = grid * (threads // 16)
    assert uaes.ff1_plan(16, fill)[2:] == (grid, threads) and uaes.ff1_plan(16, fill + 1)[2:] == (grid, threads)
    assert uaes.ff1_plan(16, fill - threads // 16)[2] == grid - 1
    return fill, fill + 1


@functools.lru_cache(maxsize=None)
def batch_answers(n):
    """records of n decimal numerals, their tweaks, and the reference's single-call answers with the shared and with
    the per-record tweaks; computed once for the largest count, shorter batches take a prefix"""
    count = grid_counts()[1]
    rng = random.Random(1000 + n)
    recs = [decimal(rng, n) for _ in range(count)]
    tweaks = [rng.randbytes(PER_TWEAK) for _ in range(count)]
    shared = [R.ref_encrypt(BATCH_KEY, SHARED_TWEAK, r)[1] for r in recs]
    per = [R.ref_encrypt(BATCH_KEY, t, r)[1] for r, t in zip(recs, tweaks)]
    return recs, tweaks, shared, per


def run_batch(decrypt, key, radix, alphabet, tweak_mem, tweak_len, stride, count, n, src, dst, verdicts):
    L = uaes.engine()
    fn = L.uaes_ff1_decrypt_batch if decrypt else L.uaes_ff1_encrypt_batch
    return fn(len(key) * 8, kbuf(key), radix, kbuf(alphabet) if alphabet else None, tweak_mem.ptr if tweak_mem else None,
              tweak_len, stride, count, n, src.ptr, dst.ptr, verdicts.ptr if verdicts else None)


def batch_lengths():
    return [16, 19, 6, plan_limits()[0]]


@pytest.mark.parametrize("which", ["1", "3", "4", "5", "63", "64", "65", "fill", "stride"])
@pytest.mark.parametrize("nth", [0, 1, 2, 3])
def test_batches(nth, which):
    n = batch_lengths()[nth]
    count = {"fill": grid_counts()[0], "stride": grid_counts()[1]}.get(which) or int(which)
    if which == "fill":
        _, _, grid, threads = uaes.ff1_plan(n, count)
        assert count == grid * (threads // 16) and uaes.ff1_plan(n, count + 1)[2] == grid
    recs, tweaks, shared, per = batch_answers(n)
    pt = b"".join(recs[:count])
    for per_record in (False, True):
        want = b"".join((per if per_record else shared)[:count])
        tw = b"".join(tweaks[:count]) if per_record else SHARED_TWEAK
        tl, stride = (PER_TWEAK, PER_TWEAK) if per_record else (len(SHARED_TWEAK), 0)
        for device, off in ((False, 0), (True, 0), (True, 1), (False, 3)):
            src, dst, twm = Mem(pt, device, off), Mem(b"", device, off, size=len(pt)), Mem(tw, device, off)
            ver = Mem(b"", device, off, size=count, fill=7)
            case = (n, count, per_record, device, off)
            assert run_batch(0, BATCH_KEY, 10, R.DECIMAL, twm, tl, stride, count, n, src, dst, ver) == 0, case
            got = dst.get()
            if got != want:
                bad = [m for m in range(count) if got[m * n:(m + 1) * n] != want[m * n:(m + 1) * n]]
                raise AssertionError("%r: %d records differ, the first at %d" % (case, len(bad), bad[0]))
            assert ver.get() == bytes([1]) * count and dst.intact() and ver.intact() and src.get() == pt, case
        # and back, in place, in device memory
        buf_, twm = Mem(want, True, 1), Mem(tw, True, 0)
        assert run_batch(1, BATCH_KEY, 10, R.DECIMAL, twm, tl, stride, count, n, buf_, buf_, None) == 0
        assert buf_.get() == pt and buf_.intact(), (n, count, per_record, "decrypt in place")


@pytest.mark.parametrize("decrypt", [0, 1])
def test_batch_with_bytes_that_are_no_numerals(decrypt):
    n, count = 19, 150
    name, _, grid, threads = uaes.ff1_plan(n, count)
    per = threads // 16                                        # records per workgroup
    assert grid >= 3 and grid * per >= count
    bad = sorted({0, per - 1, per, 2 * per - 1, 77, count - 1})
    recs, tweaks, shared, perans = batch_answers(n)
    good_in = (perans if decrypt else recs)[:count]
    good_out = (recs if decrypt else perans)[:count]
    rng = random.Random(5)
    inp = list(good_in)
    for k, m in enumerate(bad):
        r = bytearray(inp[m])
        r[(0, n // 2, n - 1)[k % 3]] = rng.choice(b"/:aA\x00\xff")
        inp[m] = bytes(r)
    for device in (False, True):
        for with_verdicts in (True, False):
            src, dst = Mem(b"".join(inp), device, 1), Mem(b"", device, 1, size=n * count, fill=0x5C)
            twm = Mem(b"".join(tweaks[:count]), device)
            ver = Mem(b"", device, 0, size=count, fill=7) if with_verdicts else None
            rc = run_batch(decrypt, BATCH_KEY, 10, R.DECIMAL, twm, PER_TWEAK, PER_TWEAK, count, n, src, dst, ver)
            assert rc == (E_DECRYPTION if decrypt else E_ENCRYPTION), (device, with_verdicts)
            got = dst.get()
            for m in range(count):
                want = bytes([0x5C]) * n if m in bad else good_out[m]
                assert got[m * n:(m + 1) * n] == want, (decrypt, device, m)
            assert dst.intact()
            if ver:
                assert ver.get() == bytes(0 if m in bad else 1 for m in range(count)) and ver.intact()


def test_batch_limits():
    batch, _ = plan_limits()
    rng = random.Random(3)
    n = batch + 1
    src, dst, ver = Mem(decimal(rng, 2 * n)), Mem(b"", size=2 * n), Mem(b"", size=2, fill=7)
    for decrypt in (0, 1):
        assert run_batch(decrypt, BATCH_KEY, 10, R.DECIMAL, None, 0, 0, 2, n, src, dst, ver) == E_DATALENGTH
        assert run_batch(decrypt, BATCH_KEY, 10, R.DECIMAL, None, 0, 0, 2, 5, src, dst, ver) == E_DATALENGTH
        assert run_batch(decrypt, BATCH_KEY, 10, R.DECIMAL, None, 0, 0, 0, 16, src, dst, ver) == 0
    assert dst.get() == bytes([0x5C]) * (2 * n) and ver.get() == bytes([7, 7])
    assert run_batch(0, BATCH_KEY, 257, None, None, 0, 0, 2, 16, src, dst, ver) == -2
    assert run_batch(0, BATCH_KEY, 10, b"0123456780", None, 0, 0, 2, 16, src, dst, ver) == -2
    assert uaes.AES_FPE_encrypt(BATCH_KEY, b"", b"12345/7", prefill=9) == (E_ENCRYPTION, bytes([9]) * 7)
    assert uaes.AES_FPE_decrypt(BATCH_KEY, b"", b"1234567" * 40 + b"a", prefill=9) == (E_DECRYPTION, bytes([9]) * 281)


def test_fuzz_round_trips(orc):
    _, top = plan_limits()
    rng = random.Random(20261018)
    for k in range(60):
        radix = rng.choice([2, 3, 10, 10, 16, 36, 62, 100, 255, 256, rng.randrange(2, 257)])
        lo = R.minlen(radix)
        n = rng.choice([lo, rng.randrange(lo, 80), rng.randrange(lo, 80), rng.randrange(lo, 400), rng.randrange(lo, top + 1)])
        key, tweak = rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(rng.choice([0, 1, 7, 16, 40]))
        digits = bytes(rng.randrange(radix) for _ in range(n))
        case = (k, radix, n, key.hex(), tweak.hex())
        rc, ct = uaes.AES_FPE_encrypt(key, tweak, digits, None, radix)
        assert rc == 0 and len(ct) == n and all(c < radix for c in ct) and ct != digits, case
        assert uaes.AES_FPE_decrypt(key, tweak, ct, None, radix) == (0, digits), case
        if n <= 200:
            assert ct == bytes(R.model(orc, key, tweak, list(digits), radix)), case
