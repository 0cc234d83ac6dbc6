"""FF3-1 (SP 800-38G revision 1) on the GPU (uaes_ff3.hip): the FF3-1 stanzas of the reference's vector file, what the
reference compiled with FF_X 3 gave (tests/golden/ff3_ref_vectors.json), other radices against the specification model
at every length each of them takes (with the texts at which a half reaches radix^m = 2^96 exactly), the fourth tweak
byte that both tweak halves share, batches whose counts come from the planner (shared and per-record tweaks at two
strides, host and device arrays, odd base addresses), batches with bytes that are no numerals, the limits, and a seeded
fuzz of round trips.  Every failing case prints the tuple that reproduces it."""
import ctypes as C
import functools
import random

import pytest

import micro_aes_amd as uaes
from tests import ff3_ref as R
from tests.guarded_mem import Mem

pytestmark = pytest.mark.gpu

E_ARG, E_DATALENGTH, E_DECRYPTION, E_ENCRYPTION = -2, 1, 0x1D, 0x1E
RADICES = [2, 3, 16, 26, 36, 64, 95, 255, 256]
FOURTH = [0x0F, 0xF0, 0xFF, 0xA5]


def kbuf(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def test_the_calls_below_run_on_the_gpu():
    """the single calls of this file must reach k_ff3: the host policy that would keep them on the host is off"""
    assert uaes.host_policy()[1] == 0


def test_vector_file(golden_dir):
    vs = R.vectors(golden_dir)
    assert len(vs) == 22 and sorted(set(len(v["alphabet"]) for v in vs)) == [10, 26, 36, 64]
    for v in vs:
        assert uaes.AES_FF3_encrypt(v["key"], v["tweak"], v["pt"], v["alphabet"]) == (0, v["ct"]), v
        assert uaes.AES_FF3_decrypt(v["key"], v["tweak"], v["ct"], v["alphabet"]) == (0, v["pt"]), v


def test_recorded_reference(golden_dir):
    entries, refusals = R.fixtures(golden_dir)
    assert sorted(set(len(e["key"]) for e in entries)) == [16, 24, 32]
    for bits in (128, 192, 256):
        assert set(range(6, 57)) <= set(len(e["pt"]) for e in entries if len(e["key"]) * 8 == bits and e["what"] == "seeded")
    for e in entries:
        assert uaes.AES_FF3_encrypt(e["key"], e["tweak"], e["pt"]) == (0, e["ct"]), e
        assert uaes.AES_FF3_decrypt(e["key"], e["tweak"], e["ct"]) == (0, e["pt"]), e
    assert len(refusals) == 3
    for r in refusals:                                         # the reference's one code per direction, output untouched
        n, fill = len(r["text"]), bytes([r["prefill"]])
        assert (r["encrypt_code"], r["decrypt_code"]) == (E_ENCRYPTION, E_DECRYPTION) and r["encrypt_out"] == fill * (n + 2)
        want = E_DATALENGTH if n in (5, 57) else None
        assert uaes.AES_FF3_encrypt(r["key"], r["tweak"], r["text"], prefill=r["prefill"]) == (want or E_ENCRYPTION, fill * n), r
        assert uaes.AES_FF3_decrypt(r["key"], r["tweak"], r["text"], prefill=r["prefill"]) == (want or E_DECRYPTION, fill * n), r


@pytest.mark.parametrize("radix", RADICES)
def test_radices_against_the_model(orc, radix):
    """every length the radix takes, raw digit values and a shuffled alphabet; then the all-zero and all-(radix - 1)
    texts at minlen, maxlen - 1 and maxlen: at radix 2 / 16 / 64 / 256 a half of the longest text reaches radix^m = 2^96
    exactly (192, 48, 32 and 24 numerals)"""
    rng = random.Random(radix)
    lo, hi = R.minlen(radix), R.maxlen(radix)
    assert uaes.ff3_maxlen(radix) == hi
    if radix in (2, 16, 64, 256):
        assert radix ** (hi // 2) == 1 << 96 and hi == {2: 192, 16: 48, 64: 32, 256: 24}[radix]
    alphabet = bytes(rng.sample(range(256), radix))
    cases = [[rng.randrange(radix) for _ in range(n)] for n in range(lo, hi + 1)]
    cases += [[d] * n for n in (lo, hi - 1, hi) for d in (0, radix - 1)]
    for digits in cases:
        key, tweak = rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(7)
        want = R.model(orc, key, tweak, digits, radix)
        case = (radix, len(digits), key.hex(), tweak.hex(), digits[:2])
        assert uaes.AES_FF3_encrypt(key, tweak, bytes(digits), None, radix) == (0, bytes(want)), case
        assert uaes.AES_FF3_decrypt(key, tweak, bytes(want), None, radix) == (0, bytes(digits)), case
        text, ct = bytes(alphabet[d] for d in digits), bytes(alphabet[d] for d in want)
        assert uaes.AES_FF3_encrypt(key, tweak, text, alphabet) == (0, ct), case
        assert uaes.AES_FF3_decrypt(key, tweak, ct, alphabet) == (0, text), case


def test_fourth_tweak_byte(orc):
    rng = random.Random(13)
    for b3 in FOURTH:
        for radix, n in ((10, 6), (10, 19), (10, 56), (36, 21), (2, 192)):
            key, tweak = rng.randbytes(rng.choice([16, 24, 32])), bytearray(rng.randbytes(7))
            tweak[3] = b3
            digits = [rng.randrange(radix) for _ in range(n)]
            want = R.model(orc, key, bytes(tweak), digits, radix)
            case = (b3, radix, n, key.hex(), tweak.hex())
            assert uaes.AES_FF3_encrypt(key, bytes(tweak), bytes(digits), None, radix) == (0, bytes(want)), case
            assert uaes.AES_FF3_decrypt(key, bytes(tweak), bytes(want), None, radix) == (0, bytes(digits)), case


# ---- batches ----------------------------------------------------------------------------------------------------------
BATCH_KEY = bytes(range(0x40, 0x50))
SHARED_TWEAK = bytes(range(0xA1, 0xA8))
POOL = 131            # distinct (record, tweak) pairs of a batch; record m is pair m % POOL
BATCH_SHAPES = [(10, 16), (10, 19), (10, 6), (10, 56), (2, 192)]


@functools.lru_cache(maxsize=None)
def grid_counts():
    """(a count that fills the planner's grid exactly, one more: the kernel strides)"""
    _, _, grid, threads = uaes.ff3_plan(16, 1 << 24)          # far more records than the grid holds: the cap
    fill = grid * (threads // 16)
    assert uaes.ff3_plan(16, fill)[2:] == (grid, threads) and uaes.ff3_plan(16, fill + 1)[2:] == (grid, threads)
    assert uaes.ff3_plan(16, fill - threads // 16)[2] == grid - 1
    return fill, fill + 1


_answers = {}


def batch_answers(orc, radix, n):
    """POOL records of n numerals and their tweaks with the model's answers under the shared and under the per-record
    tweaks, computed once.  A batch's record m is pair m % POOL: a record or tweak taken from the wrong index shows
    unless the indices differ by a multiple of 131, which no stride of the kernel (16, 64, the grid) is."""
    if (radix, n) not in _answers:
        rng = random.Random(1000 * radix + n)
        alphabet = R.DECIMAL if radix == 10 else bytes(range(radix))
        recs = [[rng.randrange(radix) for _ in range(n)] for _ in range(POOL)]
        tweaks = [rng.randbytes(7) for _ in range(POOL)]
        text = lambda rows: [bytes(alphabet[d] for d in r) for r in rows]
        _answers[radix, n] = (text(recs), tweaks, text(R.model_batch(orc, BATCH_KEY, [SHARED_TWEAK] * POOL, recs, radix)),
                              text(R.model_batch(orc, BATCH_KEY, tweaks, recs, radix)), alphabet)
    return _answers[radix, n]


def cyc(rows, count):
    return b"".join(rows[m % POOL] for m in range(count))


def run_batch(decrypt, key, radix, alphabet, tweak_mem, stride, count, n, src, dst, verdicts):
    L = uaes.engine()
    fn = L.uaes_ff3_decrypt_batch if decrypt else L.uaes_ff3_encrypt_batch
    return fn(len(key) * 8, kbuf(key), radix, kbuf(alphabet) if alphabet else None, tweak_mem.ptr if tweak_mem else None,
              stride, count, n, src.ptr, dst.ptr, verdicts.ptr if verdicts else None)


@pytest.mark.parametrize("which", ["1", "3", "4", "5", "63", "64", "65", "fill", "stride"])
@pytest.mark.parametrize("shape", BATCH_SHAPES, ids=lambda s: "r%dn%d" % s)
def test_batches(orc, shape, which):
    radix, n = shape
    count = {"fill": grid_counts()[0], "stride": grid_counts()[1]}.get(which) or int(which)
    if which == "fill":
        _, _, grid, threads = uaes.ff3_plan(n, count, radix)
        assert count == grid * (threads // 16) and uaes.ff3_plan(n, count + 1, radix)[2] == grid
    recs, tweaks, shared, per, alphabet = batch_answers(orc, radix, n)
    pt = cyc(recs, count)
    placements = ((False, 0), (True, 0), (True, 1), (False, 3))
    for stride in (0, 7, 9):
        want = cyc(per if stride else shared, count)
        tw = cyc([t + bytes([0xEE]) * (stride - 7) for t in tweaks], count)[:(count - 1) * stride + 7] if stride else SHARED_TWEAK
        for device, off in placements:
            src, dst, twm = Mem(pt, device, off), Mem(b"", device, off, size=len(pt)), Mem(tw, device, off)
            ver = Mem(b"", device, off, size=count, fill=7)
            case = (radix, n, count, stride, device, off)
            assert run_batch(0, BATCH_KEY, radix, alphabet, twm, stride, count, n, src, dst, ver) == 0, case
            got = dst.get()
            if got != want:
                bad = [m for m in range(count) if got[m * n:(m + 1) * n] != want[m * n:(m + 1) * n]]
                raise AssertionError("%r: %d records differ, the first at %d" % (case, len(bad), bad[0]))
            assert ver.get() == bytes([1]) * count and dst.intact() and ver.intact() and src.get() == pt, case
        # and back, in place, in device memory
        buf_, twm = Mem(want, True, 1), Mem(tw, True, 0)
        assert run_batch(1, BATCH_KEY, radix, alphabet, twm, stride, count, n, buf_, buf_, None) == 0
        assert buf_.get() == pt and buf_.intact(), (radix, n, count, stride, "decrypt in place")


@pytest.mark.parametrize("decrypt", [0, 1])
def test_batch_with_bytes_that_are_no_numerals(orc, decrypt):
    n, count = 19, 150
    name, _, grid, threads = uaes.ff3_plan(n, count)
    per = threads // 16                                        # records per workgroup
    assert name == "ff3.batch" and grid >= 3 and grid * per >= count
    bad = sorted({0, per - 1, per, 2 * per - 1, 77, count - 1})
    assert len(bad) == 6
    recs, tweaks, shared, perans, alphabet = batch_answers(orc, 10, n)
    good_in = [(perans if decrypt else recs)[m % POOL] for m in range(count)]
    good_out = [(recs if decrypt else perans)[m % POOL] for m in range(count)]
    rng = random.Random(5)
    inp = list(good_in)
    for k, m in enumerate(bad):
        r = bytearray(inp[m])
        r[(0, n // 2, n - 1)[k % 3]] = rng.choice(b"/:aA\x00\xff")
        inp[m] = bytes(r)
    for device in (False, True):
        for with_verdicts in (True, False):
            src, dst = Mem(b"".join(inp), device, 1), Mem(b"", device, 1, size=n * count, fill=0x5C)
            twm = Mem(cyc(tweaks, count), device)
            ver = Mem(b"", device, 0, size=count, fill=7) if with_verdicts else None
            rc = run_batch(decrypt, BATCH_KEY, 10, R.DECIMAL, twm, 7, count, n, src, dst, ver)
            assert rc == (E_DECRYPTION if decrypt else E_ENCRYPTION), (device, with_verdicts)
            got = dst.get()
            for m in range(count):
                want = bytes([0x5C]) * n if m in bad else good_out[m]
                assert got[m * n:(m + 1) * n] == want, (decrypt, device, m)
            assert dst.intact()
            if ver:
                assert ver.get() == bytes(0 if m in bad else 1 for m in range(count)) and ver.intact()


def test_limits():
    rng = random.Random(3)
    twm = Mem(SHARED_TWEAK)
    for radix, alphabet in ((10, R.DECIMAL), (2, None), (256, None)):
        lo, hi = R.minlen(radix), R.maxlen(radix)
        n = hi + 1
        src, dst, ver = Mem(bytes(rng.choice(alphabet or b"\0\1") for _ in range(2 * n))), Mem(b"", size=2 * n), Mem(b"", size=2, fill=7)
        for decrypt in (0, 1):
            assert run_batch(decrypt, BATCH_KEY, radix, alphabet, twm, 0, 2, n, src, dst, ver) == E_DATALENGTH, radix
            assert run_batch(decrypt, BATCH_KEY, radix, alphabet, twm, 0, 2, lo - 1, src, dst, ver) == E_DATALENGTH, radix
            assert run_batch(decrypt, BATCH_KEY, radix, alphabet, twm, 0, 0, lo, src, dst, ver) == 0, radix
            fn = uaes.AES_FF3_decrypt if decrypt else uaes.AES_FF3_encrypt
            for k in (lo - 1, n):
                assert fn(BATCH_KEY, SHARED_TWEAK, src.get()[:k], alphabet, radix, prefill=9) == (E_DATALENGTH, bytes([9]) * k)
        assert dst.get() == bytes([0x5C]) * (2 * n) and ver.get() == bytes([7, 7]) and dst.intact() and ver.intact()
    src, dst, ver = Mem(b"1234567890123456" * 2), Mem(b"", size=32), Mem(b"", size=2, fill=7)
    assert run_batch(0, BATCH_KEY, 257, None, twm, 0, 2, 16, src, dst, ver) == E_ARG
    assert run_batch(0, BATCH_KEY, 10, b"0123456780", twm, 0, 2, 16, src, dst, ver) == E_ARG
    assert dst.get() == bytes([0x5C]) * 32 and ver.get() == bytes([7, 7])
    assert uaes.AES_FF3_encrypt(BATCH_KEY, SHARED_TWEAK, b"12345/7", prefill=9) == (E_ENCRYPTION, bytes([9]) * 7)
    assert uaes.AES_FF3_decrypt(BATCH_KEY, SHARED_TWEAK, b"1234567" * 7 + b"a", prefill=9) == (E_DECRYPTION, bytes([9]) * 50)


def test_fuzz_round_trips(orc):
    rng = random.Random(20261019)
    for k in range(60):
        radix = rng.choice([2, 256, 3, 10, 10, 16, 36, 62, 100, 255, rng.randrange(2, 257)])
        lo, hi = R.minlen(radix), R.maxlen(radix)
        n = rng.choice([lo, hi, rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1)])
        key, tweak = rng.randbytes(rng.choice([16, 24, 32])), rng.randbytes(7)
        digits = bytes(rng.randrange(radix) for _ in range(n))
        case = (k, radix, n, key.hex(), tweak.hex())
        rc, ct = uaes.AES_FF3_encrypt(key, tweak, digits, None, radix)
        assert rc == 0 and len(ct) == n and all(c < radix for c in ct) and ct != digits, case
        assert uaes.AES_FF3_decrypt(key, tweak, ct, None, radix) == (0, digits), case
        assert ct == bytes(R.model(orc, key, tweak, list(digits), radix)), case
