"""SIV with a vector of associated data on the GPU (k_s2v_v, k_s2v_batch_v: uaes_eax_siv.hip), everything against
tests/siv_v_ref.py: the fixtures (RFC 5297 A.2 included), single calls at every component count around the number of rows
the plan hook reports and every text length around the block and the small / long boundary it reports, forgeries of every
part under both settings of the wipe switch, host / device / odd-offset / in-place placement between guard bytes, and
batches at every wave and workgroup edge with and without a length per record."""
import ctypes as C
import random

import pytest

import micro_aes_amd as uaes
from tests import siv_v_ref as R
from tests.guarded_mem import FILL, Mem

pytestmark = pytest.mark.gpu

E_ARG = -2
AD_MAX, BATCH_AD_MAX = 126, 8                   # UAES_SIV_AD_MAX, UAES_SIV_BATCH_AD_MAX (include/uaes_hip.h)
AD_SIZES = (0, 1, 15, 16, 17, 32, 33)
BATCH_AD_SIZES = (0, 1, 13, 16, 17)


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def rows():
    return uaes.siv_v_plan(0, 1)[3]


def boundary():
    """the longest text of the small arrangement, found by walking the plan hook"""
    lo, hi = 0, 1 << 26
    assert uaes.siv_v_plan(lo, 1)[0] == "s2v.small.v" and uaes.siv_v_plan(hi, 1)[0] == "s2v.long.v"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if uaes.siv_v_plan(mid, 1)[0] == "s2v.small.v" else (lo, mid)
    return lo


def nads():
    r = rows()
    return [0, 1, 2, 3, 5, r - 1, r, r + 1, 2 * r + 1, AD_MAX]


def text_lengths():
    b = boundary()
    return [0, 1, 15, 16, 17, 31, 32, 33, b - 1, b, b + 1, (1 << 20) + 5]


def key_of(rng, k):
    return rng.randbytes((32, 48, 64)[k % 3])


def test_the_plan_supports_the_cases():
    r, b = rows(), boundary()
    assert 2 <= r and 2 * r + 1 <= AD_MAX and b >= 64
    assert uaes.siv_v_plan(b, r)[:2] == ("s2v.small.v", 1) and uaes.siv_v_plan(b + 1, r)[:2] == ("s2v.long.v", 2)
    assert uaes.siv_v_plan((1 << 20) + 5, AD_MAX, decrypt=True)[:2] == ("s2v.long.v", 2)


def test_fixtures():
    cases = R.fixtures()
    assert {len(c["keys"]) for c in cases} == {32, 48, 64}
    for c in cases:
        assert uaes.AES_SIV_encrypt_v(c["keys"], c["ads"], c["pt"]) == (c["iv"], c["ct"]), c["name"]
        assert uaes.AES_SIV_decrypt_v(c["keys"], c["iv"], c["ads"], c["ct"]) == (0, c["pt"]), c["name"]
    a2, = [c for c in cases if c["name"] == "rfc5297.A2"]
    assert a2["iv"].hex() == "7bdb6e3b432667eb06f4d14bff2fbd0f" and len(a2["ads"]) == 3


@pytest.mark.parametrize("k", range(10))
def test_single_calls(k):
    """component count k of the list (0, 1, 2, 3, 5, R - 1, R, R + 1, 2 R + 1, 126) x every text length, encrypt then
    decrypt; the key size goes round"""
    nad = nads()[k]
    rng = random.Random(1000 + k)
    for j, n in enumerate(text_lengths()):
        keys = key_of(rng, k + j)
        ads = [rng.randbytes(rng.choice(AD_SIZES)) for _ in range(nad)]
        if nad:
            ads[rng.randrange(nad)] = b"" if j % 2 else rng.randbytes(33)       # an empty component somewhere, every other text
        pt = rng.randbytes(n)
        want = R.siv_encrypt(keys, ads, pt)
        got = uaes.AES_SIV_encrypt_v(keys, ads, pt)
        assert got == want, (nad, n, len(keys), [len(a) for a in ads])
        assert uaes.AES_SIV_decrypt_v(keys, got[0], ads, got[1]) == (0, pt), (nad, n, len(keys))


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_what_the_component_list_means(bits):
    rng = random.Random(bits)
    keys = rng.randbytes(bits // 4)
    for n in (0, 7, 16, 40, boundary() + 1):
        pt, ad = rng.randbytes(n), rng.randbytes(1 + n % 50)
        assert uaes.AES_SIV_encrypt_v(keys, [], pt) == uaes.AES_SIV_encrypt(keys, b"", pt)
        assert uaes.AES_SIV_encrypt_v(keys, [ad], pt) == uaes.AES_SIV_encrypt(keys, ad, pt)
        empty = uaes.AES_SIV_encrypt_v(keys, [b""], pt)
        assert empty == R.siv_encrypt(keys, [b""], pt) and empty != uaes.AES_SIV_encrypt_v(keys, [], pt)
        lists = ([b"ab", b"c"], [b"a", b"bc"], [b"abc"])
        got = [uaes.AES_SIV_encrypt_v(keys, ads, pt) for ads in lists]
        assert got == [R.siv_encrypt(keys, ads, pt) for ads in lists] and len({iv for iv, _ in got}) == 3


@pytest.mark.parametrize("wipe", [0, 1])
def test_forgeries_in_each_part(wipe):
    rng = random.Random(50 + wipe)
    eng = uaes.engine()
    eng.uaes_set_wipe_on_auth_failure(wipe)
    try:
        for k, n in enumerate((0, 5, 16, 70, boundary(), boundary() + 1)):
            keys = key_of(rng, k)
            ads = [rng.randbytes(20), rng.randbytes(7), rng.randbytes(16), rng.randbytes(33)]
            pt = rng.randbytes(n)
            iv, ct = uaes.AES_SIV_encrypt_v(keys, ads, pt)
            joined = b"".join(ads)
            forged = [(flip(iv, 2 + k), ads, ct), (iv, [ads[1], ads[0]] + ads[2:], ct), (iv, [joined[:19], joined[19:27]] + ads[2:], ct),
                      (iv, ads + [b""], ct), (iv, ads[:3], ct)]
            forged += [(iv, [flip(a, 3 + k) if i == j else a for j, a in enumerate(ads)], ct) for i in range(4)]
            if n:
                forged += [(iv, ads, flip(ct, 8 * n - 3)), (iv, ads, flip(ct, 0))]
            for f_iv, f_ads, f_ct in forged:
                rc, text = uaes.AES_SIV_decrypt_v(keys, f_iv, f_ads, f_ct, prefill=0x5C)
                want_rc, want_text = R.siv_decrypt(keys, f_iv, f_ads, f_ct)
                assert rc == want_rc == 0x1A, (n, len(f_ads))
                assert text == (bytes(n) if wipe else want_text), (n, len(f_ads))      # zeroed, or released as CTR made it
    finally:
        eng.uaes_set_wipe_on_auth_failure(0)


def call_v(decrypt, keys, iv, adl, ad, src, n, dst):
    """the raw calls; iv, ad, src, dst: Mem"""
    L = uaes.engine()
    lens = (C.c_size_t * max(len(adl), 1))(*adl) if adl else None
    if decrypt:
        return L.uaes_siv_decrypt_v(len(keys) * 4, keys, iv.ptr, len(adl), lens, ad.ptr, src.ptr, n, dst.ptr)
    return L.uaes_siv_encrypt_v(len(keys) * 4, keys, len(adl), lens, ad.ptr, src.ptr, n, iv.ptr, dst.ptr)


PLACES = [("host", False, 0, 0, 0), ("device", True, 0, 0, 0), ("device odd offsets", True, 1, 3, 1),
          ("device, odd text only", True, 0, 2, 0), ("host text, device components", None, 3, 0, 0)]


@pytest.mark.parametrize("place", PLACES, ids=[p[0] for p in PLACES])
def test_placement_with_guards(place):
    _, dev, ad_off, text_off, iv_off = place
    rng = random.Random(hash(place[0]) & 0xffff)
    for k, (nad, n) in enumerate(((0, 17), (1, 16), (3, 33), (rows() + 1, 100), (5, boundary() + 1))):
        keys = key_of(rng, k)
        ads = [rng.randbytes(rng.choice(AD_SIZES)) for _ in range(nad)]
        adl, pt = [len(a) for a in ads], rng.randbytes(n)
        want_iv, want_ct = R.siv_encrypt(keys, ads, pt)
        text_dev = bool(dev)
        ad = Mem(b"".join(ads), device=dev is not False, off=ad_off)
        src, dst = Mem(pt, device=text_dev, off=text_off), Mem(b"", device=text_dev, off=text_off, size=n)
        iv = Mem(b"", device=text_dev, off=iv_off, size=16)
        assert call_v(False, keys, iv, adl, ad, src, n, dst) == 0, (nad, n)
        assert (iv.get(), dst.get()) == (want_iv, want_ct), (nad, n)
        assert ad.intact() and src.intact() and dst.intact() and iv.intact() and src.get() == pt
        back = Mem(b"", device=text_dev, off=text_off, size=n)
        assert call_v(True, keys, iv, adl, ad, dst, n, back) == 0 and back.get() == pt and back.intact()
        # in place, both directions
        buf = Mem(pt, device=text_dev, off=text_off)
        assert call_v(False, keys, iv, adl, ad, buf, n, buf) == 0 and buf.get() == want_ct and buf.intact()
        assert call_v(True, keys, iv, adl, ad, buf, n, buf) == 0 and buf.get() == pt and buf.intact()


# ---- batches ----------------------------------------------------------------------------------------------------------

def ragged(rng, nmsg, ml):
    """a length per record: 0 and an entry above the slot among them"""
    lens = [rng.randrange(ml + 1) for _ in range(nmsg)]
    lens[0] = 0
    lens[-1] = ml + 7
    if nmsg > 2:
        lens[1] = ml
    return lens


def expect_batch(keys, ads, texts, lens):
    ml = len(texts[0]) if texts else 0
    out = []
    for m, (a, t) in enumerate(zip(ads, texts)):
        n = ml if lens is None else min(lens[m], ml)
        iv, ct = R.siv_encrypt(keys, a, t[:n])
        out.append((iv, ct + bytes([FILL]) * (ml - n)))
    return out


@pytest.mark.parametrize("nmsg", [1, 3, 4, 5, 63, 64, 65, 4096])
def test_batches(nmsg):
    """every slot size x every component count x lens NULL / ragged (the largest batch: every slot size x both, the
    component count going round), every record against the reference, the unwritten rest of each slot the prefill"""
    rng = random.Random(nmsg)
    k = 0
    for ml in (0, 1, 16, 17, 48):
        for nad in (1, 2, 3, 8) if nmsg < 4096 else ((1, 2, 3, 8)[(ml + 1) % 4],):
            for with_lens in (False, True):
                k += 1
                keys = key_of(rng, k)
                shape = [rng.choice(BATCH_AD_SIZES) for _ in range(nad)]
                shape[rng.randrange(nad)] = (17, 0, 13)[k % 3]
                ads = [[rng.randbytes(s) for s in shape] for _ in range(nmsg)]
                texts = [rng.randbytes(ml) for _ in range(nmsg)]
                lens = ragged(rng, nmsg, ml) if with_lens else None
                want = expect_batch(keys, ads, texts, lens)
                ivs, cts = uaes.siv_batch_v(keys, ads, texts, prefill=FILL, lens=lens)
                assert list(zip(ivs, cts)) == want, (nmsg, ml, shape, with_lens)
                rc, pts, verdicts = uaes.siv_batch_v(keys, ads, cts, decrypt=True, ivs=ivs, prefill=FILL, lens=lens)
                cut = [t if lens is None else t[:min(n, ml)] + bytes([FILL]) * (ml - min(n, ml)) for t, n in zip(texts, lens or texts)]
                assert (rc, pts, verdicts) == (0, cut, [1] * nmsg), (nmsg, ml, shape, with_lens)


@pytest.mark.parametrize("wipe", [0, 1])
def test_batch_forgeries_at_the_edges_of_waves(wipe):
    """forged records at the first and last row of a wave and of the batch, one part each"""
    rng = random.Random(70 + wipe)
    nmsg, ml, shape = 131, 33, [13, 0, 16]
    keys = rng.randbytes(32)
    ads = [[rng.randbytes(s) for s in shape] for _ in range(nmsg)]
    texts = [rng.randbytes(ml) for _ in range(nmsg)]
    lens = [ml] * nmsg
    lens[4], lens[64] = 20, 0
    ivs, cts = uaes.siv_batch_v(keys, ads, texts, lens=lens)
    f_ivs, f_cts, f_ads = list(ivs), list(cts), [list(a) for a in ads]
    f_ivs[0] = flip(ivs[0], 9)                                   # first row of the first wave
    f_cts[3] = flip(cts[3], 100)                                 # its last row
    f_ads[4][0] = flip(ads[4][0], 5)                             # first row of the second wave (a shorter record)
    f_ads[63] = [ads[63][0] + ads[63][2][:0], b"", ads[63][2][::-1]]   # last row of the first workgroup's worth
    f_ivs[64] = flip(ivs[64], 1)                                 # an empty record
    f_ads[127][2] = flip(ads[127][2], 77)
    f_cts[nmsg - 1] = flip(cts[nmsg - 1], 3)                     # the last record of the batch
    bad = {0, 3, 4, 63, 64, 127, nmsg - 1}
    eng = uaes.engine()
    eng.uaes_set_wipe_on_auth_failure(wipe)
    try:
        rc, pts, verdicts = uaes.siv_batch_v(keys, f_ads, f_cts, decrypt=True, ivs=f_ivs, prefill=FILL, lens=lens)
    finally:
        eng.uaes_set_wipe_on_auth_failure(0)
    assert rc == 0x1A and verdicts == [0 if m in bad else 1 for m in range(nmsg)]
    for m in range(nmsg):
        n = lens[m]
        want_rc, text = R.siv_decrypt(keys, f_ivs[m], f_ads[m], f_cts[m][:n])
        assert (want_rc != 0) == (m in bad), m
        if m in bad and wipe:
            text = bytes(n)
        assert pts[m] == text + bytes([FILL]) * (ml - n), m


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_one_component_without_lens_is_the_old_batch(bits):
    rng = random.Random(bits)
    keys = rng.randbytes(bits // 4)
    for nmsg, ml, al in ((1, 16, 13), (65, 17, 16), (300, 48, 1), (64, 0, 17)):
        aads = [rng.randbytes(al) for _ in range(nmsg)]
        texts = [rng.randbytes(ml) for _ in range(nmsg)]
        old = uaes.siv_batch(keys, aads, texts)
        assert uaes.siv_batch_v(keys, [[a] for a in aads], texts) == old, (nmsg, ml, al)
        rc, pts, verdicts = uaes.siv_batch_v(keys, [[a] for a in aads], old[1], decrypt=True, ivs=old[0])
        assert (rc, pts, verdicts) == uaes.siv_batch(keys, aads, old[1], decrypt=True, ivs=old[0]) == (0, texts, [1] * nmsg)


def u32s(lens):
    return b"".join(int(n).to_bytes(4, "little") for n in lens)


BATCH_PLACES = [("device", True, 0), ("device odd offsets", True, 1), ("host odd offsets", False, 3)]


@pytest.mark.parametrize("place", BATCH_PLACES, ids=[p[0] for p in BATCH_PLACES])
def test_batch_placement_with_guards(place):
    _, dev, off = place
    rng = random.Random(len(place[0]))
    L = uaes.engine()
    for nmsg, ml, shape in ((5, 17, [13, 16]), (65, 48, [0, 17, 1]), (64, 16, [16])):
        keys = rng.randbytes(32)
        ads = [[rng.randbytes(s) for s in shape] for _ in range(nmsg)]
        texts = [rng.randbytes(ml) for _ in range(nmsg)]
        lens = ragged(rng, nmsg, ml)
        want = expect_batch(keys, ads, texts, lens)
        adl = (C.c_size_t * len(shape))(*shape)
        a = Mem(b"".join(b"".join(r) for r in ads), device=dev, off=off)
        lv = Mem(u32s(lens), device=dev, off=0)                                 # (a device array of lengths: 4-byte aligned)
        src, dst = Mem(b"".join(texts), device=dev, off=off), Mem(b"", device=dev, off=off, size=nmsg * ml)
        ivs = Mem(b"", device=dev, off=off, size=16 * nmsg)
        head = (256 // 2, keys, nmsg, ml, lv.ptr, len(shape), adl, a.ptr)
        assert L.uaes_siv_encrypt_batch_v(*head, src.ptr, ivs.ptr, dst.ptr) == 0
        assert ivs.get() == b"".join(w[0] for w in want) and dst.get() == b"".join(w[1] for w in want), (nmsg, ml)
        assert all(m.intact() for m in (a, lv, src, dst, ivs))
        back, verdicts = Mem(b"", device=dev, off=off, size=nmsg * ml), Mem(b"", device=dev, off=off, size=nmsg)
        assert L.uaes_siv_decrypt_batch_v(*head, ivs.ptr, dst.ptr, back.ptr, verdicts.ptr) == 0
        assert verdicts.get() == bytes([1]) * nmsg and back.intact() and verdicts.intact()
        assert back.get() == b"".join(t[:min(n, ml)] + bytes([FILL]) * (ml - min(n, ml)) for t, n in zip(texts, lens))
        if dev:                                                                 # a misaligned device array of lengths is refused
            odd = Mem(u32s(lens), device=True, off=2)
            before = dst.raw()
            assert L.uaes_siv_encrypt_batch_v(256 // 2, keys, nmsg, ml, odd.ptr, len(shape), adl, a.ptr, src.ptr, ivs.ptr, dst.ptr) == E_ARG
            assert dst.raw() == before
