"""SIV with a vector of associated data (uaes_siv_encrypt_v / uaes_siv_decrypt_v and the _batch_v calls) without a GPU:
the engine's host path (forced on with uaes.host_policy, restored after) against tests/golden/siv_v_vectors.json (RFC
5297 A.1 and A.2, cases recorded from libcrypto) and tests/siv_v_ref.py; what the component list means; forgeries; every
argument the calls refuse with UAES_E_ARG before the device is touched; the planner hook."""
import ctypes as C
import random

import pytest

import micro_aes_amd as uaes
from tests import eax_siv_ref as R1
from tests import siv_v_ref as R
from tests.test_abi_and_host import declared_functions

E_ARG = -2                                      # UAES_E_ARG (include/uaes_hip.h)
AD_MAX, BATCH_AD_MAX = 126, 8                   # UAES_SIV_AD_MAX, UAES_SIV_BATCH_AD_MAX (include/uaes_hip.h)
NAMES = {"uaes_siv_encrypt_v", "uaes_siv_decrypt_v", "uaes_siv_encrypt_batch_v", "uaes_siv_decrypt_batch_v",
         "uaes_debug_plan_siv_v"}


@pytest.fixture
def host_forced():
    prev = uaes.host_policy(max_bytes=1 << 30, chains=1)
    yield
    uaes.host_policy(*prev)


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def test_fixtures_in_both_directions(host_forced):
    cases = R.fixtures()
    assert len(cases) >= 60 and {c["name"] for c in cases} >= {"rfc5297.A1", "rfc5297.A2"}
    assert {len(c["keys"]) for c in cases} == {32, 48, 64}
    assert any(b"" in c["ads"] for c in cases) and any(c["source"].startswith("libcrypto") for c in cases)
    for c in cases:
        assert uaes.AES_SIV_encrypt_v(c["keys"], c["ads"], c["pt"]) == (c["iv"], c["ct"]), c["name"]
        assert uaes.AES_SIV_decrypt_v(c["keys"], c["iv"], c["ads"], c["ct"]) == (0, c["pt"]), c["name"]
        assert R.siv_encrypt(c["keys"], c["ads"], c["pt"]) == (c["iv"], c["ct"]), c["name"]


def test_rfc5297_a2_is_nonce_based_siv(host_forced):
    a2, = [c for c in R.fixtures() if c["name"] == "rfc5297.A2"]
    assert len(a2["ads"]) == 3 and a2["ads"][2].hex() == "09f911029d74e35bd84156c5635688c0"
    assert a2["iv"].hex() == "7bdb6e3b432667eb06f4d14bff2fbd0f"
    assert uaes.AES_SIV_encrypt_v(a2["keys"], a2["ads"], a2["pt"]) == (a2["iv"], a2["ct"])


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_the_reference_agrees_with_the_single_component_calls(bits):
    """tests/siv_v_ref.py with zero or one non-empty component is the compiled reference's AES_SIV_encrypt"""
    rng = random.Random(bits)
    for n in (0, 1, 15, 16, 17, 33, 200):
        keys, ad, pt = rng.randbytes(bits // 4), rng.randbytes(1 + n % 40), rng.randbytes(n)
        assert R.siv_encrypt(keys, [ad], pt) == R1.siv_encrypt(bits, keys, ad, pt)
        assert R.siv_encrypt(keys, [], pt) == R1.siv_encrypt(bits, keys, b"", pt)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_what_the_component_list_means(host_forced, bits):
    rng = random.Random(100 + bits)
    keys = rng.randbytes(bits // 4)
    for n in (0, 5, 16, 40):
        pt, ad = rng.randbytes(n), rng.randbytes(1 + n)
        # no component = the old call without AAD; one non-empty component = the old call
        assert uaes.AES_SIV_encrypt_v(keys, [], pt) == uaes.AES_SIV_encrypt(keys, b"", pt)
        assert uaes.AES_SIV_encrypt_v(keys, [ad], pt) == uaes.AES_SIV_encrypt(keys, ad, pt)
        # an empty component is a component
        empty = uaes.AES_SIV_encrypt_v(keys, [b""], pt)
        assert empty == R.siv_encrypt(keys, [b""], pt) and empty != uaes.AES_SIV_encrypt_v(keys, [], pt)
        assert uaes.AES_SIV_encrypt_v(keys, [b"", b""], pt) not in (empty, uaes.AES_SIV_encrypt_v(keys, [], pt))
        # order and boundaries are bound
        three = [uaes.AES_SIV_encrypt_v(keys, ads, pt) for ads in ([b"ab", b"c"], [b"a", b"bc"], [b"abc"], [b"c", b"ab"])]
        assert len({iv for iv, _ in three}) == 4
        for ads, got in zip(([b"ab", b"c"], [b"a", b"bc"], [b"abc"], [b"c", b"ab"]), three):
            assert got == R.siv_encrypt(keys, ads, pt)
    ads = [rng.randbytes(rng.choice((0, 1, 15, 16, 17, 32, 33))) for _ in range(AD_MAX)]
    pt = rng.randbytes(50)
    iv, ct = uaes.AES_SIV_encrypt_v(keys, ads, pt)
    assert (iv, ct) == R.siv_encrypt(keys, ads, pt)
    assert uaes.AES_SIV_decrypt_v(keys, iv, ads, ct) == (0, pt)


def test_forgeries(host_forced):
    rng = random.Random(12)
    keys = rng.randbytes(32)
    ads, pt = [rng.randbytes(20), rng.randbytes(7), rng.randbytes(16)], rng.randbytes(70)
    iv, ct = uaes.AES_SIV_encrypt_v(keys, ads, pt)
    joined = b"".join(ads)
    forged = [(flip(iv, 2), ads, ct), (iv, ads, flip(ct, 30)),
              (iv, [ads[1], ads[0], ads[2]], ct), (iv, [ads[0], ads[2], ads[1]], ct),          # two components swapped
              (iv, [joined[:19], joined[19:27], joined[27:]], ct), (iv, [joined[:20], joined[20:]], ct)]   # a moved boundary
    forged += [(iv, [flip(a, 3) if k == j else a for j, a in enumerate(ads)], ct) for k in range(3)]
    for f_iv, f_ads, f_ct in forged:
        rc, text = uaes.AES_SIV_decrypt_v(keys, f_iv, f_ads, f_ct, prefill=0x5C)
        assert rc == 0x1A
        assert (rc, text) == R.siv_decrypt(keys, f_iv, f_ads, f_ct)              # the text is released
    eng = uaes.engine()
    eng.uaes_set_wipe_on_auth_failure(1)
    try:
        assert uaes.AES_SIV_decrypt_v(keys, iv, ads, flip(ct, 3), prefill=0x5C) == (0x1A, bytes(len(pt)))
    finally:
        eng.uaes_set_wipe_on_auth_failure(0)


def single(nad=2, lens=True, ad=True, bits=128, keys=bytes(64), each=3, src=True, dst=True, iv=True, n=16):
    """(encrypt's code, decrypt's code, the output buffers) of the single calls; True = a buffer, None = NULL"""
    L = uaes.engine()
    adl = (C.c_size_t * max(nad, 1))(*([each] * max(nad, 1))) if lens else None
    a = (C.c_uint8 * 1024)() if ad else None
    o1, o2 = (C.c_uint8 * 64)(*([0x5C] * 64)), (C.c_uint8 * 64)(*([0x5C] * 64))
    ivb = (C.c_uint8 * 16)(*([0x5C] * 16))
    text = (C.c_uint8 * 64)()
    enc = L.uaes_siv_encrypt_v(bits, keys, nad, adl, a, text if src else None, n, ivb if iv else None, o1 if dst else None)
    dec = L.uaes_siv_decrypt_v(bits, keys, ivb if iv else None, nad, adl, a, text if src else None, n, o2 if dst else None)
    return enc, dec, bytes(o1) + bytes(o2) + bytes(ivb)


SINGLE_REFUSED = [("too many components", dict(nad=AD_MAX + 1)), ("NULL adLens", dict(lens=None)),
                  ("lengths overflow", dict(nad=2, each=1 << 63)), ("NULL aData", dict(ad=None)),
                  ("keybits 100", dict(bits=100)), ("keybits 0", dict(bits=0)), ("NULL keys", dict(keys=None)),
                  ("NULL iv", dict(iv=None)), ("NULL input", dict(src=None)), ("NULL output", dict(dst=None))]


@pytest.mark.parametrize("case", SINGLE_REFUSED, ids=[c[0] for c in SINGLE_REFUSED])
def test_single_calls_refuse(case, host_forced):
    enc, dec, out = single(**case[1])
    assert (enc, dec) == (E_ARG, E_ARG), case
    assert set(out) == {0x5C}                                                    # the outputs are untouched
    assert uaes.engine().uaes_last_error()


def test_single_calls_take_what_is_allowed(host_forced):
    for ok in (dict(), dict(nad=0, lens=None, ad=None), dict(nad=AD_MAX), dict(nad=3, each=0, ad=None), dict(n=0, src=None, dst=None),
               dict(bits=192), dict(bits=256)):
        enc, dec, _ = single(**ok)
        assert enc == 0 and dec in (0, 0x1A), ok                                 # (the decrypt is handed a made-up IV)


def batch(nmsg=2, msg_bytes=16, nad=2, each=3, adl=True, bits=128, keys=bytes(64), lens=False, aad=True, src=True, dst=True,
          ivs=True, verdicts=True):
    """(encrypt's code, decrypt's code) of the batch calls for one set of arguments; a refused call reads nothing"""
    L = uaes.engine()
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))() if on else None)             # noqa: E731
    small = nmsg if nmsg < 1 << 16 else 1
    lv = (C.c_uint32 * small)(*([msg_bytes & 0xffffffff] * small)) if lens else None
    al = (C.c_size_t * max(nad, 1))(*([each] * max(nad, 1))) if adl else None
    head = (bits, keys, nmsg, msg_bytes, lv, nad, al, buf(aad, small * min(nad * each, 1024)))
    text = lambda on: buf(on, small * min(msg_bytes, 64))                        # noqa: E731
    enc = L.uaes_siv_encrypt_batch_v(*head, text(src), buf(ivs, small * 16), text(dst))
    dec = L.uaes_siv_decrypt_batch_v(*head, buf(ivs, small * 16), text(src), text(dst), buf(verdicts, small))
    return enc, dec


BATCH_REFUSED = [("too many components", dict(nad=BATCH_AD_MAX + 1)), ("NULL adLens", dict(adl=None)),
                 ("lengths overflow", dict(each=1 << 63)), ("slot above UINT32_MAX", dict(msg_bytes=1 << 32)),
                 ("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("count overflows", dict(nmsg=(1 << 64) - 1, msg_bytes=0)),
                 ("AAD overflows", dict(nmsg=1 << 50, msg_bytes=0, each=0x8000)),
                 ("keybits 100", dict(bits=100)), ("keybits 0", dict(bits=0)), ("NULL keys", dict(keys=None)),
                 ("NULL aData", dict(aad=None)), ("NULL input", dict(src=None)), ("NULL output", dict(dst=None)),
                 ("NULL IVs", dict(ivs=None))]


@pytest.mark.parametrize("case", BATCH_REFUSED, ids=[c[0] for c in BATCH_REFUSED])
def test_batches_refuse(case):
    assert batch(**case[1]) == (E_ARG, E_ARG), case
    assert uaes.engine().uaes_last_error()


def test_batches_null_verdicts_and_no_records():
    assert batch(verdicts=None)[1] == E_ARG
    # no records: nothing to do, and nothing is looked at but the sizes and the keys
    assert batch(nmsg=0) == (0, 0)
    assert batch(nmsg=0, aad=None, src=None, dst=None, ivs=None, verdicts=None) == (0, 0)
    assert batch(nmsg=0, bits=100) == (E_ARG, E_ARG) and batch(nmsg=0, keys=None) == (E_ARG, E_ARG)
    assert batch(nmsg=0, nad=BATCH_AD_MAX + 1) == (E_ARG, E_ARG) and batch(nmsg=0, msg_bytes=1 << 32) == (E_ARG, E_ARG)
    # without a device a well-formed call gets as far as the device
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(), dict(bits=192), dict(bits=256), dict(msg_bytes=0, src=None, dst=None), dict(nad=0, adl=None, aad=None),
                   dict(nad=BATCH_AD_MAX), dict(each=0, aad=None), dict(lens=True)):
            assert batch(nmsg=1, **ok) == (-1, -1), ok                           # UAES_E_HIP: no usable device


def test_declared_and_mirrored():
    assert NAMES <= set(declared_functions("uaes_hip.h"))
    assert NAMES <= set(uaes.EXPORTS)
    assert uaes.siv_batch_v(bytes(32), [], []) == ([], []) and uaes.siv_batch_v(bytes(32), [], [], decrypt=True, ivs=[]) == (0, [], [])
    with pytest.raises(ValueError):
        uaes.siv_batch_v(bytes(32), [[b"a"], [b"ab"]], [b"x", b"y"])             # other lengths in the second record
    with pytest.raises(ValueError):
        uaes.siv_batch_v(bytes(32), [[b"a"]], [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.siv_batch_v(bytes(32), [[b"a"], [b"b"]], [b"x", b"y"], decrypt=True, ivs=[bytes(16)])


def test_planner_without_a_device():
    small = uaes.eax_siv_plan(True, 0)[3]
    lo, hi = 0, 1 << 26                                    # the one boundary of the single calls, found by bisection
    assert uaes.siv_v_plan(lo, 3)[0] == "s2v.small.v" and uaes.siv_v_plan(hi, 3)[0] == "s2v.long.v"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if uaes.siv_v_plan(mid, 3)[0] == "s2v.small.v" else (lo, mid)
    assert lo == small                                     # the same boundary as the one-aData calls
    rows = uaes.siv_v_plan(0, 1)[3]
    assert 1 <= rows <= 63                                 # rows of a 1024-thread workgroup, one wave's apart for the text
    for dec in (False, True):
        for nad in (0, 1, rows, rows + 1, AD_MAX):
            assert uaes.siv_v_plan(lo, nad, decrypt=dec) == ("s2v.small.v", 1, 1, rows)
            assert uaes.siv_v_plan(hi, nad, decrypt=dec) == ("s2v.long.v", 2, 1, rows)
        assert uaes.siv_v_plan(64, BATCH_AD_MAX, nmsg=4096, decrypt=dec)[:2] == ("s2v.batch.v", 1)
        assert uaes.siv_v_plan(64, 2, nmsg=4096, decrypt=dec)[3] == 1
    assert uaes.siv_v_plan(16, AD_MAX + 1) is None and uaes.siv_v_plan(16, BATCH_AD_MAX + 1, nmsg=2) is None
    assert uaes.siv_v_plan(16, BATCH_AD_MAX + 1, nmsg=1) is not None
    assert uaes.siv_v_plan(16, 1, decrypt=2) is None
    # the rows of the one-aData calls are what they were
    assert uaes.eax_siv_plan(True, small)[:2] == ("s2v.small", 1) and uaes.eax_siv_plan(True, small + 1)[:2] == ("s2v.long", 2)
