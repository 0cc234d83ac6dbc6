"""XAES-256-GCM (C2SP; uaes_xaes256gcm_*) without a device: the reference composition against the specification's
vectors and accumulated test, the host-only key derivation (both branches of CMAC's doubling), the declarations, every
argument the calls refuse before a device is touched, the xaes.gcm row of csrc/uaes_plan.h, the one-message calls on the
engine's host data path (all 10 000 iterations of the accumulated test), and that no call leaves a key schedule behind."""
import ctypes as C

import pytest

import micro_aes_amd as uaes
from tests import key_wipe_cases as kw
from tests import xaes_ref
from tests.test_abi_and_host import declared_functions

E_ARG, AUTH = -2, 0x1A                          # UAES_E_ARG, UAES_E_AUTHENTICATION (include/uaes_hip.h)
BATCH_MAX = 65535                               # UAES_XAES_GCM_BATCH_MAX (csrc/uaes_plan.h)
NAMES = ["uaes_xaes256gcm_derive", "uaes_xaes256gcm_encrypt", "uaes_xaes256gcm_decrypt", "uaes_xaes256gcm_encrypt_batch",
         "uaes_xaes256gcm_decrypt_batch", "uaes_debug_plan_xaes256gcm_batch"]
KEY, NONCE = bytes(range(1, 33)), bytes(range(0x40, 0x58))


@pytest.fixture()
def host_path():
    prev = uaes.host_policy(1 << 62, 1, 1)
    yield
    uaes.host_policy(*prev)


def test_the_reference_reproduces_the_specification():
    for v in xaes_ref.vectors():
        assert xaes_ref.derive(v["key"], v["nonce"]) == v["kx"] == xaes_ref.derive_by_cmac(v["key"], v["nonce"])
        assert xaes_ref.encrypt(v["key"], v["nonce"], v["aad"], v["plaintext"]) == v["output"]
        assert xaes_ref.decrypt(v["key"], v["nonce"], v["aad"], v["output"]) == (0, v["plaintext"])
    outs = (xaes_ref.encrypt(k, n, a, p) for k, n, p, a in xaes_ref.accumulated())      # (consumes exactly stream_bytes)
    assert xaes_ref.accumulated_digest(outs) == xaes_ref.golden()["accumulated"]["digest"]
    xaes_ref.check_vectors_through_the_reference()                                      # where oracle/_ref is present


def test_derive():
    for v in xaes_ref.vectors():
        assert uaes.xaes256gcm_derive(v["key"], v["nonce"]) == v["kx"]
    top_set, top_clear = xaes_ref.keys_by_top_bit_of_l()
    assert xaes_ref.big_l(top_set)[0] >> 7 == 1 and xaes_ref.big_l(top_clear)[0] >> 7 == 0
    for key in (top_set, top_clear):                                                    # the 0x87 branch of the doubling, and the other
        for nonce in (NONCE, bytes(24), b"\xff" * 24):
            assert uaes.xaes256gcm_derive(key, nonce) == xaes_ref.derive(key, nonce), (key.hex(), nonce.hex())
    # only the first half of the nonce makes the key
    assert uaes.xaes256gcm_derive(KEY, NONCE) == uaes.xaes256gcm_derive(KEY, NONCE[:12] + bytes(12))
    assert uaes.xaes256gcm_derive(KEY, NONCE) != uaes.xaes256gcm_derive(KEY, xaes_ref.flip(NONCE, 95))
    for bad in ((KEY[:31], NONCE), (KEY, NONCE[:23]), (KEY + b"x", NONCE)):
        with pytest.raises(ValueError):
            uaes.xaes256gcm_derive(*bad)


def test_declared_and_mirrored():
    names = declared_functions("uaes_hip.h")
    L = uaes.engine()
    for n in NAMES:
        assert n in names and n in uaes.EXPORTS and getattr(L, n), n
    assert not [n for n in kw.keyed_exports() if "xaes" in n]                           # one key size: no keybits argument
    assert uaes.xaes256gcm_batch(KEY, [], None, []) == ([], [])
    assert uaes.xaes256gcm_batch(KEY, [], None, [], decrypt=True, tags=[]) == (0, [], [])
    with pytest.raises(ValueError):
        uaes.xaes256gcm_batch(KEY, [bytes(24)], None, [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.xaes256gcm_batch(KEY, [bytes(12)], None, [b"x"])
    with pytest.raises(ValueError):
        uaes.xaes256gcm_batch(KEY[:16], [bytes(24)], None, [b"x"])


def batch_calls(nmsg=2, msg_bytes=16, lens=None, aad_bytes=3, key=KEY, nonces=True, aad=True, src=True, dst=True, tags=True,
                verdicts=True):
    """(encrypt's code, decrypt's code) for one set of arguments; True = a buffer that is large enough, None = NULL"""
    L = uaes.engine()
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))() if on else None)             # noqa: E731
    small = nmsg if nmsg < 1 << 16 else 1                                        # (a refused call reads nothing)
    room = small * msg_bytes if msg_bytes <= BATCH_MAX else 1
    a = (key, nmsg, msg_bytes, lens, buf(nonces, small * 24), buf(aad, small * aad_bytes if aad_bytes <= BATCH_MAX else 1),
         aad_bytes, buf(src, room))
    enc = L.uaes_xaes256gcm_encrypt_batch(*a, buf(dst, room), buf(tags, small * 16))
    dec = L.uaes_xaes256gcm_decrypt_batch(*a, buf(tags, small * 16), buf(dst, room), buf(verdicts, small))
    return enc, dec


REFUSED = [("record too long", dict(msg_bytes=BATCH_MAX + 1)), ("record far too long", dict(msg_bytes=1 << 40)),
           ("AAD too long", dict(aad_bytes=BATCH_MAX + 1)), ("AAD far too long", dict(aad_bytes=1 << 33)),
           ("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("count overflows", dict(nmsg=(1 << 64) - 1, msg_bytes=0)),
           ("nonces overflow", dict(nmsg=(1 << 64) // 24 + 1, msg_bytes=0, aad_bytes=0)),
           ("NULL key", dict(key=None)), ("NULL nonces", dict(nonces=None)), ("NULL AAD", dict(aad=None)),
           ("NULL input", dict(src=None)), ("NULL output", dict(dst=None)), ("NULL tags", dict(tags=None))]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_batches(case):
    assert batch_calls(**case[1]) == (E_ARG, E_ARG), case
    assert uaes.engine().uaes_last_error()


def test_refused_single_calls():
    L = uaes.engine()
    B = (C.c_uint8 * 64)()
    for fn in (L.uaes_xaes256gcm_encrypt, L.uaes_xaes256gcm_decrypt):
        assert fn(None, NONCE, None, 0, B, 16, B) == E_ARG                              # key
        assert fn(KEY, None, None, 0, B, 16, B) == E_ARG                                # nonce
        assert fn(KEY, NONCE, None, 0, None, 16, B) == E_ARG                            # input
        assert fn(KEY, NONCE, None, 0, B, 16, None) == E_ARG                            # output
        assert fn(KEY, NONCE, None, 3, B, 16, B) == E_ARG                               # AAD
    assert L.uaes_xaes256gcm_derive(None, NONCE, B) == E_ARG and L.uaes_xaes256gcm_derive(KEY, None, B) == E_ARG
    assert L.uaes_xaes256gcm_derive(KEY, NONCE, None) == E_ARG


def test_null_verdicts_an_empty_batch_and_lens_without_text():
    import torch
    no_device = not torch.cuda.is_available()
    # no records: nothing to do, and nothing is looked at but the lengths and the key
    assert batch_calls(nmsg=0) == (0, 0)
    assert batch_calls(nmsg=0, nonces=None, aad=None, src=None, dst=None, tags=None, verdicts=None) == (0, 0)
    assert batch_calls(nmsg=0, msg_bytes=BATCH_MAX + 1) == (E_ARG, E_ARG) and batch_calls(nmsg=0, aad_bytes=BATCH_MAX + 1) == (E_ARG, E_ARG)
    if no_device:
        # accepted arguments get as far as the device (UAES_E_HIP: no usable device) -- NULL verdicts among them, the limits
        # themselves, and lens with records of no bytes, which no AEAD batch refuses: the GCM-SIV batch answers the same
        for ok in (dict(verdicts=None), dict(msg_bytes=BATCH_MAX), dict(aad_bytes=BATCH_MAX), dict(msg_bytes=0, src=None, dst=None),
                   dict(aad_bytes=0, aad=None), dict(msg_bytes=0, lens=(C.c_uint32 * 2)(0, 0))):
            assert batch_calls(**ok) == (-1, -1), ok
        L, lens, B = uaes.engine(), (C.c_uint32 * 2)(0, 0), (C.c_uint8 * 64)()
        assert L.uaes_gcmsiv_encrypt_batch(256, KEY, 2, 0, lens, B, None, 0, None, None, B) == -1


def test_the_plan_without_a_device():
    assert uaes.xaes256gcm_batch_plan(64, 1 << 20) == ("xaes.gcm", 1, 256, 1024)        # a 256-CU part without a device
    for length in (0, 64, BATCH_MAX):
        for n in (1, 4, 5, 64, 65, 8192, 8193, 1 << 20):
            for dec in (False, True):
                plan = uaes.xaes256gcm_batch_plan(length, n, decrypt=dec)
                assert plan[:2] == ("xaes.gcm", 1), (length, n, dec, plan)
                assert plan[2:] == uaes.gcmsiv_batch_plan(length, n, decrypt=dec)[2:], (length, n, dec, plan)
    assert uaes.xaes256gcm_batch_plan(BATCH_MAX + 1, 3) is None and uaes.xaes256gcm_batch_plan(1 << 40, 3) is None
    hook = uaes.engine().uaes_debug_plan_xaes256gcm_batch
    assert hook(2, 64, 3, None) is None and hook(-1, 64, 3, None) is None
    assert hook(1, 64, 3, None) == b"xaes.gcm"                                          # (`out` may be NULL)


def test_vectors_on_the_host_path(host_path):
    for v in xaes_ref.vectors():
        assert uaes.xaes256gcm_encrypt(v["key"], v["nonce"], v["aad"], v["plaintext"]) == v["output"]
        assert uaes.xaes256gcm_decrypt(v["key"], v["nonce"], v["aad"], v["output"]) == (0, v["plaintext"])
        forged = xaes_ref.flip(v["output"], 8 * len(v["output"]) - 3)                   # a bit of the tag
        assert uaes.xaes256gcm_decrypt(v["key"], v["nonce"], v["aad"], forged, prefill=0xAB) == (AUTH, b"\xab" * len(v["plaintext"]))
        assert uaes.xaes256gcm_decrypt(v["key"], xaes_ref.flip(v["nonce"], 40), v["aad"], v["output"])[0] == AUTH
        assert uaes.xaes256gcm_decrypt(v["key"], xaes_ref.flip(v["nonce"], 140), v["aad"], v["output"])[0] == AUTH


def test_the_accumulated_test_on_the_host_path(host_path):
    outs = []
    for i, (key, nonce, pt, aad) in enumerate(xaes_ref.accumulated()):
        outs.append(uaes.xaes256gcm_encrypt(key, nonce, aad, pt))
        if i < 200:
            assert uaes.xaes256gcm_decrypt(key, nonce, aad, outs[-1]) == (0, pt), i
    assert len(outs) == xaes_ref.golden()["accumulated"]["iterations"] == 10000
    assert xaes_ref.accumulated_digest(outs) == xaes_ref.golden()["accumulated"]["digest"]


def test_no_call_leaves_a_key_schedule_behind(host_path):
    B = kw.buf()
    kw.checked("uaes_xaes256gcm_derive", (KEY, NONCE, B), kw.OK)
    kw.checked("uaes_xaes256gcm_derive", (KEY, NONCE, None), kw.ARG)
    for name in ("uaes_xaes256gcm_encrypt", "uaes_xaes256gcm_decrypt"):                  # refused behind the derivation
        kw.checked(name, (KEY, NONCE, None, 0, None, 16, B), kw.ARG)
        kw.checked(name, (KEY, None, None, 0, B, 16, B), kw.ARG)
    # a refused batch: the size (before the key), and a missing input (behind the key's expansion)
    kw.checked("uaes_xaes256gcm_encrypt_batch", (KEY, 1, BATCH_MAX + 1, None, NONCE, None, 0, B, B, B), kw.ARG)
    kw.checked("uaes_xaes256gcm_encrypt_batch", (KEY, 1, 16, None, NONCE, None, 0, None, B, B), kw.ARG)
    kw.checked("uaes_xaes256gcm_decrypt_batch", (KEY, 1, 16, None, NONCE, None, 0, None, B, B, B), kw.ARG)
    kw.checked("uaes_xaes256gcm_encrypt_batch", (KEY, 0, 16, None, None, None, 0, None, None, None), kw.OK)
    for n in (16, 17):
        pt, ct, out = kw.text(n), kw.buf(n + 16), kw.buf(n + 16)
        kw.checked("uaes_xaes256gcm_encrypt", (KEY, NONCE, b"hdr", 3, pt, n, ct), kw.OK)
        assert bytes(ct)[:n + 16] == xaes_ref.encrypt(KEY, NONCE, b"hdr", pt)
        kw.checked("uaes_xaes256gcm_decrypt", (KEY, NONCE, b"hdr", 3, ct, n, out), kw.OK)
        assert bytes(out)[:n] == pt
        ct[n + 15] ^= 1
        kw.checked("uaes_xaes256gcm_decrypt", (KEY, NONCE, b"hdr", 3, ct, n, out), kw.AUTH)
