"""The OCB batches (uaes_ocb_encrypt_batch / uaes_ocb_decrypt_batch) without a device: the ocb.batch row of
csrc/uaes_plan.h, every argument the calls refuse with UAES_E_ARG before the device is touched, and the declarations."""
import ctypes as C

import pytest

import micro_aes_amd as uaes
from tests.test_abi_and_host import declared_functions

E_ARG = -2                                      # UAES_E_ARG (include/uaes_hip.h)
OCB_BATCH_MAX = 65535                           # UAES_OCB_BATCH_MAX (csrc/uaes_plan.h)
NAMES = {"uaes_ocb_encrypt_batch", "uaes_ocb_decrypt_batch", "uaes_debug_plan_ocb_batch"}


def test_the_plan_without_a_device():
    for n in (1, 4, 5, 8192, 8193, 1 << 20):
        for dec in (False, True):
            plan = uaes.ocb_batch_plan(64, n, decrypt=dec)
            assert plan[:2] == ("ocb.batch", 1), (n, dec, plan)
            assert plan[2:] == uaes.chain_plan("ccm_batch", 64, n)[2:], (n, dec, plan)
    assert uaes.ocb_batch_plan(64, 1 << 20) == ("ocb.batch", 1, 256, 1024)      # a 256-CU part without a device
    assert uaes.ocb_batch_plan(0, 3) == ("ocb.batch", 1, 1, 256)
    assert uaes.ocb_batch_plan(OCB_BATCH_MAX, 3)[0] == "ocb.batch"
    assert uaes.ocb_batch_plan(OCB_BATCH_MAX + 1, 3) is None and uaes.ocb_batch_plan(OCB_BATCH_MAX + 1, 3, decrypt=True) is None
    hook = uaes.engine().uaes_debug_plan_ocb_batch
    assert hook(2, 64, 3, None) is None and hook(-1, 64, 3, None) is None
    assert hook(1, 64, 3, None) == b"ocb.batch"                                  # (out may be NULL)


def calls(nonce_len=12, tag_len=16, nmsg=2, msg_bytes=16, lens=None, aad_bytes=3, bits=128, key=bytes(16), nonces=True,
          aad=True, src=True, dst=True, tags=True, verdicts=True):
    """(encrypt's code, decrypt's code) for one set of arguments; True = a buffer that is large enough, None = NULL"""
    L = uaes.engine()
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))() if on else None)             # noqa: E731
    small = nmsg if nmsg < 1 << 16 else 1                                        # (a refused call reads nothing)
    room = lambda n: small * (n if n <= OCB_BATCH_MAX else 64)                  # noqa: E731
    a = (bits, key, nonce_len, tag_len, nmsg, msg_bytes, lens, buf(nonces, small * 15), buf(aad, room(aad_bytes)),
         aad_bytes, buf(src, room(msg_bytes)))
    enc = L.uaes_ocb_encrypt_batch(*a, buf(dst, room(msg_bytes)), buf(tags, small * 16))
    dec = L.uaes_ocb_decrypt_batch(*a, buf(tags, small * 16), buf(dst, room(msg_bytes)), buf(verdicts, small))
    return enc, dec


REFUSED = [("nonce 0", dict(nonce_len=0)), ("nonce 16", dict(nonce_len=16)),
           ("tag 0", dict(tag_len=0)), ("tag 17", dict(tag_len=17)),
           ("record too long", dict(msg_bytes=OCB_BATCH_MAX + 1)), ("record far too long", dict(msg_bytes=1 << 40)),
           ("AAD too long", dict(aad_bytes=OCB_BATCH_MAX + 1)), ("AAD 1 << 33", dict(aad_bytes=1 << 33)),
           ("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("count overflows", dict(nmsg=(1 << 64) - 1, msg_bytes=0)),
           ("AAD overflows", dict(nmsg=1 << 50, msg_bytes=0, aad_bytes=0xFEFF)),
           ("keybits", dict(bits=100)), ("NULL key", dict(key=None)),
           ("NULL nonces", dict(nonces=None)), ("NULL AAD", dict(aad=None)), ("NULL input", dict(src=None)),
           ("NULL output", dict(dst=None)), ("NULL tags", dict(tags=None))]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_arguments(case):
    assert calls(**case[1]) == (E_ARG, E_ARG), case
    assert uaes.engine().uaes_last_error()


def test_null_verdicts_and_an_empty_batch():
    assert calls(verdicts=None)[1] == E_ARG
    assert uaes.engine().uaes_last_error()
    # no records: nothing to do, and nothing is looked at but the lengths and the key
    assert calls(nmsg=0) == (0, 0)
    assert calls(nmsg=0, nonces=None, aad=None, src=None, dst=None, tags=None, verdicts=None) == (0, 0)
    assert calls(nmsg=0, nonce_len=16) == (E_ARG, E_ARG) and calls(nmsg=0, msg_bytes=OCB_BATCH_MAX + 1) == (E_ARG, E_ARG)
    # the limits themselves are arguments like any other: without a device they get as far as the device
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(msg_bytes=OCB_BATCH_MAX), dict(aad_bytes=OCB_BATCH_MAX), dict(nonce_len=1, tag_len=1),
                   dict(nonce_len=15, tag_len=16), dict(msg_bytes=0, src=None, dst=None), dict(aad_bytes=0, aad=None)):
            assert calls(nmsg=1, **ok) == (-1, -1), ok                           # UAES_E_HIP: no usable device


def test_declared_and_mirrored():
    assert NAMES <= set(declared_functions("uaes_hip.h"))
    assert NAMES <= set(uaes.EXPORTS)
    assert uaes.ocb_batch(bytes(16), [], None, []) == ([], []) and uaes.ocb_batch(bytes(16), [], None, [], decrypt=True, tags=[]) == (0, [], [])
    with pytest.raises(ValueError):
        uaes.ocb_batch(bytes(16), [bytes(12)], None, [b"x", b"y"])
