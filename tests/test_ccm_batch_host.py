"""The CCM batches (uaes_ccm_encrypt_batch / uaes_ccm_decrypt_batch) without a device: the ccm.batch row of
csrc/uaes_plan.h, every argument the calls refuse with UAES_E_ARG before the device is touched, and the declarations."""
import ctypes as C

import pytest

import micro_aes_amd as uaes
from tests.test_abi_and_host import declared_functions

E_ARG = -2                                      # UAES_E_ARG (include/uaes_hip.h)
CCM_BATCH_MAX = 65535                           # UAES_CCM_BATCH_MAX (csrc/uaes_plan.h)


def test_the_plan_without_a_device():
    for n in (1, 4, 5, 8192, 8193, 1 << 20):
        for dec in (False, True):
            plan = uaes.chain_plan("ccm_batch", 64, n, decrypt=dec)
            assert plan[:2] == ("ccm.batch", 1), (n, dec, plan)
            row = uaes.chain_plan("cbc_batch", 64, n)
            if row[0] == "batch.row":
                assert plan[2:] == row[2:], (n, dec, plan, row)
    assert uaes.chain_plan("cbc_batch", 64, 8193)[0] == "batch.row"             # (so the comparison above was made)
    assert uaes.chain_plan("ccm_batch", 64, 1 << 20) == ("ccm.batch", 1, 256, 1024)     # a 256-CU part without a device
    assert uaes.chain_plan("ccm_batch", 0, 3) == ("ccm.batch", 1, 1, 256)
    assert uaes.chain_plan("ccm_batch", CCM_BATCH_MAX, 3)[0] == "ccm.batch"
    hook = uaes.engine().uaes_debug_plan_chain
    what = uaes.CHAIN_WHAT["ccm_batch"]
    assert hook(what, 0, CCM_BATCH_MAX + 1, 3, None) is None and hook(what, 2, 64, 3, None) is None


def calls(nonce_len=13, tag_len=8, nmsg=2, msg_bytes=16, lens=None, aad_bytes=3, bits=128, key=bytes(16), nonces=True,
          aad=True, src=True, dst=True, tags=True, verdicts=True):
    """(encrypt's code, decrypt's code) for one set of arguments; True = a buffer that is large enough, None = NULL"""
    L = uaes.engine()
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))() if on else None)             # noqa: E731
    small = nmsg if nmsg < 1 << 16 else 1                                        # (a refused call reads nothing)
    a = (bits, key, nonce_len, tag_len, nmsg, msg_bytes, lens, buf(nonces, small * 13), buf(aad, small * min(aad_bytes, 64)),
         aad_bytes, buf(src, small * min(msg_bytes, 64)))
    enc = L.uaes_ccm_encrypt_batch(*a, buf(dst, small * min(msg_bytes, 64)), buf(tags, small * 16))
    dec = L.uaes_ccm_decrypt_batch(*a, buf(tags, small * 16), buf(dst, small * min(msg_bytes, 64)), buf(verdicts, small))
    return enc, dec


REFUSED = [("nonce 6", dict(nonce_len=6)), ("nonce 14", dict(nonce_len=14)), ("nonce 0", dict(nonce_len=0)),
           ("tag 2", dict(tag_len=2)), ("tag 5", dict(tag_len=5)), ("tag 15", dict(tag_len=15)), ("tag 18", dict(tag_len=18)),
           ("tag 0", dict(tag_len=0)),
           ("record too long", dict(msg_bytes=CCM_BATCH_MAX + 1)), ("record far too long", dict(msg_bytes=1 << 40)),
           ("AAD 0xFF00", dict(aad_bytes=0xFF00)), ("AAD 1 << 33", dict(aad_bytes=1 << 33)),
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
    # no records: nothing to do, and nothing is looked at but the lengths and the key
    assert calls(nmsg=0) == (0, 0)
    assert calls(nmsg=0, nonces=None, aad=None, src=None, dst=None, tags=None, verdicts=None) == (0, 0)
    assert calls(nmsg=0, nonce_len=14) == (E_ARG, E_ARG) and calls(nmsg=0, msg_bytes=CCM_BATCH_MAX + 1) == (E_ARG, E_ARG)
    # the limits themselves are arguments like any other: without a device they get as far as the device
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(msg_bytes=CCM_BATCH_MAX), dict(aad_bytes=0xFEFF), dict(nonce_len=7, tag_len=4), dict(nonce_len=13, tag_len=16),
                   dict(msg_bytes=0, src=None, dst=None), dict(aad_bytes=0, aad=None)):
            assert calls(nmsg=1, **ok) == (-1, -1), ok                           # UAES_E_HIP: no usable device


def test_declared_and_mirrored():
    names = declared_functions("uaes_hip.h")
    assert "uaes_ccm_encrypt_batch" in names and "uaes_ccm_decrypt_batch" in names
    assert {"uaes_ccm_encrypt_batch", "uaes_ccm_decrypt_batch"} <= set(uaes.EXPORTS)
    assert uaes.ccm_batch(bytes(16), [], None, []) == ([], []) and uaes.ccm_batch(bytes(16), [], None, [], decrypt=True, tags=[]) == (0, [], [])
    with pytest.raises(ValueError):
        uaes.ccm_batch(bytes(16), [bytes(13)], None, [b"x", b"y"])
