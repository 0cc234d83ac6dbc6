"""The EAX and SIV batches (uaes_eax_encrypt_batch / uaes_eax_decrypt_batch, uaes_siv_encrypt_batch /
uaes_siv_decrypt_batch) without a device: every argument the calls refuse with UAES_E_ARG before the device is touched,
and the declarations.  (Their plan rows: tests/test_eax_siv_host.py.)"""
import ctypes as C

import pytest

import micro_aes_amd as uaes
from tests.test_abi_and_host import declared_functions

E_ARG = -2                                      # UAES_E_ARG (include/uaes_hip.h)
NAMES = {"uaes_eax_encrypt_batch", "uaes_eax_decrypt_batch", "uaes_siv_encrypt_batch", "uaes_siv_decrypt_batch"}


def calls(siv, nmsg=2, msg_bytes=16, nonce_len=12, aad_bytes=3, bits=128, key=bytes(64), nonces=True, aad=True, src=True,
          dst=True, tags=True, verdicts=True):
    """(encrypt's code, decrypt's code) for one set of arguments; True = a buffer that is large enough, None = NULL.
    SIV takes a pair of keys of `bits` each, no nonces, and its IVs where EAX has its tags."""
    L = uaes.engine()
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))() if on else None)             # noqa: E731
    small = nmsg if nmsg < 1 << 16 else 1                                        # (a refused call reads nothing)
    head = (bits, key, nmsg, msg_bytes)
    a = (buf(aad, small * min(aad_bytes, 64)), aad_bytes)
    text = lambda on: buf(on, small * min(msg_bytes, 64))                        # noqa: E731
    if siv:
        enc = L.uaes_siv_encrypt_batch(*head, *a, text(src), buf(tags, small * 16), text(dst))
        dec = L.uaes_siv_decrypt_batch(*head, *a, buf(tags, small * 16), text(src), text(dst), buf(verdicts, small))
    else:
        n = (buf(nonces, small * min(nonce_len, 64)), nonce_len)
        enc = L.uaes_eax_encrypt_batch(*head, *n, *a, text(src), text(dst), buf(tags, small * 16))
        dec = L.uaes_eax_decrypt_batch(*head, *n, *a, text(src), buf(tags, small * 16), text(dst), buf(verdicts, small))
    return enc, dec


REFUSED = [("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("count overflows", dict(nmsg=(1 << 64) - 1, msg_bytes=0)),
           ("AAD overflows", dict(nmsg=1 << 50, msg_bytes=0, aad_bytes=0xFEFF)),
           ("keybits 100", dict(bits=100)), ("keybits 0", dict(bits=0)), ("NULL key", dict(key=None)),
           ("NULL AAD", dict(aad=None)), ("NULL input", dict(src=None)), ("NULL output", dict(dst=None)),
           ("NULL tags or IVs", dict(tags=None))]
MODES = [False, True]
MODE_IDS = ["eax", "siv"]


@pytest.mark.parametrize("siv", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_arguments(case, siv):
    assert calls(siv, **case[1]) == (E_ARG, E_ARG), case
    assert uaes.engine().uaes_last_error()


def test_eax_nonces():
    assert calls(False, nonces=None) == (E_ARG, E_ARG)
    assert uaes.engine().uaes_last_error()
    assert calls(False, nmsg=(1 << 64) // 8, msg_bytes=0, aad_bytes=0, nonce_len=16) == (E_ARG, E_ARG)     # the nonces overflow


@pytest.mark.parametrize("siv", MODES, ids=MODE_IDS)
def test_null_verdicts_and_an_empty_batch(siv):
    assert calls(siv, verdicts=None)[1] == E_ARG
    assert uaes.engine().uaes_last_error()
    # no records: nothing to do, and nothing is looked at but the lengths and the key
    assert calls(siv, nmsg=0) == (0, 0)
    assert calls(siv, nmsg=0, nonces=None, aad=None, src=None, dst=None, tags=None, verdicts=None) == (0, 0)
    assert calls(siv, nmsg=0, bits=100) == (E_ARG, E_ARG) and calls(siv, nmsg=0, key=None) == (E_ARG, E_ARG)
    # without a device a well-formed call gets as far as the device
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(), dict(bits=192), dict(bits=256), dict(msg_bytes=0, src=None, dst=None),
                   dict(aad_bytes=0, aad=None), dict(nonce_len=0, nonces=None), dict(nonce_len=1), dict(nonce_len=64)):
            assert calls(siv, nmsg=1, **ok) == (-1, -1), ok                      # UAES_E_HIP: no usable device


def test_declared_and_mirrored():
    assert NAMES <= set(declared_functions("uaes_hip.h"))
    assert NAMES <= set(uaes.EXPORTS)
    assert uaes.eax_batch(bytes(16), [], None, []) == ([], []) and uaes.eax_batch(bytes(16), [], None, [], decrypt=True, tags=[]) == (0, [], [])
    assert uaes.siv_batch(bytes(32), None, []) == ([], []) and uaes.siv_batch(bytes(32), None, [], decrypt=True, ivs=[]) == (0, [], [])
    with pytest.raises(ValueError):
        uaes.eax_batch(bytes(16), [bytes(12)], None, [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.siv_batch(bytes(32), [b"a"], [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.siv_batch(bytes(32), None, [b"x", b"y"], decrypt=True, ivs=[bytes(16)])
