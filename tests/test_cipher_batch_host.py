"""The cipher batches (uaes_cbc_decrypt_batch, uaes_cbc_encrypt_blocks_batch, uaes_cbc_decrypt_blocks_batch,
uaes_cfb_encrypt_batch, uaes_cfb_decrypt_batch, uaes_ofb_xcrypt_batch, uaes_ctr_xcrypt_batch) without a device: the
cipher.batch row of csrc/uaes_plan.h, every argument the calls refuse with UAES_E_ARG before the device is touched, an
empty batch, and the declarations."""
import ctypes as C

import pytest

import micro_aes_amd as uaes
from tests.test_abi_and_host import declared_functions

E_ARG = -2                                      # UAES_E_ARG (include/uaes_hip.h)
FILL = 0x5C
CBC = ("uaes_cbc_decrypt_batch", "uaes_cbc_encrypt_blocks_batch", "uaes_cbc_decrypt_blocks_batch")
LENS = ("uaes_cfb_encrypt_batch", "uaes_cfb_decrypt_batch", "uaes_ofb_xcrypt_batch", "uaes_ctr_xcrypt_batch")
NAMES = set(CBC) | set(LENS) | {"uaes_debug_plan_cipher_batch"}


def test_the_plan_without_a_device():
    for mode in uaes.CIPHER_BATCH_MODES:
        for n in (1, 4, 5, 8192, 8193, 1 << 20):
            plan = uaes.cipher_batch_plan(n, mode, 64)
            assert plan[:2] == ("cipher.batch", 1), (mode, n, plan)
            assert plan[2:] == uaes.chain_plan("ccm_batch", 64, n)[2:], (mode, n, plan)       # every row batch's shape
        assert uaes.cipher_batch_plan(1 << 20, mode, 16) == ("cipher.batch", 1, 256, 1024)      # a 256-CU part without a device
        assert uaes.cipher_batch_plan(3, mode, 16) == ("cipher.batch", 1, 1, 256)
        assert uaes.cipher_batch_plan(0, mode, 16) == ("cipher.batch", 1, 1, 256)
        assert uaes.cipher_batch_plan(1 << 40, mode, 16)[:2] == ("cipher.batch", 1)              # no cap on the records
    assert uaes.cipher_batch_plan(8192, "ctr", 16)[3] == 256 and uaes.cipher_batch_plan(8193, "ctr", 16)[3] == 1024
    for mode in uaes.CIPHER_BATCH_MODES[:3]:                                                  # CBC: whole blocks, at least one
        assert [uaes.cipher_batch_plan(3, mode, n) is None for n in (0, 8, 16, 24, 32, 1 << 33)] == [True, True, False, True, False, False]
    for mode in uaes.CIPHER_BATCH_MODES[3:]:                                                  # the others: what 32 bits can say
        assert [uaes.cipher_batch_plan(3, mode, n) is None for n in (0, 1, 0xFFFFFFFF, 1 << 32)] == [False, False, False, True]
    hook = uaes.engine().uaes_debug_plan_cipher_batch
    assert hook(7, 16, 3, None) is None and hook(-1, 16, 3, None) is None
    assert hook(6, 16, 3, None) == b"cipher.batch"                                            # (out may be NULL)
    assert uaes.cipher_batch_plan(3) == uaes.cipher_batch_plan(3, 6, 16)


def call(name, bits=128, key=bytes(16), nmsg=2, msg_bytes=16, ivs=True, src=True, dst=True):
    """(the call's code, whether the output still is as it was); True = a buffer that is large enough, None = NULL"""
    small = nmsg * msg_bytes if nmsg * msg_bytes < 1 << 16 else 64                            # (a refused call reads nothing)
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))(*([FILL] * max(n, 1))) if on else None)      # noqa: E731
    o = buf(dst, small)
    a = (bits, key, buf(ivs, 16 * min(nmsg, 64)), nmsg, msg_bytes) + ((None,) if name in LENS else ()) + (buf(src, small), o)
    rc = getattr(uaes.engine(), name)(*a)
    return rc, o is None or set(bytes(o)) == {FILL}


REFUSED = [("NULL ivs", dict(ivs=None)), ("NULL input", dict(src=None)), ("NULL output", dict(dst=None)),
           ("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("far overflows", dict(nmsg=1 << 62, msg_bytes=1 << 20)),
           ("IVs overflow", dict(nmsg=(1 << 64) // 16, msg_bytes=16)), ("keybits", dict(bits=100)), ("NULL key", dict(key=None))]


@pytest.mark.parametrize("name", CBC + LENS)
@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_arguments(case, name):
    assert call(name, **case[1]) == (E_ARG, True), (case, name)
    assert uaes.engine().uaes_last_error()


@pytest.mark.parametrize("name", CBC)
@pytest.mark.parametrize("size", [0, 8, 24])
def test_cbc_takes_whole_blocks_only(name, size):
    assert call(name, msg_bytes=size) == (E_ARG, True)
    assert b"batched CBC: every message must be a whole number of blocks" in uaes.engine().uaes_last_error()
    assert call(name, msg_bytes=size, nmsg=0) == (E_ARG, True)                                # a bad size is one with no records, too


@pytest.mark.parametrize("name", LENS)
def test_record_sizes_of_the_lens_modes(name):
    assert call(name, msg_bytes=1 << 32) == (E_ARG, True)                                    # more than a 32-bit length can say
    assert call(name, msg_bytes=0) == (0, True)                                               # records of no bytes: nothing to do
    assert call(name, msg_bytes=0, src=None, dst=None) == (0, True)


@pytest.mark.parametrize("name", CBC + LENS)
def test_an_empty_batch(name):
    """no records: nothing to do, and nothing is looked at but the sizes and the key"""
    assert call(name, nmsg=0) == (0, True)
    assert call(name, nmsg=0, ivs=None, src=None, dst=None) == (0, True)
    assert call(name, nmsg=0, bits=100)[0] == E_ARG
    # a good call gets as far as the device: without one it fails there, not earlier
    import torch
    if not torch.cuda.is_available():
        assert call(name, nmsg=1)[0] == -1                                                    # UAES_E_HIP: no usable device


def test_declared_and_mirrored():
    assert NAMES <= set(declared_functions("uaes_hip.h"))
    assert NAMES <= set(uaes.EXPORTS)
    L = uaes.engine()
    for n in NAMES:
        assert getattr(L, n).argtypes is not None, n
    key = bytes(16)
    assert uaes.cbc_decrypt_batch(key, [], []) == [] and uaes.cbc_blocks_batch(key, [], []) == []
    assert uaes.cbc_blocks_batch(key, [], [], decrypt=True) == [] and uaes.cfb_batch(key, [], []) == []
    assert uaes.cfb_batch(key, [], [], decrypt=True) == [] and uaes.ofb_batch(key, [], []) == [] and uaes.ctr_batch(key, [], []) == []
    with pytest.raises(ValueError):
        uaes.cbc_decrypt_batch(key, [bytes(16)] * 2, [bytes(16), bytes(32)])                  # CBC: equal sizes
    with pytest.raises(ValueError):
        uaes.ctr_batch(key, [bytes(16)], [b"x", b"y"])                                        # one counter block per record
    with pytest.raises(ValueError):
        uaes.cfb_batch(key, [bytes(12)], [b"x"])                                              # of 16 bytes
