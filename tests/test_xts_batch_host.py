"""The XTS batches (uaes_xts_encrypt_batch, uaes_xts_decrypt_batch, uaes_xts_sector_list) without a device: the xts.batch
row of csrc/uaes_plan.h, every argument the calls refuse before the device is touched and the order they are refused
in, an empty batch, the declarations, the wrappers and the key schedules' wipe: every call made here, refused or accepted,
leaves the count of live key schedules where it was (call())."""
import ctypes as C

import pytest

import micro_aes_amd as uaes
from tests.test_abi_and_host import declared_functions

E_HIP, E_ARG, E_DATALENGTH = -1, -2, 1          # include/uaes_hip.h
FILL = 0x5C
BATCH = ("uaes_xts_encrypt_batch", "uaes_xts_decrypt_batch")
CALLS = BATCH + ("uaes_xts_sector_list",)
NAMES = set(CALLS) | {"uaes_debug_plan_xts_batch"}


def test_the_plan_without_a_device():
    for n in (1, 4, 5, 8192, 8193, 1 << 20, 1 << 40):
        plan = uaes.xts_batch_plan(n, 64)
        assert plan[:2] == ("xts.batch", 1), (n, plan)
        assert plan[2:] == uaes.chain_plan("ccm_batch", 64, n)[2:], (n, plan)                  # every row batch's shape
    assert uaes.xts_batch_plan(1 << 20, 16) == ("xts.batch", 1, 256, 1024)                      # a 256-CU part without a device
    assert uaes.xts_batch_plan(3) == ("xts.batch", 1, 1, 256) == uaes.xts_batch_plan(0)
    assert uaes.xts_batch_plan(8192)[3] == 256 and uaes.xts_batch_plan(8193)[3] == 1024
    assert [uaes.xts_batch_plan(3, n) is None for n in (0, 1, 15, 16, 17, 520, 0xFFFFFFFF, 1 << 32)] == \
        [True, True, True, False, False, False, False, True]
    hook = uaes.engine().uaes_debug_plan_xts_batch
    assert hook(15, 3, None) is None and hook(1 << 32, 3, None) is None
    assert hook(16, 3, None) == b"xts.batch"                                                   # (out may be NULL)
    out = (C.c_int * 4)()
    assert hook(33, 8193, out) == b"xts.batch" and list(out) == [1, 129, 1024, 64]


LIVE = uaes.engine().uaes_debug_live_key_schedules          # the calls leave it where it was: 0 in a process of its own


def call(name, bits=128, keys=bytes(32), nmsg=2, msg_bytes=16, tweaks=True, src=True, dst=True):
    """(the call's code, whether the output still is as it was); True = a buffer that is large enough, None = NULL"""
    small = nmsg * msg_bytes if nmsg * msg_bytes < 1 << 16 else 64                            # (a refused call reads nothing)
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))(*([FILL] * max(n, 1))) if on else None)      # noqa: E731
    o = buf(dst, small)
    if keys is not None and bits in (192, 256):
        keys = bytes(bits // 4)
    if name in BATCH:
        a = (bits, keys, buf(tweaks, 16 * min(nmsg, 64)), nmsg, msg_bytes, None, buf(src, small), o)
    else:
        a = (bits, keys, buf(tweaks, 8 * min(nmsg, 64)), nmsg, msg_bytes, buf(src, small), o, 1)
    live = LIVE()
    rc = getattr(uaes.engine(), name)(*a)
    assert LIVE() == live, (name, "left %d key schedule(s) behind" % (LIVE() - live))
    return rc, o is None or set(bytes(o)) == {FILL}


REFUSED = [("NULL tweaks", dict(tweaks=None)), ("NULL input", dict(src=None)), ("NULL output", dict(dst=None)),
           ("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("far overflows", dict(nmsg=1 << 62, msg_bytes=1 << 20)),
           ("tweaks overflow", dict(nmsg=(1 << 64) // 16, msg_bytes=16)), ("unit above 32 bits", dict(msg_bytes=1 << 32)),
           ("keybits", dict(bits=100)), ("NULL key", dict(keys=None))]


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_arguments(case, name):
    assert call(name, **case[1]) == (E_ARG, True), (case, name)
    assert uaes.engine().uaes_last_error()


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("size", [0, 1, 15])
def test_a_unit_below_one_block(name, size):
    assert call(name, msg_bytes=size) == (E_DATALENGTH, True), (name, size)
    assert call(name, msg_bytes=size, tweaks=None, src=None, dst=None) == (E_DATALENGTH, True)   # before the pointers
    assert call(name, msg_bytes=size, bits=100) == (E_ARG, True)                                  # after the key
    assert call(name, msg_bytes=size, nmsg=0) == (0, True)                                        # after "no units"


@pytest.mark.parametrize("name", CALLS)
def test_the_order_of_the_refusals(name):
    assert call(name, msg_bytes=1 << 32, bits=100, nmsg=0)[0] == E_ARG                            # the sizes come first
    assert call(name, msg_bytes=1 << 32, nmsg=0)[0] == E_ARG
    assert call(name, nmsg=(1 << 64) // 16, msg_bytes=8, tweaks=None) == (E_ARG, True)             # overflow before the length


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_an_empty_batch(name, bits):
    """no units: nothing to do, and nothing is looked at but the sizes and the key"""
    assert call(name, bits=bits, nmsg=0) == (0, True)
    assert call(name, bits=bits, nmsg=0, tweaks=None, src=None, dst=None) == (0, True)
    assert call(name, nmsg=0, bits=100)[0] == E_ARG
    assert call(name, nmsg=0, keys=None)[0] == E_ARG
    # a good call gets as far as the device: without one it fails there, not earlier
    import torch
    if not torch.cuda.is_available():
        assert call(name, bits=bits, nmsg=1)[0] == E_HIP                                       # no usable device
        assert call(name, bits=bits, nmsg=3, msg_bytes=33)[0] == E_HIP


def test_declared_and_mirrored():
    assert NAMES <= set(declared_functions("uaes_hip.h"))
    assert NAMES <= set(uaes.EXPORTS)
    L = uaes.engine()
    for n in NAMES:
        assert getattr(L, n).argtypes is not None, n
    keys = bytes(32)
    assert uaes.xts_batch(keys, [], []) == (0, []) and uaes.xts_batch(keys, [], [], decrypt=True) == (0, [])
    assert uaes.xts_sector_list(keys, [], 512, b"") == (0, b"")
    with pytest.raises(ValueError):
        uaes.xts_batch(keys, [bytes(16)], [bytes(16), bytes(32)])                               # one tweak per unit
    with pytest.raises(ValueError):
        uaes.xts_batch(keys, [bytes(12)], [bytes(16)])                                          # of 16 bytes
    with pytest.raises(ValueError):
        uaes.xts_batch(keys, [bytes(16), bytes(17)], [bytes(16), bytes(16)])
    with pytest.raises(ValueError):
        uaes.xts_batch(bytes(33), [bytes(16)], [bytes(16)])                                     # key1 || key2
    with pytest.raises(ValueError):
        uaes.xts_sector_list(keys, [1, 2], 512, bytes(512))                                     # a unit per sector
