"""The multi-key GCM batches (uaes_gcm_multikey_encrypt_batch / uaes_gcm_multikey_decrypt_batch) without a device: the
gcm.multikey row of csrc/uaes_plan.h, every argument the calls refuse with UAES_E_ARG before the device is touched, the
declarations, and a CPU model of the hash as k_gcm_multikey computes it (GHASH through POLYVAL on byte-reversed blocks
with the per-lane constants of uaes_perkey.hip.h), which pins the bit-order mapping before any GPU is involved."""
import ctypes as C
import random

import pytest

import micro_aes_amd as uaes
from tests.test_abi_and_host import declared_functions

E_ARG = -2                                      # UAES_E_ARG (include/uaes_hip.h)
BATCH_MAX = 65535                               # UAES_GCM_MULTIKEY_BATCH_MAX (csrc/uaes_plan.h)


def test_the_plan_without_a_device():
    assert uaes.gcm_multikey_batch_plan(64, 1 << 20) == ("gcm.multikey", 1, 256, 1024)  # a 256-CU part without a device
    for n in (1, 4, 5, 8192, 8193, 1 << 20):
        for dec in (False, True):
            plan = uaes.gcm_multikey_batch_plan(64, n, decrypt=dec)
            assert plan[:2] == ("gcm.multikey", 1), (n, dec, plan)
            assert plan[2:] == uaes.chain_plan("ccm_batch", 64, n, decrypt=dec)[2:], (n, dec, plan)
    assert uaes.gcm_multikey_batch_plan(0, 3) == ("gcm.multikey", 1, 1, 256)
    assert uaes.gcm_multikey_batch_plan(BATCH_MAX, 3)[0] == "gcm.multikey"
    assert uaes.gcm_multikey_batch_plan(BATCH_MAX + 1, 3) is None and uaes.gcm_multikey_batch_plan(1 << 40, 3) is None
    hook = uaes.engine().uaes_debug_plan_gcm_multikey_batch
    assert hook(2, 64, 3, None) is None and hook(-1, 64, 3, None) is None
    assert hook(1, 64, 3, None) == b"gcm.multikey"                               # (`out` may be NULL)


def calls(nmsg=2, msg_bytes=16, lens=None, aad_bytes=3, bits=128, tag_len=16, keys=True, nonces=True, aad=True, src=True,
          dst=True, tags=True, verdicts=True):
    """(encrypt's code, decrypt's code) for one set of arguments; True = a buffer that is large enough, None = NULL"""
    L = uaes.engine()
    buf = lambda on, n: ((C.c_uint8 * max(n, 1))() if on else None)             # noqa: E731
    small = nmsg if nmsg < 1 << 16 else 1                                        # (a refused call reads nothing)
    room = small * msg_bytes if msg_bytes <= BATCH_MAX else 1
    a = (bits, buf(keys, small * 32), tag_len, nmsg, msg_bytes, lens, buf(nonces, small * 12),
         buf(aad, small * aad_bytes if aad_bytes <= BATCH_MAX else 1), aad_bytes, buf(src, room))
    enc = L.uaes_gcm_multikey_encrypt_batch(*a, buf(dst, room), buf(tags, small * 16))
    dec = L.uaes_gcm_multikey_decrypt_batch(*a, buf(tags, small * 16), buf(dst, room), buf(verdicts, small))
    return enc, dec


REFUSED = [("keybits 0", dict(bits=0)), ("keybits 100", dict(bits=100)), ("keybits 512", dict(bits=512)),
           ("tagLen 0", dict(tag_len=0)), ("tagLen 17", dict(tag_len=17)),
           ("record too long", dict(msg_bytes=BATCH_MAX + 1)), ("record far too long", dict(msg_bytes=1 << 40)),
           ("AAD too long", dict(aad_bytes=BATCH_MAX + 1)), ("AAD far too long", dict(aad_bytes=1 << 33)),
           ("text overflows", dict(nmsg=(1 << 64) // 16, msg_bytes=32)), ("count overflows", dict(nmsg=(1 << 64) - 1, msg_bytes=0)),
           ("AAD overflows", dict(nmsg=1 << 50, msg_bytes=0, aad_bytes=BATCH_MAX)),
           ("keys overflow", dict(nmsg=(1 << 64) // 32, msg_bytes=0, aad_bytes=0, bits=256)),
           ("keys overflow at 128", dict(nmsg=(1 << 64) // 16, msg_bytes=0, aad_bytes=0, bits=128)),
           ("nonces overflow", dict(nmsg=(1 << 64) // 12 + 1, msg_bytes=0, aad_bytes=0)),
           ("NULL keys", dict(keys=None)), ("NULL nonces", dict(nonces=None)), ("NULL AAD", dict(aad=None)),
           ("NULL input", dict(src=None)), ("NULL output", dict(dst=None)), ("NULL tags", dict(tags=None))]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_arguments(case):
    assert calls(**case[1]) == (E_ARG, E_ARG), case
    assert uaes.engine().uaes_last_error()


def test_null_verdicts_and_an_empty_batch():
    assert calls(verdicts=None)[1] == E_ARG and uaes.engine().uaes_last_error()
    # no records: nothing to do, and nothing is looked at but the lengths and the key size
    assert calls(nmsg=0) == (0, 0)
    assert calls(nmsg=0, keys=None, nonces=None, aad=None, src=None, dst=None, tags=None, verdicts=None) == (0, 0)
    assert calls(nmsg=0, msg_bytes=BATCH_MAX + 1) == (E_ARG, E_ARG) and calls(nmsg=0, aad_bytes=BATCH_MAX + 1) == (E_ARG, E_ARG)
    assert calls(nmsg=0, bits=100) == (E_ARG, E_ARG) and calls(nmsg=0, tag_len=0) == (E_ARG, E_ARG)
    # the limits themselves are arguments like any other: without a device they get as far as the device
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(msg_bytes=BATCH_MAX), dict(aad_bytes=BATCH_MAX), dict(bits=192), dict(bits=256), dict(tag_len=1),
                   dict(tag_len=16), dict(msg_bytes=0, src=None, dst=None), dict(aad_bytes=0, aad=None)):
            assert calls(nmsg=1, **ok) == (-1, -1), ok                           # UAES_E_HIP: no usable device


def test_declared_and_mirrored():
    names = declared_functions("uaes_hip.h")
    new = {"uaes_gcm_multikey_encrypt_batch", "uaes_gcm_multikey_decrypt_batch", "uaes_debug_plan_gcm_multikey_batch"}
    assert new <= set(names) and new <= set(uaes.EXPORTS)
    assert uaes.gcm_multikey_batch([], [], None, []) == ([], [])
    assert uaes.gcm_multikey_batch([], [], None, [], decrypt=True, tags=[]) == (0, [], [])
    with pytest.raises(ValueError):
        uaes.gcm_multikey_batch([bytes(16)], [bytes(12)], None, [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.gcm_multikey_batch([bytes(16)], [bytes(12), bytes(12)], None, [b"x", b"y"])
    with pytest.raises(ValueError):
        uaes.gcm_multikey_batch([bytes(16)], [bytes(11)], None, [b"x"])


# ---- the hash as the kernel computes it -------------------------------------------------------------------------------
# POLYVAL's field: GF(2)[x] / P, a block read as a little-endian 128-bit integer (bit j = the coefficient of x^j)
P = (1 << 128) | (1 << 127) | (1 << 126) | (1 << 121) | 1


def mulx(a):
    a <<= 1
    return a ^ P if a >> 128 else a


def divx(a):
    """a x^-1 mod P: P's constant term is 1, so adding P clears bit 0"""
    return (a ^ P) >> 1 if a & 1 else a >> 1


def lane_constants(k):
    """kb[i][b] = K x^(8 i - 128 + b) for lane i = 0..15 and bit b = 0..7 (PvLane, pv_lane)"""
    kb = []
    for i in range(16):
        a = k
        for _ in range(128 - 8 * i):
            a = divx(a)
        row = [a]
        for _ in range(7):
            row.append(mulx(row[-1]))
        kb.append(row)
    return kb


def pv_step(s, x, kb):
    """(S ^ X) K x^-128: lane i takes byte i of S ^ X, and the sixteen partial products are XORed across the row"""
    a, acc = s ^ x, 0
    for i in range(16):
        byte = a >> (8 * i) & 0xff
        for b in range(8):
            if byte >> b & 1:
                acc ^= kb[i][b]
    return acc


def ghash_as_the_kernel(h, aad, ct):
    """GHASH_H = rev(POLYVAL_K(rev(X_1), ..)) with K = mulX(rev(H)): a reversed block as a little-endian integer is the
    block itself read big-endian; tails zero padded; the length block BE64(8 aad) || BE64(8 len)"""
    kb = lane_constants(mulx(int.from_bytes(h, "big")))
    s = 0
    for data in (aad, ct):
        for i in range(0, len(data), 16):
            s = pv_step(s, int.from_bytes(data[i:i + 16].ljust(16, b"\0"), "big"), kb)
    s = pv_step(s, int.from_bytes((8 * len(aad)).to_bytes(8, "big") + (8 * len(ct)).to_bytes(8, "big"), "big"), kb)
    return s.to_bytes(16, "big")


def test_the_hash_as_the_kernel_computes_it(orc):
    rng = random.Random(38)
    sizes = (0, 1, 15, 16, 17, 48)
    for al in sizes:
        for ml in sizes:
            h, aad, ct = rng.randbytes(16), rng.randbytes(al), rng.randbytes(ml)
            assert ghash_as_the_kernel(h, aad, ct) == orc.ghash(h, aad, ct), (h.hex(), al, ml)
    # the edges of the field: a hash key whose reversal has bit 127 set takes mulX's reduction
    for h in (bytes(15) + b"\x01", b"\x80" + bytes(15), b"\xff" * 16):
        aad, ct = rng.randbytes(17), rng.randbytes(33)
        assert ghash_as_the_kernel(h, aad, ct) == orc.ghash(h, aad, ct), h.hex()
