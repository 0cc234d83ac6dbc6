"""The key-wipe cases of EAX' (uaes_eaxp_encrypt, uaes_eaxp_decrypt, uaes_eaxp_encrypt_batch, uaes_eaxp_decrypt_batch),
for the suites that demand one of every keyed export.

As tests/test_key_wipe_cases_xts.py does for the XTS batches: tests/test_key_wipe_host.py and tests/test_gpu_key_wipe.py
read include/uaes_hip.h and fail for a keyed export that tests/key_wipe_cases.py (ARG_CASES, TEXT_CASES) or
test_gpu_key_wipe._batches has no call for.  This module adds the four calls to those lists when it is imported, and it
is named to be collected before tests/test_key_wipe_host.py, which parametrises over the lists as it is imported; folding
them into key_wipe_cases.py and _batches, where they belong, is a change to those files.

So that nothing depends on that order, the same calls are also tests of this module."""
import pytest

import micro_aes_amd as uaes
from tests import key_wipe_cases as K
from tests import test_gpu_key_wipe as G
from tests.key_wipe_cases import ARG, AUTH, B, KEY, N16, OK, HostMem, buf, checked, text

EAXP_ARG_CASES = {
    "uaes_eaxp_encrypt": ((128, KEY, None, 16, B, 16, B), ARG),                                 # no nonce
    "uaes_eaxp_decrypt": ((128, KEY, None, 16, B, 16, B), ARG),
    "uaes_eaxp_encrypt_batch": ((128, KEY, 1, 16, None, N16, 16, None, None, B, B), ARG),       # no input
    "uaes_eaxp_decrypt_batch": ((128, KEY, 1, 16, None, N16, 16, None, None, B, B, B), ARG),
}


def eaxp_text_case(n, mem):
    ct, out = mem.out(n + 4), mem.out(n + 4)
    yield "uaes_eaxp_encrypt", (128, KEY, N16, 16, mem.inp(text(n)), n, ct), OK
    yield "uaes_eaxp_decrypt", (128, KEY, N16, 16, ct, n, out), OK
    yield "uaes_eaxp_decrypt", (128, KEY, N16, 15, ct, n, out), AUTH                            # a shorter nonce


def eaxp_batches():
    """three records of 32 bytes, host arrays, as test_gpu_key_wipe._batches has them for EAX"""
    n, m = 3, 32
    pt, ct, out, macs, ver, nonces = text(n * m), buf(n * m), buf(n * m), buf(n * 4), buf(n), text(n * 16)
    yield "uaes_eaxp_encrypt_batch", (128, KEY, n, 16, None, nonces, m, None, pt, ct, macs), OK
    yield "uaes_eaxp_decrypt_batch", (128, KEY, n, 16, None, nonces, m, None, ct, macs, out, ver), OK
    macs[0] ^= 1
    yield "uaes_eaxp_decrypt_batch", (128, KEY, n, 16, None, nonces, m, None, ct, macs, out, ver), AUTH


# ---- the registration (once, whatever imports this module first)
if "uaes_eaxp_encrypt" not in K.ARG_CASES:
    K.ARG_CASES.update(EAXP_ARG_CASES)
    K.TEXT_CASES.append(eaxp_text_case)
    _batches_before = G._batches

    def _batches_with_eaxp():
        yield from _batches_before()
        yield from eaxp_batches()

    G._batches = _batches_with_eaxp


# ---- the same calls as tests of this module
def test_the_lists_hold_the_eaxp_calls():
    names = {n for n in K.keyed_exports() if n.startswith("uaes_eaxp_")}
    assert names == set(EAXP_ARG_CASES) and names <= set(K.ARG_CASES) and eaxp_text_case in K.TEXT_CASES
    assert {name for name, _, _ in eaxp_batches()} == {n for n in names if n.endswith("_batch")}


@pytest.mark.parametrize("name", sorted(EAXP_ARG_CASES))
def test_argument_error_behind_the_key_expansion_leaves_no_schedule(name):
    args, want = EAXP_ARG_CASES[name]
    checked(name, args, want)


@pytest.mark.parametrize("n", [16, 17])
def test_host_policy_forced_leaves_no_schedule(n):
    prev = uaes.host_policy(1 << 62, 1, 1)
    try:
        for name, args, want in eaxp_text_case(n, HostMem):
            checked(name, args, want)
    finally:
        uaes.host_policy(*prev)


@pytest.mark.gpu
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n", [16, 17, 16384 + 17])
def test_on_the_gpu(n, dev):
    G.run_case(eaxp_text_case, n, G.DevMem if dev else HostMem)


@pytest.mark.gpu
def test_batches_with_three_records():
    for name, args, want in eaxp_batches():
        checked(name, args, want)
