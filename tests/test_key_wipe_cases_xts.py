"""The key-wipe cases of the XTS batches (uaes_xts_encrypt_batch, uaes_xts_decrypt_batch, uaes_xts_sector_list), for the
suites that demand one of every keyed export.

tests/test_key_wipe_host.py and tests/test_gpu_key_wipe.py read include/uaes_hip.h and fail for a keyed export that
tests/key_wipe_cases.py (ARG_CASES, TEXT_CASES) or test_gpu_key_wipe._batches has no call for.  This module adds the
three calls to those lists when it is imported, and it is named to be collected before tests/test_key_wipe_host.py,
which parametrises over ARG_CASES and TEXT_CASES as it is imported: with the tests directory collected as a whole, which
is how the suite is run, the existing tests see the three exports covered and run their cases like any other's.
Collected alone, test_key_wipe_host.py reports the three exports as lacking a case; folding these lists into
key_wipe_cases.py and _batches, where they belong, is a change to those files.

The sector list stands in TEXT_CASES although it has no host path: test_key_wipe_host.py tells the exports without one
by the endings of their names, and this name has none of them.  The call always goes to the GPU, whatever the host
policy says, so its code is 0 where there is a device and UAES_E_HIP where there is none -- after both keys were
expanded, which is what the count is about.

So that nothing depends on that order, the same calls are also tests of this module: an argument error behind the key
expansion, the sector list under a forced host policy, and on the GPU the sector list with host and device memory and
the two batches, each with the count of live key schedules level across it."""
import ctypes as C

import pytest
import torch

import micro_aes_amd as uaes
from tests import key_wipe_cases as K
from tests import test_gpu_key_wipe as G
from tests.key_wipe_cases import ARG, B, KEY, OK, HostMem, buf, checked, text

HIP = -1                                        # UAES_E_HIP: no usable device

XTS_ARG_CASES = {
    "uaes_xts_encrypt_batch": ((128, KEY, None, 1, 16, None, B, B), ARG),  # no tweaks
    "uaes_xts_decrypt_batch": ((128, KEY, None, 1, 16, None, B, B), ARG),
    "uaes_xts_sector_list": ((128, KEY, None, 1, 16, B, B, 1), ARG),       # no sector numbers
}


def xts_list_text_case(n, mem):
    """two sectors of n bytes (17: each steals), out of order"""
    sectors, out = (C.c_uint64 * 2)(7, 3), mem.out(2 * n)
    yield "uaes_xts_sector_list", (128, KEY, sectors, 2, n, mem.inp(text(2 * n)), out, 1), OK if torch.cuda.is_available() else HIP


def xts_batches():
    """three units of 32 bytes, host arrays, as test_gpu_key_wipe._batches has them for the cipher batches"""
    n, m = 3, 32
    pt, ct, out, tweaks = text(n * m), buf(n * m), buf(n * m), text(n * 16)
    yield "uaes_xts_encrypt_batch", (128, KEY, tweaks, n, m, None, pt, ct), OK
    yield "uaes_xts_decrypt_batch", (128, KEY, tweaks, n, m, None, ct, out), OK


# ---- the registration (once, whatever imports this module first)
if "uaes_xts_sector_list" not in K.ARG_CASES:
    K.ARG_CASES.update(XTS_ARG_CASES)
    K.TEXT_CASES.append(xts_list_text_case)
    _batches_before = G._batches

    def _batches_with_xts():
        yield from _batches_before()
        yield from xts_batches()

    G._batches = _batches_with_xts


# ---- the same calls as tests of this module
def test_the_lists_hold_the_xts_calls():
    names = {n for n in K.keyed_exports() if n.startswith("uaes_xts_") and (n.endswith("_batch") or n.endswith("_list"))}
    assert names == set(XTS_ARG_CASES) and names <= set(K.ARG_CASES) and xts_list_text_case in K.TEXT_CASES
    assert {name for name, _, _ in xts_batches()} == {n for n in names if n.endswith("_batch")}


@pytest.mark.parametrize("name", sorted(XTS_ARG_CASES))
def test_argument_error_behind_the_key_expansion_leaves_no_schedule(name):
    args, want = XTS_ARG_CASES[name]
    checked(name, args, want)


@pytest.mark.parametrize("n", [16, 17])
def test_sector_list_ignores_the_host_policy_and_leaves_no_schedule(n):
    prev = uaes.host_policy(1 << 62, 1, 1)
    try:
        for name, args, want in xts_list_text_case(n, HostMem):
            checked(name, args, want)
    finally:
        uaes.host_policy(*prev)


@pytest.mark.gpu
@pytest.mark.parametrize("mem", [HostMem, G.DevMem], ids=["host", "dev"])
@pytest.mark.parametrize("n", [16, 17])
def test_sector_list_on_the_gpu(n, mem):
    G.run_case(xts_list_text_case, n, mem)


@pytest.mark.gpu
def test_batches_with_three_units():
    for name, args, want in xts_batches():
        checked(name, args, want)
