"""The key-wipe cases of key wrap with padding (uaes_kwp_*), for the suites that demand one of every keyed export.

tests/test_key_wipe_host.py and tests/test_gpu_key_wipe.py read include/uaes_hip.h and fail for a keyed export that
tests/key_wipe_cases.py (ARG_CASES, TEXT_CASES) or test_gpu_key_wipe._batches has no call for.  This module adds the
KWP calls to those three lists when it is imported, and it is named to be collected before tests/test_key_wipe_host.py,
which parametrises over ARG_CASES as it is imported: with the tests directory collected as a whole, which is how the
suite is run, the existing tests see the four KWP exports covered and run their cases like any other's.  Collected alone,
test_key_wipe_host.py reports the four exports as lacking a case; folding these lists into key_wipe_cases.py and
_batches, where they belong, is a change to those files.

So that nothing depends on that order, the same calls are also tests of this module: an argument error behind the key
expansion, the host path at 16 and 17 bytes with a forged input, and on the GPU the one-secret calls with host and
device memory and the two batches, each with the count of live key schedules level across it."""
import ctypes as C

import pytest

import micro_aes_amd as uaes
from tests import key_wipe_cases as K
from tests import test_gpu_key_wipe as G
from tests.key_wipe_cases import ARG, AUTH, B, DATALENGTH, KEY, OK, HostMem, buf, checked, text

KWP_ARG_CASES = {
    "uaes_kwp_wrap": ((128, KEY, B, 0, B), DATALENGTH),                  # an empty secret
    "uaes_kwp_unwrap": ((128, KEY, B, 8, B, None), DATALENGTH),
    "uaes_kwp_wrap_batch": ((128, KEY, 1, 20, None, None, B), ARG),
    "uaes_kwp_unwrap_batch": ((128, KEY, 1, 24, None, None, B, B, B), ARG),
}


def kwp_text_case(n, mem):
    wl = (n + 7) // 8 * 8 + 8                     # 16 bytes: whole semiblocks; 17: seven bytes of fill
    wrapped, out, ln = mem.out(wl), mem.out(wl - 8), C.c_size_t(0)
    yield "uaes_kwp_wrap", (128, KEY, mem.inp(text(n)), n, wrapped), OK
    yield "uaes_kwp_unwrap", (128, KEY, wrapped, wl, out, C.byref(ln)), OK
    wrapped[5] ^= 1
    yield "uaes_kwp_unwrap", (128, KEY, wrapped, wl, out, C.byref(ln)), AUTH


def kwp_batches():
    """three records of 32 bytes, host arrays, as test_gpu_key_wipe._batches has them for key wrap"""
    n, m = 3, 32
    pt, ct, out, ver, lens_out = text(n * m), buf(n * (m + 8)), buf(n * (m + 8)), buf(n), (C.c_uint32 * n)()
    yield "uaes_kwp_wrap_batch", (128, KEY, n, m, None, pt, ct), OK
    yield "uaes_kwp_unwrap_batch", (128, KEY, n, m + 8, None, ct, out, lens_out, ver), OK
    ct[1] ^= 1
    yield "uaes_kwp_unwrap_batch", (128, KEY, n, m + 8, None, ct, out, lens_out, ver), AUTH


# ---- the registration (once, whatever imports this module first)
if "uaes_kwp_wrap" not in K.ARG_CASES:
    K.ARG_CASES.update(KWP_ARG_CASES)
    K.TEXT_CASES.append(kwp_text_case)
    _batches_before = G._batches

    def _batches_with_kwp():
        yield from _batches_before()
        yield from kwp_batches()

    G._batches = _batches_with_kwp


# ---- the same calls as tests of this module
def test_the_lists_hold_the_kwp_calls():
    names = {n for n in K.keyed_exports() if n.startswith("uaes_kwp_")}
    assert names == set(KWP_ARG_CASES) and names <= set(K.ARG_CASES) and kwp_text_case in K.TEXT_CASES
    assert {name for name, _, _ in kwp_batches()} == {n for n in names if n.endswith("_batch")}


@pytest.mark.parametrize("name", sorted(KWP_ARG_CASES))
def test_argument_error_behind_the_key_expansion_leaves_no_schedule(name):
    args, want = KWP_ARG_CASES[name]
    checked(name, args, want)


@pytest.mark.parametrize("n", [16, 17])
def test_host_path_call_leaves_no_schedule(n):
    prev = uaes.host_policy(1 << 62, 1, 1)
    try:
        for name, args, want in kwp_text_case(n, HostMem):
            checked(name, args, want)
    finally:
        uaes.host_policy(*prev)


@pytest.mark.gpu
@pytest.mark.parametrize("mem", [HostMem, G.DevMem], ids=["host", "dev"])
@pytest.mark.parametrize("n", [16, 17])
def test_one_secret_calls_on_the_gpu(n, mem):
    G.run_case(kwp_text_case, n, mem)


@pytest.mark.gpu
def test_batches_with_three_records():
    for name, args, want in kwp_batches():
        checked(name, args, want)
