"""The key-wipe cases of SIV with a vector of associated data (uaes_siv_encrypt_v, uaes_siv_decrypt_v,
uaes_siv_encrypt_batch_v, uaes_siv_decrypt_batch_v), for the suites that demand one of every keyed export.

As tests/test_key_wipe_cases_xts.py does for the XTS batches: tests/test_key_wipe_host.py reads include/uaes_hip.h and
fails for a keyed export that tests/key_wipe_cases.py (ARG_CASES, TEXT_CASES) has no call for.  This module adds the four
calls to those lists when it is imported, and it is named to be collected before tests/test_key_wipe_host.py, which
parametrises over the lists as it is imported; folding them into key_wipe_cases.py, where they belong, is a change to
that file.

The two batches stand in TEXT_CASES although they have no host path: test_key_wipe_host.py tells the exports without one
by the endings of their names ("_batch"), and "_batch_v" is none of them.  They always go to the GPU, so their code is 0
where there is a device and UAES_E_HIP where there is none -- after both keys were expanded, which is what the count is
about.

So that nothing depends on that order, the same calls are also tests of this module."""
import ctypes as C

import pytest
import torch

import micro_aes_amd as uaes
from tests import key_wipe_cases as K
from tests.key_wipe_cases import ARG, AUTH, B, KEY, OK, HostMem, buf, checked, text

HIP = -1                                        # UAES_E_HIP: no usable device
ADL = (C.c_size_t * 2)(3, 5)                    # two components: "hdr" and "nonce"
AD = b"hdrnonce"

SIV_V_ARG_CASES = {
    "uaes_siv_encrypt_v": ((128, KEY, 2, ADL, AD, B, 16, None, B), ARG),                       # no IV
    "uaes_siv_decrypt_v": ((128, KEY, None, 2, ADL, AD, B, 16, B), ARG),
    "uaes_siv_encrypt_batch_v": ((128, KEY, 1, 16, None, 2, ADL, AD, None, B, B), ARG),        # no input
    "uaes_siv_decrypt_batch_v": ((128, KEY, 1, 16, None, 2, ADL, AD, B, None, B, B), ARG),
}


def siv_v_text_case(n, mem):
    iv, ct, out = buf(16), mem.out(n), mem.out(n)
    yield "uaes_siv_encrypt_v", (128, KEY, 2, ADL, AD, mem.inp(text(n)), n, iv, ct), OK
    yield "uaes_siv_decrypt_v", (128, KEY, iv, 2, ADL, AD, ct, n, out), OK
    iv[3] ^= 1
    yield "uaes_siv_decrypt_v", (128, KEY, iv, 2, ADL, AD, ct, n, out), AUTH


def siv_v_batch_text_case(n, mem):
    """two records of n bytes; the decryption reads what the encryption wrote, then a forged IV"""
    gpu = torch.cuda.is_available()
    ivs, ct, out, ver = buf(32), mem.out(2 * n), mem.out(2 * n), buf(2)
    yield "uaes_siv_encrypt_batch_v", (128, KEY, 2, n, None, 2, ADL, AD * 2, mem.inp(text(2 * n)), ivs, ct), OK if gpu else HIP
    yield "uaes_siv_decrypt_batch_v", (128, KEY, 2, n, None, 2, ADL, AD * 2, ivs, ct, out, ver), OK if gpu else HIP
    ivs[17] ^= 1
    yield "uaes_siv_decrypt_batch_v", (128, KEY, 2, n, None, 2, ADL, AD * 2, ivs, ct, out, ver), AUTH if gpu else HIP


# ---- the registration (once, whatever imports this module first)
if "uaes_siv_encrypt_v" not in K.ARG_CASES:
    K.ARG_CASES.update(SIV_V_ARG_CASES)
    K.TEXT_CASES.extend([siv_v_text_case, siv_v_batch_text_case])


# ---- the same calls as tests of this module
def test_the_lists_hold_the_siv_v_calls():
    names = {n for n in K.keyed_exports() if n.startswith("uaes_siv_") and n.endswith("_v")}
    assert names == set(SIV_V_ARG_CASES) and names <= set(K.ARG_CASES)
    assert siv_v_text_case in K.TEXT_CASES and siv_v_batch_text_case in K.TEXT_CASES


@pytest.mark.parametrize("name", sorted(SIV_V_ARG_CASES))
def test_argument_error_behind_the_key_expansion_leaves_no_schedule(name):
    args, want = SIV_V_ARG_CASES[name]
    checked(name, args, want)


@pytest.mark.parametrize("case", [siv_v_text_case, siv_v_batch_text_case], ids=["single", "batch"])
@pytest.mark.parametrize("n", [16, 17])
def test_host_policy_forced_leaves_no_schedule(n, case):
    prev = uaes.host_policy(1 << 62, 1, 1)
    try:
        for name, args, want in case(n, HostMem):
            checked(name, args, want)
    finally:
        uaes.host_policy(*prev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [siv_v_text_case, siv_v_batch_text_case], ids=["single", "batch"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("n", [16, 17])
def test_on_the_gpu(n, dev, case):
    from tests.test_gpu_key_wipe import DevMem
    for name, args, want in case(n, DevMem if dev else HostMem):
        checked(name, args, want)
