"""No call on the GPU path leaves an expanded key schedule behind: uaes_debug_live_key_schedules() is level across every
kind of call (tests/key_wipe_cases.py has the one-message calls and says what the count is).  Counts and return codes
only -- what the calls compute is the other suites' business."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import micro_aes_amd as uaes
from tests.key_wipe_cases import AUTH, KEY, N16, OK, TEXT_CASES, HostMem, buf, checked, keyed_exports, live, text

pytestmark = pytest.mark.gpu

GCMSIV = next(i for i, c in enumerate(TEXT_CASES) if "gcmsiv" in next(c(16, HostMem))[0])


class DevMem:
    """texts in device memory (the nonces, IVs, AAD and MACs of the cases stay host memory)"""
    @staticmethod
    def inp(data):
        return torch.tensor(list(data), dtype=torch.uint8, device="cuda")

    @staticmethod
    def out(n):
        return torch.zeros(n, dtype=torch.uint8, device="cuda")


def run_case(case, n, mem):
    ran = 0
    for name, args, want in case(n, mem):
        checked(name, args, want)
        ran += 1
    assert ran


@pytest.mark.parametrize("mem", [HostMem, DevMem], ids=["host", "dev"])
@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("case", range(len(TEXT_CASES)))
def test_one_message_calls(case, n, mem):
    run_case(TEXT_CASES[case], n, mem)


@pytest.mark.parametrize("mem", [HostMem, DevMem], ids=["host", "dev"])
def test_gcmsiv_just_over_the_one_launch_form(mem):
    assert uaes.plan("siv", 2046 * 16 - 32)[0] != uaes.plan("siv", 2048 * 16)[0]     # 2048 blocks: past SIV_SMALL's 2046 positions
    run_case(TEXT_CASES[GCMSIV], 2048 * 16, mem)


def test_dev_entries_on_a_stream_of_their_own():
    st = torch.cuda.Stream()
    s = C.c_void_p(st.cuda_stream)
    src, dst, mid = DevMem.inp(text(256)), DevMem.out(256 + 16), DevMem.out(256 + 16)
    status, part = torch.zeros(4, dtype=torch.int32, device="cuda"), DevMem.out(16)
    torch.cuda.synchronize()
    try:
        for name, args in (
            ("uaes_ecb_dev", (128, KEY, 0, src, 256, dst, s)),
            ("uaes_ecb_dev", (128, KEY, 1, src, 256, dst, s)),
            ("uaes_ctr_xcrypt_at_dev", (128, KEY, N16, 5, src, 256, dst, s)),
            ("uaes_xts_sectors_dev", (128, KEY, 3, 128, 2, src, dst, 1, s)),
            ("uaes_xts_sectors_dev", (128, KEY, 3, 128, 2, src, dst, 0, s)),
            ("uaes_gcm_encrypt_dev", (128, KEY, N16, None, 0, src, 256, mid, s)),
            ("uaes_gcm_decrypt_dev", (128, KEY, N16, None, 0, mid, 256, dst, status, s)),
            ("uaes_ocb_dev", (128, KEY, N16, 0, None, 0, src, 256, mid, None, s)),
            ("uaes_ocb_dev", (128, KEY, N16, 1, None, 0, mid, 256, dst, status, s)),
            ("uaes_poly1305_dev", (128, KEY, N16, src, 256, part, s)),
            ("uaes_gcm_partial_dev", (128, KEY, N16, None, 0, src, 256, 0, 256, part, s)),
            ("uaes_gcm_shard_dev", (128, KEY, N16, 0, None, 0, src, 256, 0, 256, dst, part, s)),
        ):
            checked(name, args, OK)
        st.synchronize()
        assert status[0].item() == 0                           # (the two decryptions saw the tags made right before them)
    finally:
        st.synchronize()
        uaes.engine().uaes_stream_release(s)


# ---- the batch entries, three records each, host arrays.  A decryption reads what the encryption before it wrote.
def _batches():
    n, m = 3, 32
    pt, ct, out, tags, ver = text(n * m), buf(n * (m + 8)), buf(n * (m + 8)), buf(n * 16), buf(n)
    nonces, ivs = text(n * 16), buf(n * 16)
    rows = lambda head: (128, KEY) + head + (n, m, None, nonces, b"hdr" * n, 3)      # ... lens, nonces, aData, aad_bytes
    yield "uaes_ccm_encrypt_batch", rows((12, 16)) + (pt, ct, tags), OK
    yield "uaes_ccm_decrypt_batch", rows((12, 16)) + (ct, tags, out, ver), OK
    yield "uaes_ocb_encrypt_batch", rows((12, 16)) + (pt, ct, tags), OK
    yield "uaes_ocb_decrypt_batch", rows((12, 16)) + (ct, tags, out, ver), OK
    yield "uaes_gcmsiv_encrypt_batch", rows(()) + (pt, ct, tags), OK
    yield "uaes_gcmsiv_decrypt_batch", rows(()) + (ct, tags, out, ver), OK
    yield "uaes_gcm_multikey_encrypt_batch", (128, text(n * 16), 16, n, m, None, nonces, b"hdr" * n, 3, pt, ct, tags), OK
    yield "uaes_gcm_multikey_decrypt_batch", (128, text(n * 16), 16, n, m, None, nonces, b"hdr" * n, 3, ct, tags, out, ver), OK
    yield "uaes_eax_encrypt_batch", (128, KEY, n, m, nonces, 16, b"hdr" * n, 3, pt, ct, tags), OK
    yield "uaes_eax_decrypt_batch", (128, KEY, n, m, nonces, 16, b"hdr" * n, 3, ct, tags, out, ver), OK
    tags[0] ^= 1
    yield "uaes_eax_decrypt_batch", (128, KEY, n, m, nonces, 16, b"hdr" * n, 3, ct, tags, out, ver), AUTH
    yield "uaes_siv_encrypt_batch", (128, KEY, n, m, b"hdr" * n, 3, pt, ivs, ct), OK
    yield "uaes_siv_decrypt_batch", (128, KEY, n, m, b"hdr" * n, 3, ivs, ct, out, ver), OK
    yield "uaes_cbc_encrypt_batch", (128, KEY, nonces, n, m, pt, ct), OK
    yield "uaes_cmac_batch", (128, KEY, n, m, pt, tags), OK
    yield "uaes_poly1305_batch", (128, KEY, nonces, n, m, pt, tags), OK
    for name in ("uaes_cbc_decrypt_batch", "uaes_cbc_encrypt_blocks_batch", "uaes_cbc_decrypt_blocks_batch"):
        yield name, (128, KEY, nonces, n, m, pt, ct), OK
    for name in ("uaes_cfb_encrypt_batch", "uaes_cfb_decrypt_batch", "uaes_ofb_xcrypt_batch", "uaes_ctr_xcrypt_batch"):
        yield name, (128, KEY, nonces, n, m, None, pt, ct), OK
    yield "uaes_kw_wrap_batch", (128, KEY, n, m, pt, ct), OK
    yield "uaes_kw_unwrap_batch", (128, KEY, n, m + 8, ct, out, ver), OK
    ct[1] ^= 1
    yield "uaes_kw_unwrap_batch", (128, KEY, n, m + 8, ct, out, ver), AUTH
    lens_out = (C.c_uint32 * n)()
    yield "uaes_kwp_wrap_batch", (128, KEY, n, m, None, pt, ct), OK
    yield "uaes_kwp_unwrap_batch", (128, KEY, n, m + 8, None, ct, out, lens_out, ver), OK
    ct[1] ^= 1
    yield "uaes_kwp_unwrap_batch", (128, KEY, n, m + 8, None, ct, out, lens_out, ver), AUTH
    digits = bytes(i % 10 for i in range(n * m))
    yield "uaes_ff1_encrypt_batch", (128, KEY, 10, None, nonces, 4, 16, n, m, digits, ct, ver), OK
    yield "uaes_ff1_decrypt_batch", (128, KEY, 10, None, nonces, 4, 16, n, m, ct, out, ver), OK
    yield "uaes_ff3_encrypt_batch", (128, KEY, 10, None, nonces, 16, n, m, digits, ct, ver), OK
    yield "uaes_ff3_decrypt_batch", (128, KEY, 10, None, nonces, 16, n, m, ct, out, ver), OK


def test_batch_entries_with_three_records():
    ran = set()
    for name, args, want in _batches():
        checked(name, args, want)
        ran.add(name)
    assert ran == {n for n in keyed_exports() if n.endswith("_batch")}


def test_kwp_batches_with_three_records():
    """key wrap with padding by name: the wrap, the unwrap of what it wrote, and the unwrap of a forged record"""
    ran = []
    for name, args, want in _batches():
        if name.startswith("uaes_kwp_"):
            checked(name, args, want)
            ran.append((name, want))
    assert ran == [("uaes_kwp_wrap_batch", OK), ("uaes_kwp_unwrap_batch", OK), ("uaes_kwp_unwrap_batch", AUTH)]


# ---- the slice pipeline: a long host text leaves its function through run_pipelined's return
LONG = (32 << 20) + 16


@pytest.fixture(scope="module")
def long_bufs():
    return np.zeros(LONG, dtype=np.uint8), np.empty(LONG + 16, dtype=np.uint8)


def _long_calls(src, dst):
    a, b = C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data)
    return {
        "ecb": ("uaes_ecb_encrypt", (128, KEY, a, LONG, b)),
        "ctr": ("uaes_ctr_xcrypt_at", (128, KEY, N16, 0, a, LONG, b)),
        "xts": ("uaes_xts_sectors", (128, KEY, 0, 48, LONG // 48, a, b, 1)),
        "gcm": ("uaes_gcm_encrypt", (128, KEY, N16, b"hdr", 3, a, LONG, b)),
    }


@pytest.mark.parametrize("mode", ["ecb", "ctr", "xts", "gcm"])
def test_slice_pipeline_exit(long_bufs, mode):
    assert LONG % 48 == 0
    name, args = _long_calls(*long_bufs)[mode]
    checked(name, args, OK)


def test_multi_gpu_hand_off(long_bufs):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    L = uaes.engine()
    assert L.uaes_set_devices(2, (C.c_int * 2)(0, 1), 32 << 20) == 0
    try:
        for name, args in _long_calls(*long_bufs).values():
            checked(name, args, OK)
    finally:
        assert L.uaes_set_devices(0, None, 64 << 20) == 0      # off again, the default threshold back


# ---- the long-lived holders count while they are open
def test_key_context_counts_while_it_is_open():
    before = live()
    k = uaes.GcmKey(KEY[:16])
    assert live() == before + 1
    ct = k.encrypt(N16[:12], b"hdr", text(17))
    assert k.decrypt(N16[:12], b"hdr", ct) == (0, text(17)) and live() == before + 1
    k.close()
    assert live() == before


def test_stream_counts_until_it_is_finished_or_dropped():
    before = live()
    s = uaes.GcmStream(KEY[:16], N16[:12], b"hdr")
    assert live() == before + 1
    s.update(text(32))
    s.update(text(17))
    assert len(s.finish()) == 16 and live() == before
    s = uaes.GcmStream(KEY[:16], N16[:12], b"hdr", decrypt=True)
    s.update(text(32))
    assert s.finish(bytes(16)) == AUTH and live() == before     # a wrong tag: the same way out
    s = uaes.GcmStream(KEY[:16], N16[:12])
    s.update(text(16))
    assert live() == before + 1
    del s                                                       # dropped unfinished
    assert live() == before


def test_two_threads_with_fifty_mixed_calls_each():
    before = live()
    errors = []

    def work(t):
        try:
            done = 0
            while done < 50:
                for k, case in enumerate(TEXT_CASES):
                    for name, args, want in case(16 + (k + t) % 2, HostMem):
                        rc = getattr(uaes.engine(), name)(*args)
                        assert rc == want, "%s returned %d, expected %d" % (name, rc, want)
                        done += 1
        except Exception as e:                                  # noqa: BLE001 -- reported by the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert live() == before
