"""The calls that tests/test_key_wipe_host.py (no GPU) and tests/test_gpu_key_wipe.py make to see that no keyed entry
point leaves an expanded key schedule behind: after any call, whatever it returned, uaes_debug_live_key_schedules() is
what it was before.  ARG_CASES: one call per keyed export that fails an argument check (behind the key expansion where
the function expands first).  TEXT_CASES: the one-message calls with a text of n bytes, an authenticating decryption
once with what the encryption wrote and once forged; `mem` says where the texts live (HostMem here, device memory in the
GPU test).  The return codes are the ones these calls gave before the scoped declaration existed, as literals."""
import ctypes as C
import os
import re

import micro_aes_amd as uaes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(1, 65))
N16 = bytes(range(0xA0, 0xB0))                   # nonce / IV / counter block / tweak, as long as any mode reads
DIGITS = bytes(i % 10 for i in range(17))        # an FF1 / FF3-1 text over the digit values themselves
OK, DATALENGTH, AUTH, DECRYPTION, ARG = 0, 1, 0x1A, 0x1D, -2


def buf(n=64):
    return (C.c_ubyte * n)()


def ptr(v):
    return C.c_void_p(v)


def keyed_exports():
    text = open(os.path.join(ROOT, "include", "uaes_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"UAES_STATIC_INLINE[^{;]*\{.*?\n\}", "", text, flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\b(uaes_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
                  if "keybits" in m.group(2))


def live():
    return uaes.engine().uaes_debug_live_key_schedules()


class HostMem:
    """texts in host memory: the bytes themselves, and ctypes arrays to write to"""
    @staticmethod
    def inp(data):
        return data

    @staticmethod
    def out(n):
        return buf(n)


def text(n):
    return bytes(i & 255 for i in range(n))


def checked(name, args, want):
    """one call: its return code, and the count of live schedules level across it (a tensor goes by its address)"""
    args = [C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a for a in args]
    before = live()
    rc = getattr(uaes.engine(), name)(*args)
    assert rc == want, "%s returned %d (%s), expected %d" % (name, rc, uaes.engine().uaes_last_error().decode(), want)
    assert live() == before, "%s left %d key schedule(s) behind" % (name, live() - before)


# ---- (a): name -> (arguments, return code).  B = a 64-byte buffer; the data pointer, a length or the nonce is what is wrong
B = buf()
_aead8_null_nonce = (128, KEY, None, None, 0, B, 16, B)
_ex_tag0 = (128, KEY, N16, 12, 0, None, 0, B, 16, B)
_rows_null_in = {                                 # the AEAD record batches: one record of 16 bytes, no input
    "uaes_ccm_encrypt_batch": (128, KEY, 12, 16, 1, 16, None, N16, None, 0, None, B, B),
    "uaes_ccm_decrypt_batch": (128, KEY, 12, 16, 1, 16, None, N16, None, 0, None, B, B, B),
    "uaes_ocb_encrypt_batch": (128, KEY, 12, 16, 1, 16, None, N16, None, 0, None, B, B),
    "uaes_ocb_decrypt_batch": (128, KEY, 12, 16, 1, 16, None, N16, None, 0, None, B, B, B),
    "uaes_gcmsiv_encrypt_batch": (128, KEY, 1, 16, None, N16, None, 0, None, B, B),
    "uaes_gcmsiv_decrypt_batch": (128, KEY, 1, 16, None, N16, None, 0, None, B, B, B),
    "uaes_eax_encrypt_batch": (128, KEY, 1, 16, N16, 12, None, 0, None, B, B),
    "uaes_eax_decrypt_batch": (128, KEY, 1, 16, N16, 12, None, 0, None, B, B, B),
    "uaes_siv_encrypt_batch": (128, KEY, 1, 16, None, 0, None, B, B),
    "uaes_siv_decrypt_batch": (128, KEY, 1, 16, None, 0, B, None, B, B),
}
ARG_CASES = {
    "uaes_expand_key": ((128, KEY, None, None), 10),                       # nothing to get wrong behind the expansion: Nr
    "uaes_ecb_encrypt": ((128, KEY, None, 16, None), ARG),
    "uaes_ecb_decrypt": ((128, KEY, None, 16, None), ARG),
    "uaes_ecb_encrypt_padded": ((128, KEY, 1, None, 16, None), ARG),
    "uaes_ctr_xcrypt": ((128, KEY, N16, None, 16, None), ARG),
    "uaes_ctr_xcrypt_iv": ((128, KEY, N16, 12, 1, None, 16, None), ARG),
    "uaes_ctr_xcrypt_at": ((128, KEY, N16, 0, None, 16, None), ARG),
    "uaes_xts_encrypt": ((128, KEY, N16, B, 8, B), DATALENGTH),          # a data unit of 8 bytes
    "uaes_xts_decrypt": ((128, KEY, N16, B, 8, B), DATALENGTH),
    "uaes_xts_sectors": ((128, KEY, 0, 8, 1, B, B, 1), DATALENGTH),      # sector_bytes 8
    "uaes_gcm_encrypt": (_aead8_null_nonce, ARG),
    "uaes_gcm_decrypt": (_aead8_null_nonce, ARG),
    "uaes_gcm_encrypt_iv": ((128, KEY, N16, 0, None, 0, B, 16, B), ARG),   # an empty nonce
    "uaes_gcm_decrypt_iv": ((128, KEY, N16, 0, None, 0, B, 16, B), ARG),
    "uaes_gcm_encrypt_ex": (_ex_tag0, ARG),
    "uaes_gcm_decrypt_ex": (_ex_tag0, ARG),
    "uaes_gcm_multikey_encrypt_batch": ((128, KEY, 0, 1, 16, None, N16, None, 0, B, B, B), ARG),     # tag length 0
    "uaes_gcm_multikey_decrypt_batch": ((128, KEY, 0, 1, 16, None, N16, None, 0, B, B, B, B), ARG),
    "uaes_cmac": ((128, KEY, B, 16, None), ARG),
    "uaes_ccm_encrypt": (_aead8_null_nonce, ARG),
    "uaes_ccm_decrypt": (_aead8_null_nonce, ARG),
    "uaes_ccm_encrypt_ex": (_ex_tag0, ARG),
    "uaes_ccm_decrypt_ex": (_ex_tag0, ARG),
    "uaes_eax_encrypt": (_ex_tag0, ARG),
    "uaes_eax_decrypt": (_ex_tag0, ARG),
    "uaes_siv_encrypt": ((128, KEY, None, 0, B, 16, None, B), ARG),        # no IV
    "uaes_siv_decrypt": ((128, KEY, None, None, 0, B, 16, B), ARG),
    "uaes_cbc_encrypt": ((128, KEY, N16, B, 8, B), DATALENGTH),          # ciphertext stealing wants a block
    "uaes_cbc_decrypt": ((128, KEY, N16, B, 8, B), DATALENGTH),
    "uaes_cbc_encrypt_padded": ((128, KEY, N16, 1, None, 16, None), ARG),
    "uaes_cbc_decrypt_blocks": ((128, KEY, N16, B, 17, B), DATALENGTH),
    "uaes_cfb_encrypt": ((128, KEY, N16, None, 16, None), ARG),
    "uaes_cfb_decrypt": ((128, KEY, N16, None, 16, None), ARG),
    "uaes_ofb_xcrypt": ((128, KEY, N16, None, 16, None), ARG),
    "uaes_cbc_encrypt_batch": ((128, KEY, N16, 1, 17, B, B), ARG),         # a ragged record
    "uaes_cmac_batch": ((128, KEY, 1, 16, None, B), ARG),
    "uaes_cbc_decrypt_batch": ((128, KEY, None, 1, 16, B, B), ARG),        # no IVs
    "uaes_cbc_encrypt_blocks_batch": ((128, KEY, None, 1, 16, B, B), ARG),
    "uaes_cbc_decrypt_blocks_batch": ((128, KEY, None, 1, 16, B, B), ARG),
    "uaes_cfb_encrypt_batch": ((128, KEY, None, 1, 16, None, B, B), ARG),
    "uaes_cfb_decrypt_batch": ((128, KEY, None, 1, 16, None, B, B), ARG),
    "uaes_ofb_xcrypt_batch": ((128, KEY, None, 1, 16, None, B, B), ARG),
    "uaes_ctr_xcrypt_batch": ((128, KEY, None, 1, 16, None, B, B), ARG),
    "uaes_kw_wrap": ((128, KEY, B, 8, B), DATALENGTH),                   # one semiblock
    "uaes_kw_unwrap": ((128, KEY, B, 16, B), DATALENGTH),
    "uaes_kw_wrap_batch": ((128, KEY, 1, 16, None, B), ARG),
    "uaes_kw_unwrap_batch": ((128, KEY, 1, 24, None, B, B), ARG),
    "uaes_kwp_wrap": ((128, KEY, B, 0, B), DATALENGTH),                  # an empty secret
    "uaes_kwp_unwrap": ((128, KEY, B, 8, B, None), DATALENGTH),
    "uaes_kwp_wrap_batch": ((128, KEY, 1, 20, None, None, B), ARG),
    "uaes_kwp_unwrap_batch": ((128, KEY, 1, 24, None, None, B, B, B), ARG),
    "uaes_ff1_encrypt": ((128, KEY, 10, None, None, 0, None, 10, B), ARG),
    "uaes_ff1_decrypt": ((128, KEY, 10, None, None, 0, None, 10, B), ARG),
    "uaes_ff1_encrypt_batch": ((128, KEY, 10, None, None, 0, 0, 1, 10, None, B, None), ARG),
    "uaes_ff1_decrypt_batch": ((128, KEY, 10, None, None, 0, 0, 1, 10, None, B, None), ARG),
    "uaes_ff3_encrypt": ((128, KEY, 10, None, None, DIGITS, 10, B), ARG),  # no tweak
    "uaes_ff3_decrypt": ((128, KEY, 10, None, None, DIGITS, 10, B), ARG),
    "uaes_ff3_encrypt_batch": ((128, KEY, 10, None, N16, 0, 1, 10, None, B, None), ARG),
    "uaes_ff3_decrypt_batch": ((128, KEY, 10, None, N16, 0, 1, 10, None, B, None), ARG),
    "uaes_poly1305": ((128, KEY, N16, B, 16, None), ARG),                  # (its pointers are checked before the key)
    "uaes_poly1305_dev": ((128, KEY, N16, B, 16, None, None), ARG),
    "uaes_poly1305_batch": ((128, KEY, N16, 0, 16, B, B), OK),             # behind the expansion: no messages, nothing to do
    "uaes_gcmsiv_encrypt": (_aead8_null_nonce, ARG),                       # (keybits and pointers before the key)
    "uaes_gcmsiv_decrypt": (_aead8_null_nonce, ARG),
    "uaes_ocb_encrypt": (_aead8_null_nonce, ARG),
    "uaes_ocb_decrypt": (_aead8_null_nonce, ARG),
    "uaes_ocb_encrypt_ex": (_ex_tag0, ARG),
    "uaes_ocb_decrypt_ex": (_ex_tag0, ARG),
    # the constructors of the long-lived holders: a failed expansion frees the object again
    "uaes_gcm_stream_begin": ((C.byref(C.c_void_p()), 100, KEY, N16, None, 0, 0), ARG),
    "uaes_gcm_key_new": ((C.byref(C.c_void_p()), 100, KEY), ARG),
    # the *_dev entries: a misaligned device pointer, or no nonce
    "uaes_ecb_dev": ((128, KEY, 0, ptr(0x1000), 16, ptr(0x1001), None), ARG),
    "uaes_ctr_xcrypt_at_dev": ((128, KEY, N16, 0, ptr(0x1000), 16, ptr(0x1001), None), ARG),
    "uaes_xts_sectors_dev": ((128, KEY, 0, 16, 1, ptr(0x1000), ptr(0x1001), 1, None), ARG),
    "uaes_gcm_encrypt_dev": ((128, KEY, None, None, 0, ptr(0x1000), 16, ptr(0x2000), None), ARG),
    "uaes_gcm_decrypt_dev": ((128, KEY, None, None, 0, ptr(0x1000), 16, ptr(0x2000), ptr(0x3000), None), ARG),
    "uaes_ocb_dev": ((128, KEY, None, 0, None, 0, ptr(0x1000), 16, ptr(0x2000), None, None), ARG),
    "uaes_gcm_partial_dev": ((128, KEY, None, None, 0, ptr(0x1000), 16, 0, 16, ptr(0x2000), None), ARG),
    "uaes_gcm_shard_dev": ((128, KEY, None, 0, None, 0, ptr(0x1000), 16, 0, 16, ptr(0x2000), ptr(0x3000), None), ARG),
    # the multi-GPU split hands the raw key to its workers: no devices, nothing expanded
    "uaes_mgpu_ctr_xcrypt_at": ((0, None, 128, KEY, N16, 0, B, 16, B), ARG),
    "uaes_mgpu_xts_sectors": ((0, None, 128, KEY, 0, 16, 1, B, B, 1), ARG),
    "uaes_mgpu_ecb_encrypt": ((0, None, 128, KEY, 0, B, 16, B), ARG),
    "uaes_mgpu_ecb_decrypt": ((0, None, 128, KEY, B, 16, B), ARG),
    "uaes_mgpu_gcm_encrypt": ((0, None, 128, KEY, N16, None, 0, B, 16, B), ARG),
    "uaes_mgpu_gcm_decrypt": ((0, None, 128, KEY, N16, None, 0, B, 16, B), ARG),
    "uaes_mgpu_ctr_encrypt_gather": ((0, None, 128, KEY, N16, 0, None, 16, None, 0, B), ARG),
}
ARG_CASES.update((name, (args, ARG)) for name, args in _rows_null_in.items())


# ---- texts of n bytes.  Each generator yields (export, arguments, return code); a decryption's input is what the
# encryption before it wrote, and the forged one is that with a bit flipped
def _aead(enc, dec, head, tag=16):
    def run(n, mem):
        pt, ct, out = mem.inp(text(n)), mem.out(n + 16), mem.out(n + 16)
        yield enc, (128, KEY) + head + (b"hdr", 3, pt, n, ct), OK
        yield dec, (128, KEY) + head + (b"hdr", 3, ct, n, out), OK
        ct[n + tag - 1] ^= 1
        yield dec, (128, KEY) + head + (b"hdr", 3, ct, n, out), AUTH
    return run


def _plain(name, head, tail=(), codes=(OK, OK)):
    def run(n, mem):
        yield name, (128, KEY) + head + (mem.inp(text(n)), n, mem.out(n + 32)) + tail, codes[n % 16 != 0]
    return run


def _siv(n, mem):
    iv, ct, out = buf(16), mem.out(n), mem.out(n)
    yield "uaes_siv_encrypt", (128, KEY, b"hdr", 3, mem.inp(text(n)), n, iv, ct), OK
    yield "uaes_siv_decrypt", (128, KEY, iv, b"hdr", 3, ct, n, out), OK
    iv[3] ^= 1
    yield "uaes_siv_decrypt", (128, KEY, iv, b"hdr", 3, ct, n, out), AUTH


def _kw(n, mem):
    n = (n + 7) // 8 * 8                          # whole semiblocks: 16 and 24 bytes
    wrapped, out = mem.out(n + 8), mem.out(n)
    yield "uaes_kw_wrap", (128, KEY, mem.inp(text(n)), n, wrapped), OK
    yield "uaes_kw_unwrap", (128, KEY, wrapped, n + 8, out), OK
    wrapped[5] ^= 1
    yield "uaes_kw_unwrap", (128, KEY, wrapped, n + 8, out), AUTH


def _kwp(n, mem):
    wl = (n + 7) // 8 * 8 + 8                     # 16 bytes: whole semiblocks; 17: seven bytes of fill
    wrapped, out, ln = mem.out(wl), mem.out(wl - 8), C.c_size_t(0)
    yield "uaes_kwp_wrap", (128, KEY, mem.inp(text(n)), n, wrapped), OK
    yield "uaes_kwp_unwrap", (128, KEY, wrapped, wl, out, C.byref(ln)), OK
    wrapped[5] ^= 1
    yield "uaes_kwp_unwrap", (128, KEY, wrapped, wl, out, C.byref(ln)), AUTH


def _fpe(n, mem):
    ct = mem.out(n)
    yield "uaes_ff1_encrypt", (128, KEY, 10, None, b"tw", 2, mem.inp(DIGITS[:n]), n, ct), OK
    yield "uaes_ff1_decrypt", (128, KEY, 10, None, b"tw", 2, ct, n, mem.out(n)), OK
    yield "uaes_ff3_encrypt", (128, KEY, 10, None, N16, mem.inp(DIGITS[:n]), n, ct), OK
    yield "uaes_ff3_decrypt", (128, KEY, 10, None, N16, ct, n, mem.out(n)), OK


TEXT_CASES = [
    _plain("uaes_ecb_encrypt", ()), _plain("uaes_ecb_encrypt_padded", (1,)),
    _plain("uaes_ecb_decrypt", (), codes=(OK, DECRYPTION)),               # not whole blocks: the ragged tail is reported
    _plain("uaes_ctr_xcrypt", (N16,)), _plain("uaes_ctr_xcrypt_iv", (N16, 12, 1)), _plain("uaes_ctr_xcrypt_at", (N16, 0)),
    _plain("uaes_xts_encrypt", (N16,)), _plain("uaes_xts_decrypt", (N16,)),
    lambda n, mem: iter([("uaes_xts_sectors", (128, KEY, 7, n, 1, mem.inp(text(n)), mem.out(n), 1), OK)]),
    lambda n, mem: iter([("uaes_cmac", (128, KEY, mem.inp(text(n)), n, buf(16)), OK)]),          # (a MAC goes to host memory)
    lambda n, mem: iter([("uaes_poly1305", (128, KEY, N16, mem.inp(text(n)), n, buf(16)), OK)]),
    _plain("uaes_cbc_encrypt", (N16,)), _plain("uaes_cbc_decrypt", (N16,)), _plain("uaes_cbc_encrypt_padded", (N16, 1)),
    _plain("uaes_cbc_decrypt_blocks", (N16,), codes=(OK, DATALENGTH)),    # whole blocks only
    _plain("uaes_cfb_encrypt", (N16,)), _plain("uaes_cfb_decrypt", (N16,)), _plain("uaes_ofb_xcrypt", (N16,)),
    _aead("uaes_gcm_encrypt", "uaes_gcm_decrypt", (N16,)),
    _aead("uaes_gcm_encrypt_iv", "uaes_gcm_decrypt_iv", (N16, 8)),
    _aead("uaes_gcm_encrypt_ex", "uaes_gcm_decrypt_ex", (N16, 8, 4), tag=4),
    _aead("uaes_ccm_encrypt", "uaes_ccm_decrypt", (N16,)),
    _aead("uaes_ccm_encrypt_ex", "uaes_ccm_decrypt_ex", (N16, 12, 8), tag=8),
    _aead("uaes_eax_encrypt", "uaes_eax_decrypt", (N16, 16, 16)),
    _aead("uaes_gcmsiv_encrypt", "uaes_gcmsiv_decrypt", (N16,)),
    _aead("uaes_ocb_encrypt", "uaes_ocb_decrypt", (N16,)),
    _aead("uaes_ocb_encrypt_ex", "uaes_ocb_decrypt_ex", (N16, 12, 8), tag=8),
    _siv, _kw, _fpe, _kwp,
]
