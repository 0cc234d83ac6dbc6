"""micro-aes_amd -- Python host mirror of the MI355X AES engine.

The product is ``lib/libuaes_hip.so`` (C ABI in ``include/uaes_hip.h``: hand
written gfx950 kernels behind plain-C entry points).  This package is the thin
host-side mirror of the reference's operator interface for the hot path --
``AES_ECB_encrypt`` ... ``AES_GCM_decrypt`` with the reference's argument order
(micro_aes.h:173-181, :239-249, :256-266, :294-308), minus the explicit lengths
-- plus the device-resident entry points that bench.py and the multi-GPU
sharding layer drive with ``torch`` tensors' raw pointers.  torch is only
plumbing here (device memory, streams, torch.distributed).

There is NO fallback: if the shared library is missing or no HIP device is
usable, importing ``engine()`` / calling any function raises.  (The engine's own
host data path, csrc/uaes_host.c, is opt-in: ``host_policy()`` below.)

The directory name carries a hyphen (it is the name the project was given), so
import it through the alias module at the repo root::

    import micro_aes_amd as uaes
"""
import collections
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
CSRC = os.path.join(HERE, "csrc")

M_RESULT_SUCCESS = 0
M_DATALENGTH_ERROR = 1
M_AUTHENTICATION_ERROR = 0x1A
M_DECRYPTION_ERROR = 0x1D
M_ENCRYPTION_ERROR = 0x1E

EXPORTS = [
    "uaes_init", "uaes_shutdown", "uaes_selftest", "uaes_last_error", "uaes_version", "uaes_expand_key", "uaes_stream_release",
    "uaes_set_wipe_on_auth_failure", "uaes_set_gcm_one_pass_decrypt", "uaes_clock_probe_dev",
    "uaes_ecb_encrypt", "uaes_ecb_encrypt_padded", "uaes_ecb_decrypt", "uaes_ctr_xcrypt", "uaes_ctr_xcrypt_iv", "uaes_ctr_xcrypt_at",
    "uaes_xts_encrypt", "uaes_xts_decrypt", "uaes_xts_sectors",
    "uaes_xts_encrypt_batch", "uaes_xts_decrypt_batch", "uaes_xts_sector_list", "uaes_debug_plan_xts_batch",
    "uaes_gcm_encrypt", "uaes_gcm_decrypt", "uaes_gcm_encrypt_iv", "uaes_gcm_decrypt_iv", "uaes_ghash",
    "uaes_gcm_encrypt_ex", "uaes_gcm_decrypt_ex", "uaes_ccm_encrypt_ex", "uaes_ccm_decrypt_ex",
    "uaes_ccm_encrypt_batch", "uaes_ccm_decrypt_batch",
    "uaes_ocb_encrypt_ex", "uaes_ocb_decrypt_ex",
    "uaes_ocb_encrypt_batch", "uaes_ocb_decrypt_batch", "uaes_debug_plan_ocb_batch",
    "uaes_cmac", "uaes_ccm_encrypt", "uaes_ccm_decrypt", "uaes_gcmsiv_encrypt", "uaes_gcmsiv_decrypt",
    "uaes_gcmsiv_encrypt_batch", "uaes_gcmsiv_decrypt_batch", "uaes_debug_plan_gcmsiv_batch",
    "uaes_gcm_multikey_encrypt_batch", "uaes_gcm_multikey_decrypt_batch", "uaes_debug_plan_gcm_multikey_batch",
    "uaes_xaes256gcm_derive", "uaes_xaes256gcm_encrypt", "uaes_xaes256gcm_decrypt",
    "uaes_xaes256gcm_encrypt_batch", "uaes_xaes256gcm_decrypt_batch", "uaes_debug_plan_xaes256gcm_batch",
    "uaes_ocb_encrypt", "uaes_ocb_decrypt", "uaes_ocb_dev", "uaes_debug_plan_ocb", "uaes_debug_plan_xts",
    "uaes_debug_plan_gcm_piece", "uaes_debug_gcm_stream_tables",
    "uaes_poly1305", "uaes_poly1305_dev", "uaes_poly1305_batch", "uaes_debug_plan_poly1305",
    "uaes_eax_encrypt", "uaes_eax_decrypt", "uaes_siv_encrypt", "uaes_siv_decrypt",
    "uaes_eax_encrypt_batch", "uaes_eax_decrypt_batch", "uaes_siv_encrypt_batch", "uaes_siv_decrypt_batch",
    "uaes_debug_plan_eax_siv", "uaes_debug_plan_chain",
    "uaes_eaxp_encrypt", "uaes_eaxp_decrypt", "uaes_eaxp_encrypt_batch", "uaes_eaxp_decrypt_batch", "uaes_debug_plan_eaxp",
    "uaes_siv_encrypt_v", "uaes_siv_decrypt_v", "uaes_siv_encrypt_batch_v", "uaes_siv_decrypt_batch_v", "uaes_debug_plan_siv_v",
    "uaes_kw_wrap", "uaes_kw_unwrap", "uaes_kw_wrap_batch", "uaes_kw_unwrap_batch", "uaes_debug_plan_kw",
    "uaes_kwp_wrap", "uaes_kwp_unwrap", "uaes_kwp_wrap_batch", "uaes_kwp_unwrap_batch", "uaes_debug_plan_kwp",
    "uaes_ff1_encrypt", "uaes_ff1_decrypt", "uaes_ff1_encrypt_batch", "uaes_ff1_decrypt_batch", "uaes_debug_plan_ff1",
    "uaes_ff3_maxlen", "uaes_ff3_encrypt", "uaes_ff3_decrypt", "uaes_ff3_encrypt_batch", "uaes_ff3_decrypt_batch", "uaes_debug_plan_ff3",
    "uaes_mgpu_ctr_xcrypt_at", "uaes_mgpu_xts_sectors", "uaes_mgpu_ctr_encrypt_gather", "uaes_debug_gather_stats", "uaes_debug_gcm_look", "uaes_debug_gcm_chunk_folds",
    "uaes_debug_live_key_schedules", "uaes_debug_plan", "uaes_debug_plan_at", "uaes_debug_arrangement_name", "uaes_debug_plan_disable",
    "uaes_mgpu_ecb_encrypt", "uaes_mgpu_ecb_decrypt", "uaes_mgpu_gcm_encrypt", "uaes_mgpu_gcm_decrypt",
    "uaes_set_devices", "uaes_set_producer_stream", "uaes_set_host_policy", "uaes_get_host_policy",
    "uaes_gcm_key_new", "uaes_gcm_key_free", "uaes_gcm_key_encrypt", "uaes_gcm_key_decrypt",
    "uaes_gcm_key_encrypt_dev", "uaes_gcm_key_decrypt_dev",
    "uaes_gcm_record_max", "uaes_gcm_key_encrypt_records", "uaes_gcm_key_decrypt_records",
    "uaes_gcm_key_encrypt_records_dev", "uaes_gcm_key_decrypt_records_dev",
    "uaes_gcm_key_encrypt_records_v", "uaes_gcm_key_decrypt_records_v",
    "uaes_gcm_key_encrypt_records_v_dev", "uaes_gcm_key_decrypt_records_v_dev",
    "uaes_gcm_stream_begin", "uaes_gcm_stream_update", "uaes_gcm_stream_finish", "uaes_gcm_stream_abort",
    "uaes_cbc_encrypt_batch", "uaes_cmac_batch", "uaes_cbc_encrypt", "uaes_cbc_decrypt", "uaes_cbc_encrypt_padded", "uaes_cbc_decrypt_blocks", "uaes_cfb_encrypt", "uaes_cfb_decrypt", "uaes_ofb_xcrypt",
    "uaes_cbc_decrypt_batch", "uaes_cbc_encrypt_blocks_batch", "uaes_cbc_decrypt_blocks_batch", "uaes_cfb_encrypt_batch",
    "uaes_cfb_decrypt_batch", "uaes_ofb_xcrypt_batch", "uaes_ctr_xcrypt_batch", "uaes_debug_plan_cipher_batch",
    "uaes_ecb_dev", "uaes_ctr_xcrypt_at_dev", "uaes_xts_sectors_dev",
    "uaes_gcm_encrypt_dev", "uaes_gcm_decrypt_dev", "uaes_gcm_partial_dev", "uaes_gcm_shard_dev",
]
COMPAT_EXPORTS = [
    "AES_ECB_encrypt", "AES_ECB_encrypt_pkcs7", "AES_ECB_encrypt_iso7816", "AES_ECB_decrypt",
    "AES_CTR_encrypt", "AES_CTR_decrypt", "AES_CTR_encrypt_preset", "AES_CTR_decrypt_preset", "AES_CTR_encrypt_iv",
    "AES_CBC_encrypt_nocts", "AES_CBC_encrypt_nocts_pkcs7", "AES_CBC_encrypt_nocts_iso7816", "AES_CBC_decrypt_nocts",
    "uaes_compat_set_failure_handler", "uaes_compat_set_producer_stream",
    "AES_XTS_encrypt", "AES_XTS_decrypt", "AES_GCM_encrypt", "AES_GCM_decrypt",
    "AES_GCM_encrypt_ivlen", "AES_GCM_decrypt_ivlen", "AES_GCM_encrypt_lens", "AES_GCM_decrypt_lens",
    "AES_CCM_encrypt_lens", "AES_CCM_decrypt_lens", "AES_OCB_encrypt_lens", "AES_OCB_decrypt_lens",
    "AES_CCM_encrypt", "AES_CCM_decrypt", "AES_CMAC", "GCM_SIV_encrypt", "GCM_SIV_decrypt",
    "AES_OCB_encrypt", "AES_OCB_decrypt", "AES_Poly1305", "AES_KEY_wrap", "AES_KEY_unwrap",
    "AES_FPE_encrypt", "AES_FPE_decrypt", "AES_FPE_encrypt_alpha", "AES_FPE_decrypt_alpha",
    "AES_FF3_encrypt", "AES_FF3_decrypt", "AES_FF3_encrypt_alpha", "AES_FF3_decrypt_alpha",
    "AES_EAX_encrypt", "AES_EAX_decrypt", "AES_EAX_encrypt_lens", "AES_EAX_decrypt_lens", "AES_EAXP_encrypt", "AES_EAXP_decrypt",
    "AES_SIV_encrypt", "AES_SIV_decrypt",
    "AES_CBC_encrypt", "AES_CBC_decrypt", "AES_CFB_encrypt", "AES_CFB_decrypt", "AES_OFB_encrypt", "AES_OFB_decrypt",
]


class EngineError(RuntimeError):
    pass


def build(quiet=True):
    """Compile the HIP kernels and the C host layer for gfx950, in-tree."""
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True,
                   stdout=subprocess.DEVNULL if quiet else None)


def lib_path(name="libuaes_hip.so"):
    return os.path.join(LIB_DIR, name)


_lib = None


def engine():
    """The loaded C-ABI library (ctypes.CDLL), prototypes attached."""
    global _lib
    if _lib is not None:
        return _lib
    # torch wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, same
    # SONAME as /opt/rocm's).  Two HIP runtimes in one process do not work
    # ("No HIP GPUs are available" from whichever initialises second), so when
    # torch is installed let it load its runtime FIRST; our library then binds
    # to that same copy.  A plain C caller simply uses the system ROCm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = lib_path()
    if not os.path.exists(path):
        raise EngineError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (there is no CPU fallback)" % path)
    L = C.CDLL(path)
    sz, i, vp, u64 = C.c_size_t, C.c_int, C.c_void_p, C.c_uint64
    L.uaes_init.restype = i
    L.uaes_selftest.restype = i
    L.uaes_last_error.restype = C.c_char_p
    L.uaes_version.restype = C.c_char_p
    for n in ("uaes_ecb_encrypt", "uaes_ecb_decrypt"):
        getattr(L, n).argtypes = [i, vp, vp, sz, vp]
    L.uaes_stream_release.argtypes = [vp]
    L.uaes_clock_probe_dev.argtypes = [vp, C.c_uint, vp]
    L.uaes_cbc_encrypt_batch.argtypes = [i, vp, vp, sz, sz, vp, vp]
    L.uaes_cmac_batch.argtypes = [i, vp, sz, sz, vp, vp]
    for n in ("uaes_cbc_decrypt_batch", "uaes_cbc_encrypt_blocks_batch", "uaes_cbc_decrypt_blocks_batch"):
        getattr(L, n).argtypes = [i, vp, vp, sz, sz, vp, vp]
    for n in ("uaes_cfb_encrypt_batch", "uaes_cfb_decrypt_batch", "uaes_ofb_xcrypt_batch", "uaes_ctr_xcrypt_batch"):
        getattr(L, n).argtypes = [i, vp, vp, sz, sz, vp, vp, vp]
    L.uaes_debug_plan_cipher_batch.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_cipher_batch.restype = C.c_char_p
    L.uaes_ecb_encrypt_padded.argtypes = [i, vp, i, vp, sz, vp]
    L.uaes_ctr_xcrypt.argtypes = [i, vp, vp, vp, sz, vp]
    L.uaes_ctr_xcrypt_at.argtypes = [i, vp, vp, u64, vp, sz, vp]
    L.uaes_ctr_xcrypt_iv.argtypes = [i, vp, vp, sz, u64, vp, sz, vp]
    L.uaes_cbc_encrypt_padded.argtypes = [i, vp, vp, i, vp, sz, vp]
    L.uaes_cbc_decrypt_blocks.argtypes = [i, vp, vp, vp, sz, vp]
    for n in ("uaes_xts_encrypt", "uaes_xts_decrypt"):
        getattr(L, n).argtypes = [i, vp, vp, vp, sz, vp]
    L.uaes_xts_sectors.argtypes = [i, vp, u64, sz, sz, vp, vp, i]
    for n in ("uaes_xts_encrypt_batch", "uaes_xts_decrypt_batch"):
        getattr(L, n).argtypes = [i, vp, vp, sz, sz, vp, vp, vp]
    L.uaes_xts_sector_list.argtypes = [i, vp, vp, sz, sz, vp, vp, i]
    L.uaes_debug_plan_xts_batch.argtypes = [sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_xts_batch.restype = C.c_char_p
    for n in ("uaes_gcm_encrypt", "uaes_gcm_decrypt"):
        getattr(L, n).argtypes = [i, vp, vp, vp, sz, vp, sz, vp]
    for n in ("uaes_gcm_encrypt_iv", "uaes_gcm_decrypt_iv"):
        getattr(L, n).argtypes = [i, vp, vp, sz, vp, sz, vp, sz, vp]
    for n in ("uaes_gcm_encrypt_ex", "uaes_gcm_decrypt_ex", "uaes_ccm_encrypt_ex", "uaes_ccm_decrypt_ex",
              "uaes_ocb_encrypt_ex", "uaes_ocb_decrypt_ex"):
        getattr(L, n).argtypes = [i, vp, vp, sz, sz, vp, sz, vp, sz, vp]
    L.uaes_ghash.argtypes = [vp, vp, sz, vp, sz, vp]
    L.uaes_cmac.argtypes = [i, vp, vp, sz, vp]
    L.uaes_poly1305.argtypes = [i, vp, vp, vp, sz, vp]
    L.uaes_poly1305_dev.argtypes = [i, vp, vp, vp, sz, vp, vp]
    L.uaes_poly1305_batch.argtypes = [i, vp, vp, sz, sz, vp, vp]
    L.uaes_debug_plan_poly1305.argtypes = [sz, sz, C.POINTER(C.c_int)]
    L.uaes_eax_encrypt.argtypes = [i, vp, vp, sz, sz, vp, sz, vp, sz, vp]
    L.uaes_eax_decrypt.argtypes = [i, vp, vp, sz, sz, vp, sz, vp, sz, vp]
    L.uaes_siv_encrypt.argtypes = [i, vp, vp, sz, vp, sz, vp, vp]
    L.uaes_siv_decrypt.argtypes = [i, vp, vp, vp, sz, vp, sz, vp]
    L.uaes_eax_encrypt_batch.argtypes = [i, vp, sz, sz, vp, sz, vp, sz, vp, vp, vp]
    L.uaes_eax_decrypt_batch.argtypes = [i, vp, sz, sz, vp, sz, vp, sz, vp, vp, vp, vp]
    L.uaes_ccm_encrypt_batch.argtypes = [i, vp, sz, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp]
    L.uaes_ccm_decrypt_batch.argtypes = [i, vp, sz, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.uaes_ocb_encrypt_batch.argtypes = [i, vp, sz, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp]
    L.uaes_ocb_decrypt_batch.argtypes = [i, vp, sz, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.uaes_debug_plan_ocb_batch.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_ocb_batch.restype = C.c_char_p
    L.uaes_gcmsiv_encrypt_batch.argtypes = [i, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp]
    L.uaes_gcmsiv_decrypt_batch.argtypes = [i, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.uaes_debug_plan_gcmsiv_batch.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_gcmsiv_batch.restype = C.c_char_p
    L.uaes_gcm_multikey_encrypt_batch.argtypes = [i, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp]
    L.uaes_gcm_multikey_decrypt_batch.argtypes = [i, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.uaes_debug_plan_gcm_multikey_batch.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_gcm_multikey_batch.restype = C.c_char_p
    L.uaes_xaes256gcm_derive.argtypes = [vp, vp, vp]
    L.uaes_xaes256gcm_encrypt.argtypes = [vp, vp, vp, sz, vp, sz, vp]
    L.uaes_xaes256gcm_decrypt.argtypes = [vp, vp, vp, sz, vp, sz, vp]
    L.uaes_xaes256gcm_encrypt_batch.argtypes = [vp, sz, sz, vp, vp, vp, sz, vp, vp, vp]
    L.uaes_xaes256gcm_decrypt_batch.argtypes = [vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    L.uaes_debug_plan_xaes256gcm_batch.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_xaes256gcm_batch.restype = C.c_char_p
    L.uaes_siv_encrypt_batch.argtypes = [i, vp, sz, sz, vp, sz, vp, vp, vp]
    L.uaes_siv_decrypt_batch.argtypes = [i, vp, sz, sz, vp, sz, vp, vp, vp, vp]
    L.uaes_debug_plan_eax_siv.argtypes = [i, i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_eax_siv.restype = C.c_char_p
    L.uaes_eaxp_encrypt.argtypes = [i, vp, vp, sz, vp, sz, vp]
    L.uaes_eaxp_decrypt.argtypes = [i, vp, vp, sz, vp, sz, vp]
    L.uaes_eaxp_encrypt_batch.argtypes = [i, vp, sz, sz, vp, vp, sz, vp, vp, vp, vp]
    L.uaes_eaxp_decrypt_batch.argtypes = [i, vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp]
    L.uaes_debug_plan_eaxp.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_eaxp.restype = C.c_char_p
    L.uaes_siv_encrypt_v.argtypes = [i, vp, sz, vp, vp, vp, sz, vp, vp]
    L.uaes_siv_decrypt_v.argtypes = [i, vp, vp, sz, vp, vp, vp, sz, vp]
    L.uaes_siv_encrypt_batch_v.argtypes = [i, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]
    L.uaes_siv_decrypt_batch_v.argtypes = [i, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp, vp]
    L.uaes_debug_plan_siv_v.argtypes = [i, sz, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_siv_v.restype = C.c_char_p
    L.uaes_debug_plan_poly1305.restype = C.c_char_p
    L.uaes_debug_plan_chain.argtypes = [i, i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_chain.restype = C.c_char_p
    L.uaes_kw_wrap.argtypes = [i, vp, vp, sz, vp]
    L.uaes_kw_unwrap.argtypes = [i, vp, vp, sz, vp]
    L.uaes_kw_wrap_batch.argtypes = [i, vp, sz, sz, vp, vp]
    L.uaes_kw_unwrap_batch.argtypes = [i, vp, sz, sz, vp, vp, vp]
    L.uaes_debug_plan_kw.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_kw.restype = C.c_char_p
    L.uaes_kwp_wrap.argtypes = [i, vp, vp, sz, vp]
    L.uaes_kwp_unwrap.argtypes = [i, vp, vp, sz, vp, C.POINTER(sz)]
    L.uaes_kwp_wrap_batch.argtypes = [i, vp, sz, sz, vp, vp, vp]
    L.uaes_kwp_unwrap_batch.argtypes = [i, vp, sz, sz, vp, vp, vp, vp, vp]
    L.uaes_debug_plan_kwp.argtypes = [i, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_kwp.restype = C.c_char_p
    L.uaes_debug_plan_ocb.argtypes = [i, sz, sz, i, C.POINTER(C.c_int)]
    L.uaes_debug_plan_ocb.restype = C.c_char_p
    L.uaes_debug_plan_xts.argtypes = [sz, sz, i, C.POINTER(C.c_uint64)]
    L.uaes_debug_plan_xts.restype = C.c_char_p
    L.uaes_debug_plan_gcm_piece.argtypes = [i, sz, u64, C.POINTER(C.c_int)]
    L.uaes_debug_gcm_stream_tables.argtypes = [vp]
    L.uaes_debug_gcm_stream_tables.restype = C.c_uint
    for n in ("uaes_ff1_encrypt", "uaes_ff1_decrypt"):
        getattr(L, n).argtypes = [i, vp, C.c_uint, vp, vp, sz, vp, sz, vp]
    for n in ("uaes_ff1_encrypt_batch", "uaes_ff1_decrypt_batch"):
        getattr(L, n).argtypes = [i, vp, C.c_uint, vp, vp, sz, sz, sz, sz, vp, vp, vp]
    L.uaes_debug_plan_ff1.argtypes = [i, C.c_uint, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_ff1.restype = C.c_char_p
    L.uaes_ff3_maxlen.argtypes = [C.c_uint]
    L.uaes_ff3_maxlen.restype = sz
    for n in ("uaes_ff3_encrypt", "uaes_ff3_decrypt"):
        getattr(L, n).argtypes = [i, vp, C.c_uint, vp, vp, vp, sz, vp]
    for n in ("uaes_ff3_encrypt_batch", "uaes_ff3_decrypt_batch"):
        getattr(L, n).argtypes = [i, vp, C.c_uint, vp, vp, sz, sz, sz, vp, vp, vp]
    L.uaes_debug_plan_ff3.argtypes = [i, C.c_uint, sz, sz, C.POINTER(C.c_int)]
    L.uaes_debug_plan_ff3.restype = C.c_char_p
    for n in ("uaes_cbc_encrypt", "uaes_cbc_decrypt", "uaes_cbc_decrypt_blocks", "uaes_cfb_encrypt", "uaes_cfb_decrypt", "uaes_ofb_xcrypt"):
        getattr(L, n).argtypes = [i, vp, vp, vp, sz, vp]
    for n in ("uaes_ccm_encrypt", "uaes_ccm_decrypt", "uaes_gcmsiv_encrypt", "uaes_gcmsiv_decrypt",
              "uaes_ocb_encrypt", "uaes_ocb_decrypt"):
        getattr(L, n).argtypes = [i, vp, vp, vp, sz, vp, sz, vp]
    L.uaes_mgpu_ctr_xcrypt_at.argtypes = [i, C.POINTER(C.c_int), i, vp, vp, u64, vp, sz, vp]
    L.uaes_mgpu_xts_sectors.argtypes = [i, C.POINTER(C.c_int), i, vp, u64, sz, sz, vp, vp, i]
    L.uaes_mgpu_ctr_encrypt_gather.argtypes = [i, C.POINTER(C.c_int), i, vp, vp, u64, C.POINTER(vp), sz, C.POINTER(vp), i, vp]
    if hasattr(L, "uaes_debug_gcm_look"):              # (an older build loaded for an A/B run has no test hooks)
        L.uaes_debug_gather_stats.argtypes = [C.POINTER(C.c_ulong)]
        L.uaes_debug_gather_stats.restype = None
        L.uaes_debug_gcm_look.argtypes = [C.c_ulonglong]
        L.uaes_debug_gcm_look.restype = None
        L.uaes_debug_gcm_chunk_folds.argtypes = [C.POINTER(C.c_uint)]
    if hasattr(L, "uaes_debug_plan"):
        L.uaes_debug_plan.argtypes = [i, i, sz, sz, C.c_uint, C.POINTER(C.c_int)]
        L.uaes_debug_arrangement_name.argtypes = [i]
        L.uaes_debug_arrangement_name.restype = C.c_char_p
        L.uaes_debug_plan_disable.argtypes = [C.c_uint]
        L.uaes_debug_plan_disable.restype = None
    if hasattr(L, "uaes_debug_live_key_schedules"):
        L.uaes_debug_live_key_schedules.argtypes = []
    if hasattr(L, "uaes_debug_plan_at"):
        L.uaes_debug_plan_at.argtypes = [i, i, sz, sz, C.c_uint, vp, C.POINTER(C.c_int)]
    L.uaes_mgpu_ecb_encrypt.argtypes = [i, C.POINTER(C.c_int), i, vp, i, vp, sz, vp]
    L.uaes_mgpu_ecb_decrypt.argtypes = [i, C.POINTER(C.c_int), i, vp, vp, sz, vp]
    for n in ("uaes_mgpu_gcm_encrypt", "uaes_mgpu_gcm_decrypt"):
        getattr(L, n).argtypes = [i, C.POINTER(C.c_int), i, vp, vp, vp, sz, vp, sz, vp]
    L.uaes_set_devices.argtypes = [i, C.POINTER(C.c_int), sz]
    L.uaes_set_host_policy.argtypes = [sz, i, i]
    L.uaes_get_host_policy.argtypes = [C.POINTER(sz), C.POINTER(i), C.POINTER(i)]
    L.uaes_set_producer_stream.argtypes = [vp]
    L.uaes_gcm_key_new.argtypes = [C.POINTER(vp), i, vp]
    L.uaes_gcm_key_free.argtypes = [vp]
    L.uaes_gcm_key_free.restype = None
    L.uaes_gcm_key_encrypt.argtypes = [vp, vp, vp, sz, vp, sz, vp]
    L.uaes_gcm_key_decrypt.argtypes = [vp, vp, vp, sz, vp, sz, vp]
    L.uaes_gcm_key_encrypt_dev.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp]
    L.uaes_gcm_key_decrypt_dev.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, vp]
    L.uaes_gcm_record_max.argtypes = [sz]
    L.uaes_gcm_record_max.restype = sz
    L.uaes_gcm_key_encrypt_records.argtypes = [vp, sz, vp, vp, sz, sz, vp, sz, sz, vp, sz]
    L.uaes_gcm_key_decrypt_records.argtypes = [vp, sz, vp, vp, sz, sz, vp, sz, sz, vp, sz, vp]
    L.uaes_gcm_key_encrypt_records_dev.argtypes = [vp, sz, vp, vp, sz, sz, vp, sz, sz, vp, sz, vp]
    L.uaes_gcm_key_decrypt_records_dev.argtypes = [vp, sz, vp, vp, sz, sz, vp, sz, sz, vp, sz, vp, vp, vp]
    L.uaes_gcm_key_encrypt_records_v.argtypes = [vp, sz, vp, vp, sz, sz, vp, vp, sz, sz, vp, sz]
    L.uaes_gcm_key_decrypt_records_v.argtypes = [vp, sz, vp, vp, sz, sz, vp, vp, sz, sz, vp, sz, vp]
    L.uaes_gcm_key_encrypt_records_v_dev.argtypes = [vp, sz, vp, vp, sz, sz, vp, vp, sz, sz, vp, sz, vp]
    L.uaes_gcm_key_decrypt_records_v_dev.argtypes = [vp, sz, vp, vp, sz, sz, vp, vp, sz, sz, vp, sz, vp, vp, vp]
    L.uaes_gcm_stream_begin.argtypes = [C.POINTER(vp), i, vp, vp, vp, sz, i]
    L.uaes_gcm_stream_update.argtypes = [vp, vp, sz, vp]
    L.uaes_gcm_stream_finish.argtypes = [vp, vp]
    L.uaes_gcm_stream_abort.argtypes = [vp]
    L.uaes_gcm_stream_abort.restype = None
    L.uaes_ocb_dev.argtypes = [i, vp, vp, i, vp, sz, vp, sz, vp, vp, vp]
    L.uaes_ecb_dev.argtypes = [i, vp, i, vp, sz, vp, vp]
    L.uaes_ctr_xcrypt_at_dev.argtypes = [i, vp, vp, u64, vp, sz, vp, vp]
    L.uaes_xts_sectors_dev.argtypes = [i, vp, u64, sz, sz, vp, vp, i, vp]
    L.uaes_gcm_encrypt_dev.argtypes = [i, vp, vp, vp, sz, vp, sz, vp, vp]
    L.uaes_gcm_decrypt_dev.argtypes = [i, vp, vp, vp, sz, vp, sz, vp, vp, vp]
    L.uaes_gcm_partial_dev.argtypes = [i, vp, vp, vp, u64, vp, sz, u64, u64, vp, vp]
    L.uaes_gcm_shard_dev.argtypes = [i, vp, vp, i, vp, u64, vp, sz, u64, u64, vp, vp, vp]
    L.uaes_expand_key.argtypes = [i, vp, vp, vp]
    for n in EXPORTS:
        if n.startswith("uaes_debug_") and not hasattr(L, n):
            continue
        if n not in ("uaes_last_error", "uaes_version", "uaes_gcm_key_free", "uaes_gcm_stream_abort", "uaes_debug_gather_stats", "uaes_debug_gcm_look",
                     "uaes_debug_arrangement_name", "uaes_debug_plan_disable", "uaes_debug_plan_poly1305",
                     "uaes_debug_plan_eax_siv", "uaes_debug_plan_chain", "uaes_debug_plan_kw", "uaes_debug_plan_kwp", "uaes_debug_plan_ff1",
                     "uaes_debug_plan_ff3", "uaes_ff3_maxlen", "uaes_debug_plan_gcmsiv_batch", "uaes_debug_plan_ocb", "uaes_debug_plan_xts",
                     "uaes_debug_gcm_stream_tables", "uaes_debug_plan_ocb_batch", "uaes_debug_plan_gcm_multikey_batch", "uaes_debug_plan_cipher_batch",
                     "uaes_debug_plan_xaes256gcm_batch", "uaes_debug_plan_xts_batch", "uaes_debug_plan_siv_v", "uaes_debug_plan_eaxp"):
            getattr(L, n).restype = i
    _lib = L
    return L


def _check(rc, what):
    if rc < 0:
        raise EngineError("%s failed (%d): %s" % (what, rc, engine().uaes_last_error().decode()))
    return rc


def _in(b):
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def _fixed(b, n, what):
    """a fixed-size argument (iv, nonce, tweak, counter block): the C side copies exactly n bytes"""
    b = bytes(b)
    if len(b) != n:
        raise ValueError("%s must be exactly %d bytes (got %d)" % (what, n, len(b)))
    return (C.c_uint8 * n).from_buffer_copy(b)


def _fixed_bytes(b, n):
    b = bytes(b)
    if len(b) != n:
        raise ValueError("expected exactly %d bytes (got %d)" % (n, len(b)))
    return b


def _out(n, fill=0):
    buf = (C.c_uint8 * max(n, 1))()
    if fill:
        C.memset(buf, fill, max(n, 1))
    return buf


def _split(buf, size, n):
    """the n records of `size` bytes a batch call left back to back in buf"""
    return [buf[i * size:(i + 1) * size] for i in range(n)]


def _bits(key, mult=1):
    bits = len(key) * 8 // mult
    if bits not in (128, 192, 256):
        raise ValueError("key must be %s bytes" % "/".join(str(mult * k) for k in (16, 24, 32)))
    return bits


# ---------------------------------------------------------------------------
# host-buffer API: same names and argument meaning as the reference
# ---------------------------------------------------------------------------
def AES_ECB_encrypt(key, pntxt, padding=0):
    """micro_aes.c:636.  padding = the reference's AES_PADDING (micro_aes.h:79): 0 returns
    ceil(len/16)*16 bytes (zero padded tail), 1 (PKCS#7) / 2 (ISO 7816-4) always add a block."""
    if padding not in (0, 1, 2):
        raise ValueError("padding must be 0, 1 or 2")
    n = (len(pntxt) // 16 + 1) * 16 if padding else (len(pntxt) + 15) // 16 * 16
    o = _out(n)
    _check(engine().uaes_ecb_encrypt_padded(_bits(key), _in(key), padding, _in(pntxt), len(pntxt), o),
           "AES_ECB_encrypt")
    return bytes(o)[:n]


def AES_ECB_decrypt(key, crtxt):
    """micro_aes.c:663.  Returns (code, plaintext); code 0x1D on a ragged length."""
    o = _out(len(crtxt))
    rc = _check(engine().uaes_ecb_decrypt(_bits(key), _in(key), _in(crtxt), len(crtxt), o), "AES_ECB_decrypt")
    return rc, bytes(o)[: len(crtxt)]


def AES_CTR_encrypt(key, iv, pntxt, iv_length=12, start_value=1):
    """micro_aes.c:962.  iv: 12 bytes; counter block = iv || 00000001.  iv_length / start_value = the reference's
    compile-time CTR_IV_LENGTH (<= 16) / CTR_START_VALUE (micro_aes.h:98-99; 12 / 1 = the default build)."""
    o = _out(len(pntxt))
    if not 0 <= iv_length <= 16 or not 0 <= start_value < 1 << 64:
        raise ValueError("iv_length: 0..16; start_value: a 64-bit unsigned integer")
    if iv_length == 12 and start_value == 1:
        _check(engine().uaes_ctr_xcrypt(_bits(key), _in(key), _fixed(iv, 12, "iv"), _in(pntxt), len(pntxt), o), "AES_CTR_encrypt")
    else:
        _check(engine().uaes_ctr_xcrypt_iv(_bits(key), _in(key), _fixed(iv, iv_length, "iv"), iv_length, start_value,
                                           _in(pntxt), len(pntxt), o), "AES_CTR_encrypt")
    return bytes(o)[: len(pntxt)]


AES_CTR_decrypt = AES_CTR_encrypt            # micro_aes.c:986-990


def ctr_xcrypt_at(key, ctr0, block_offset, data):
    """Sharding extension: explicit 16-byte counter block + 56-bit block offset."""
    o = _out(len(data))
    _check(engine().uaes_ctr_xcrypt_at(_bits(key), _in(key), _fixed(ctr0, 16, "ctr0"), block_offset, _in(data), len(data), o),
           "uaes_ctr_xcrypt_at")
    return bytes(o)[: len(data)]


def _xts(fn, name, keys, tweak, data, prefill):
    o = _out(len(data), prefill)
    rc = _check(fn(_bits(keys, 2), _in(keys), None if tweak is None else _fixed(tweak, 16, "tweak"), _in(data), len(data), o), name)
    return rc, bytes(o)[: len(data)]


def AES_XTS_encrypt(keys, tweak, pntxt, prefill=0):
    """micro_aes.c:1066.  Returns (code, ciphertext); code 1 if len < 16 (output untouched)."""
    return _xts(engine().uaes_xts_encrypt, "AES_XTS_encrypt", keys, tweak, pntxt, prefill)


def AES_XTS_decrypt(keys, tweak, crtxt, prefill=0):
    """micro_aes.c:1085."""
    return _xts(engine().uaes_xts_decrypt, "AES_XTS_decrypt", keys, tweak, crtxt, prefill)


def xts_sectors(keys, first_sector, sector_bytes, data, encrypt=True):
    """Batch extension: data unit i has tweak LE128(first_sector + i)."""
    assert sector_bytes > 0 and len(data) % sector_bytes == 0
    o = _out(len(data))
    rc = _check(engine().uaes_xts_sectors(_bits(keys, 2), _in(keys), first_sector, sector_bytes,
                                          len(data) // sector_bytes, _in(data), o, 1 if encrypt else 0),
                "uaes_xts_sectors")
    return rc, bytes(o)[: len(data)]


def xts_batch(keys, tweaks, units, decrypt=False):
    """XTS of many data units, a 16-byte tweak each, one launch: == [AES_XTS_encrypt(keys, tw, u)[1] for tw, u in ...]
    (decrypt: AES_XTS_decrypt).  The units may differ in length: they travel in slots of the longest one, with their
    lengths as the call's `lens`.  Returns (code, units); code 1 if a unit is below 16 bytes -- that unit comes back as
    zeros of its length, every other one is done."""
    n = len(units)
    if len(tweaks) != n or any(len(t) != 16 for t in tweaks):
        raise ValueError("one 16-byte tweak per unit")
    if n == 0:
        return 0, []
    sizes = [len(u) for u in units]
    size = max(sizes)
    lens = (C.c_uint32 * n)(*sizes) if min(sizes) != size else None
    packed = b"".join(bytes(u) + bytes(size - len(u)) for u in units)
    o = _out(n * size)
    name = "uaes_xts_decrypt_batch" if decrypt else "uaes_xts_encrypt_batch"
    rc = _check(getattr(engine(), name)(_bits(keys, 2), _in(keys), _in(b"".join(bytes(t) for t in tweaks)), n, size, lens,
                                        _in(packed), o), name)
    raw = bytes(o)
    return rc, [raw[m * size: m * size + sizes[m]] for m in range(n)]


def xts_sector_list(keys, sectors, sector_bytes, data, encrypt=True):
    """The storage form of xts_batch: unit m of `data` (sector_bytes each) has the tweak LE128(sectors[m]); the sectors
    come in any order and may repeat.  Returns (code, output); code 1 if sector_bytes < 16 (output untouched)."""
    n = len(sectors)
    if sector_bytes <= 0 or len(data) != n * sector_bytes:
        raise ValueError("data must hold one unit of sector_bytes per sector")
    if n == 0:
        return 0, b""
    o = _out(len(data))
    rc = _check(engine().uaes_xts_sector_list(_bits(keys, 2), _in(keys), (C.c_uint64 * n)(*sectors), n, sector_bytes,
                                              _in(data), o, 1 if encrypt else 0), "uaes_xts_sector_list")
    return rc, bytes(o)[: len(data)]


def xts_batch_plan(nmsg, length=16):
    """What an XTS batch or sector list of nmsg units of `length` bytes would run (uaes_debug_plan_xts_batch):
    (arrangement, launches, workgroups, threads per workgroup), or None for a length XTS does not have."""
    out = (C.c_int * 4)()
    name = engine().uaes_debug_plan_xts_batch(length, nmsg, out)
    return None if name is None else (name.decode(), out[0], out[1], out[2])


def _taglen(tag_len, lo, hi, even, what):
    if not (lo <= tag_len <= hi) or (even and tag_len % 2):
        raise ValueError("%s tag length %d (%s%d..%d)" % (what, tag_len, "even, " if even else "", lo, hi))
    return tag_len


def AES_GCM_encrypt(key, nonce, aData, pntxt, tag_len=16):
    """micro_aes.c:1164.  Returns ciphertext || tag.  len(nonce) / tag_len are the reference's GCM_NONCE_LEN /
    GCM_TAG_LEN: 12 / 16 by default, any other nonce length >= 1 derives J0 = GHASH(nonce) (:1145-1149)."""
    if len(nonce) < 1:
        raise ValueError("empty nonce")
    _taglen(tag_len, 1, 16, False, "GCM")
    o = _out(len(pntxt) + 16)
    _check(engine().uaes_gcm_encrypt_ex(_bits(key), _in(key), _in(nonce), len(nonce), tag_len, _in(aData), len(aData),
                                        _in(pntxt), len(pntxt), o), "AES_GCM_encrypt")
    return bytes(o)[: len(pntxt) + tag_len]


def AES_GCM_decrypt(key, nonce, aData, crtxt_and_tag, prefill=0, tag_len=16):
    """micro_aes.c:1192.  Returns (code, plaintext); code 0x1A and an untouched
    (prefilled) buffer when authentication fails."""
    _taglen(tag_len, 1, 16, False, "GCM")
    n = len(crtxt_and_tag) - tag_len
    o = _out(n, prefill)
    if len(nonce) < 1:
        raise ValueError("empty nonce")
    rc = _check(engine().uaes_gcm_decrypt_ex(_bits(key), _in(key), _in(nonce), len(nonce), tag_len, _in(aData), len(aData),
                                             _in(crtxt_and_tag), n, o), "AES_GCM_decrypt")
    return rc, bytes(o)[:n]


def _fb(fn, name, key, iVec, data, prefill=0):
    o = _out(len(data), prefill)
    rc = _check(fn(_bits(key), _in(key), _fixed(iVec, 16, "iVec"), _in(data), len(data), o), name)
    return rc, bytes(o)[: len(data)]


def AES_CBC_encrypt(key, iVec, pntxt, prefill=0, cts=True, padding=0):
    """micro_aes.c:697 (CS3 ciphertext stealing).  Returns (code, ciphertext); code 1 if len < 16.
    cts=False: a build with CTS 0 (micro_aes.h:56) -- no stealing, any length, the last chunk padded like ECB's
    with padding = AES_PADDING (micro_aes.c:727-733): 16 * (len // 16 + (len % 16 or padding != 0)) bytes."""
    if cts:
        return _fb(engine().uaes_cbc_encrypt, "AES_CBC_encrypt", key, iVec, pntxt, prefill)
    if padding not in (0, 1, 2):
        raise ValueError("padding must be 0, 1 or 2")
    n = len(pntxt) // 16 * 16 + (16 if (len(pntxt) % 16 or padding) else 0)
    o = _out(n, prefill)
    rc = _check(engine().uaes_cbc_encrypt_padded(_bits(key), _in(key), _fixed(iVec, 16, "iVec"), padding,
                                                 _in(pntxt), len(pntxt), o), "AES_CBC_encrypt")
    return rc, bytes(o)[:n]


def AES_CBC_decrypt(key, iVec, crtxt, prefill=0, cts=True):
    """micro_aes.c:746.  cts=False: the CTS 0 build -- whole blocks only (code 1 otherwise, :761), padding left in place."""
    return _fb(engine().uaes_cbc_decrypt if cts else engine().uaes_cbc_decrypt_blocks, "AES_CBC_decrypt", key, iVec, crtxt, prefill)


def cbc_encrypt_batch(key, ivs, messages):
    """Independent CBC chains, one GPU lane each: == [AES_CBC_encrypt(key, iv, m)[1] for iv, m in ...]."""
    n = len(messages)
    if n == 0:
        return []
    size = len(messages[0])
    if any(len(m) != size for m in messages) or len(ivs) != n or any(len(v) != 16 for v in ivs):
        raise ValueError("equal-sized messages and one 16-byte IV per message")
    o = _out(n * size)
    _check(engine().uaes_cbc_encrypt_batch(_bits(key), _in(key), _in(b"".join(ivs)), n, size,
                                           _in(b"".join(messages)), o), "uaes_cbc_encrypt_batch")
    raw = bytes(o)
    return _split(raw, size, n)


CIPHER_BATCH_MODES = ("cbc_decrypt", "cbc_decrypt_blocks", "cbc_encrypt_blocks", "cfb_encrypt", "cfb_decrypt", "ofb", "ctr")


def _cipher_batch(name, key, ivs, records, ragged):
    """What the cipher batches share (uaes_cbc_*_batch, uaes_cfb_*_batch, uaes_ofb_xcrypt_batch, uaes_ctr_xcrypt_batch):
    one 16-byte IV (CTR: first counter block) per record, the records packed into slots of the longest one, the call and
    the split.  ragged: the call takes `lens`, and records of different lengths become it; else they must be equal."""
    n = len(records)
    if len(ivs) != n or any(len(v) != 16 for v in ivs):
        raise ValueError("one 16-byte IV per record")
    if n == 0:
        return []
    sizes = [len(r) for r in records]
    size = max(sizes)
    if not ragged and min(sizes) != size:
        raise ValueError("equal-sized messages")
    lens = (C.c_uint32 * n)(*sizes) if min(sizes) != size else None
    packed = b"".join(bytes(r) + bytes(size - len(r)) for r in records)
    o = _out(n * size)
    args = (_bits(key), _in(key), _in(b"".join(bytes(v) for v in ivs)), n, size) + ((lens,) if ragged else ()) + (_in(packed), o)
    _check(getattr(engine(), name)(*args), name)
    raw = bytes(o)
    return [raw[m * size: m * size + sizes[m]] for m in range(n)]


def cbc_decrypt_batch(key, ivs, messages):
    """The inverse of cbc_encrypt_batch, CS3 swap included: == [AES_CBC_decrypt(key, iv, m)[1] for iv, m in ...]."""
    return _cipher_batch("uaes_cbc_decrypt_batch", key, ivs, messages, False)


def cbc_blocks_batch(key, ivs, messages, decrypt=False):
    """Ordinary CBC over whole blocks, no swap: == [AES_CBC_encrypt(key, iv, m, cts=False)[1] ...], or with decrypt
    [AES_CBC_decrypt(key, iv, m, cts=False)[1] ...]."""
    return _cipher_batch("uaes_cbc_decrypt_blocks_batch" if decrypt else "uaes_cbc_encrypt_blocks_batch", key, ivs, messages, False)


def cfb_batch(key, ivs, messages, decrypt=False):
    """CFB of many records, an IV each: == [AES_CFB_encrypt(key, iv, m) ...] (decrypt: AES_CFB_decrypt).  The records
    may differ in length: they travel in slots of the longest one, with their lengths as the call's `lens`."""
    return _cipher_batch("uaes_cfb_decrypt_batch" if decrypt else "uaes_cfb_encrypt_batch", key, ivs, messages, True)


def ofb_batch(key, ivs, messages):
    """OFB of many records, an IV each: == [AES_OFB_encrypt(key, iv, m) ...]; lengths as in cfb_batch."""
    return _cipher_batch("uaes_ofb_xcrypt_batch", key, ivs, messages, True)


def ctr_batch(key, ctrs, messages):
    """CTR of many records, a 16-byte first counter block each: == [ctr_xcrypt_at(key, ctr0, 0, m) ...]; lengths as in
    cfb_batch."""
    return _cipher_batch("uaes_ctr_xcrypt_batch", key, ctrs, messages, True)


def cipher_batch_plan(nmsg, mode="ctr", length=16):
    """What a cipher batch of nmsg records of `length` bytes would run (uaes_debug_plan_cipher_batch): (arrangement,
    launches, workgroups, threads per workgroup), or None for arguments that make no sense.  mode: a name from
    CIPHER_BATCH_MODES or its number."""
    return _batch_plan("uaes_debug_plan_cipher_batch", CIPHER_BATCH_MODES.index(mode) if isinstance(mode, str) else int(mode),
                       length, nmsg)


def cmac_batch(key, messages):
    """Independent CMACs, one GPU lane each: == [AES_CMAC(key, m) for m in messages]."""
    n = len(messages)
    if n == 0:
        return []
    size = len(messages[0])
    if any(len(m) != size for m in messages):
        raise ValueError("equal-sized messages")
    o = _out(n * 16)
    _check(engine().uaes_cmac_batch(_bits(key), _in(key), n, size, _in(b"".join(messages)), o), "uaes_cmac_batch")
    raw = bytes(o)
    return _split(raw, 16, n)


def AES_CFB_encrypt(key, iVec, pntxt):
    """micro_aes.c:825."""
    return _fb(engine().uaes_cfb_encrypt, "AES_CFB_encrypt", key, iVec, pntxt)[1]


def AES_CFB_decrypt(key, iVec, crtxt):
    """micro_aes.c:839."""
    return _fb(engine().uaes_cfb_decrypt, "AES_CFB_decrypt", key, iVec, crtxt)[1]


def AES_OFB_encrypt(key, iVec, data):
    """micro_aes.c:861; decrypt is the same function (:887)."""
    return _fb(engine().uaes_ofb_xcrypt, "AES_OFB_encrypt", key, iVec, data)[1]


AES_OFB_decrypt = AES_OFB_encrypt


def AES_CMAC(key, data):
    """micro_aes.c:1108.  Returns the 16-byte CMAC."""
    o = _out(16)
    _check(engine().uaes_cmac(_bits(key), _in(key), _in(data), len(data), o), "AES_CMAC")
    return bytes(o)


def _poly_bits(keys):
    bits = (len(keys) - 16) * 8
    if bits not in (128, 192, 256):
        raise ValueError("keys = k || r: 32, 40 or 48 bytes (got %d)" % len(keys))
    return bits


def AES_Poly1305(keys, nonce, data):
    """micro_aes.c:1955.  keys = k || r (key size from len(keys) - 16); returns the 16-byte mac."""
    o = _out(16)
    _check(engine().uaes_poly1305(_poly_bits(keys), _in(keys), _fixed(nonce, 16, "nonce"), _in(data), len(data), o),
           "AES_Poly1305")
    return bytes(o)


def poly1305_batch(keys, nonces, messages):
    """One key pair, a nonce per message, equal-sized messages, one GPU wave each: == [AES_Poly1305(keys, n, m)]."""
    n = len(messages)
    if len(nonces) != n:
        raise ValueError("one nonce per message")
    if n == 0:
        return []
    size = len(messages[0])
    if any(len(m) != size for m in messages):
        raise ValueError("equal-sized messages")
    if any(len(x) != 16 for x in nonces):
        raise ValueError("16-byte nonces")
    o = _out(n * 16)
    _check(engine().uaes_poly1305_batch(_poly_bits(keys), _in(keys), _in(b"".join(nonces)), n, size,
                                        _in(b"".join(messages)), o), "uaes_poly1305_batch")
    raw = bytes(o)
    return _split(raw, 16, n)


def poly1305_plan(len, nmsg=1):
    """What a Poly1305 call would run (uaes_debug_plan_poly1305): (arrangement, launches, workgroups, blocks per thread)."""
    out = (C.c_int * 3)()
    name = engine().uaes_debug_plan_poly1305(len, nmsg, out)
    return name.decode(), out[0], out[1], out[2]


def AES_EAX_encrypt(key, nonce, aData, pntxt, tag_len=16):
    """micro_aes.c:1560.  Any nonce length (the reference's EAX_NONCE_LEN, 16 by default), tag_len = EAX_TAG_LEN
    (1..16); returns ciphertext || tag."""
    _taglen(tag_len, 1, 16, False, "EAX")
    o = _out(len(pntxt) + 16)
    _check(engine().uaes_eax_encrypt(_bits(key), _in(key), _in(nonce), len(nonce), tag_len, _in(aData), len(aData),
                                     _in(pntxt), len(pntxt), o), "AES_EAX_encrypt")
    return bytes(o)[: len(pntxt) + tag_len]


def AES_EAX_decrypt(key, nonce, aData, crtxt_and_tag, prefill=0, tag_len=16):
    """micro_aes.c:1613.  Returns (code, text); the tag is checked first, so on 0x1A the text is the untouched
    prefill."""
    _taglen(tag_len, 1, 16, False, "EAX")
    n = len(crtxt_and_tag) - tag_len
    if n < 0:
        raise ValueError("shorter than the tag")
    o = _out(n, prefill)
    rc = _check(engine().uaes_eax_decrypt(_bits(key), _in(key), _in(nonce), len(nonce), tag_len, _in(aData), len(aData),
                                          _in(crtxt_and_tag), n, o), "AES_EAX_decrypt")
    return rc, bytes(o)[:n]


def AES_SIV_encrypt(keys, aData, pntxt):
    """micro_aes.c:1373 (RFC 5297).  keys = K_s2v || K_ctr (32, 48 or 64 bytes); returns (iv, ciphertext)."""
    iv, o = _out(16), _out(len(pntxt))
    _check(engine().uaes_siv_encrypt(_bits(keys, 2), _in(keys), _in(aData), len(aData), _in(pntxt), len(pntxt), iv, o),
           "AES_SIV_encrypt")
    return bytes(iv), bytes(o)[: len(pntxt)]


def AES_SIV_decrypt(keys, iv, aData, crtxt, prefill=0):
    """micro_aes.c:1394.  Returns (code, text); on 0x1A the text is the decryption (zeros under the wipe switch)."""
    o = _out(len(crtxt), prefill)
    rc = _check(engine().uaes_siv_decrypt(_bits(keys, 2), _in(keys), _fixed(iv, 16, "iv"), _in(aData), len(aData),
                                          _in(crtxt), len(crtxt), o), "AES_SIV_decrypt")
    return rc, bytes(o)[: len(crtxt)]


def _ad_vector(ads):
    """a list of components as the _v calls take it: (nad, adLens or None, the components back to back)"""
    ads = [bytes(a) for a in ads]
    return len(ads), ((C.c_size_t * len(ads))(*[len(a) for a in ads]) if ads else None), _in(b"".join(ads))


def AES_SIV_encrypt_v(keys, ads, pntxt):
    """SIV with RFC 5297's vector of associated data (uaes_siv_encrypt_v): ads = a list of bytes, an empty one still a
    component, the nonce of nonce-based SIV the last one.  Returns (iv, ciphertext)."""
    iv, o = _out(16), _out(len(pntxt))
    _check(engine().uaes_siv_encrypt_v(_bits(keys, 2), _in(keys), *_ad_vector(ads), _in(pntxt), len(pntxt), iv, o),
           "AES_SIV_encrypt_v")
    return bytes(iv), bytes(o)[: len(pntxt)]


def AES_SIV_decrypt_v(keys, iv, ads, crtxt, prefill=0):
    """uaes_siv_decrypt_v.  Returns (code, text); on 0x1A the text is the decryption (zeros under the wipe switch)."""
    o = _out(len(crtxt), prefill)
    rc = _check(engine().uaes_siv_decrypt_v(_bits(keys, 2), _in(keys), _fixed(iv, 16, "iv"), *_ad_vector(ads),
                                            _in(crtxt), len(crtxt), o), "AES_SIV_decrypt_v")
    return rc, bytes(o)[: len(crtxt)]


def _records(items, what):
    n = len(items)
    size = len(items[0]) if n else 0
    if any(len(x) != size for x in items):
        raise ValueError("equal-sized %s" % what)
    return size, b"".join(bytes(x) for x in items)


def _aead_batch(fn, what, per_record, aads, texts, lens, decrypt, tags, tag_len, prefill, head, tags_first=False):
    """What the AEAD record batches share (eax_batch, ccm_batch, gcmsiv_batch, gcm_multikey_batch, ocb_batch, siv_batch):
    one item per record in every list, the packing, the buffers, the uaes_<fn>_encrypt_batch / _decrypt_batch call and
    the split.  per_record: the mode's own lists (AADs, tags and lens are everybody's); head(n, ml, lv): the mode's own
    checks, then the call's arguments before the AAD; tags_first: SIV's IVs stand before the text, in the call and in
    what an encryption returns.  Returns (texts, tags), or (code, texts, verdicts) for a decryption."""
    n = len(texts)
    aads = aads if aads is not None else [b""] * n
    if any(len(x) != n for x in per_record + [aads]) or (decrypt and (tags is None or len(tags) != n)) or \
            (lens is not None and len(lens) != n):
        raise ValueError("one %s per record" % what)
    if n == 0:
        return (0, [], []) if decrypt else ([], [])
    al, ab = _records(aads, "AADs")
    ml, mb = _records(texts, "texts")
    lv = (C.c_uint32 * n)(*lens) if lens is not None else None
    name = "uaes_%s_%s_batch" % (fn, "decrypt" if decrypt else "encrypt")
    call = getattr(engine(), name)
    a = tuple(head(n, ml, lv)) + (_in(ab), al)
    o = _out(n * ml, prefill)
    if not decrypt:
        t = _out(n * tag_len)
        _check(call(*a, _in(mb), *((t, o) if tags_first else (o, t))), name)
        out, tr = _split(bytes(o), ml, n), _split(bytes(t), tag_len, n)
        return (tr, out) if tags_first else (out, tr)
    v, t = _out(n), _in(b"".join(tags))
    rc = _check(call(*a, *((t, _in(mb)) if tags_first else (_in(mb), t)), o, v), name)
    return rc, _split(bytes(o), ml, n), list(bytes(v)[:n])


def _batch_plan(hook, direction, length, nmsg):
    """(arrangement, launches, workgroups, threads per workgroup) from a row batch's plan hook, or None"""
    out = (C.c_int * 3)()
    name = getattr(engine(), hook)(direction, length, nmsg, out)
    return None if name is None else (name.decode(), out[0], out[1], out[2])


def _nonce_tag_batch(fn, key, nonces, aads, texts, tag_len, decrypt, tags, prefill, lens):
    """ccm_batch and ocb_batch: the nonce and tag lengths are arguments of the call"""
    def head(n, ml, lv):
        nl, nb = _records(nonces, "nonces")
        if decrypt and any(len(x) != tag_len for x in tags):
            raise ValueError("tags of tag_len bytes")
        return _bits(key), _in(key), nl, tag_len, n, ml, lv, _in(nb)
    return _aead_batch(fn, "nonce, AAD (tag and length)", [nonces], aads, texts, lens, decrypt, tags, tag_len, prefill, head)


def eax_batch(key, nonces, aads, texts, decrypt=False, tags=None, prefill=0):
    """EAX of many records under one key (uaes_eax_*_batch): equal-sized nonces, AADs (or None) and texts.
    encrypt: returns (ciphertexts, 16-byte tags); decrypt (tags given): returns (code, plaintexts, verdicts), a
    forged record's plaintext stays the prefill."""
    def head(n, ml, lv):
        nl, nb = _records(nonces, "nonces")
        return _bits(key), _in(key), n, ml, _in(nb), nl
    return _aead_batch("eax", "nonce, AAD (and tag)", [nonces], aads, texts, None, decrypt, tags, 16, prefill, head)


def eaxp_encrypt(key, nonce, pntxt):
    """EAX' (ANSI C12.22 / IEEE 1703; micro_aes.c:1563 built with EAXP 1).  Any nonce length, no associated data;
    returns ciphertext || 4-byte mac."""
    o = _out(len(pntxt) + 4)
    _check(engine().uaes_eaxp_encrypt(_bits(key), _in(key), _in(nonce), len(nonce), _in(pntxt), len(pntxt), o), "eaxp_encrypt")
    return bytes(o)[: len(pntxt) + 4]


def eaxp_decrypt(key, nonce, crtxt_and_mac, prefill=0):
    """micro_aes.c:1611 built with EAXP 1.  Returns (code, text); the mac is checked first, so on 0x1A the text is the
    untouched prefill."""
    n = len(crtxt_and_mac) - 4
    if n < 0:
        raise ValueError("shorter than the mac")
    o = _out(n, prefill)
    rc = _check(engine().uaes_eaxp_decrypt(_bits(key), _in(key), _in(nonce), len(nonce), _in(crtxt_and_mac), n, o), "eaxp_decrypt")
    return rc, bytes(o)[:n]


def _eaxp_batch(key, nonces, texts, decrypt, macs, prefill, nlens, lens):
    n = len(texts)
    if len(nonces) != n or (decrypt and (macs is None or len(macs) != n)) or \
            any(x is not None and len(x) != n for x in (nlens, lens)):
        raise ValueError("one nonce (mac and lengths) per record")
    if n == 0:
        return (0, [], []) if decrypt else ([], [])
    nl, nb = _records(nonces, "nonce slots")
    ml, mb = _records(texts, "text slots")
    nv, lv = ((C.c_uint32 * n)(*x) if x is not None else None for x in (nlens, lens))
    a = (_bits(key), _in(key), n, nl, nv, _in(nb), ml, lv)
    o = _out(n * ml, prefill)
    if not decrypt:
        t = _out(n * 4)
        _check(engine().uaes_eaxp_encrypt_batch(*a, _in(mb), o, t), "uaes_eaxp_encrypt_batch")
        return _split(bytes(o), ml, n), _split(bytes(t), 4, n)
    if any(len(x) != 4 for x in macs):
        raise ValueError("4-byte macs")
    v = _out(n)
    rc = _check(engine().uaes_eaxp_decrypt_batch(*a, _in(mb), _in(b"".join(macs)), o, v), "uaes_eaxp_decrypt_batch")
    return rc, _split(bytes(o), ml, n), list(bytes(v)[:n])


def eaxp_encrypt_batch(key, nonces, texts, nlens=None, lens=None, prefill=0):
    """EAX' of many records under one key (uaes_eaxp_encrypt_batch): equal-sized nonce slots and text slots; nlens / lens
    (optional, one per record): record m is the first lens[m] bytes of its text under the first nlens[m] bytes of its
    nonce, and the rest of its output slot stays the prefill.  Returns (ciphertexts, 4-byte macs)."""
    return _eaxp_batch(key, nonces, texts, False, None, prefill, nlens, lens)


def eaxp_decrypt_batch(key, nonces, texts, macs, nlens=None, lens=None, prefill=0):
    """uaes_eaxp_decrypt_batch.  Returns (code, plaintexts, verdicts); a forged record's plaintext stays the prefill."""
    return _eaxp_batch(key, nonces, texts, True, macs, prefill, nlens, lens)


def ccm_batch(key, nonces, aads, texts, tag_len=16, decrypt=False, tags=None, prefill=0, lens=None):
    """CCM of many records under one key (uaes_ccm_*_batch): equal-sized nonces (7..13 bytes), AADs (or None) and
    texts.  encrypt: returns (ciphertexts, tag_len-byte tags); decrypt (tags given): returns (code, plaintexts,
    verdicts); like the reference's CCM a forged record's plaintext is what CTR made of it (zeros under
    wipe_on_auth_failure).  lens (optional, one per record): record m is the first lens[m] bytes of its text, and the
    rest of its output slot stays the prefill."""
    return _nonce_tag_batch("ccm", key, nonces, aads, texts, tag_len, decrypt, tags, prefill, lens)


def gcmsiv_batch(key, nonces, aads, texts, decrypt=False, tags=None, prefill=0, lens=None):
    """GCM-SIV (RFC 8452) of many records under one master key (uaes_gcmsiv_*_batch): 12-byte nonces, equal-sized AADs
    (or None) and texts.  encrypt: returns (ciphertexts, 16-byte tags); decrypt (tags given): returns (code, plaintexts,
    verdicts); like the reference's GCM-SIV a forged record's plaintext is what CTR made of it (zeros under
    wipe_on_auth_failure).  lens (optional, one per record): record m is the first lens[m] bytes of its text, and the
    rest of its output slot stays the prefill."""
    def head(n, ml, lv):
        if any(len(x) != 12 for x in nonces) or (decrypt and any(len(x) != 16 for x in tags)):
            raise ValueError("nonces of 12 bytes (tags of 16)")
        return _bits(key), _in(key), n, ml, lv, _in(b"".join(nonces))
    return _aead_batch("gcmsiv", "nonce, AAD (tag and length)", [nonces], aads, texts, lens, decrypt, tags, 16, prefill, head)


def gcmsiv_batch_plan(length, nmsg, decrypt=False):
    """What a GCM-SIV batch of nmsg records of `length` bytes would run (uaes_debug_plan_gcmsiv_batch): (arrangement,
    launches, workgroups, threads per workgroup), or None for arguments that make no sense."""
    return _batch_plan("uaes_debug_plan_gcmsiv_batch", int(bool(decrypt)), length, nmsg)


def gcm_multikey_batch(keys, nonces, aads, texts, decrypt=False, tags=None, tag_len=16, prefill=0, lens=None):
    """GCM of many records, each under a key of its own (uaes_gcm_multikey_*_batch): equal-sized keys (16, 24 or 32
    bytes), 12-byte nonces, equal-sized AADs (or None) and texts.  encrypt: returns (ciphertexts, tag_len-byte tags);
    decrypt (tags given): returns (code, plaintexts, verdicts); a forged record's output slot is untouched: it stays
    the prefill, whatever wipe_on_auth_failure says.  lens (optional, one per record): record m is the first lens[m]
    bytes of its text, and the rest of its output slot stays the prefill."""
    def head(n, ml, lv):
        if any(len(x) != 12 for x in nonces) or (decrypt and any(len(x) != tag_len for x in tags)):
            raise ValueError("nonces of 12 bytes (tags of tag_len)")
        kl, kb = _records(keys, "keys")
        return 8 * kl, _in(kb), tag_len, n, ml, lv, _in(b"".join(nonces))
    return _aead_batch("gcm_multikey", "key, nonce, AAD (tag and length)", [keys, nonces], aads, texts, lens, decrypt, tags, tag_len,
                       prefill, head)


def gcm_multikey_batch_plan(length, nmsg, decrypt=False):
    """What a multi-key GCM batch of nmsg records of `length` bytes would run (uaes_debug_plan_gcm_multikey_batch):
    (arrangement, launches, workgroups, threads per workgroup), or None for arguments that make no sense."""
    return _batch_plan("uaes_debug_plan_gcm_multikey_batch", int(bool(decrypt)), length, nmsg)


def xaes256gcm_derive(key, nonce):
    """The AES-256 key XAES-256-GCM (C2SP) runs GCM under for this 32-byte key and 24-byte nonce: CMAC_K(00 01 58 00 ||
    nonce[:12]) || CMAC_K(00 02 58 00 || nonce[:12]) (uaes_xaes256gcm_derive; the host cipher, no device)."""
    o = _out(32)
    _check(engine().uaes_xaes256gcm_derive(_fixed(key, 32, "key"), _fixed(nonce, 24, "nonce"), o), "xaes256gcm_derive")
    return bytes(o)


def xaes256gcm_encrypt(key, nonce, aad, pt):
    """XAES-256-GCM (c2sp.org/XAES-256-GCM): a 32-byte key, a 24-byte nonce; returns ciphertext || 16-byte tag."""
    o = _out(len(pt) + 16)
    _check(engine().uaes_xaes256gcm_encrypt(_fixed(key, 32, "key"), _fixed(nonce, 24, "nonce"), _in(aad), len(aad),
                                            _in(pt), len(pt), o), "xaes256gcm_encrypt")
    return bytes(o)[: len(pt) + 16]


def xaes256gcm_decrypt(key, nonce, aad, ct_and_tag, prefill=0):
    """Returns (code, text); the tag is checked first, so on 0x1A the text is the untouched prefill."""
    n = len(ct_and_tag) - 16
    if n < 0:
        raise ValueError("shorter than the tag")
    o = _out(n, prefill)
    rc = _check(engine().uaes_xaes256gcm_decrypt(_fixed(key, 32, "key"), _fixed(nonce, 24, "nonce"), _in(aad), len(aad),
                                                 _in(ct_and_tag), n, o), "xaes256gcm_decrypt")
    return rc, bytes(o)[:n]


def xaes256gcm_batch(key, nonces, aads, texts, decrypt=False, tags=None, prefill=0, lens=None):
    """XAES-256-GCM of many records under one 32-byte master key (uaes_xaes256gcm_*_batch): 24-byte nonces, equal-sized
    AADs (or None) and texts; every record derives the key of its nonce in the kernel.  encrypt: returns (ciphertexts,
    16-byte tags); decrypt (tags given): returns (code, plaintexts, verdicts); a forged record's output slot is
    untouched: it stays the prefill, whatever wipe_on_auth_failure says.  lens (optional, one per record): record m is the
    first lens[m] bytes of its text, and the rest of its output slot stays the prefill."""
    def head(n, ml, lv):
        if any(len(x) != 24 for x in nonces) or (decrypt and any(len(x) != 16 for x in tags)):
            raise ValueError("nonces of 24 bytes (tags of 16)")
        return _fixed(key, 32, "key"), n, ml, lv, _in(b"".join(nonces))
    return _aead_batch("xaes256gcm", "nonce, AAD (tag and length)", [nonces], aads, texts, lens, decrypt, tags, 16, prefill, head)


def xaes256gcm_batch_plan(length, nmsg, decrypt=False):
    """What an XAES-256-GCM batch of nmsg records of `length` bytes would run (uaes_debug_plan_xaes256gcm_batch):
    (arrangement, launches, workgroups, threads per workgroup), or None for arguments that make no sense."""
    return _batch_plan("uaes_debug_plan_xaes256gcm_batch", int(bool(decrypt)), length, nmsg)


def ocb_batch(key, nonces, aads, texts, tag_len=16, decrypt=False, tags=None, prefill=0, lens=None):
    """OCB (RFC 7253) of many records under one key (uaes_ocb_*_batch): equal-sized nonces (1..15 bytes), AADs (or
    None) and texts.  encrypt: returns (ciphertexts, tag_len-byte tags); decrypt (tags given): returns (code, plaintexts,
    verdicts); like the reference's OCB a forged record's plaintext is its decryption (zeros under
    wipe_on_auth_failure).  lens (optional, one per record): record m is the first lens[m] bytes of its text, and the
    rest of its output slot stays the prefill."""
    return _nonce_tag_batch("ocb", key, nonces, aads, texts, tag_len, decrypt, tags, prefill, lens)


def ocb_batch_plan(length, nmsg, decrypt=False):
    """What an OCB batch of nmsg records of `length` bytes would run (uaes_debug_plan_ocb_batch): (arrangement,
    launches, workgroups, threads per workgroup), or None for arguments that make no sense.  decrypt may also be an
    int: a direction other than 0 / 1 has no plan."""
    return _batch_plan("uaes_debug_plan_ocb_batch", int(decrypt), length, nmsg)


def siv_batch(keys, aads, texts, decrypt=False, ivs=None, prefill=0):
    """SIV (RFC 5297) of many records under one key pair (uaes_siv_*_batch): equal-sized AADs (or None) and texts.
    encrypt: returns (ivs, ciphertexts); decrypt (ivs given): returns (code, plaintexts, verdicts)."""
    def head(n, ml, lv):
        return _bits(keys, 2), _in(keys), n, ml
    return _aead_batch("siv", "AAD (and IV)", [], aads, texts, None, decrypt, ivs, 16, prefill, head, tags_first=True)


def siv_batch_v(keys, ads, texts, decrypt=False, ivs=None, prefill=0, lens=None):
    """SIV with a vector of associated data over many records under one key pair (uaes_siv_*_batch_v): ads[m] = the list
    of record m's components, the same number and the same lengths in every record; equal-sized texts.  encrypt: returns
    (ivs, ciphertexts); decrypt (ivs given): returns (code, plaintexts, verdicts).  lens (optional, one per record):
    record m is the first lens[m] bytes of its text, and the rest of its output slot stays the prefill."""
    shape = [len(a) for a in ads[0]] if len(ads) else []
    if any([len(a) for a in rec] != shape for rec in ads):
        raise ValueError("the same component lengths in every record")
    adl = (C.c_size_t * len(shape))(*shape) if shape else None

    def head(n, ml, lv):
        return _bits(keys, 2), _in(keys), n, ml, lv, len(shape), adl
    n = len(texts)
    if len(ads) != n or (decrypt and (ivs is None or len(ivs) != n)) or (lens is not None and len(lens) != n):
        raise ValueError("one component list (and IV and length) per record")
    if n == 0:
        return (0, [], []) if decrypt else ([], [])
    ml, mb = _records(texts, "texts")
    lv = (C.c_uint32 * n)(*lens) if lens is not None else None
    name = "uaes_siv_%s_batch_v" % ("decrypt" if decrypt else "encrypt")
    a = head(n, ml, lv) + (_in(b"".join(b"".join(bytes(x) for x in rec) for rec in ads)),)
    o = _out(n * ml, prefill)
    if not decrypt:
        t = _out(n * 16)
        _check(getattr(engine(), name)(*a, _in(mb), t, o), name)
        return _split(bytes(t), 16, n), _split(bytes(o), ml, n)
    v = _out(n)
    rc = _check(getattr(engine(), name)(*a, _in(b"".join(ivs)), _in(mb), o, v), name)
    return rc, _split(bytes(o), ml, n), list(bytes(v)[:n])


def siv_v_plan(length, nad, nmsg=1, decrypt=False):
    """What a SIV call with nad components of associated data would run (uaes_debug_plan_siv_v; nmsg >= 2: a batch):
    (arrangement, launches, workgroups, rows the components are dealt over), or None for arguments that make no sense.
    decrypt may also be an int: a direction other than 0 / 1 has no plan."""
    out = (C.c_int * 3)()
    name = engine().uaes_debug_plan_siv_v(int(decrypt), length, nad, nmsg, out)
    return None if name is None else (name.decode(), out[0], out[1], out[2])


def eax_siv_plan(siv, length, nmsg=1, decrypt=False):
    """What an EAX (siv=False) / SIV call would run (uaes_debug_plan_eax_siv): (arrangement, launches, workgroups,
    longest text of the small arrangement)."""
    out = (C.c_int * 3)()
    name = engine().uaes_debug_plan_eax_siv(int(bool(siv)), int(bool(decrypt)), length, nmsg, out)
    return name.decode(), out[0], out[1], out[2]


def eaxp_plan(length, nmsg=1, decrypt=False):
    """What an EAX' call would run (uaes_debug_plan_eaxp): as eax_siv_plan."""
    out = (C.c_int * 3)()
    name = engine().uaes_debug_plan_eaxp(int(bool(decrypt)), length, nmsg, out)
    return name.decode(), out[0], out[1], out[2]


CHAIN_WHAT = {"cbc": 0, "cfb": 1, "ofb": 2, "cmac": 3, "ccm": 4, "cbc_batch": 5, "cmac_batch": 6, "cbc_nocts": 7,
              "ccm_batch": 9}


def chain_plan(what, a, b=0, decrypt=False):
    """What a CBC / CFB / OFB / CMAC / CCM call or a batch of chains would run (uaes_debug_plan_chain): (arrangement,
    launches, workgroups of the main kernel, its threads per workgroup).  a = bytes of text (batches: bytes per
    message), b = messages of a batch."""
    out = (C.c_int * 3)()
    name = engine().uaes_debug_plan_chain(CHAIN_WHAT[what], int(bool(decrypt)), a, b, out)
    if name is None:
        raise ValueError("no plan for %s of %d bytes (%d messages, decrypt=%s)" % (what, a, b, bool(decrypt)))
    return name.decode(), out[0], out[1], out[2]


def _kw(pad, unwrap, kek, data, prefill):
    """The one-secret calls of key wrap and key wrap with padding: padding fills the wrapped form up to whole semiblocks,
    and its unwrap also answers the secret's length"""
    n = max(len(data) - 8, 0) if unwrap else ((len(data) + 7) // 8 * 8 if pad else len(data)) + 8
    o = _out(n, prefill)
    way = "unwrap" if unwrap else "wrap"
    ln = C.c_size_t(0)
    tail = (C.byref(ln),) if pad and unwrap else ()
    fn = getattr(engine(), "uaes_%s_%s" % ("kwp" if pad else "kw", way))
    rc = _check(fn(_bits(kek), _in(kek), _in(data), len(data), o, *tail), "uaes_kwp_" + way if pad else "AES_KEY_" + way)
    return (rc, bytes(o)[:n]) + ((ln.value,) if tail else ())


def AES_KEY_wrap(kek, secret, prefill=0):
    """micro_aes.c:1829 (RFC 3394).  Returns (code, output buffer of len(secret) + 8 bytes): code 1 for a secret that is
    no multiple of 8 bytes or shorter than 16, the buffer untouched then."""
    return _kw(False, False, kek, secret, prefill)


def AES_KEY_unwrap(kek, wrapped, prefill=0):
    """micro_aes.c:1865.  Returns (code, output buffer of len(wrapped) - 8 bytes); like the reference the unwrapped
    bytes are returned even when the code is 0x1A (zeros under the wipe switch)."""
    return _kw(False, True, kek, wrapped, prefill)


def _kw_batch(pad, kek, records, unwrap, slot, prefill):
    """The batches of key wrap and key wrap with padding.  Padding takes records of any length, each in a slot, passes a
    length per record unless every record fills its slot, and its unwrap also answers the secrets' lengths."""
    n = len(records)
    if n == 0:
        return ((0, [], [], []) if pad else (0, [], [])) if unwrap else (0, [])
    lens = None
    if pad:
        slot = max(len(r) for r in records) if slot is None else slot
        if any(len(r) > slot for r in records):
            raise ValueError("a record longer than its slot")
        if any(len(r) != slot for r in records):
            lens = (C.c_uint32 * n)(*[len(r) for r in records])
        rb = b"".join(bytes(r) + bytes(slot - len(r)) for r in records)
    else:
        slot, rb = _records(records, "records")
    whole = (lambda x: (x + 7) // 8 * 8) if pad else (lambda x: x)
    oslot = max(slot - 8, 0) if unwrap else whole(slot) + 8
    o, v, lo = _out(n * oslot, prefill), _out(n), (C.c_uint32 * n)()
    name = "uaes_%s_%s_batch" % ("kwp" if pad else "kw", "unwrap" if unwrap else "wrap")
    args = ((lens,) if pad else ()) + (_in(rb), o) + ((lo,) if pad and unwrap else ()) + ((v,) if unwrap else ())
    rc = _check(getattr(engine(), name)(_bits(kek), _in(kek), n, slot, *args), name)
    raw = bytes(o)
    outs = [raw[m * oslot:m * oslot + (max(len(r) - 8, 0) if unwrap else whole(len(r)) + 8)] for m, r in enumerate(records)]
    if not unwrap:
        return rc, outs
    return (rc, outs) + ((list(lo),) if pad else ()) + (list(bytes(v)[:n]),)


def kw_batch(kek, records, unwrap=False, prefill=0):
    """Key wrap of many equal-sized records under one key-encryption key (uaes_kw_*_batch).  wrap: returns (code, wrapped
    records); unwrap: returns (code, secrets, verdicts)."""
    return _kw_batch(False, kek, records, unwrap, None, prefill)


def _kw_plan(hook, length, nkeys, unwrap):
    out = (C.c_int * 3)()
    name = getattr(engine(), hook)(int(bool(unwrap)), length, nkeys, out)
    return None if name is None else (name.decode(), out[0], out[1], out[2])


def kw_plan(length, nkeys=0, unwrap=False):
    """What a key wrap of a secret of `length` bytes would run (uaes_debug_plan_kw; nkeys 0: the one-secret calls, else a
    batch): (arrangement, launches, workgroups, threads per workgroup), or None for arguments that make no sense."""
    return _kw_plan("uaes_debug_plan_kw", length, nkeys, unwrap)


def kwp_wrapped_len(n):
    """uaes_kwp_wrapped_len: bytes of the wrapped form of a secret of n bytes; 0 for a length KWP does not take"""
    return (n + 7) // 8 * 8 + 8 if 1 <= n <= 0xFFFFFFFF else 0


def kwp_wrap(kek, secret, prefill=0):
    """Key wrap with padding, RFC 5649 (uaes_kwp_wrap): a secret of any length from 1 byte.  Returns (code, output buffer
    of 8 * ceil(len / 8) + 8 bytes): code 1 for an empty secret, the buffer untouched then."""
    return _kw(True, False, kek, secret, prefill)


def kwp_unwrap(kek, wrapped, prefill=0):
    """uaes_kwp_unwrap.  Returns (code, output buffer of len(wrapped) - 8 bytes, length of the secret): the secret is the
    first `length` bytes of the buffer and zeros follow; code 0x1A comes with length 0 and what the chain made (zeros
    under the wipe switch), code 1 (a length that is no multiple of 8 or below 16) with the buffer untouched."""
    return _kw(True, True, kek, wrapped, prefill)


def kwp_batch(kek, records, unwrap=False, slot=None, prefill=0):
    """Key wrap with padding of many records under one key-encryption key, each with a length of its own
    (uaes_kwp_*_batch).  slot = bytes per input record slot (default: the longest record).  wrap: returns (code, wrapped
    records); unwrap: returns (code, unwrapped records of len(wrapped) - 8 bytes each, lengths of the secrets, verdicts).
    A record whose length the call refuses comes back as the prefill."""
    return _kw_batch(True, kek, records, unwrap, slot, prefill)


def kwp_plan(length, nkeys=0, unwrap=False):
    """What a key wrap with padding would run (uaes_debug_plan_kwp; length = bytes of the secret, or of the wrapped form
    - 8 for an unwrap; nkeys 0: the one-secret calls, else a batch): (arrangement, launches, workgroups, threads per
    workgroup), or None for arguments that make no sense."""
    return _kw_plan("uaes_debug_plan_kwp", length, nkeys, unwrap)


FF3_TWEAK_LEN = 7


def _fpe_alpha(alphabet, radix):
    """(radix, alphabet argument): alphabet = the bytes of the numerals, or None with radix = raw digit values"""
    if alphabet is None:
        if radix is None:
            raise ValueError("an alphabet or a radix")
        return radix, None
    alphabet = bytes(alphabet)
    return len(alphabet), _in(alphabet)


def _ff3_tweak(tweak):
    if len(tweak) != FF3_TWEAK_LEN:
        raise ValueError("FF3-1 tweak of %d bytes (%d)" % (len(tweak), FF3_TWEAK_LEN))
    return bytes(tweak)


def _fpe(ff3, decrypt, key, tweak, text, alphabet, radix, prefill):
    """The one-text calls of FF1 and FF3-1: FF1 passes the tweak's length, FF3-1's is fixed"""
    radix, a = _fpe_alpha(alphabet, radix)
    o = _out(len(text), prefill)
    fn = getattr(engine(), "uaes_%s_%s" % ("ff3" if ff3 else "ff1", "decrypt" if decrypt else "encrypt"))
    tw = (_in(_ff3_tweak(tweak)),) if ff3 else (_in(tweak), len(tweak))
    rc = fn(_bits(key), _in(key), radix, a, *tw, _in(text), len(text), o)
    if rc < 0 and rc != -2:
        _check(rc, "AES_%s_%s" % ("FF3" if ff3 else "FPE", "decrypt" if decrypt else "encrypt"))
    return rc, bytes(o)[:len(text)]


def AES_FPE_encrypt(key, tweak, text, alphabet=b"0123456789", radix=None, prefill=0):
    """micro_aes.c:2326 (FF1, SP 800-38G).  text = numerals, one byte each, out of `alphabet` (alphabet=None: raw digit
    values below `radix`).  Returns (code, output): 0; 1 for a text shorter than the radix's minimum or longer than
    4096; -2 for a radix outside 2..256 or a repeated alphabet byte; 0x1E for a byte that is no numeral; the output is
    the prefill unless the code is 0."""
    return _fpe(False, False, key, tweak, text, alphabet, radix, prefill)


def AES_FPE_decrypt(key, tweak, text, alphabet=b"0123456789", radix=None, prefill=0):
    """micro_aes.c:2343.  As AES_FPE_encrypt; 0x1D for a byte that is no numeral."""
    return _fpe(False, True, key, tweak, text, alphabet, radix, prefill)


def AES_FF3_encrypt(key, tweak, text, alphabet=b"0123456789", radix=None, prefill=0):
    """micro_aes.c:2326 built with FF_X 3 (FF3-1, SP 800-38G revision 1).  tweak = 7 bytes; text = numerals, one byte
    each, out of `alphabet` (alphabet=None: raw digit values below `radix`).  Returns (code, output): 0; 1 for a text
    shorter than the radix's minimum or longer than ff3_maxlen(radix); -2 for a radix outside 2..256 or a repeated
    alphabet byte; 0x1E for a byte that is no numeral; the output is the prefill unless the code is 0."""
    return _fpe(True, False, key, tweak, text, alphabet, radix, prefill)


def AES_FF3_decrypt(key, tweak, text, alphabet=b"0123456789", radix=None, prefill=0):
    """micro_aes.c:2343 built with FF_X 3.  As AES_FF3_encrypt; 0x1D for a byte that is no numeral."""
    return _fpe(True, True, key, tweak, text, alphabet, radix, prefill)


def _fpe_batch(ff3, key, tweaks, records, alphabet, radix, decrypt, prefill, verdicts):
    """The batches of FF1 and FF3-1: FF1 passes the tweaks' length, FF3-1's is fixed"""
    n = len(records)
    radix, a = _fpe_alpha(alphabet, radix)
    if isinstance(tweaks, (bytes, bytearray)):
        tl, stride, tb = len(tweaks), 0, _ff3_tweak(tweaks) if ff3 else bytes(tweaks)
    else:
        if len(tweaks) != n:
            raise ValueError("one tweak per record")
        tl, tb = _records([_ff3_tweak(t) for t in tweaks] if ff3 else tweaks, "tweaks")
        stride = tl
    rl, rb = _records(records, "records")
    o = _out(n * rl, prefill)
    v = _out(n)
    name = "uaes_%s_batch" % ("ff3" if ff3 else "ff1")
    fn = getattr(engine(), name.replace("batch", "decrypt_batch" if decrypt else "encrypt_batch"))
    tw = (_in(tb), stride) if ff3 else (_in(tb), tl, stride)
    rc = fn(_bits(key), _in(key), radix, a, *tw, n, rl, _in(rb), o, v if verdicts else None)
    if rc < 0 and rc != -2:
        _check(rc, name)
    raw = bytes(o)
    return rc, _split(raw, rl, n), list(bytes(v)[:n])


def ff1_batch(key, tweaks, records, alphabet=b"0123456789", radix=None, decrypt=False, prefill=0, verdicts=True):
    """FF1 of many equal-sized records under one key (uaes_ff1_*_batch).  tweaks = one tweak (bytes) for all records or a
    list of equal-sized tweaks, one per record.  Returns (code, outputs, verdicts): a record with a byte that is no
    numeral keeps the prefill and has verdict 0."""
    return _fpe_batch(False, key, tweaks, records, alphabet, radix, decrypt, prefill, verdicts)


def ff3_batch(key, tweaks, records, alphabet=b"0123456789", radix=None, decrypt=False, prefill=0, verdicts=True):
    """FF3-1 of many equal-sized records under one key (uaes_ff3_*_batch).  tweaks = one 7-byte tweak (bytes) for all
    records or a list of them, one per record.  Returns (code, outputs, verdicts): a record with a byte that is no
    numeral keeps the prefill and has verdict 0."""
    return _fpe_batch(True, key, tweaks, records, alphabet, radix, decrypt, prefill, verdicts)


def _fpe_plan(hook, length, nrec, radix, decrypt):
    out = (C.c_int * 3)()
    name = getattr(engine(), hook)(int(bool(decrypt)), radix, length, nrec, out)
    return None if name is None else (name.decode(), out[0], out[1], out[2])


def ff1_plan(length, nrec=0, radix=10, decrypt=False):
    """What FF1 over a text of `length` numerals would run (uaes_debug_plan_ff1; nrec 0: the one-text calls, else a
    batch): (arrangement, launches, workgroups, threads per workgroup), or None for arguments that make no sense."""
    return _fpe_plan("uaes_debug_plan_ff1", length, nrec, radix, decrypt)


def ff3_plan(length, nrec=0, radix=10, decrypt=False):
    """What FF3-1 over a text of `length` numerals would run (uaes_debug_plan_ff3; nrec 0: the one-text calls, else a
    batch): (arrangement, launches, workgroups, threads per workgroup), or None for arguments that make no sense."""
    return _fpe_plan("uaes_debug_plan_ff3", length, nrec, radix, decrypt)


def ff3_maxlen(radix):
    """2 floor(log_radix 2^96), the longest FF3-1 text at this radix; 0 for a radix outside 2..256"""
    return int(engine().uaes_ff3_maxlen(radix))


_compat = {}


def compat(bits):
    """libmicro_aes_hip_<bits>.so (the reference's compile-time API, include/micro_aes.h) with the prototypes of the
    key-wrap pair attached: char AES_KEY_wrap(kek, secret, secretLen, wrapped), char AES_KEY_unwrap(kek, wrapped,
    wrapLen, secret), and of the FF1 pairs: char AES_FPE_encrypt(key, tweak, tweakLen, in, len, out) and
    AES_FPE_encrypt_alpha(alphabet, radix, key, ...)."""
    if bits not in _compat:
        engine()
        lib = C.CDLL(lib_path("libmicro_aes_hip_%d.so" % bits))
        for n in ("AES_KEY_wrap", "AES_KEY_unwrap"):
            getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, n).restype = C.c_char
        for n in ("AES_FPE_encrypt", "AES_FPE_decrypt"):
            getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, n).restype = C.c_char
        for n in ("AES_FPE_encrypt_alpha", "AES_FPE_decrypt_alpha"):
            getattr(lib, n).argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, n).restype = C.c_char
        for n in ("AES_FF3_encrypt", "AES_FF3_decrypt"):
            getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, n).restype = C.c_char
        for n in ("AES_FF3_encrypt_alpha", "AES_FF3_decrypt_alpha"):
            getattr(lib, n).argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            getattr(lib, n).restype = C.c_char
        _compat[bits] = lib
    return _compat[bits]


def _ccm_nonce(nonce):
    if not 7 <= len(nonce) <= 13:
        raise ValueError("CCM nonce of %d bytes (7..13)" % len(nonce))
    return _in(nonce)


def AES_CCM_encrypt(key, nonce, aData, pntxt, tag_len=16):
    """micro_aes.c:1268.  len(nonce) / tag_len are the reference's CCM_NONCE_LEN (7..13; 11 by default) and
    CCM_TAG_LEN (even, 4..16); returns ciphertext || tag."""
    _taglen(tag_len, 4, 16, True, "CCM")
    o = _out(len(pntxt) + 16)
    _check(engine().uaes_ccm_encrypt_ex(_bits(key), _in(key), _ccm_nonce(nonce), len(nonce), tag_len, _in(aData), len(aData),
                                        _in(pntxt), len(pntxt), o), "AES_CCM_encrypt")
    return bytes(o)[: len(pntxt) + tag_len]


def AES_CCM_decrypt(key, nonce, aData, crtxt_and_tag, prefill=0, tag_len=16):
    """micro_aes.c:1294.  Returns (code, text); like the reference the decrypted
    text is returned even when the code is 0x1A."""
    _taglen(tag_len, 4, 16, True, "CCM")
    n = len(crtxt_and_tag) - tag_len
    o = _out(n, prefill)
    rc = _check(engine().uaes_ccm_decrypt_ex(_bits(key), _in(key), _ccm_nonce(nonce), len(nonce), tag_len, _in(aData),
                                             len(aData), _in(crtxt_and_tag), n, o), "AES_CCM_decrypt")
    return rc, bytes(o)[:n]


def GCM_SIV_encrypt(key, nonce, aData, pntxt):
    """micro_aes.c:1473 (RFC 8452).  Returns ciphertext || 16-byte tag."""
    o = _out(len(pntxt) + 16)
    _check(engine().uaes_gcmsiv_encrypt(_bits(key), _in(key), _fixed(nonce, 12, "nonce"), _in(aData), len(aData),
                                        _in(pntxt), len(pntxt), o), "GCM_SIV_encrypt")
    return bytes(o)[: len(pntxt) + 16]


def GCM_SIV_decrypt(key, nonce, aData, crtxt_and_tag, prefill=0):
    """micro_aes.c:1494.  Returns (code, text)."""
    n = len(crtxt_and_tag) - 16
    o = _out(n, prefill)
    rc = _check(engine().uaes_gcmsiv_decrypt(_bits(key), _in(key), _fixed(nonce, 12, "nonce"), _in(aData), len(aData),
                                             _in(crtxt_and_tag), n, o), "GCM_SIV_decrypt")
    return rc, bytes(o)[:n]


def _ocb_nonce(nonce):
    if not 1 <= len(nonce) <= 15:
        raise ValueError("OCB nonce of %d bytes (1..15)" % len(nonce))
    return _in(nonce)


def AES_OCB_encrypt(key, nonce, aData, pntxt, tag_len=16):
    """micro_aes.c:1774 (RFC 7253).  len(nonce) / tag_len are the reference's OCB_NONCE_LEN (1..15; 12 by default)
    and OCB_TAG_LEN (1..16).  Returns ciphertext || tag."""
    _taglen(tag_len, 1, 16, False, "OCB")
    o = _out(len(pntxt) + 16)
    _check(engine().uaes_ocb_encrypt_ex(_bits(key), _in(key), _ocb_nonce(nonce), len(nonce), tag_len, _in(aData), len(aData),
                                        _in(pntxt), len(pntxt), o), "AES_OCB_encrypt")
    return bytes(o)[: len(pntxt) + tag_len]


def AES_OCB_decrypt(key, nonce, aData, crtxt_and_tag, prefill=0, tag_len=16):
    """micro_aes.c:1797.  Returns (code, text); the text is written even on 0x1A."""
    _taglen(tag_len, 1, 16, False, "OCB")
    n = len(crtxt_and_tag) - tag_len
    o = _out(n, prefill)
    rc = _check(engine().uaes_ocb_decrypt_ex(_bits(key), _in(key), _ocb_nonce(nonce), len(nonce), tag_len, _in(aData),
                                             len(aData), _in(crtxt_and_tag), n, o), "AES_OCB_decrypt")
    return rc, bytes(o)[:n]


# ---------------------------------------------------------------------------
# one process, several GPUs (uaes_mgpu_*): `devices` = list of HIP ordinals (an ordinal may repeat)
# ---------------------------------------------------------------------------
def _devs(devices):
    devices = list(devices)
    return len(devices), (C.c_int * len(devices))(*devices)


def _buf(x):
    """host bytes -> ctypes copy; an int is taken as a raw (device) address"""
    return C.c_void_p(x) if isinstance(x, int) else _in(x)


def mgpu_ecb_encrypt(devices, key, pntxt, padding=0):
    n, d = _devs(devices)
    m = (len(pntxt) // 16 + 1) * 16 if padding else (len(pntxt) + 15) // 16 * 16
    o = _out(m)
    _check(engine().uaes_mgpu_ecb_encrypt(n, d, _bits(key), _in(key), padding, _in(pntxt), len(pntxt), o), "uaes_mgpu_ecb_encrypt")
    return bytes(o)[:m]


def mgpu_ecb_decrypt(devices, key, crtxt, prefill=0):
    n, d = _devs(devices)
    o = _out(len(crtxt), prefill)
    rc = _check(engine().uaes_mgpu_ecb_decrypt(n, d, _bits(key), _in(key), _in(crtxt), len(crtxt), o), "uaes_mgpu_ecb_decrypt")
    return rc, bytes(o)[: len(crtxt)]


def mgpu_gcm_encrypt(devices, key, nonce, aData, pntxt):
    """== AES_GCM_encrypt, the text cut into one 16-byte aligned slice per device (uaes_mgpu_gcm_encrypt)."""
    n, d = _devs(devices)
    o = _out(len(pntxt) + 16)
    _check(engine().uaes_mgpu_gcm_encrypt(n, d, _bits(key), _in(key), _fixed(nonce, 12, "nonce"), _in(aData), len(aData),
                                          _in(pntxt), len(pntxt), o), "uaes_mgpu_gcm_encrypt")
    return bytes(o)[: len(pntxt) + 16]


def mgpu_gcm_decrypt(devices, key, nonce, aData, crtxt_and_tag, prefill=0):
    """== AES_GCM_decrypt: (code, plaintext); 0x1A and an untouched (prefilled) buffer on a forgery (N7 across devices)."""
    n, d = _devs(devices)
    m = len(crtxt_and_tag) - 16
    o = _out(m, prefill)
    rc = _check(engine().uaes_mgpu_gcm_decrypt(n, d, _bits(key), _in(key), _fixed(nonce, 12, "nonce"), _in(aData), len(aData),
                                               _in(crtxt_and_tag), m, o), "uaes_mgpu_gcm_decrypt")
    return rc, bytes(o)[:m]


def mgpu_gcm_dev(devices, key, nonce, aad, src_ptr, nbytes, dst_ptr, decrypt=False):
    """the same on raw device addresses (ints): encrypt writes nbytes + 16 at dst_ptr; decrypt reads nbytes + 16"""
    n, d = _devs(devices)
    fn = engine().uaes_mgpu_gcm_decrypt if decrypt else engine().uaes_mgpu_gcm_encrypt
    return _check(fn(n, d, _bits(key), _in(key), _fixed(nonce, 12, "nonce"), _in(aad or b""), len(aad or b""),
                     C.c_void_p(src_ptr), nbytes, C.c_void_p(dst_ptr)), "uaes_mgpu_gcm_*")


class GcmKey:
    """GCM key context (uaes_gcm_key_*): the key's GHASH tables are built once; encrypt / decrypt then equal
    AES_GCM_encrypt / AES_GCM_decrypt bit for bit.  One call at a time per object."""

    def __init__(self, key):
        self._h = C.c_void_p()
        _check(engine().uaes_gcm_key_new(C.byref(self._h), _bits(key), _in(key)), "uaes_gcm_key_new")

    def encrypt(self, nonce, aData, pntxt):
        o = _out(len(pntxt) + 16)
        _check(engine().uaes_gcm_key_encrypt(self._h, _fixed(nonce, 12, "nonce"), _in(aData), len(aData),
                                             _in(pntxt), len(pntxt), o), "uaes_gcm_key_encrypt")
        return bytes(o)[: len(pntxt) + 16]

    def decrypt(self, nonce, aData, crtxt_and_tag, prefill=0):
        n = len(crtxt_and_tag) - 16
        o = _out(n, prefill)
        rc = _check(engine().uaes_gcm_key_decrypt(self._h, _fixed(nonce, 12, "nonce"), _in(aData), len(aData),
                                                  _in(crtxt_and_tag), n, o), "uaes_gcm_key_decrypt")
        return rc, bytes(o)[:n]

    def encrypt_dev(self, nonce, aad, src, nbytes, dst, stream=None):
        _check(engine().uaes_gcm_key_encrypt_dev(self._h, _fixed(nonce, 12, "nonce"), _ptr(aad),
                                                 0 if aad is None else aad.numel(), _ptr(src), nbytes, _ptr(dst),
                                                 _stream(stream)), "uaes_gcm_key_encrypt_dev")

    def decrypt_dev(self, nonce, aad, src, nbytes, dst, status, stream=None):
        _check(engine().uaes_gcm_key_decrypt_dev(self._h, _fixed(nonce, 12, "nonce"), _ptr(aad),
                                                 0 if aad is None else aad.numel(), _ptr(src), nbytes, _ptr(dst),
                                                 _ptr(status), _stream(stream)), "uaes_gcm_key_decrypt_dev")

    @staticmethod
    def record_max(aad_len=0):
        """longest record (bytes) the record calls take with aad_len bytes of AAD per record"""
        return int(engine().uaes_gcm_record_max(aad_len))

    def encrypt_records(self, nonces, aads, records, stride=None):
        """Many equally long messages in one launch (uaes_gcm_key_encrypt_records).  nonces: list of 12-byte
        values; aads: one bytes object for all records or a list of equally long ones; records: list of equally
        long plaintexts.  Returns the list of ciphertext || tag, each equal to encrypt() of that record."""
        n = len(records)
        if n == 0:
            return []
        rec_len = len(records[0])
        if any(len(r) != rec_len for r in records) or len(nonces) != n:
            raise ValueError("records must be equally long and have one nonce each")
        stride = stride or (rec_len + 16 + 15) // 16 * 16
        aad, aad_len, aad_stride = self._pack_aads(aads, n)
        src = bytearray(stride * n)
        for r, rec in enumerate(records):
            src[r * stride: r * stride + rec_len] = rec
        dst = _out(stride * n)
        _check(engine().uaes_gcm_key_encrypt_records(self._h, n, _in(b"".join(_fixed_bytes(x, 12) for x in nonces)),
                                                     _in(aad), aad_len, aad_stride, _in(bytes(src)), rec_len, stride,
                                                     dst, stride), "uaes_gcm_key_encrypt_records")
        b = bytes(dst)
        return [b[r * stride: r * stride + rec_len + 16] for r in range(n)]

    def decrypt_records(self, nonces, aads, records, prefill=0, stride=None):
        """records: list of equally long ciphertext || tag.  Returns (code, verdicts, texts): code 0 or 0x1A (some
        record failed), verdicts[r] 0 / 0x1A, texts[r] the plaintext -- `prefill` bytes where the tag was wrong (N7)."""
        n = len(records)
        if n == 0:
            return 0, [], []
        rec_len = len(records[0]) - 16
        if rec_len < 0 or any(len(r) != rec_len + 16 for r in records) or len(nonces) != n:
            raise ValueError("records must be equally long (text || tag) and have one nonce each")
        stride = stride or (rec_len + 16 + 15) // 16 * 16
        aad, aad_len, aad_stride = self._pack_aads(aads, n)
        src = bytearray(stride * n)
        for r, rec in enumerate(records):
            src[r * stride: r * stride + rec_len + 16] = rec
        dst = _out(stride * n, prefill)
        ver = _out(n, 0x55)
        rc = _check(engine().uaes_gcm_key_decrypt_records(self._h, n, _in(b"".join(_fixed_bytes(x, 12) for x in nonces)),
                                                          _in(aad), aad_len, aad_stride, _in(bytes(src)), rec_len, stride,
                                                          dst, stride, ver), "uaes_gcm_key_decrypt_records")
        b = bytes(dst)
        return rc, list(bytes(ver)), [b[r * stride: r * stride + rec_len] for r in range(n)]

    def encrypt_records_v(self, nonces, aads, records, max_len=None, stride=None):
        """records of DIFFERENT lengths in equal slots (uaes_gcm_key_encrypt_records_v).  Returns the list of
        ciphertext || tag, each equal to encrypt() of that record."""
        n = len(records)
        if n == 0:
            return []
        max_len = max(len(r) for r in records) if max_len is None else max_len
        stride = stride or (max_len + 16 + 15) // 16 * 16
        aad, aad_len, aad_stride = self._pack_aads(aads, n)
        src = bytearray(stride * n)
        for r, rec in enumerate(records):
            src[r * stride: r * stride + len(rec)] = rec
        lens = (C.c_uint32 * n)(*[len(r) for r in records])
        dst = _out(stride * n)
        _check(engine().uaes_gcm_key_encrypt_records_v(self._h, n, _in(b"".join(_fixed_bytes(x, 12) for x in nonces)),
                                                       _in(aad), aad_len, aad_stride, _in(bytes(src)), lens, max_len, stride,
                                                       dst, stride), "uaes_gcm_key_encrypt_records_v")
        b = bytes(dst)
        return [b[r * stride: r * stride + len(records[r]) + 16] for r in range(n)]

    def decrypt_records_v(self, nonces, aads, records, prefill=0, max_len=None, stride=None):
        """records: list of ciphertext || tag of different lengths.  Returns (code, verdicts, texts)."""
        n = len(records)
        if n == 0:
            return 0, [], []
        tl = [len(r) - 16 for r in records]
        max_len = max(tl) if max_len is None else max_len
        stride = stride or (max_len + 16 + 15) // 16 * 16
        aad, aad_len, aad_stride = self._pack_aads(aads, n)
        src = bytearray(stride * n)
        for r, rec in enumerate(records):
            src[r * stride: r * stride + len(rec)] = rec
        lens = (C.c_uint32 * n)(*tl)
        dst = _out(stride * n, prefill)
        ver = _out(n, 0x55)
        rc = _check(engine().uaes_gcm_key_decrypt_records_v(self._h, n, _in(b"".join(_fixed_bytes(x, 12) for x in nonces)),
                                                            _in(aad), aad_len, aad_stride, _in(bytes(src)), lens, max_len, stride,
                                                            dst, stride, ver), "uaes_gcm_key_decrypt_records_v")
        b = bytes(dst)
        return rc, list(bytes(ver)), [b[r * stride: r * stride + tl[r]] for r in range(n)]

    @staticmethod
    def _pack_aads(aads, n):
        if isinstance(aads, (bytes, bytearray)):
            return bytes(aads), len(aads), 0
        if len(aads) != n or any(len(a) != len(aads[0]) for a in aads):
            raise ValueError("one equally long AAD per record (or one bytes object for all)")
        return b"".join(aads), len(aads[0]), len(aads[0])

    def encrypt_records_dev(self, nrec, nonces, aad, aad_len, aad_stride, src, rec_len, in_stride, dst, out_stride, stream=None):
        """device tensors (uint8): nonces 12 * nrec bytes; enqueues on `stream`"""
        _check(engine().uaes_gcm_key_encrypt_records_dev(self._h, nrec, _ptr(nonces), _ptr(aad), aad_len, aad_stride, _ptr(src),
                                                         rec_len, in_stride, _ptr(dst), out_stride, _stream(stream)),
               "uaes_gcm_key_encrypt_records_dev")

    def decrypt_records_dev(self, nrec, nonces, aad, aad_len, aad_stride, src, rec_len, in_stride, dst, out_stride,
                            verdicts, status, stream=None):
        _check(engine().uaes_gcm_key_decrypt_records_dev(self._h, nrec, _ptr(nonces), _ptr(aad), aad_len, aad_stride, _ptr(src),
                                                         rec_len, in_stride, _ptr(dst), out_stride, _ptr(verdicts), _ptr(status),
                                                         _stream(stream)), "uaes_gcm_key_decrypt_records_dev")

    def close(self):
        if getattr(self, "_h", None):
            engine().uaes_gcm_key_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: the module globals may be gone already
            pass


class GcmStream:
    """One GCM message fed in pieces (uaes_gcm_stream_*): same bytes as AES_GCM_encrypt/decrypt."""

    def __init__(self, key, nonce, aData=b"", decrypt=False):
        self._h = C.c_void_p()
        _check(engine().uaes_gcm_stream_begin(C.byref(self._h), _bits(key), _in(key), _fixed(nonce, 12, "nonce"), _in(aData),
                                              len(aData), 1 if decrypt else 0), "uaes_gcm_stream_begin")
        self._decrypt = decrypt

    def update(self, piece):
        o = _out(len(piece))
        _check(engine().uaes_gcm_stream_update(self._h, _in(piece), len(piece), o), "uaes_gcm_stream_update")
        return bytes(o)[: len(piece)]

    def update_dev(self, src, n, dst):
        """One piece of n bytes in device memory: src and dst are torch tensors or raw device pointers, handed straight
        to uaes_gcm_stream_update; dst may be src.  Returns when the piece is done."""
        s, d = (C.c_void_p(t if isinstance(t, int) else t.data_ptr()) for t in (src, dst))
        _check(engine().uaes_gcm_stream_update(self._h, s, n, d), "uaes_gcm_stream_update")

    def tables(self):
        """The stream's table cache (uaes_debug_gcm_stream_tables) as (valid, logA, has_B, has_striped)."""
        w = engine().uaes_debug_gcm_stream_tables(self._h)
        return bool(w >> 31), w & 0xff, bool((w >> 8) & 1), bool((w >> 9) & 1)

    def finish(self, tag=None):
        """encrypt: returns the tag; decrypt: returns 0 or M_AUTHENTICATION_ERROR for the given tag."""
        t = _fixed(tag if self._decrypt else bytes(16), 16, "tag")
        h, self._h = self._h, None
        rc = _check(engine().uaes_gcm_stream_finish(h, t), "uaes_gcm_stream_finish")
        return rc if self._decrypt else bytes(t)

    def abort(self):
        """give the stream up (uaes_gcm_stream_abort); a stream that is dropped unfinished is aborted too"""
        if getattr(self, "_h", None):
            engine().uaes_gcm_stream_abort(self._h)
            self._h = None

    def __del__(self):
        self.abort()


MODES = {"ecb": 0, "ctr": 1, "xts": 2, "gcm": 3, "ocb": 4, "siv": 5}


def plan(mode, a, b=0, direction=0, flags=0, counter=None):
    """What a call would run (uaes_debug_plan): (arrangement name, launches, workgroups, positions per thread).
    counter: the CTR call's first 16-byte counter block or the GCM call's J0 (uaes_debug_plan_at); None = a 12-byte
    IV / nonce."""
    out = (C.c_int * 4)()
    if counter is None:
        _check(engine().uaes_debug_plan(MODES[mode], direction, a, b, flags, out), "uaes_debug_plan")
    else:
        _check(engine().uaes_debug_plan_at(MODES[mode], direction, a, b, flags, _fixed(counter, 16, "counter"), out),
               "uaes_debug_plan_at")
    return engine().uaes_debug_arrangement_name(out[0]).decode(), out[1], out[2], out[3]


def plan_gcm_piece(length, done=0, decrypt=False):
    """What uaes_gcm_stream_update runs for a piece of `length` bytes behind `done` bytes of text (uaes_debug_plan_gcm_piece):
    (arrangement name, launches, workgroups, positions per thread); "gcm.levels" = not taken, the absorb path."""
    out = (C.c_int * 4)()
    _check(engine().uaes_debug_plan_gcm_piece(int(bool(decrypt)), length, done, out), "uaes_debug_plan_gcm_piece")
    return engine().uaes_debug_arrangement_name(out[0]).decode(), out[1], out[2], out[3]


def plan_ocb(length, aad_len=0, decrypt=False, aad_aligned=True):
    """The launch shape of an OCB call in the runs arrangement (uaes_debug_plan_ocb): (run, run_aad, threads per
    workgroup, workgroups, hash_blocks) -- the chunks a wave takes at once over the text / over long associated data,
    and the whole blocks of associated data that all workgroups hash.  None where the call is "ocb.small"."""
    out = (C.c_int * 5)()
    name = engine().uaes_debug_plan_ocb(int(bool(decrypt)), length, aad_len, int(bool(aad_aligned)), out)
    if name is None:
        raise ValueError("no OCB plan for these arguments")
    return tuple(out) if name == b"ocb.runs" else None


XtsPlan = collections.namedtuple("XtsPlan", "name threads grid cps nmain chunks serial aligned allfull")


def xts_plan(sector_bytes, nsectors=1, explicit_tweak=False):
    """The launch shape of an XTS call (uaes_debug_plan_xts): the arrangement's name, threads per workgroup and workgroups
    of its main kernel, the 256-block chunks per unit, the chunks of the kernel's main loop, the chunks in all (the rest
    goes by quarters), and whether the unit's chunk tweaks are walked by one thread, every block is 16-byte aligned and
    every chunk is whole."""
    out = (C.c_uint64 * 8)()
    name = engine().uaes_debug_plan_xts(sector_bytes, nsectors, int(bool(explicit_tweak)), out)
    if name is None:
        raise ValueError("no XTS plan for these arguments")
    return XtsPlan(name.decode(), *[int(v) for v in out[:5]], *[bool(v) for v in out[5:]])


def arrangement_id(name):
    L = engine()
    for k in range(64):
        if L.uaes_debug_arrangement_name(k) == name.encode():
            return k
    raise KeyError(name)


def ghash(H, aData, crtxt):
    """gHash of micro_aes.c:1127 with an explicit subkey (test hook)."""
    o = _out(16)
    _check(engine().uaes_ghash(_fixed(H, 16, "H"), _in(aData), len(aData), _in(crtxt), len(crtxt), o), "uaes_ghash")
    return bytes(o)


def selftest():
    return _check(engine().uaes_selftest(), "uaes_selftest")


def host_policy(max_bytes=None, chains=None, fallback=None):
    """Get / set the opt-in host data path (uaes_set_host_policy).  Returns the policy in force BEFORE the call as
    (max_bytes, chains, fallback); arguments left None keep their value.  Default (0, 0, 0): GPU always."""
    mb, ch, fb = C.c_size_t(), C.c_int(), C.c_int()
    engine().uaes_get_host_policy(C.byref(mb), C.byref(ch), C.byref(fb))
    prev = (mb.value, ch.value, fb.value)
    if max_bytes is not None or chains is not None or fallback is not None:
        engine().uaes_set_host_policy(prev[0] if max_bytes is None else max_bytes,
                                      prev[1] if chains is None else int(chains),
                                      prev[2] if fallback is None else int(fallback))
    return prev


# ---------------------------------------------------------------------------
# device-resident API (torch tensors are only carriers of raw device pointers)
# ---------------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return C.c_void_p(stream.cuda_stream)


def ctr_xcrypt_dev(key, ctr0, block_offset, src, dst, nbytes=None, stream=None):
    """Enqueue CTR over device tensors (uint8, contiguous).  No synchronisation."""
    n = src.numel() * src.element_size() if nbytes is None else nbytes
    _check(engine().uaes_ctr_xcrypt_at_dev(_bits(key), _in(key), _fixed(ctr0, 16, "ctr0"), block_offset,
                                           _ptr(src), n, _ptr(dst), _stream(stream)), "uaes_ctr_xcrypt_at_dev")


def ecb_dev(key, src, dst, decrypt=False, nbytes=None, stream=None):
    n = src.numel() * src.element_size() if nbytes is None else nbytes
    _check(engine().uaes_ecb_dev(_bits(key), _in(key), 1 if decrypt else 0, _ptr(src), n, _ptr(dst),
                                 _stream(stream)), "uaes_ecb_dev")


def xts_sectors_dev(keys, first_sector, sector_bytes, nsectors, src, dst, encrypt=True, stream=None):
    _check(engine().uaes_xts_sectors_dev(_bits(keys, 2), _in(keys), first_sector, sector_bytes, nsectors,
                                         _ptr(src), _ptr(dst), 1 if encrypt else 0, _stream(stream)),
           "uaes_xts_sectors_dev")


def gcm_encrypt_dev(key, nonce, aad, src, nbytes, dst, stream=None):
    """dst must hold nbytes + 16 (tag appended)."""
    _check(engine().uaes_gcm_encrypt_dev(_bits(key), _in(key), _fixed(nonce, 12, "nonce"), _ptr(aad),
                                         0 if aad is None else aad.numel(), _ptr(src), nbytes, _ptr(dst),
                                         _stream(stream)), "uaes_gcm_encrypt_dev")


def gcm_decrypt_dev(key, nonce, aad, src, nbytes, dst, status, stream=None):
    """src holds nbytes + 16 (ciphertext || tag); status: int32 device tensor."""
    _check(engine().uaes_gcm_decrypt_dev(_bits(key), _in(key), _fixed(nonce, 12, "nonce"), _ptr(aad),
                                         0 if aad is None else aad.numel(), _ptr(src), nbytes, _ptr(dst),
                                         _ptr(status), _stream(stream)), "uaes_gcm_decrypt_dev")


def ocb_dev(key, nonce, aad, src, nbytes, dst, decrypt=False, status=None, stream=None):
    """encrypt: dst holds nbytes + 16; decrypt: src holds nbytes + 16, status = int32 device tensor."""
    _check(engine().uaes_ocb_dev(_bits(key), _in(key), _fixed(nonce, 12, "nonce"), 1 if decrypt else 0, _ptr(aad),
                                 0 if aad is None else aad.numel(), _ptr(src), nbytes, _ptr(dst),
                                 _ptr(status), _stream(stream)), "uaes_ocb_dev")


def poly1305_dev(keys, nonce, src, nbytes, mac, stream=None):
    """Enqueue the Poly1305-AES mac of nbytes of the device tensor src into the 16-byte device tensor mac."""
    _check(engine().uaes_poly1305_dev(_poly_bits(keys), _in(keys), _fixed(nonce, 16, "nonce"), _ptr(src), nbytes,
                                      _ptr(mac), _stream(stream)), "uaes_poly1305_dev")


def gcm_partial_dev(key, nonce, aad, total_aad_len, ct_shard, shard_len, shard_offset, total_len, partial,
                    stream=None):
    """This shard's 16-byte share of the GCM tag (see uaes_gcm_partial_dev)."""
    _check(engine().uaes_gcm_partial_dev(_bits(key), _in(key), _fixed(nonce, 12, "nonce"), _ptr(aad), total_aad_len,
                                         _ptr(ct_shard), shard_len, shard_offset, total_len, _ptr(partial),
                                         _stream(stream)), "uaes_gcm_partial_dev")


def gcm_shard_dev(key, nonce, mode, aad, total_aad_len, src, shard_len, shard_offset, total_len, dst, partial, stream=None):
    """This shard's CTR pass (mode 0 encrypt / 2 decrypt; 1 = hash only) fused with its 16-byte share of the tag
    (uaes_gcm_shard_dev): one pass over the text."""
    _check(engine().uaes_gcm_shard_dev(_bits(key), _in(key), _fixed(nonce, 12, "nonce"), mode, _ptr(aad), total_aad_len,
                                       _ptr(src), shard_len, shard_offset, total_len, _ptr(dst), _ptr(partial),
                                       _stream(stream)), "uaes_gcm_shard_dev")
