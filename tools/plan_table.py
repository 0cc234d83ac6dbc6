#!/usr/bin/env python3
"""Print the table of arrangements (csrc/uaes_plan.h) as this device -- or, without one, a 256-CU MI355X -- decides it:
every boundary at which the arrangement (or its GHASH positions per thread) changes, found by bisection over
uaes_debug_plan().  DESIGN.md section 3 quotes this output."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import micro_aes_amd as uaes

MIB = 1 << 20


def pts(lo, hi, unit):
    ks, j = {0, 1, 2, 3, 5, 7}, 1
    while (1 << j) * unit <= hi * 2:
        ks.update({(1 << j) - 1, 1 << j, (1 << j) + 1, 3 << (j - 1)})
        j += 1
    return sorted(k * unit for k in ks if lo <= k * unit <= hi)


def walk(title, fn, lo, hi, unit=16, fmt=lambda n: "%11d B (%9.3f MiB)" % (n, n / MIB)):
    print(title)
    p = pts(lo, hi, unit)
    cur = fn(p[0])
    print("    from %s  %-13s launches %d%s" % (fmt(p[0]), cur[0], cur[1], ("  positions/thread %d" % cur[3]) if cur[3] else ""))
    for left, right in zip(p, p[1:]):
        rl = fn(left)
        while (rl[0], rl[3]) != (fn(right)[0], fn(right)[3]):
            a, b = left, right
            while b - a > unit:
                m = (a + b) // 2 // unit * unit
                if (fn(m)[0], fn(m)[3]) == (rl[0], rl[3]):
                    a = m
                else:
                    b = m
            nb = fn(b)
            print("    from %s  %-13s launches %d%s" % (fmt(b), nb[0], nb[1], ("  positions/thread %d" % nb[3]) if nb[3] else ""))
            left, rl = b, nb


walk("ECB", lambda n: uaes.plan("ecb", n), 0, 64 * MIB)
walk("CTR (56-bit big-endian counter)", lambda n: uaes.plan("ctr", n), 0, 64 * MIB)
walk("XTS, one data unit of n bytes", lambda n: uaes.plan("xts", max(n, 16), 1), 16, 64 * MIB)
for sector in (512, 4096):
    walk("XTS, k data units of %d bytes" % sector, lambda k: uaes.plan("xts", sector, max(k, 1)), 1, (8 << 30) // sector, 1,
         lambda k: "%9d units (%9.3f MiB)" % (k, k * sector / MIB))
walk("GCM encrypt", lambda n: uaes.plan("gcm", n), 0, 2048 * MIB)
walk("GCM decrypt, tag first (default, N7)", lambda n: uaes.plan("gcm", n, 0, 1), 0, 2048 * MIB)
walk("GCM decrypt, one pass (uaes_set_gcm_one_pass_decrypt)", lambda n: uaes.plan("gcm", n, 0, 2), 0, 2048 * MIB)
walk("OCB", lambda n: uaes.plan("ocb", n), 0, 64 * MIB)
walk("GCM-SIV", lambda n: uaes.plan("siv", n), 0, 2048 * MIB)
walk("Poly1305-AES, one message", lambda n: uaes.poly1305_plan(n)[:3] + (0,), 0, 2048 * MIB)
walk("Poly1305-AES, batches of k messages of 1 KiB", lambda k: uaes.poly1305_plan(1024, max(k, 2))[:3] + (0,), 2, 1 << 20, 1,
     lambda k: "%9d msgs (%9.3f MiB)" % (k, k * 1024 / MIB))
print("EAX / SIV (RFC 5297): one launch up to UAES_EAX_SIV_SMALL_MAX = %d bytes of text" % uaes.eax_siv_plan(False, 0)[3])
walk("EAX encrypt", lambda n: uaes.eax_siv_plan(False, n)[:2] + (0, 0), 0, 64 * MIB)
walk("EAX decrypt", lambda n: uaes.eax_siv_plan(False, n, decrypt=True)[:2] + (0, 0), 0, 64 * MIB)
walk("EAX' encrypt", lambda n: uaes.eaxp_plan(n)[:2] + (0, 0), 0, 64 * MIB)
walk("EAX' decrypt", lambda n: uaes.eaxp_plan(n, decrypt=True)[:2] + (0, 0), 0, 64 * MIB)
walk("EAX' batch, k records of 64 bytes", lambda k: uaes.eaxp_plan(64, max(k, 2))[:2] + (0, 0), 2, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
walk("SIV (RFC 5297)", lambda n: uaes.eax_siv_plan(True, n)[:2] + (0, 0), 0, 64 * MIB)
print("SIV with a vector of associated data: the components of one call are dealt over %d rows of sixteen lanes" % uaes.siv_v_plan(0, 1)[3])
for dec in (False, True):
    walk("SIV %s, 3 components" % ("decrypt" if dec else "encrypt"), lambda n: uaes.siv_v_plan(n, 3, decrypt=dec)[:2] + (0, 0), 0, 64 * MIB, 1)
walk("SIV batch with components, k records of 64 bytes (positions/thread: rows per record's components)",
     lambda k: uaes.siv_v_plan(64, 2, max(k, 2))[:2] + (0, uaes.siv_v_plan(64, 2, max(k, 2))[3]), 2, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
for what in ("cbc", "cfb", "cbc_nocts"):
    walk("%s decrypt" % what.upper(), lambda n: uaes.chain_plan(what, max(n, 16), decrypt=True)[:2] + (0, 0), 16, 64 * MIB)
walk("CBC / CFB encrypt, OFB, CMAC", lambda n: uaes.chain_plan("cbc", max(n, 16))[:2] + (0, 0), 16, 64 * MIB)
walk("CCM", lambda n: uaes.chain_plan("ccm", n)[:2] + (0, 0), 0, 64 * MIB, 1)
for what in ("cbc_batch", "cmac_batch"):
    walk("%s, k messages of 1 KiB (positions/thread: threads per workgroup)" % what,
         lambda k: uaes.chain_plan(what, 1024, max(k, 1))[:2] + (0, uaes.chain_plan(what, 1024, max(k, 1))[3]), 1, 1 << 20, 1,
         lambda k: "%9d msgs (%9.3f MiB)" % (k, k * 1024 / MIB))
def ccm_batch_plan(k, n=64):
    try:
        return uaes.chain_plan("ccm_batch", n, max(k, 1))
    except ValueError:
        return None


top = max(n for n in range(65000, 66000) if ccm_batch_plan(2, n) is not None)
print("CCM batches: a record holds at most UAES_CCM_BATCH_MAX = %d bytes of text" % top)
walk("CCM batch, k records of 64 bytes (positions/thread: threads per workgroup)",
     lambda k: ccm_batch_plan(k)[:2] + (0, ccm_batch_plan(k)[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
top = max(n for n in range(65000, 66000) if uaes.gcmsiv_batch_plan(n, 2) is not None)
print("GCM-SIV batches: a record holds at most UAES_GCMSIV_BATCH_MAX = %d bytes of text" % top)
walk("GCM-SIV batch, k records of 64 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.gcmsiv_batch_plan(64, max(k, 1))[:2] + (0, uaes.gcmsiv_batch_plan(64, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
top = max(n for n in range(65000, 66000) if uaes.gcm_multikey_batch_plan(n, 2) is not None)
print("Multi-key GCM batches: a record holds at most UAES_GCM_MULTIKEY_BATCH_MAX = %d bytes of text" % top)
walk("Multi-key GCM batch, k records of 64 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.gcm_multikey_batch_plan(64, max(k, 1))[:2] + (0, uaes.gcm_multikey_batch_plan(64, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
top = max(n for n in range(65000, 66000) if uaes.xaes256gcm_batch_plan(n, 2) is not None)
print("XAES-256-GCM batches: a record holds at most UAES_XAES_GCM_BATCH_MAX = %d bytes of text" % top)
walk("XAES-256-GCM batch, k records of 64 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.xaes256gcm_batch_plan(64, max(k, 1))[:2] + (0, uaes.xaes256gcm_batch_plan(64, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
top = max(n for n in range(65000, 66000) if uaes.ocb_batch_plan(n, 2) is not None)
print("OCB batches: a record holds at most UAES_OCB_BATCH_MAX = %d bytes of text" % top)
walk("OCB batch, k records of 64 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.ocb_batch_plan(64, max(k, 1))[:2] + (0, uaes.ocb_batch_plan(64, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
walk("Cipher batch (CBC decrypt / blocks, CFB, OFB, CTR), k records of 64 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.cipher_batch_plan(max(k, 1), "ctr", 64)[:2] + (0, uaes.cipher_batch_plan(max(k, 1), "ctr", 64)[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 64 / MIB))
walk("XTS batch and sector list, k units of 512 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.xts_batch_plan(max(k, 1), 512)[:2] + (0, uaes.xts_batch_plan(max(k, 1), 512)[3]), 1, 1 << 20, 1,
     lambda k: "%9d units   (%9.3f MiB)" % (k, k * 512 / MIB))
for dec in (False, True):
    walk("KW %s, one secret of n bytes" % ("unwrap" if dec else "wrap"),
         lambda n: uaes.kw_plan(max(n, 16), unwrap=dec)[:2] + (0, 0), 16, 64 * MIB, 8)
top = max(n for n in range(16, 1 << 13, 8) if uaes.kw_plan(n, 2) is not None)
print("KW batches: a record holds at most UAES_KW_BATCH_MAX = %d bytes of secret" % top)
walk("KW batch, k secrets of 32 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.kw_plan(32, max(k, 1))[:2] + (0, uaes.kw_plan(32, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d keys (%9.3f MiB)" % (k, k * 32 / MIB))
walk("KWP wrap, one secret of n bytes",
     lambda n: uaes.kwp_plan(max(n, 1))[:2] + (0, 0), 1, 64 * MIB, 1)
walk("KWP unwrap, one wrapped form of n + 8 bytes",
     lambda n: uaes.kwp_plan(max(n, 8), unwrap=True)[:2] + (0, 0), 8, 64 * MIB, 8)
top = max(n for n in range(1, 1 << 13) if uaes.kwp_plan(n, 2) is not None)
print("KWP batches: a secret's slot holds at most UAES_KW_BATCH_MAX = %d bytes, each record with a length of its own" % top)
walk("KWP batch, k secrets in slots of 20 bytes (positions/thread: threads per workgroup)",
     lambda k: uaes.kwp_plan(20, max(k, 1))[:2] + (0, uaes.kwp_plan(20, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d keys (%9.3f MiB)" % (k, k * 20 / MIB))
for dec in (False, True):
    walk("FF1 %s, one decimal text of n numerals" % ("decrypt" if dec else "encrypt"),
         lambda n: uaes.ff1_plan(max(n, 6), decrypt=dec)[:2] + (0, 0), 6, 4096, 1, lambda n: "%11d numerals" % n)
top = max(n for n in range(6, 8200) if uaes.ff1_plan(n) is not None)
btop = max(n for n in range(6, 8200) if uaes.ff1_plan(n, 2) is not None)
print("FF1: a text holds at most UAES_FF1_MAX = %d numerals, a batch record at most UAES_FF1_BATCH_MAX = %d" % (top, btop))
walk("FF1 batch, k decimal records of 16 numerals (positions/thread: threads per workgroup)",
     lambda k: uaes.ff1_plan(16, max(k, 1))[:2] + (0, uaes.ff1_plan(16, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 16 / MIB))
for radix in (2, 10, 36, 256):
    print("FF3-1, radix %d: one text of %d..%d numerals" % (radix, min(n for n in range(1, 200) if uaes.ff3_plan(n, radix=radix)),
                                                          uaes.ff3_maxlen(radix)))
walk("FF3-1 encrypt, one decimal text of n numerals",
     lambda n: uaes.ff3_plan(max(n, 6))[:2] + (0, 0), 6, uaes.ff3_maxlen(10), 1, lambda n: "%11d numerals" % n)
walk("FF3-1 batch, k decimal records of 16 numerals (positions/thread: threads per workgroup)",
     lambda k: uaes.ff3_plan(16, max(k, 1))[:2] + (0, uaes.ff3_plan(16, max(k, 1))[3]), 1, 1 << 20, 1,
     lambda k: "%9d records (%9.3f MiB)" % (k, k * 16 / MIB))
