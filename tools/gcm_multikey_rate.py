#!/usr/bin/env python3
"""Multi-key GCM batch rates, written as markdown (to profiles/gcm_multikey_batch_rate.md unless --out names another file):
  short     2^10 device-resident records of 16 bytes, each under a key of its own, as ONE
            uaes_gcm_multikey_encrypt_batch / uaes_gcm_multikey_decrypt_batch call, against 2^10 uaes_gcm_encrypt calls,
            one record and one key each, on the same data in the same run
  batch     2^20 device-resident records of 16, 64 and 1024 bytes through uaes_gcm_multikey_encrypt_batch /
            uaes_gcm_multikey_decrypt_batch, and beside each uaes_gcmsiv_encrypt_batch / uaes_gcmsiv_decrypt_batch and
            uaes_gcm_key_encrypt_records / uaes_gcm_key_decrypt_records at the same shape -- those two under ONE key
AES-128 and AES-256, 12 bytes of AAD per record, 16-byte tags, the keys in device memory.  Every figure: warm-up, then
REPS repetitions; median, minimum and maximum.  The calls are synchronous, so every figure includes the host round trip.
  --xaes    instead: 2^20 device-resident records of 16, 64 and 1024 bytes through uaes_xaes256gcm_encrypt_batch /
            uaes_xaes256gcm_decrypt_batch (24-byte nonces, the key of every record derived in the kernel), and beside each
            the multi-key batch at AES-256 on the same texts; to profiles/xaes_gcm_batch_rate.md unless --out names a file
Usage: gcm_multikey_rate.py [--xaes] [--out FILE] [--quick]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import micro_aes_amd as uaes

L = uaes.engine()
REPS = 9
NONCE, AAD = 12, 12


def reps_of(fn, calls, reps=REPS):
    """microseconds per call: `reps` timed windows of `calls` synchronous calls each, after a warm-up window"""
    for _ in range(max(calls // 4, 2)):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return out


def cell(us):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(us), min(us), max(us))


def p(t):
    return C.c_void_p(t.data_ptr())


def rand(n):
    return torch.randint(0, 256, (max(n, 1),), dtype=torch.uint8, device="cuda")


def shape(bits, key, n, ml, calls, emit):
    """the rows of one (key size, record size, record count); returns the medians by call name"""
    texts, nonces, aads, keys = rand(n * ml), rand(n * NONCE), rand(n * AAD), rand(n * bits // 8)
    out, back = torch.zeros_like(texts), torch.zeros_like(texts)
    tags, stags = torch.zeros(n * 16, dtype=torch.uint8, device="cuda"), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    verdicts = torch.zeros(n, dtype=torch.uint8, device="cuda")
    sout = torch.zeros_like(texts)
    # the GCM record calls: ciphertext || tag per record, AAD at a stride of 16
    gaad, gout, gback = rand(n * 16), torch.zeros(n * (ml + 16), dtype=torch.uint8, device="cuda"), torch.zeros_like(texts)
    gk = C.c_void_p()
    assert L.uaes_gcm_key_new(C.byref(gk), bits, key) == 0
    enc = lambda: L.uaes_gcm_multikey_encrypt_batch(bits, p(keys), 16, n, ml, None, p(nonces), p(aads), AAD, p(texts), p(out), p(tags))
    dec = lambda: L.uaes_gcm_multikey_decrypt_batch(bits, p(keys), 16, n, ml, None, p(nonces), p(aads), AAD, p(out), p(tags), p(back),
                                                    p(verdicts))
    siv = lambda: L.uaes_gcmsiv_encrypt_batch(bits, key, n, ml, None, p(nonces), p(aads), AAD, p(texts), p(sout), p(stags))
    sivd = lambda: L.uaes_gcmsiv_decrypt_batch(bits, key, n, ml, None, p(nonces), p(aads), AAD, p(sout), p(stags), p(back), p(verdicts))
    gcm = lambda: L.uaes_gcm_key_encrypt_records(gk, n, p(nonces), p(gaad), AAD, 16, p(texts), ml, ml, p(gout), ml + 16)
    gcmd = lambda: L.uaes_gcm_key_decrypt_records(gk, n, p(nonces), p(gaad), AAD, 16, p(gout), ml, ml + 16, p(gback), ml, None)
    assert enc() == 0 and dec() == 0 and torch.equal(back, texts) and not torch.equal(out, texts) and bool(verdicts.all())
    assert siv() == 0 and gcm() == 0 and gcmd() == 0 and torch.equal(gback, texts)
    plan = uaes.gcm_multikey_batch_plan(ml, n)
    splan = uaes.gcmsiv_batch_plan(ml, n)
    runs = (("gcm multi-key encrypt", enc, "%s %d x %d" % (plan[0], plan[2], plan[3])),
            ("gcm multi-key decrypt", dec, "%s %d x %d" % (plan[0], plan[2], plan[3])),
            ("gcm-siv encrypt (one key)", siv, "%s %d x %d" % (splan[0], splan[2], splan[3])),
            ("gcm-siv decrypt (one key)", sivd, "%s %d x %d" % (splan[0], splan[2], splan[3])),
            ("gcm records encrypt (one key)", gcm, "k_gcm_records"), ("gcm records decrypt (one key)", gcmd, "k_gcm_records"))
    med = {}
    for name, fn, pl in runs:
        assert fn() == 0, name
        us = reps_of(fn, calls)
        med[name] = statistics.median(us)
        emit("| AES-%d | %d B | 2^%d | %s | %s | %s | %.3g | %.0f | %.2f |" % (
            bits, ml, n.bit_length() - 1, name, pl, cell(us), n / med[name] * 1e6, n * ml / med[name] * 1e6 / (1 << 20),
            med[name] * 1e3 / n))
    L.uaes_gcm_key_free(gk)
    return med


def xaes_main(quick, out_path):
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    emit("# XAES-256-GCM batches: measured rates\n")
    emit("Output of `tools/gcm_multikey_rate.py --xaes` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d "
         "windows after a warm-up window; the calls are synchronous, so every figure includes the host round trip.  "
         "Device-resident arrays; %d bytes of AAD per record, 16-byte tags; 24-byte nonces for XAES-256-GCM, 12-byte nonces "
         "and a 32-byte key per record for the multi-key rows, which run in the same process on the same texts.\n"
         % (props.name, props.multi_processor_count, REPS, AAD))
    if quick:
        emit("(Run with `--quick`: fewer calls per window.)\n")
    emit("Row steps per record, from the code: k_xaes_gcm_batch does what k_gcm_multikey<14> does and one two-block step of "
         "the cipher in front of it (the two halves of the nonce's key under the master key); it reads 24 bytes of nonce "
         "where the multi-key kernel reads 32 bytes of key and 12 of nonce.\n")
    emit("| record | records | call | plan | us per call | records per second | MiB/s of text | ns per record |\n"
         "|---|---|---|---|---|---|---|---|")
    key = (C.c_uint8 * 32).from_buffer_copy(bytes(range(32)))
    n, calls = 1 << 20, 3 if quick else 10
    ratios = []
    for ml in (16, 64, 1024):
        texts, xnonces, aads, keys = rand(n * ml), rand(n * 24), rand(n * AAD), rand(n * 32)
        out, back = torch.zeros_like(texts), torch.zeros_like(texts)
        mout = torch.zeros_like(texts)
        tags, mtags = torch.zeros(n * 16, dtype=torch.uint8, device="cuda"), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        verdicts = torch.zeros(n, dtype=torch.uint8, device="cuda")
        xenc = lambda: L.uaes_xaes256gcm_encrypt_batch(key, n, ml, None, p(xnonces), p(aads), AAD, p(texts), p(out), p(tags))
        xdec = lambda: L.uaes_xaes256gcm_decrypt_batch(key, n, ml, None, p(xnonces), p(aads), AAD, p(out), p(tags), p(back), p(verdicts))
        menc = lambda: L.uaes_gcm_multikey_encrypt_batch(256, p(keys), 16, n, ml, None, p(xnonces), p(aads), AAD, p(texts), p(mout), p(mtags))
        mdec = lambda: L.uaes_gcm_multikey_decrypt_batch(256, p(keys), 16, n, ml, None, p(xnonces), p(aads), AAD, p(mout), p(mtags), p(back),
                                                         p(verdicts))
        assert xenc() == 0 and xdec() == 0 and torch.equal(back, texts) and not torch.equal(out, texts) and bool(verdicts.all())
        assert menc() == 0 and mdec() == 0 and torch.equal(back, texts) and bool(verdicts.all())
        xplan, mplan = uaes.xaes256gcm_batch_plan(ml, n), uaes.gcm_multikey_batch_plan(ml, n)
        med = {}
        for name, fn, pl in (("xaes-256-gcm encrypt", xenc, xplan), ("xaes-256-gcm decrypt", xdec, xplan),
                             ("gcm multi-key encrypt, AES-256", menc, mplan), ("gcm multi-key decrypt, AES-256", mdec, mplan)):
            assert fn() == 0, name
            us = reps_of(fn, calls)
            med[name] = statistics.median(us)
            emit("| %d B | 2^20 | %s | %s %d x %d | %s | %.3g | %.0f | %.2f |" % (
                ml, name, pl[0], pl[2], pl[3], cell(us), n / med[name] * 1e6, n * ml / med[name] * 1e6 / (1 << 20), med[name] * 1e3 / n))
        ratios.append((ml, med["xaes-256-gcm encrypt"] / med["gcm multi-key encrypt, AES-256"],
                       med["xaes-256-gcm decrypt"] / med["gcm multi-key decrypt, AES-256"]))
        del texts, out, back, mout
        torch.cuda.empty_cache()
    emit("")
    emit("Time of an XAES-256-GCM batch call as a multiple of the multi-key AES-256 call at the same shape:\n")
    emit("| record | encrypt | decrypt |\n|---|---|---|")
    for ml, e, d in ratios:
        emit("| %d B | %.2f | %.2f |" % (ml, e, d))
    emit("")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


def main():
    quick = "--quick" in sys.argv
    if "--xaes" in sys.argv:
        return xaes_main(quick, sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                         else os.path.join(ROOT, "profiles", "xaes_gcm_batch_rate.md"))
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "gcm_multikey_batch_rate.md")
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    emit("# Multi-key GCM batches: measured rates\n")
    emit("Output of `tools/gcm_multikey_rate.py` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows "
         "after a warm-up window; the calls are synchronous, so every figure includes the host round trip.  "
         "Device-resident arrays, the keys included; 12-byte nonces, %d bytes of AAD per record, 16-byte tags.  The multi-key "
         "rows give every record a key of its own; the GCM-SIV and GCM-record rows run under one key.\n"
         % (props.name, props.multi_processor_count, REPS, AAD))
    if quick:
        emit("(Run with `--quick`: fewer calls per window.)\n")
    emit("Row steps per record, from the code (one block of the cipher or one hash block each): 10 / 13 serial SubWords of "
         "key expansion (AES-128 / AES-256), one step for H and Enc(J0), the hash key, then ceil(aad / 16) + ceil(len / 16) "
         "+ 1 hash blocks and ceil(len / 16) keystream blocks; decrypt walks the text twice (hash, then keystream).  GCM-SIV "
         "adds 2 + keybits / 64 derivation blocks and a tag block; the GCM records share H and its tables between all "
         "records.\n")
    keys = {bits: (C.c_uint8 * (bits // 8)).from_buffer_copy(bytes(range(bits // 8))) for bits in (128, 256)}
    head = ("| key | record | records | call | plan | us per call | records per second | MiB/s of text | ns per record |\n"
            "|---|---|---|---|---|---|---|---|---|")

    emit("## 2^10 records of 16 bytes: one call against 2^10 calls\n")
    emit(head)
    n, ml = 1 << 10, 16
    singles_rows = []
    for bits in (128, 256):
        med = shape(bits, keys[bits], n, ml, 50 if quick else 200, emit)
        texts, aads = rand(n * ml), rand(n * AAD)
        outs = torch.zeros(n * (ml + 16), dtype=torch.uint8, device="cuda")
        nonce = [(C.c_uint8 * NONCE).from_buffer_copy(bytes((7 * m + i) & 0xff for i in range(NONCE))) for m in range(n)]
        kb = bits // 8
        skey = [(C.c_uint8 * kb).from_buffer_copy(bytes((11 * m + 3 * i) & 0xff for i in range(kb))) for m in range(n)]
        tb, ob, ab = texts.data_ptr(), outs.data_ptr(), aads.data_ptr()

        def singles():
            for m in range(n):
                L.uaes_gcm_encrypt(bits, skey[m], nonce[m], C.c_void_p(ab + m * AAD), AAD, C.c_void_p(tb + m * ml), ml,
                                   C.c_void_p(ob + m * (ml + 16)))
        assert L.uaes_gcm_encrypt(bits, skey[0], nonce[0], C.c_void_p(ab), AAD, C.c_void_p(tb), ml, C.c_void_p(ob)) == 0
        us = [u / n for u in reps_of(singles, 1, 3 if quick else REPS)]
        one = statistics.median(us)
        singles_rows.append("| AES-%d | 16 B | 2^10 uaes_gcm_encrypt, a key each | %.2f (%.2f .. %.2f) | %.3g | %.1f |"
                            % (bits, one, min(us), max(us), 1e6 / one, med["gcm multi-key encrypt"] / one))
    emit("")
    emit("| key | record | calls | us per call | records per second | the batch call of 2^10 records, in single calls |\n|---|---|---|---|---|---|")
    for r in singles_rows:
        emit(r)
    emit("\n(Looped through ctypes: the call overhead of about a microsecond is inside these figures.)\n")

    emit("## 2^20 records\n")
    emit(head)
    n = 1 << 20
    ratios = []
    for bits in (128, 256):
        for ml in (16, 64, 1024):
            med = shape(bits, keys[bits], n, ml, 3 if quick else 10, emit)
            ratios.append((bits, ml, med["gcm multi-key encrypt"] / med["gcm-siv encrypt (one key)"],
                           med["gcm multi-key decrypt"] / med["gcm-siv decrypt (one key)"],
                           med["gcm multi-key encrypt"] / med["gcm records encrypt (one key)"],
                           med["gcm multi-key decrypt"] / med["gcm records decrypt (one key)"]))
            torch.cuda.empty_cache()
    emit("")
    emit("Time of a multi-key GCM batch call as a multiple of the other two at the same shape (encrypt, decrypt):\n")
    emit("| key | record | / gcm-siv batch | / gcm records |\n|---|---|---|---|")
    for bits, ml, se, sd, ge, gd in ratios:
        emit("| AES-%d | %d B | %.2f, %.2f | %.2f, %.2f |" % (bits, ml, se, sd, ge, gd))
    emit("")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
