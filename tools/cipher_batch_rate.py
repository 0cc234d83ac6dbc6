#!/usr/bin/env python3
"""Cipher batch rates, written as markdown (to profiles/cipher_batch_rate.md unless --out names another file):
  batch     device-resident records through the seven cipher batches (uaes_cbc_decrypt_batch, uaes_cbc_*_blocks_batch,
            uaes_cfb_*_batch, uaes_ofb_xcrypt_batch, uaes_ctr_xcrypt_batch): one call of 2^10 records of 16 bytes,
            2^20 records of 16, 64 and 1024 bytes, and 2^16 records of 64 and 1024 bytes (where uaes_cbc_encrypt_batch
            still is the sixteen-lane arrangement the cipher batches are)
  beside    uaes_ccm_encrypt_batch at every shape, timed TWICE (the difference of the two is the run-to-run spread the
            conditions below allow), and uaes_cbc_encrypt_batch at every shape
  single    2^10 one-message calls of every mode, one record each, on the same device-resident data
Two conditions are checked and printed: the CTR batch takes no longer than the CCM batch at the same shape, and CBC over
blocks (encrypt) takes as long as uaes_cbc_encrypt_batch, both within the spread of the two CCM runs.
Every figure: warm-up, then REPS repetitions; median, minimum and maximum.  The calls are synchronous, so every figure
includes the host round trip.  AES-128 and AES-256.
Usage: cipher_batch_rate.py [--out FILE] [--quick]"""
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
NONCE, TAG, AAD = 13, 8, 13                     # the CCM comparator's, as tools/ccm_rate.py has them
# (log2 records, bytes per record).  2^16 records is where uaes_cbc_encrypt_batch still runs sixteen lanes per record, the
# arrangement of the cipher batches; at 2^20 it runs one lane per record
SHAPES = ((10, 16), (16, 64), (16, 1024), (20, 16), (20, 64), (20, 1024))
# mode -> (batch entry point, takes lens, the one-message call as f(bits, key, iv, in, len, out))
MODES = {
    "cbc decrypt (CS3)": ("uaes_cbc_decrypt_batch", False, lambda b, k, v, i, n, o: L.uaes_cbc_decrypt(b, k, v, i, n, o)),
    "cbc decrypt blocks": ("uaes_cbc_decrypt_blocks_batch", False, lambda b, k, v, i, n, o: L.uaes_cbc_decrypt_blocks(b, k, v, i, n, o)),
    "cbc encrypt blocks": ("uaes_cbc_encrypt_blocks_batch", False, lambda b, k, v, i, n, o: L.uaes_cbc_encrypt_padded(b, k, v, 0, i, n, o)),
    "cfb encrypt": ("uaes_cfb_encrypt_batch", True, lambda b, k, v, i, n, o: L.uaes_cfb_encrypt(b, k, v, i, n, o)),
    "cfb decrypt": ("uaes_cfb_decrypt_batch", True, lambda b, k, v, i, n, o: L.uaes_cfb_decrypt(b, k, v, i, n, o)),
    "ofb": ("uaes_ofb_xcrypt_batch", True, lambda b, k, v, i, n, o: L.uaes_ofb_xcrypt(b, k, v, i, n, o)),
    "ctr": ("uaes_ctr_xcrypt_batch", True, lambda b, k, v, i, n, o: L.uaes_ctr_xcrypt_at(b, k, v, 0, i, n, o)),
}


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


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "cipher_batch_rate.md")
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    emit("# Cipher batches: measured rates\n")
    emit("Output of `tools/cipher_batch_rate.py` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows "
         "after a warm-up window; the calls are synchronous, so every figure includes the host round trip.  Device-resident "
         "arrays; the CCM comparator has %d-byte nonces, %d-byte tags and %d bytes of AAD per record.\n"
         % (props.name, props.multi_processor_count, REPS, NONCE, TAG, AAD))
    if quick:
        emit("(Run with `--quick`: fewer calls per window.)\n")
    emit("Row steps per record of b blocks, from the code: CBC encrypt over blocks, CFB encrypt, OFB b; CBC decrypt over "
         "blocks, CFB decrypt, CTR ceil(b / 2); CBC decrypt with the swap ceil((b - 2) / 2) + 1 from two blocks on; CCM "
         "1 + ceil((2 + aad) / 16) + b; uaes_cbc_encrypt_batch b (sixteen lanes per record up to 81 919 records, one lane "
         "per record beyond: at 2^20 records it is another arrangement than the cipher batches').\n")
    verdicts = []
    for bits in (128, 256):
        key = (C.c_uint8 * (bits // 8)).from_buffer_copy(bytes(range(bits // 8)))
        emit("## AES-%d\n" % bits)
        emit("| record | records | call | us per call | records per second | GiB/s of text | 2^10 one-message calls, us EACH |\n|---|---|---|---|---|---|---|")
        for lg, ml in SHAPES:
            n = 1 << lg
            texts = torch.randint(0, 256, (n * ml,), dtype=torch.uint8, device="cuda")
            ivs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda")
            nonces = torch.randint(0, 256, (n * NONCE,), dtype=torch.uint8, device="cuda")
            aads = torch.randint(0, 256, (n * AAD,), dtype=torch.uint8, device="cuda")
            out, back = torch.zeros_like(texts), torch.zeros_like(texts)
            tags = torch.zeros(n * TAG, dtype=torch.uint8, device="cuda")
            calls = (3 if quick else 8) if lg == 20 else (10 if quick else 40) if lg == 16 else (50 if quick else 200)
            med = {}

            def batch_fn(name, src, dst):
                entry, has_lens = MODES[name][:2]
                f = getattr(L, entry)
                a = (bits, key, p(ivs), n, ml) + ((None,) if has_lens else ()) + (p(src), p(dst))
                return lambda: f(*a)
            # correctness first: every decrypting form undoes its encrypting one, OFB and CTR undo themselves
            for enc, dec in (("cbc encrypt blocks", "cbc decrypt blocks"), ("cfb encrypt", "cfb decrypt"), ("ofb", "ofb"), ("ctr", "ctr")):
                back.zero_()
                assert batch_fn(enc, texts, out)() == 0 and batch_fn(dec, out, back)() == 0
                assert torch.equal(back, texts) and not torch.equal(out, texts), (enc, lg, ml)
            back.zero_()
            assert L.uaes_cbc_encrypt_batch(bits, key, p(ivs), n, ml, p(texts), p(out)) == 0
            assert batch_fn("cbc decrypt (CS3)", out, back)() == 0 and torch.equal(back, texts)
            singles = {}
            if lg == 10:                                      # the one-message calls on the same records
                iv_h = [(C.c_uint8 * 16).from_buffer_copy(bytes((7 * m + i) & 0xff for i in range(16))) for m in range(n)]
                tb, ob = texts.data_ptr(), out.data_ptr()
                for name, (_, _, one) in MODES.items():
                    def loop(one=one):
                        for m in range(n):
                            one(bits, key, iv_h[m], C.c_void_p(tb + m * ml), ml, C.c_void_p(ob + m * ml))
                    assert one(bits, key, iv_h[0], C.c_void_p(tb), ml, C.c_void_p(ob)) == 0
                    singles[name] = statistics.median([u / n for u in reps_of(loop, 1, 3 if quick else 5)])
            runs = [(name, batch_fn(name, texts, out)) for name in MODES]
            ccm = lambda: L.uaes_ccm_encrypt_batch(bits, key, NONCE, TAG, n, ml, None, p(nonces), p(aads), AAD, p(texts), p(out), p(tags))
            cbc = lambda: L.uaes_cbc_encrypt_batch(bits, key, p(ivs), n, ml, p(texts), p(out))
            runs = [("ccm encrypt batch, first run", ccm)] + runs + [("uaes_cbc_encrypt_batch", cbc), ("ccm encrypt batch, second run", ccm)]
            for name, fn in runs:
                assert fn() == 0, name
                us = reps_of(fn, calls)
                med[name] = statistics.median(us)
                emit("| %d B | 2^%d | %s | %s | %.3g | %.1f | %s |" % (ml, lg, name, cell(us), n / med[name] * 1e6,
                                                                     n * ml / med[name] * 1e6 / (1 << 30),
                                                                     ("%.1f" % singles[name]) if name in singles else ""))
            c1, c2 = med["ccm encrypt batch, first run"], med["ccm encrypt batch, second run"]
            spread = abs(c1 - c2)
            ok_ctr = med["ctr"] <= min(c1, c2) + spread
            ok_cbc = abs(med["cbc encrypt blocks"] - med["uaes_cbc_encrypt_batch"]) <= spread or \
                med["cbc encrypt blocks"] <= med["uaes_cbc_encrypt_batch"]
            verdicts.append("AES-%d, 2^%d x %d B: CCM %.1f and %.1f us (spread %.1f); CTR %.1f us: %s; CBC over blocks %.1f us "
                            "against uaes_cbc_encrypt_batch (%s) %.1f us, %+.1f us: %s"
                            % (bits, lg, ml, c1, c2, spread, med["ctr"], "holds" if ok_ctr else "FAILS", med["cbc encrypt blocks"],
                               uaes.chain_plan("cbc_batch", ml, n)[0], med["uaes_cbc_encrypt_batch"],
                               med["cbc encrypt blocks"] - med["uaes_cbc_encrypt_batch"], "holds" if ok_cbc else "FAILS"))
            del texts, ivs, nonces, aads, out, back, tags
            torch.cuda.empty_cache()
        emit("")
    emit("## The two conditions\n")
    emit("The CTR batch must not take longer than the CCM batch at the same shape, and CBC over blocks (encrypt) must not "
         "take longer than uaes_cbc_encrypt_batch, either beyond the spread the two CCM runs show.\n")
    for v in verdicts:
        emit("- " + v)
    emit("\n(The one-message calls are looped through ctypes: the call overhead of about a microsecond is inside their figures.)\n")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
