#!/usr/bin/env python3
"""EAX' batch rates, written as markdown (to profiles/eaxp_batch_rate.md unless --out names another file): 2^20
device-resident records of 16, 64 and 1024 bytes with 32-byte nonces through uaes_eaxp_encrypt_batch /
uaes_eaxp_decrypt_batch, and beside each uaes_eax_encrypt_batch / uaes_eax_decrypt_batch at the same shape (32-byte
nonces, no associated data, its 16-byte tags) as the yardstick.
Every figure: warm-up, then REPS windows; median, minimum and maximum.  The calls are synchronous, so every figure
includes the host round trip.  AES-128.
Usage: eaxp_rate.py [--out FILE] [--quick]"""
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
REPS, NONCE, LG = 9, 32, 20


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


def p(t):
    return C.c_void_p(t.data_ptr())


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "eaxp_batch_rate.md")
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    key = (C.c_uint8 * 16).from_buffer_copy(bytes(range(16)))
    n, calls = 1 << LG, 3 if quick else 10
    emit("# EAX' batches: measured rates\n")
    emit("Output of `tools/eaxp_rate.py%s` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows of %d "
         "calls after a warm-up window; the calls are synchronous, so every figure includes the host round trip.  AES-128, "
         "2^%d records, device-resident arrays, %d-byte nonces, no lengths per record; EAX without associated data and with "
         "its 16-byte tags, EAX' with its 4-byte macs.\n" % (" --quick" if quick else "", props.name, props.multi_processor_count,
                                                              REPS, calls, LG, NONCE))
    emit("Blocks of the cipher per record, from the code: EAX' 1 (subkeys, per workgroup) + %d (nonce) + ceil(len / 16) steps "
         "of a keystream block and a chain block together (row_encrypt2) + 1; EAX the same plus 1 ([0]_16 in front of the "
         "nonce) + 1 (the empty header's OMAC) + 1 ([2]_16 in front of the text, paired with keystream block 0).\n" % (NONCE // 16))
    emit("| record | call | plan | us per call | records per second | GiB/s of text | ns per record, EAX' / EAX |\n|---|---|---|---|---|---|---|")
    ratios = []
    for ml in (16, 64, 1024):
        texts = torch.randint(0, 256, (n * ml,), dtype=torch.uint8, device="cuda")
        nonces = torch.randint(0, 256, (n * NONCE,), dtype=torch.uint8, device="cuda")
        out, back = torch.zeros_like(texts), torch.zeros_like(texts)
        macs = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        tags = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        verdicts = torch.zeros(n, dtype=torch.uint8, device="cuda")
        enc = lambda: L.uaes_eaxp_encrypt_batch(128, key, n, NONCE, None, p(nonces), ml, None, p(texts), p(out), p(macs))
        dec = lambda: L.uaes_eaxp_decrypt_batch(128, key, n, NONCE, None, p(nonces), ml, None, p(out), p(macs), p(back), p(verdicts))
        eax = lambda: L.uaes_eax_encrypt_batch(128, key, n, ml, p(nonces), NONCE, None, 0, p(texts), p(out), p(tags))
        eaxd = lambda: L.uaes_eax_decrypt_batch(128, key, n, ml, p(nonces), NONCE, None, 0, p(out), p(tags), p(back), p(verdicts))
        med = {}
        plan, eplan = uaes.eaxp_plan(ml, n), uaes.eax_siv_plan(False, ml, n)
        for name, fn, pl in (("eax encrypt", eax, eplan), ("eax decrypt", eaxd, eplan), ("eax' encrypt", enc, plan), ("eax' decrypt", dec, plan)):
            back.zero_()
            assert fn() == 0
            if "decrypt" in name:
                assert torch.equal(back, texts) and bool(verdicts.all())        # of the encryption right before it
            us = reps_of(fn, calls)
            med[name] = statistics.median(us)
            other = name.replace("eax'", "eax")
            ratio = "" if name == other else "%.2f / %.2f = %.2f" % (med[name] * 1e3 / n, med[other] * 1e3 / n, med[name] / med[other])
            emit("| %d B | %s | %s %d | %.1f (%.1f .. %.1f) | %.3g | %.1f | %s |" % (
                ml, name, pl[0], pl[2], med[name], min(us), max(us), n / med[name] * 1e6, n * ml / med[name] * 1e6 / (1 << 30), ratio))
        ratios.append((ml, med["eax' encrypt"] / med["eax encrypt"], med["eax' decrypt"] / med["eax decrypt"]))
        del texts, nonces, out, back, macs, tags, verdicts
        torch.cuda.empty_cache()
    emit("")
    emit("EAX' against EAX in the same direction (time per call, encrypt, decrypt): "
         + ", ".join("%d B: %.2f, %.2f" % r for r in ratios) + ".\n")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
