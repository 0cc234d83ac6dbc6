#!/usr/bin/env python3
"""CCM batch rates, written as markdown (to profiles/ccm_batch_rate.md unless --out names another file):
  batch     device-resident records of 16, 64 and 1024 bytes at 2^10, 2^16 and 2^20 records through
            uaes_ccm_encrypt_batch / uaes_ccm_decrypt_batch (13-byte nonces, 8-byte tags, 13 bytes of AAD per record),
            and beside each uaes_eax_encrypt_batch / uaes_eax_decrypt_batch at the same shape (13-byte nonces, 13
            bytes of AAD, its 16-byte tags)
  single    2^10 uaes_ccm_encrypt_ex calls, one record each, on the same device-resident data
Every figure: warm-up, then REPS repetitions; median, minimum and maximum.  The calls are synchronous, so every figure
includes the host round trip.  AES-128.
Usage: ccm_rate.py [--out FILE] [--quick]"""
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
NONCE, TAG, AAD = 13, 8, 13


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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ccm_batch_rate.md")
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    key = (C.c_uint8 * 16).from_buffer_copy(bytes(range(16)))
    emit("# CCM batches: measured rates\n")
    emit("Output of `tools/ccm_rate.py` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows after "
         "a warm-up window; the calls are synchronous, so every figure includes the host round trip.  AES-128, "
         "device-resident arrays, %d-byte nonces, %d bytes of AAD per record; CCM tags of %d bytes, EAX tags of 16.\n"
         % (props.name, props.multi_processor_count, REPS, NONCE, AAD, TAG))
    if quick:
        emit("(Run with `--quick`: fewer calls per window.)\n")
    emit("## Batches\n")
    emit("Row steps per record, from the code: CCM 1 + ceil((2 + aad) / 16) + ceil(len / 16), every step a MAC block "
         "and a counter block together (row_encrypt2); EAX encrypt 1 (subkeys, per workgroup) + 2 (nonce) + 2 (AAD) + "
         "1 + ceil(len / 16), the text steps and the one before them doubled the same way.\n")
    emit("The last column sets a CCM call against the EAX call of the same direction.\n")
    emit("| record | records | call | plan | us per call | records per second | MiB/s of text | ns per record, CCM / EAX |\n"
         "|---|---|---|---|---|---|---|---|")
    ratios, extra = [], []
    for ml in (16, 64, 1024):
        for lg in (10, 16, 20):
            n = 1 << lg
            texts = torch.randint(0, 256, (n * ml,), dtype=torch.uint8, device="cuda")
            nonces = torch.randint(0, 256, (n * NONCE,), dtype=torch.uint8, device="cuda")
            aads = torch.randint(0, 256, (n * AAD,), dtype=torch.uint8, device="cuda")
            out, back = torch.zeros_like(texts), torch.zeros_like(texts)
            tags = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            etags = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            verdicts = torch.zeros(n, dtype=torch.uint8, device="cuda")
            enc = lambda: L.uaes_ccm_encrypt_batch(128, key, NONCE, TAG, n, ml, None, p(nonces), p(aads), AAD, p(texts), p(out), p(tags))
            dec = lambda: L.uaes_ccm_decrypt_batch(128, key, NONCE, TAG, n, ml, None, p(nonces), p(aads), AAD, p(out), p(tags),
                                                   p(back), p(verdicts))
            eax = lambda: L.uaes_eax_encrypt_batch(128, key, n, ml, p(nonces), NONCE, p(aads), AAD, p(texts), p(back), p(etags))
            eaxd = lambda: L.uaes_eax_decrypt_batch(128, key, n, ml, p(nonces), NONCE, p(aads), AAD, p(back), p(etags), p(out),
                                                    p(verdicts))
            assert enc() == 0 and dec() == 0 and torch.equal(back, texts) and not torch.equal(out, texts) and bool(verdicts.all())
            plan = uaes.chain_plan("ccm_batch", ml, n)
            eplan = uaes.eax_siv_plan(False, ml, n)
            calls = (3 if quick else 10) if lg == 20 else (10 if quick else 40) if lg == 16 else (50 if quick else 200)
            med, cells = {}, {}
            runs = (("ccm encrypt", enc, "%s %d x %d" % (plan[0], plan[2], plan[3])),
                    ("ccm decrypt", dec, "%s %d x %d" % (plan[0], plan[2], plan[3])),
                    ("eax encrypt", eax, "%s %d" % (eplan[0], eplan[2])),
                    ("eax decrypt", eaxd, "%s %d" % (eplan[0], eplan[2])))
            for name, fn, _ in runs:
                assert fn() == 0
                us = reps_of(fn, calls)
                med[name], cells[name] = statistics.median(us), cell(us)
            assert torch.equal(out, texts) and bool(verdicts.all())             # (the EAX decryption's plaintext)
            for name, _, pl in runs:
                other = name.replace("ccm", "eax")
                ratio = "" if name == other else "%.2f / %.2f = %.2f" % (med[name] * 1e3 / n, med[other] * 1e3 / n, med[name] / med[other])
                emit("| %d B | 2^%d | %s | %s | %s | %.3g | %.0f | %s |" % (ml, lg, name, pl, cells[name], n / med[name] * 1e6,
                                                                         n * ml / med[name] * 1e6 / (1 << 20), ratio))
            ratios.append((ml, lg, med["ccm encrypt"] / med["eax encrypt"], med["ccm decrypt"] / med["eax decrypt"]))
            extra.append((ml, lg, med["ccm decrypt"] - med["ccm encrypt"], med["ccm decrypt"] / med["eax encrypt"]))
            del texts, nonces, aads, out, back, tags, etags, verdicts
            torch.cuda.empty_cache()
    emit("")
    slower = [(ml, lg, e, d) for ml, lg, e, d in ratios if e > 1.0 or d > 1.0]
    emit("CCM takes no more time per record than the EAX batch at %d of the %d shapes.%s\n"
         % (len(ratios) - len(slower), len(ratios),
            "" if not slower else "  Slower (encrypt, decrypt, each against EAX in the same direction): " +
            ", ".join("%d B x 2^%d: %.2f, %.2f" % s for s in slower) + "."))
    emit("A CCM decryption against the EAX ENCRYPTION of the same shape (us per call more than the CCM encryption, ratio "
         "to EAX encrypt): " + ", ".join("%d B x 2^%d: +%.1f, %.2f" % e for e in extra) + ".  What the code shows as "
         "the cause where that ratio is above 1: the kernel's decrypting direction is the encrypting one plus a tag load, "
         "a ballot and a verdict byte per record, but the host side of every decrypting batch (aead_rows_staged, "
         "uaes_engine_modes.c) clears the `bad` word before the launch (hipMemsetAsync) and fetches it after it "
         "(a hipMemcpyAsync to host memory in front of the stream synchronisation), which the encrypting call does "
         "not: a cost per call, not per record, that a short call cannot hide.\n")
    emit("## One call per record\n")
    emit("| record | calls | us per call | records per second |\n|---|---|---|---|")
    n = 1 << 10
    for ml in (16, 64, 1024):
        texts = torch.randint(0, 256, (n * ml,), dtype=torch.uint8, device="cuda")
        outs = torch.zeros(n * (ml + 16), dtype=torch.uint8, device="cuda")
        aads = torch.randint(0, 256, (n * AAD,), dtype=torch.uint8, device="cuda")
        nonce = [(C.c_uint8 * NONCE).from_buffer_copy(bytes((7 * m + i) & 0xff for i in range(NONCE))) for m in range(n)]
        tb, ob, ab = texts.data_ptr(), outs.data_ptr(), aads.data_ptr()

        def singles():
            for m in range(n):
                L.uaes_ccm_encrypt_ex(128, key, nonce[m], NONCE, TAG, C.c_void_p(ab + m * AAD), AAD, C.c_void_p(tb + m * ml), ml,
                                      C.c_void_p(ob + m * (ml + 16)))
        assert L.uaes_ccm_encrypt_ex(128, key, nonce[0], NONCE, TAG, C.c_void_p(ab), AAD, C.c_void_p(tb), ml, C.c_void_p(ob)) == 0
        us = [u / n for u in reps_of(singles, 1, 3 if quick else REPS)]
        emit("| %d B | 2^10 uaes_ccm_encrypt_ex | %s | %.3g |" % (ml, "%.2f (%.2f .. %.2f)" % (statistics.median(us), min(us), max(us)),
                                                                 1e6 / statistics.median(us)))
    emit("\n(Looped through ctypes: the call overhead of about a microsecond is inside these figures.)\n")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
