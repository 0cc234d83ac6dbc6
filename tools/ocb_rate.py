#!/usr/bin/env python3
"""OCB batch rates, written as markdown (to profiles/ocb_batch_rate.md unless --out names another file):
  batch     device-resident records of 16, 64 and 1024 bytes at 2^10, 2^16 and 2^20 records through
            uaes_ocb_encrypt_batch / uaes_ocb_decrypt_batch (12-byte nonces, 16-byte tags, 12 bytes of AAD per record),
            and beside each uaes_ccm_encrypt_batch / uaes_ccm_decrypt_batch at the same shape, in the same run
  single    2^10 uaes_ocb_encrypt_ex calls, one record each, on the same device-resident data
Every figure: warm-up, then REPS repetitions; median, minimum and maximum.  The calls are synchronous, so every figure
includes the host round trip.  AES-128.
Usage: ocb_rate.py [--out FILE] [--quick]"""
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
NONCE, TAG, AAD = 12, 16, 12


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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ocb_batch_rate.md")
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    key = (C.c_uint8 * 16).from_buffer_copy(bytes(range(16)))
    emit("# OCB batches: measured rates\n")
    emit("Output of `tools/ocb_rate.py` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows after "
         "a warm-up window; the calls are synchronous, so every figure includes the host round trip.  AES-128, "
         "device-resident arrays, %d-byte nonces, %d-byte tags, %d bytes of AAD per record, for OCB and CCM alike.\n"
         % (props.name, props.multi_processor_count, REPS, NONCE, TAG, AAD))
    if quick:
        emit("(Run with `--quick`: fewer calls per window.)\n")
    emit("## Batches\n")
    emit("Row steps per record, from the code (a = blocks of AAD, the ragged one included, b = whole blocks of text, r = 1 "
         "for a ragged one): OCB 1 (K_top || A_1) + ceil((a - 1) / 2) + floor(b / 2), then encrypting ceil((b % 2 + r + 1) / "
         "2) (the last odd block, the pad and the tag in pairs), decrypting b % 2 + r + 1 (one after the other, and every "
         "forward block of a decrypting record goes through the plain Te0); CCM 1 + ceil((2 + aad) / 16) + ceil(len / 16).  "
         "At these shapes, OCB encrypt / OCB decrypt / CCM: 16 B 2 / 3 / 3, 64 B 4 / 4 / 6, 1024 B 34 / 34 / 66.  The 64-byte "
         "shape is the one that compares the two directions of OCB step for step: two of the decrypting record's four "
         "steps (K_top || A_1 and the tag) read the plain table.\n")
    emit("The last column sets an OCB call against the CCM call of the same direction.\n")
    emit("| record | records | call | plan | us per call | records per second | MiB/s of text | ns per record, OCB / CCM |\n"
         "|---|---|---|---|---|---|---|---|")
    ratios, med_at = [], {}
    for ml in (16, 64, 1024):
        for lg in (10, 16, 20):
            n = 1 << lg
            texts = torch.randint(0, 256, (n * ml,), dtype=torch.uint8, device="cuda")
            nonces = torch.randint(0, 256, (n * NONCE,), dtype=torch.uint8, device="cuda")
            aads = torch.randint(0, 256, (n * AAD,), dtype=torch.uint8, device="cuda")
            out, back, cout = torch.zeros_like(texts), torch.zeros_like(texts), torch.zeros_like(texts)
            tags = torch.zeros(n * TAG, dtype=torch.uint8, device="cuda")
            ctags = torch.zeros(n * TAG, dtype=torch.uint8, device="cuda")
            verdicts = torch.zeros(n, dtype=torch.uint8, device="cuda")
            enc = lambda: L.uaes_ocb_encrypt_batch(128, key, NONCE, TAG, n, ml, None, p(nonces), p(aads), AAD, p(texts), p(out), p(tags))
            dec = lambda: L.uaes_ocb_decrypt_batch(128, key, NONCE, TAG, n, ml, None, p(nonces), p(aads), AAD, p(out), p(tags),
                                                   p(back), p(verdicts))
            ccm = lambda: L.uaes_ccm_encrypt_batch(128, key, NONCE, TAG, n, ml, None, p(nonces), p(aads), AAD, p(texts), p(cout), p(ctags))
            ccmd = lambda: L.uaes_ccm_decrypt_batch(128, key, NONCE, TAG, n, ml, None, p(nonces), p(aads), AAD, p(cout), p(ctags),
                                                    p(back), p(verdicts))
            assert enc() == 0 and dec() == 0 and torch.equal(back, texts) and not torch.equal(out, texts) and bool(verdicts.all())
            back.zero_()
            assert ccm() == 0 and ccmd() == 0 and torch.equal(back, texts) and bool(verdicts.all())
            plan = uaes.ocb_batch_plan(ml, n)
            cplan = uaes.chain_plan("ccm_batch", ml, n)
            calls = (3 if quick else 10) if lg == 20 else (10 if quick else 40) if lg == 16 else (50 if quick else 200)
            med, cells = {}, {}
            runs = (("ocb encrypt", enc, "%s %d x %d" % (plan[0], plan[2], plan[3])),
                    ("ocb decrypt", dec, "%s %d x %d" % (plan[0], plan[2], plan[3])),
                    ("ccm encrypt", ccm, "%s %d x %d" % (cplan[0], cplan[2], cplan[3])),
                    ("ccm decrypt", ccmd, "%s %d x %d" % (cplan[0], cplan[2], cplan[3])))
            for name, fn, _ in runs:
                assert fn() == 0
                us = reps_of(fn, calls)
                med[name], cells[name] = statistics.median(us), cell(us)
            assert torch.equal(back, texts) and bool(verdicts.all())
            for name, _, pl in runs:
                other = name.replace("ocb", "ccm")
                ratio = "" if name == other else "%.2f / %.2f = %.2f" % (med[name] * 1e3 / n, med[other] * 1e3 / n, med[name] / med[other])
                emit("| %d B | 2^%d | %s | %s | %s | %.3g | %.0f | %s |" % (ml, lg, name, pl, cells[name], n / med[name] * 1e6,
                                                                         n * ml / med[name] * 1e6 / (1 << 20), ratio))
            ratios.append((ml, lg, med["ocb encrypt"] / med["ccm encrypt"], med["ocb decrypt"] / med["ccm decrypt"]))
            med_at[(ml, lg)] = dict(med)
            del texts, nonces, aads, out, back, cout, tags, ctags, verdicts
            torch.cuda.empty_cache()
    emit("")
    emit("OCB time / CCM time (encrypt, decrypt): " + ", ".join("%d B x 2^%d: %.2f, %.2f" % r for r in ratios) + ".\n")
    big = [r for r in ratios if r[0] == 1024]
    faster = [r for r in big if r[2] < 1.0 and r[3] < 1.0]
    emit("At 1024-byte records, where an OCB record has about half the serial steps of a CCM record, OCB is the faster one "
         "in both directions at %d of the %d record counts%s.\n"
         % (len(faster), len(big), "" if len(faster) == len(big) else
            " (not at: " + ", ".join("2^%d: encrypt %.2f, decrypt %.2f" % (lg, e, d) for _, lg, e, d in big if e >= 1.0 or d >= 1.0) + ")"))
    emit("An OCB decryption against the OCB encryption of the same shape (us per call more, ratio): " +
         ", ".join("%d B x 2^%d: %+.1f, %.2f" % (ml, lg, m["ocb decrypt"] - m["ocb encrypt"], m["ocb decrypt"] / m["ocb encrypt"])
                   for (ml, lg), m in med_at.items()) +
         ".  Beside it, what a decrypting CCM call -- whose kernel has one table set and one direction -- costs more than "
         "an encrypting one at the same shape, mostly the host side's clearing and fetching of the failure word: " +
         ", ".join("%d B x 2^%d: %+.1f" % (ml, lg, m["ccm decrypt"] - m["ccm encrypt"]) for (ml, lg), m in med_at.items()) +
         " us.  Only where OCB's difference is the larger of the two does the decrypting OCB kernel show a cost of its "
         "own.  What the code has there that the encrypting kernel has not (not timed apart): its forward blocks "
         "(K_top || A_1, the pad, the tag) read the plain, unreplicated Te0, where the lanes of a wave can meet on LDS "
         "banks; pad and tag are two steps, not one; it requests its text half as far ahead.\n")
    emit("## One call per record\n")
    emit("| record | calls | us per call | records per second | one 2^10-record batch call, us |\n|---|---|---|---|---|")
    n = 1 << 10
    for ml in (16, 64, 1024):
        texts = torch.randint(0, 256, (n * ml,), dtype=torch.uint8, device="cuda")
        outs = torch.zeros(n * (ml + 16), dtype=torch.uint8, device="cuda")
        aads = torch.randint(0, 256, (n * AAD,), dtype=torch.uint8, device="cuda")
        nonce = [(C.c_uint8 * NONCE).from_buffer_copy(bytes((7 * m + i) & 0xff for i in range(NONCE))) for m in range(n)]
        tb, ob, ab = texts.data_ptr(), outs.data_ptr(), aads.data_ptr()

        def singles():
            for m in range(n):
                L.uaes_ocb_encrypt_ex(128, key, nonce[m], NONCE, TAG, C.c_void_p(ab + m * AAD), AAD, C.c_void_p(tb + m * ml), ml,
                                      C.c_void_p(ob + m * (ml + 16)))
        assert L.uaes_ocb_encrypt_ex(128, key, nonce[0], NONCE, TAG, C.c_void_p(ab), AAD, C.c_void_p(tb), ml, C.c_void_p(ob)) == 0
        us = [u / n for u in reps_of(singles, 1, 3 if quick else REPS)]
        emit("| %d B | 2^10 uaes_ocb_encrypt_ex | %s | %.3g | %.1f |"
             % (ml, "%.2f (%.2f .. %.2f)" % (statistics.median(us), min(us), max(us)), 1e6 / statistics.median(us),
                med_at[(ml, 10)]["ocb encrypt"]))
    emit("\n(Looped through ctypes: the call overhead of about a microsecond is inside these figures.)\n")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
