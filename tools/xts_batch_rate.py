#!/usr/bin/env python3
"""XTS batch rates, written as markdown (to profiles/xts_batch_rate.md unless --out names another file):
  batch     device-resident units through uaes_xts_encrypt_batch, uaes_xts_decrypt_batch and uaes_xts_sector_list: one
            call of 2^10 units of 16 bytes, and 2^20 units of 16, 64, 512, 1024 and 4096 bytes
  beside    uaes_ctr_xcrypt_batch at every shape, timed TWICE, first and last (the difference of the two is the
            run-to-run spread the conditions allow), and uaes_xts_sectors over the same bytes as contiguous sectors
  single    2^10 one-unit uaes_xts_encrypt / uaes_xts_decrypt calls, one unit each, on the same device-resident data
No ratio is fixed in advance.  What can be derived is the row-step ratio against the CTR batch, (1 + ceil(b / 2)) :
ceil(b / 2) for b whole blocks; the measured ratio is printed beside it, with the excess in microseconds.
Every figure: warm-up, then REPS repetitions; median, minimum and maximum.  The calls are synchronous, so every figure
includes the host round trip.  AES-128 and AES-256, both directions.
Usage: xts_batch_rate.py [--out FILE] [--quick]"""
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
SHAPES = ((10, 16), (20, 16), (20, 64), (20, 512), (20, 1024), (20, 4096))     # (log2 units, bytes per unit)
FIRST_SECTOR = 0x123456789


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


def reading(excess, emit):
    """excess: (bits, log2 units, bytes) -> (excess in us, the encrypting call in us, whether uaes_xts_sectors was faster)"""
    emit("\n## What the excess is, and where the contiguous call wins\n")
    for bits in (128, 256):
        pct = ", ".join("%d B %+.1f %%" % (ml, 100 * x / e) for (kb, lg, ml), (x, e, _) in sorted(excess.items()) if kb == bits and lg == 20)
        wins = [ml for (kb, lg, ml), (_, _, run_wins) in sorted(excess.items()) if kb == bits and lg == 20 and run_wins]
        loses = [ml for (kb, lg, ml), (_, _, run_wins) in sorted(excess.items()) if kb == bits and lg == 20 and not run_wins]
        emit("- AES-%d, 2^20 units: excess as a share of the encrypting call: %s.  uaes_xts_sectors is the faster call for a "
             "contiguous run at %s bytes per unit, the batch at %s." % (bits, pct, ", ".join(map(str, wins)) or "no size",
                                                                        ", ".join(map(str, loses)) or "no size"))
    emit("\nWhere the excess is negative the call is not its row steps: a short unit's time is what every row batch pays per "
         "launch and per unit -- the table fill, the unit's loads and stores, the host round trip -- and the CTR batch pays "
         "the same, so the measured ratio stays below the derived one.  Where it is positive it is what a step of the XTS "
         "batch does and a step of the CTR batch does not: per pair of blocks two multiplications of T (one DPP move, a "
         "shift and the fold each) and the XOR of T into both blocks on either side of the cipher, where CTR XORs once; per "
         "launch key 2's schedule and, decrypting, the 1 KiB plain table behind the inverse tables, whose lookups the one "
         "tweak block of every unit takes (the sixteen lanes of a row share its banks).  The parts were not timed apart and "
         "no counters were collected.\n")
    emit("A contiguous run of equal sectors remains uaes_xts_sectors' job wherever the list above says so: it spreads a "
         "unit's blocks over many lanes and derives the tweaks of a chunk from one another, where the batch walks each unit "
         "on sixteen lanes.  The batch and the sector list are for what that call cannot take: scattered sector numbers, a "
         "raw tweak per unit, lengths per unit.\n")


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "xts_batch_rate.md")
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    emit("# XTS batches: measured rates\n")
    emit("Output of `tools/xts_batch_rate.py` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows "
         "after a warm-up window; the calls are synchronous, so every figure includes the host round trip.  Device-resident "
         "arrays (texts, tweaks, sector numbers); the key pair in host memory.  `xts sectors` is uaes_xts_sectors over the "
         "same bytes as one contiguous run of sectors from %#x.\n" % (props.name, props.multi_processor_count, REPS, FIRST_SECTOR))
    if quick:
        emit("(Run with `--quick`: fewer calls per window.)\n")
    emit("Row steps per unit of b whole blocks, from the code: the XTS batch 1 + ceil(b / 2) (T = Enc_key2(tweak), then two "
         "blocks per step), the CTR batch ceil(b / 2).  The derived ratio is that of the steps; the measured one is the "
         "encrypting XTS batch over the mean of the two CTR runs.\n")
    summary, excess = [], {}
    for bits in (128, 256):
        keys = (C.c_uint8 * (bits // 4)).from_buffer_copy(bytes((3 * i + 1) & 0xff for i in range(bits // 4)))
        emit("## AES-%d\n" % bits)
        emit("| unit | units | call | us per call | units per second | GiB/s of text | 2^10 one-unit calls, us EACH |\n|---|---|---|---|---|---|---|")
        for lg, ml in SHAPES:
            n = 1 << lg
            texts = torch.randint(0, 256, (n * ml,), dtype=torch.uint8, device="cuda")
            tweaks = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda")
            ctrs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda")
            sectors = torch.arange(FIRST_SECTOR, FIRST_SECTOR + n, dtype=torch.int64, device="cuda")
            out, back = torch.zeros_like(texts), torch.zeros_like(texts)
            calls = (3 if quick else 8) if lg == 20 else (50 if quick else 200)
            enc = lambda: L.uaes_xts_encrypt_batch(bits, keys, p(tweaks), n, ml, None, p(texts), p(out))
            dec = lambda: L.uaes_xts_decrypt_batch(bits, keys, p(tweaks), n, ml, None, p(texts), p(out))
            lst = lambda: L.uaes_xts_sector_list(bits, keys, p(sectors), n, ml, p(texts), p(out), 1)
            lsd = lambda: L.uaes_xts_sector_list(bits, keys, p(sectors), n, ml, p(texts), p(out), 0)
            run = lambda: L.uaes_xts_sectors(bits, keys, FIRST_SECTOR, ml, n, p(texts), p(out), 1)
            rud = lambda: L.uaes_xts_sectors(bits, keys, FIRST_SECTOR, ml, n, p(texts), p(out), 0)
            ctr = lambda: L.uaes_ctr_xcrypt_batch(bits, keys, p(ctrs), n, ml, None, p(texts), p(out))
            # correctness first: decrypting undoes encrypting, and a contiguous list is the contiguous call
            assert enc() == 0 and L.uaes_xts_decrypt_batch(bits, keys, p(tweaks), n, ml, None, p(out), p(back)) == 0
            assert torch.equal(back, texts) and not torch.equal(out, texts), (bits, lg, ml)
            assert lst() == 0 and L.uaes_xts_sectors(bits, keys, FIRST_SECTOR, ml, n, p(texts), p(back), 1) == 0
            assert torch.equal(back, out), (bits, lg, ml, "sector list")
            singles = {}
            if lg == 10:                                      # the one-unit calls on the same units
                tw_h = [(C.c_uint8 * 16).from_buffer_copy(bytes((7 * m + i) & 0xff for i in range(16))) for m in range(n)]
                tb, ob = texts.data_ptr(), out.data_ptr()
                for name, one in (("xts encrypt batch", L.uaes_xts_encrypt), ("xts decrypt batch", L.uaes_xts_decrypt)):
                    def loop(one=one):
                        for m in range(n):
                            one(bits, keys, tw_h[m], C.c_void_p(tb + m * ml), ml, C.c_void_p(ob + m * ml))
                    assert one(bits, keys, tw_h[0], C.c_void_p(tb), ml, C.c_void_p(ob)) == 0
                    singles[name] = statistics.median([u / n for u in reps_of(loop, 1, 3 if quick else 5)])
            med = {}
            for name, fn in (("ctr batch, first run", ctr), ("xts encrypt batch", enc), ("xts sectors, encrypt", run),
                             ("xts decrypt batch", dec), ("xts sectors, decrypt", rud), ("xts sector list, encrypt", lst),
                             ("xts sector list, decrypt", lsd), ("ctr batch, second run", ctr)):
                assert fn() == 0, name
                us = reps_of(fn, calls)
                med[name] = statistics.median(us)
                emit("| %d B | 2^%d | %s | %s | %.3g | %.1f | %s |" % (ml, lg, name, cell(us), n / med[name] * 1e6,
                                                                     n * ml / med[name] * 1e6 / (1 << 30),
                                                                     ("%.1f" % singles[name]) if name in singles else ""))
            c1, c2 = med["ctr batch, first run"], med["ctr batch, second run"]
            cm, b = (c1 + c2) / 2, ml // 16
            derived = (1 + (b + 1) // 2) / ((b + 1) // 2)
            e, d = med["xts encrypt batch"], med["xts decrypt batch"]
            summary.append("| AES-%d | 2^%d x %d B | %.1f, %.1f (spread %.1f) | %.1f | %.1f | %d : %d = %.3f | %.3f | %+.1f | %.3f | %.1f / %.1f | %s |"
                           % (bits, lg, ml, c1, c2, abs(c1 - c2), e, d, 1 + (b + 1) // 2, (b + 1) // 2, derived, e / cm,
                              e - derived * cm, d / cm, med["xts sectors, encrypt"], med["xts sectors, decrypt"],
                              "the batch" if e <= med["xts sectors, encrypt"] else "xts sectors"))
            excess[(bits, lg, ml)] = (e - derived * cm, e, med["xts sectors, encrypt"] < e)
            del texts, tweaks, ctrs, sectors, out, back
            torch.cuda.empty_cache()
        emit("")
    emit("## Against the CTR batch and the contiguous call\n")
    emit("Microseconds per call (medians).  Excess = the encrypting batch minus the derived ratio times the CTR batch: what "
         "the row steps do not explain.\n")
    emit("| key | shape | ctr batch, two runs | xts encrypt batch | xts decrypt batch | derived ratio | measured, encrypt | excess, us "
         "| measured, decrypt | xts sectors, encrypt / decrypt | faster for a contiguous run |\n|---|---|---|---|---|---|---|---|---|---|---|")
    for s in summary:
        emit(s)
    reading(excess, emit)
    emit("(The one-unit calls are looped through ctypes: the call overhead of about a microsecond is inside their figures.)\n")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
