#!/usr/bin/env python3
"""SIV (RFC 5297) with a vector of associated data: measured rates, written as markdown (to profiles/siv_v_rate.md unless
--out names another file).  With --parent FILE, FILE is a libuaes_hip.so built from the parent commit, loaded beside
this tree's; the two are timed in turn in the same process:
  regression   uaes_siv_encrypt and uaes_siv_decrypt at 64 B, 16 KiB, 16 KiB + 1 and 1 MiB of text, uaes_siv_encrypt_batch
               at 2^10 / 2^16 / 2^20 records of 16 / 64 / 1024 B.  Every shape: parent, parent again (the difference of
               the two is the run-to-run spread), then new, parent, new.  No call of this tree may be slower than the
               parent by more than that spread.
  one part     the _v calls with ONE component at the same shapes, against the parent's one-aData call
  components   one small call (64 B of text) with 1, 4, 16, 64 and 126 components of 64 B, and the one-aData call over
               the same bytes concatenated (another IV: S2V binds the boundaries; it shows what a serial chain costs)
  batch        2^20 records of 64 B with the components (13 B, a 16 B nonce) in one uaes_siv_encrypt_batch_v call,
               against 2^10 uaes_siv_encrypt_v calls, extrapolated
The library this tree loads first and the one --parent names second do not sit in the same place in the process: run the
tool once more with --parent naming a COPY of this tree's library to see that arrangement's own offset (the control
section of profiles/siv_v_rate.md).
Every figure: a warm-up window, then REPS windows; the median of their microseconds per call (minimum .. maximum).  The
calls are synchronous, so every figure includes the host round trip.  Device-resident arrays.  AES-128 and AES-256.
Usage: siv_v_rate.py [--parent FILE] [--out FILE] [--quick]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import micro_aes_amd as uaes

NEW = uaes.engine()
REPS = 7
AAD = 32                                        # bytes of associated data in the regression shapes
SINGLE = (64, 16384, 16385, 1 << 20)
BATCH = ((10, 16), (10, 64), (10, 1024), (16, 16), (16, 64), (16, 1024), (20, 16), (20, 64), (20, 1024))


def parent_library(path):
    L = C.CDLL(path)
    i, vp, sz = C.c_int, C.c_void_p, C.c_size_t
    L.uaes_siv_encrypt.argtypes = [i, vp, vp, sz, vp, sz, vp, vp]
    L.uaes_siv_decrypt.argtypes = [i, vp, vp, vp, sz, vp, sz, vp]
    L.uaes_siv_encrypt_batch.argtypes = [i, vp, sz, sz, vp, sz, vp, vp, vp]
    return L


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


def compare(emit, verdicts, what, old, new, one, calls, parent):
    """one shape: parent, parent, new, parent, new (and the one-component _v call); returns the medians"""
    assert new() == 0 and one() == 0
    if parent:
        assert old() == 0
        runs = [reps_of(old, calls), reps_of(old, calls), reps_of(new, calls), reps_of(old, calls), reps_of(new, calls)]
        pm = [statistics.median(r) for r in (runs[0], runs[1], runs[3])]
        nm = [statistics.median(r) for r in (runs[2], runs[4])]
        spread, base, mine = max(pm) - min(pm), statistics.median(pm), statistics.median(nm)
        ok = mine <= base + spread
        verdicts.append("%s: parent %.1f us (spread %.1f), new %.1f us, %+.1f us: %s" % (what, base, spread, mine, mine - base,
                                                                                         "holds" if ok else "FAILS"))
    else:
        runs = [reps_of(new, calls)]
        base = spread = None
        mine = statistics.median(runs[0])
    v = reps_of(one, calls)
    vm = statistics.median(v)
    emit("| %s | %s | %s | %s | %s | %s |" % (what, ("%.1f / %.1f / %.1f" % tuple(pm)) if parent else "not measured",
                                             ("%.1f" % spread) if parent else "", " / ".join("%.1f" % statistics.median(r) for r in (runs[2:5:2] if parent else runs)),
                                             cell(v), ("%+.1f" % (vm - base)) if parent else ""))
    return base, mine, vm


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "siv_v_rate.md")
    OLD = parent_library(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    rows, verdicts = [], []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    emit("# SIV with a vector of associated data: measured rates\n")
    emit("Output of `tools/siv_v_rate.py%s` on %s (%d CUs).  Microseconds per call are medians of %d windows after a warm-up "
         "window (minimum .. maximum where one run is shown); the calls are synchronous, so every figure includes the host "
         "round trip.  Device-resident arrays; %d bytes of associated data in the regression shapes.\n"
         % (" --parent FILE" if OLD else "", props.name, props.multi_processor_count, REPS, AAD))
    if quick:
        emit("(Run with `--quick`: fewer calls per window.)\n")
    if not OLD:
        emit("No parent library was given: the parent columns and the regression verdicts are not measured.\n")
    size_t = C.c_size_t
    for bits in (128, 256):
        keys = (C.c_uint8 * (bits // 4)).from_buffer_copy(bytes(range(bits // 4)))
        emit("## AES-%d: the one-aData calls against the parent, and the _v calls with one component\n" % bits)
        emit("| call and shape | parent: run 1 / 2 / 3 | spread | new: run 1 / 2 | _v, one component | _v minus parent |\n|---|---|---|---|---|---|")
        one_len = (size_t * 1)(AAD)
        for n in SINGLE:
            aad, src, dst, iv = rand(AAD), rand(n), rand(n), rand(16)
            calls = (3 if quick else 6) if n >= 1 << 20 else (20 if quick else 60) if n > 1024 else (50 if quick else 200)
            for dec in (0, 1):
                if dec:
                    assert NEW.uaes_siv_encrypt(bits, keys, p(aad), AAD, p(src), n, p(iv), p(dst)) == 0
                    a, b = dst, src.clone()
                    f = lambda L: (lambda: L.uaes_siv_decrypt(bits, keys, p(iv), p(aad), AAD, p(a), n, p(b)))
                    one = lambda: NEW.uaes_siv_decrypt_v(bits, keys, p(iv), 1, one_len, p(aad), p(a), n, p(b))
                else:
                    f = lambda L: (lambda: L.uaes_siv_encrypt(bits, keys, p(aad), AAD, p(src), n, p(iv), p(dst)))
                    one = lambda: NEW.uaes_siv_encrypt_v(bits, keys, 1, one_len, p(aad), p(src), n, p(iv), p(dst))
                compare(emit, verdicts, "AES-%d uaes_siv_%s, %d B" % (bits, "decrypt" if dec else "encrypt", n),
                        f(OLD) if OLD else None, f(NEW), one, calls, OLD)
        for lg, ml in BATCH:
            n = 1 << lg
            aads, src, dst, ivs = rand(n * AAD), rand(n * ml), rand(n * ml), rand(n * 16)
            calls = (3 if quick else 6) if lg == 20 else (10 if quick else 40) if lg == 16 else (50 if quick else 200)
            f = lambda L: (lambda: L.uaes_siv_encrypt_batch(bits, keys, n, ml, p(aads), AAD, p(src), p(ivs), p(dst)))
            one = lambda: NEW.uaes_siv_encrypt_batch_v(bits, keys, n, ml, None, 1, one_len, p(aads), p(src), p(ivs), p(dst))
            compare(emit, verdicts, "AES-%d uaes_siv_encrypt_batch, 2^%d x %d B" % (bits, lg, ml), f(OLD) if OLD else None, f(NEW),
                    one, calls, OLD)
            del aads, src, dst, ivs
            torch.cuda.empty_cache()
        emit("")
        emit("## AES-%d: what the vector buys\n" % bits)
        emit("| one call, 64 B of text | uaes_siv_encrypt_v, us | uaes_siv_encrypt over the same bytes as ONE aData, us |\n|---|---|---|")
        src, dst, iv = rand(64), rand(64), rand(16)
        for nad in (1, 4, 16, 64, 126):
            ad, lens = rand(64 * nad), (size_t * nad)(*([64] * nad))
            v = reps_of(lambda: NEW.uaes_siv_encrypt_v(bits, keys, nad, lens, p(ad), p(src), 64, p(iv), p(dst)), 50 if quick else 200)
            o = reps_of(lambda: NEW.uaes_siv_encrypt(bits, keys, p(ad), 64 * nad, p(src), 64, p(iv), p(dst)), 50 if quick else 200)
            emit("| %d components of 64 B | %s | %s |" % (nad, cell(v), cell(o)))
        emit("")
        n, ml, shape = 1 << 20, 64, (13, 16)
        lens2 = (size_t * 2)(*shape)
        ads, src, dst, ivs = rand(n * sum(shape)), rand(n * ml), rand(n * ml), rand(n * 16)
        b = reps_of(lambda: NEW.uaes_siv_encrypt_batch_v(bits, keys, n, ml, None, 2, lens2, p(ads), p(src), p(ivs), p(dst)), 3 if quick else 6)
        ab, sb, db, ib = ads.data_ptr(), src.data_ptr(), dst.data_ptr(), ivs.data_ptr()
        vp = C.c_void_p

        def loop():
            for m in range(1024):
                NEW.uaes_siv_encrypt_v(bits, keys, 2, lens2, vp(ab + 29 * m), vp(sb + ml * m), ml, vp(ib + 16 * m), vp(db + ml * m))
        s = [u / 1024 for u in reps_of(loop, 1, 3)]
        bm, sm = statistics.median(b), statistics.median(s)
        emit("2^20 records of %d B with the components (13 B, 16 B): one uaes_siv_encrypt_batch_v call %s us, %.3g records per "
             "second; 2^10 uaes_siv_encrypt_v calls take %s us EACH, so 2^20 of them would take %.0f us: the batch is %.0f times "
             "faster.\n" % (ml, cell(b), n / bm * 1e6, cell(s), sm * n, sm * n / bm))
        del ads, src, dst, ivs
        torch.cuda.empty_cache()
    emit("## No regression\n")
    if OLD:
        emit("A call of this tree must not take longer than the parent's by more than the spread of the parent's own three runs.\n")
        for v in verdicts:
            emit("- " + v)
    else:
        emit("Not measured: no parent library was given.")
    emit("\n(The one-message calls of the last comparison are looped through ctypes: the call overhead of about a microsecond is "
         "inside their figures.)\n")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
