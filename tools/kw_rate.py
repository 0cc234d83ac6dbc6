#!/usr/bin/env python3
"""AES key wrap (RFC 3394) and key wrap with padding (RFC 5649) rates, written as markdown (to profiles/kw_rate.md unless
--out names another file).  Key wrap:
  latency   one 32-byte secret through uaes_kw_wrap / uaes_kw_unwrap, host data and device data (host round trip
            included: the calls are synchronous)
  batch     65 536 secrets of 32 bytes, device-resident, uaes_kw_wrap_batch / uaes_kw_unwrap_batch: keys per second
  per step  one long chain (64 KiB of secret, kw.global) in both directions against a short one: microseconds per chain
            step of row_encrypt and of row_decrypt, next to the per-block time of the CMAC chain (row_encrypt) over the
            same number of blocks in the same run
  cpu       the compiled reference's AES_KEY_wrap / AES_KEY_unwrap looped on one host core (oracle/_ref)
Key wrap with padding, in the same run (kwp_sections):
  latency   one secret of 7, 20, 32, 4096 and 4097 bytes through uaes_kwp_wrap / uaes_kwp_unwrap, host and device data
  batch     2^10 and 2^20 records of 20, 32 and 256 bytes, device-resident, both directions; at 32 and 256 bytes the KW
            batch of the same shape is timed twice, once before and once after the KWP batch, and the spread of those two
            runs is the margin the KWP batch is held against
  mixed     2^20 records whose lengths cycle through 1, 8, 9 and 256 (lens) against 2^20 records of 256 bytes
Every figure: warm-up, then REPS repetitions; median, minimum and maximum.  AES-128 unless said otherwise.
Usage: kw_rate.py [--out FILE] [--quick]"""
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
    return "%.2f (%.2f .. %.2f)" % (statistics.median(us), min(us), max(us))


def dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")


def kwp_sections(emit, quick):
    """key wrap with padding beside key wrap (the module's docstring); the outputs are checked before they are timed"""
    bits = 128
    kek = (C.c_uint8 * 16).from_buffer_copy(bytes(range(16)))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    emit("# AES key wrap with padding (RFC 5649): measured rates, same run\n")
    emit("## Latency of one secret, AES-128\n")
    emit("| call | bytes | arrangement | data | us per call |\n|---|---|---|---|---|")
    for m in (7, 20, 32, 4096, 4097):
        secret = bytes((37 * i + 11) & 0xFF for i in range(m))
        rc, wrapped = uaes.kwp_wrap(bytes(kek), secret)
        assert rc == 0 and uaes.kwp_unwrap(bytes(kek), wrapped)[0::2] == (0, m)
        wl, ln = len(wrapped), C.c_size_t(0)
        hs, hw, ho = (C.c_uint8 * m).from_buffer_copy(secret), (C.c_uint8 * wl).from_buffer_copy(wrapped), (C.c_uint8 * wl)()
        ds, dw, do = dev(secret), dev(wrapped), dev(bytes(wl + 64))
        calls = (20 if quick else 50) if m > 1024 else (100 if quick else 400)
        name = uaes.kwp_plan(m)[0]
        for data, a, b, o in (("host", hs, hw, ho), ("device", ptr(ds), ptr(dw), ptr(do))):
            emit("| uaes_kwp_wrap | %d | %s | %s | %s |" % (m, name, data, cell(reps_of(lambda: L.uaes_kwp_wrap(bits, kek, a, m, o), calls))))
            emit("| uaes_kwp_unwrap | %d | %s | %s | %s |" %
                 (m, name, data, cell(reps_of(lambda: L.uaes_kwp_unwrap(bits, kek, b, wl, o, C.byref(ln)), calls))))
        assert bytes(do.cpu().numpy())[:m] == secret and ln.value == m
    emit("")
    top = 1 << 14 if quick else 1 << 20
    slot_max = 256
    secrets = torch.randint(0, 256, (top * slot_max,), dtype=torch.uint8, device="cuda")
    wrapped = torch.zeros(top * (slot_max + 8), dtype=torch.uint8, device="cuda")
    wrapped_kw = torch.zeros(top * (slot_max + 8), dtype=torch.uint8, device="cuda")      # each family unwraps its own
    back = torch.zeros(top * slot_max, dtype=torch.uint8, device="cuda")
    ver = torch.zeros(top, dtype=torch.uint8, device="cuda")
    lo = torch.zeros(top, dtype=torch.int32, device="cuda")
    p_s, p_w, p_k, p_b, p_v, p_l = (ptr(t) for t in (secrets, wrapped, wrapped_kw, back, ver, lo))

    def kw_pair(n, size):
        assert L.uaes_kw_wrap_batch(bits, kek, n, size, p_s, p_k) == 0
        assert L.uaes_kw_unwrap_batch(bits, kek, n, size + 8, p_k, p_b, p_v) == 0
        assert torch.equal(back[:n * size], secrets[:n * size]) and int(ver[:n].sum()) == n
        return (lambda: L.uaes_kw_wrap_batch(bits, kek, n, size, p_s, p_k),
                lambda: L.uaes_kw_unwrap_batch(bits, kek, n, size + 8, p_k, p_b, p_v))

    def kwp_pair(n, size, lens=None, wlens=None, expect=None):
        ws = (size + 7) // 8 * 8 + 8
        assert L.uaes_kwp_wrap_batch(bits, kek, n, size, lens, p_s, p_w) == 0
        assert L.uaes_kwp_unwrap_batch(bits, kek, n, ws, wlens, p_w, p_b, p_l, p_v) == 0
        assert int(ver[:n].sum()) == n and int(lo[:n].sum()) == (expect if expect is not None else n * size)
        if lens is None and size % 8 == 0:
            assert torch.equal(back[:n * size], secrets[:n * size])
        return (lambda: L.uaes_kwp_wrap_batch(bits, kek, n, size, lens, p_s, p_w),
                lambda: L.uaes_kwp_unwrap_batch(bits, kek, n, ws, wlens, p_w, p_b, p_l, p_v))

    emit("## Batches, device-resident, AES-128: KWP beside the KW batch of the same shape\n")
    emit("Each KW shape is timed twice, before (A) and after (B) the KWP batch of that shape.  The margin is the spread "
         "of those two runs: (largest - smallest window) / median over the windows of both.  The KWP batch runs the same "
         "chain plus the length check, so its median is held against the median of the two KW runs plus that margin.\n")
    emit("| records | bytes | direction | KW A, us | KWP, us | KW B, us | KWP / KW | margin | verdict |\n|---|---|---|---|---|---|---|---|---|")
    verdicts = []
    for n in ((1 << 10, top) if not quick else (1 << 10,)):
        calls = 5 if n > 1 << 16 else 40
        for size in (20, 32, 256):
            kwp = kwp_pair(n, size)
            if size % 8:
                for d in (0, 1):
                    emit("| %d | %d | %s | - | %s | - | - | - | KW takes no such length |" %
                         (n, size, ("wrap", "unwrap")[d], cell(reps_of(kwp[d], calls))))
                continue
            kw = kw_pair(n, size)
            for d in (0, 1):
                a = reps_of(kw[d], calls)
                p = reps_of(kwp[d], calls)
                b = reps_of(kw[d], calls)
                both = a + b
                margin = (max(both) - min(both)) / statistics.median(both)
                ratio = statistics.median(p) / statistics.median(both)
                ok = ratio <= 1 + margin
                verdicts.append((n, size, d, ratio, margin, ok))
                emit("| %d | %d | %s | %s | %s | %s | %.3f | %.3f | %s |" %
                     (n, size, ("wrap", "unwrap")[d], cell(a), cell(p), cell(b), ratio, margin, "within" if ok else "EXCEEDS"))
    emit("")
    over = [v for v in verdicts if not v[5]]
    if over:
        emit("KWP exceeds the margin at %s.  This tool times whole calls: it does not say where inside the call the "
             "time goes; that was not found here.\n" %
             ", ".join("%d x %d B %s (%.3f against 1 + %.3f)" % (n, size, ("wrap", "unwrap")[d], r, m) for n, size, d, r, m, _ in over))
    else:
        emit("KWP stays within the margin at every shape KW can be timed at.\n")
    n = top
    cyc = torch.tensor([1, 8, 9, 256], dtype=torch.int32, device="cuda").repeat(n // 4)
    wcyc = (cyc + 7) // 8 * 8 + 8
    expect = int(cyc.sum())
    mixed = kwp_pair(n, 256, ptr(cyc), ptr(wcyc), expect)
    uniform = kwp_pair(n, 256)
    emit("## A batch of mixed lengths against a uniform one: %d records, slots of 256 bytes, lens cycling 1, 8, 9, 256\n" % n)
    emit("A wave costs its longest row, and every wave of the mixed batch holds one 256-byte record, so the mixed batch "
         "cannot take longer than the uniform one but for its lens array; it moves about a quarter of the bytes.\n")
    emit("| direction | uniform 256 B, us | mixed, us | mixed / uniform |\n|---|---|---|---|")
    for d in (0, 1):
        u = reps_of(uniform[d], 5)
        x = reps_of(mixed[d], 5)
        emit("| %s | %s | %s | %.3f |" % (("wrap", "unwrap")[d], cell(u), cell(x), statistics.median(x) / statistics.median(u)))
    emit("")


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kw_rate.md")
    rows = []

    def emit(line):                                       # printed as it comes: a long run shows where it is
        rows.append(line)
        print(line, flush=True)
    props = torch.cuda.get_device_properties(0)
    emit("# AES key wrap (RFC 3394): measured rates\n")
    emit("Output of `tools/kw_rate.py` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows "
         "after a warm-up window; the calls are synchronous, so every figure includes the host round trip.\n"
         % (props.name, props.multi_processor_count, REPS))
    for bits in (128, 256):
        kek = (C.c_uint8 * (bits // 8)).from_buffer_copy(bytes(range(bits // 8)))
        secret = bytes(range(32))
        rc, wrapped = uaes.AES_KEY_wrap(bytes(kek), secret)
        assert rc == 0
        hs, hw = (C.c_uint8 * 32).from_buffer_copy(secret), (C.c_uint8 * 40).from_buffer_copy(wrapped)
        ho = (C.c_uint8 * 40)()
        ds, dw, do = dev(secret), dev(wrapped), dev(bytes(64))
        ps, pw, po = (C.c_void_p(t.data_ptr()) for t in (ds, dw, do))
        emit("## Latency of one 32-byte secret, AES-%d\n" % bits)
        emit("| call | data | us per call |\n|---|---|---|")
        calls = 100 if quick else 400
        emit("| uaes_kw_wrap | host | %s |" % cell(reps_of(lambda: L.uaes_kw_wrap(bits, kek, hs, 32, ho), calls)))
        emit("| uaes_kw_unwrap | host | %s |" % cell(reps_of(lambda: L.uaes_kw_unwrap(bits, kek, hw, 40, ho), calls)))
        emit("| uaes_kw_wrap | device | %s |" % cell(reps_of(lambda: L.uaes_kw_wrap(bits, kek, ps, 32, po), calls)))
        emit("| uaes_kw_unwrap | device | %s |" % cell(reps_of(lambda: L.uaes_kw_unwrap(bits, kek, pw, 40, po), calls)))
        assert bytes(do.cpu().numpy())[:32] == secret
        emit("")
    kek = (C.c_uint8 * 16).from_buffer_copy(bytes(range(16)))
    nkeys = 65536
    secrets = torch.randint(0, 256, (nkeys * 32,), dtype=torch.uint8, device="cuda")
    wrapped = torch.zeros(nkeys * 40, dtype=torch.uint8, device="cuda")
    back = torch.zeros(nkeys * 32, dtype=torch.uint8, device="cuda")
    ver = torch.zeros(nkeys, dtype=torch.uint8, device="cuda")
    p_s, p_w, p_b, p_v = (C.c_void_p(t.data_ptr()) for t in (secrets, wrapped, back, ver))
    assert L.uaes_kw_wrap_batch(128, kek, nkeys, 32, p_s, p_w) == 0
    assert L.uaes_kw_unwrap_batch(128, kek, nkeys, 40, p_w, p_b, p_v) == 0
    assert torch.equal(back, secrets) and int(ver.sum()) == nkeys
    plan = uaes.kw_plan(32, nkeys)
    emit("## Batch of %d secrets of 32 bytes, device-resident, AES-128 (%s: %d workgroups of %d threads)\n" %
         (nkeys, plan[0], plan[2], plan[3]))
    emit("| call | us per call | keys per second (median) | chain steps per second |\n|---|---|---|---|")
    for name, fn in (("uaes_kw_wrap_batch", lambda: L.uaes_kw_wrap_batch(128, kek, nkeys, 32, p_s, p_w)),
                     ("uaes_kw_unwrap_batch", lambda: L.uaes_kw_unwrap_batch(128, kek, nkeys, 40, p_w, p_b, p_v))):
        us = reps_of(fn, 5 if quick else 20)
        med = statistics.median(us)
        emit("| %s | %s | %.3g | %.3g |" % (name, cell(us), nkeys / med * 1e6, nkeys * 24 / med * 1e6))
    emit("")
    # one chain: the cost of a step, from two lengths of the same arrangement
    short_n, long_n = 1024, 8192
    big = torch.randint(0, 256, (8 * long_n + 8,), dtype=torch.uint8, device="cuda")
    outb = torch.zeros(8 * long_n + 64, dtype=torch.uint8, device="cuda")
    wr = {n: torch.zeros(8 * n + 8, dtype=torch.uint8, device="cuda") for n in (short_n, long_n)}
    p_i, p_o = C.c_void_p(big.data_ptr()), C.c_void_p(outb.data_ptr())
    p_wr = {n: C.c_void_p(t.data_ptr()) for n, t in wr.items()}
    msg = torch.randint(0, 256, (16 * 6 * long_n,), dtype=torch.uint8, device="cuda")
    p_m = C.c_void_p(msg.data_ptr())
    mac = (C.c_uint8 * 16)()
    emit("## One chain: microseconds per step (kw.global, %d against %d semiblocks; CMAC over as many blocks)\n" % (long_n, short_n))
    emit("| chain | AES | us per step or block |\n|---|---|---|")
    per = {}
    for bits in (128, 256):
        k = (C.c_uint8 * (bits // 8)).from_buffer_copy(bytes(range(bits // 8)))
        assert uaes.kw_plan(8 * short_n)[0] == "kw.global"
        for n in (short_n, long_n):                       # the unwrap is timed on what the wrap made: authentic, rc 0
            assert L.uaes_kw_wrap(bits, k, p_i, 8 * n, p_wr[n]) == 0
            assert L.uaes_kw_unwrap(bits, k, p_wr[n], 8 * n + 8, p_o) == 0
            assert torch.equal(outb[:8 * n], big[:8 * n])
        for name, fn in (("wrap (row_encrypt)", lambda n: L.uaes_kw_wrap(bits, k, p_i, 8 * n, p_o)),
                         ("unwrap (row_decrypt)", lambda n: L.uaes_kw_unwrap(bits, k, p_wr[n], 8 * n + 8, p_o)),
                         ("CMAC (row_encrypt)", lambda n: L.uaes_cmac(bits, k, p_m, 16 * 6 * n, mac))):
            calls = 3 if quick else 6
            a = reps_of(lambda: fn(long_n), calls)
            b = reps_of(lambda: fn(short_n), calls)
            steps = [(x - y) / (6 * (long_n - short_n)) for x, y in zip(sorted(a), sorted(b))]
            per[name, bits] = statistics.median(steps)
            emit("| %s | %d | %.4f (%.4f .. %.4f) |" % (name, bits, per[name, bits], min(steps), max(steps)))
    emit("")
    for bits in (128, 256):
        emit("AES-%d: a step of the unwrap chain takes %.2f times a step of the wrap chain, and a wrap step %.2f times a "
             "block of the CMAC chain.\n" % (bits, per["unwrap (row_decrypt)", bits] / per["wrap (row_encrypt)", bits],
                                             per["wrap (row_encrypt)", bits] / per["CMAC (row_encrypt)", bits]))
    ref = os.path.join(ROOT, "oracle", "_ref", "libmicroaes_ref_128.so")
    if os.path.exists(ref):
        R = C.CDLL(ref)
        for n in ("AES_KEY_wrap", "AES_KEY_unwrap"):
            getattr(R, n).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        secret = (C.c_uint8 * 32).from_buffer_copy(bytes(range(32)))
        w, o = (C.c_uint8 * 40)(), (C.c_uint8 * 40)()
        R.AES_KEY_wrap(kek, secret, 32, w)
        loops = 2000 if quick else 20000
        emit("## The reference on one host core of the same machine, 32-byte secrets, AES-128\n")
        emit("| call | us per call | keys per second (median) |\n|---|---|---|")
        for name, fn in (("AES_KEY_wrap", lambda: R.AES_KEY_wrap(kek, secret, 32, o)),
                         ("AES_KEY_unwrap", lambda: R.AES_KEY_unwrap(kek, w, 40, o))):
            us = []
            for _ in range(REPS + 1):
                t0 = time.perf_counter()
                for _ in range(loops):
                    fn()
                us.append((time.perf_counter() - t0) / loops * 1e6)
            us = us[1:]
            emit("| %s | %s | %.3g |" % (name, cell(us), 1e6 / statistics.median(us)))
        emit("\n(Looped through ctypes: the call overhead of about a microsecond is inside these figures.)\n")
    kwp_sections(emit, quick)
    text = "\n".join(rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
