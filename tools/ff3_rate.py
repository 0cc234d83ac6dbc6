#!/usr/bin/env python3
"""FF3-1 (SP 800-38G revision 1) rates, written as markdown (to profiles/ff3_rate.md unless --out names another file):
  batch     16-digit decimal records, device-resident, uaes_ff3_encrypt_batch / uaes_ff3_decrypt_batch at 2^10, 2^16
            and 2^20 records, with one tweak for all records and with a tweak per record: records per second.  The
            yardstick is the FF1 batch of the same shape (uaes_ff1_encrypt_batch, 8-byte tweaks), measured in the same
            run: FF3-1 does less cipher work per record (8 blocks against FF1's 10 MACs, S blocks and E(P)).
  latency   one 16-digit text through uaes_ff3_encrypt, host data and device data (the calls are synchronous: the host
            round trip is included)
  cpu       the engine's own host path (uaes_set_host_policy) looped on one host core
Every figure: warm-up, then REPS repetitions; median, minimum and maximum.  AES-128.
Usage: ff3_rate.py [--out FILE] [--quick]"""
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
DIGITS = 16
TWEAK = 7
FF1_TWEAK = 8
DEC = (C.c_uint8 * 10).from_buffer_copy(b"0123456789")


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


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ff3_rate.md")
    rows = []
    emit = rows.append
    props = torch.cuda.get_device_properties(0)
    key = (C.c_uint8 * 16).from_buffer_copy(bytes(range(16)))
    emit("# FF3-1 (SP 800-38G revision 1): measured rates\n")
    emit("Output of `tools/ff3_rate.py` on %s (%d CUs).  Microseconds are median (minimum .. maximum) of %d windows "
         "after a warm-up window; the calls are synchronous, so every figure includes the host round trip.  AES-128, "
         "decimal records of %d digits, tweaks of %d bytes (FF1 rows: %d).\n"
         % (props.name, props.multi_processor_count, REPS, DIGITS, TWEAK, FF1_TWEAK))
    if quick:
        emit("(Run with `--quick`: 5 calls per window for the 2^16 and 2^20 batches, 50 for 2^10, 100 for the 16-digit calls.)\n")
    emit("## Batches, device-resident\n")
    emit("| records | mode | tweak | call | plan | us per call | records per second (median) |\n|---|---|---|---|---|---|---|")
    for lg in (10, 16, 20):
        n = 1 << lg
        recs = (torch.randint(0, 10, (n * DIGITS,), dtype=torch.uint8, device="cuda") + 48).contiguous()
        tweaks = torch.randint(0, 256, (n * FF1_TWEAK,), dtype=torch.uint8, device="cuda")
        out = torch.zeros(n * DIGITS, dtype=torch.uint8, device="cuda")
        back = torch.zeros(n * DIGITS, dtype=torch.uint8, device="cuda")
        p_r, p_t, p_o, p_b = (C.c_void_p(t.data_ptr()) for t in (recs, tweaks, out, back))
        calls = (5 if quick else 20) if lg >= 16 else (50 if quick else 200)
        plan = uaes.ff3_plan(DIGITS, n)
        for label, stride in (("shared", 0), ("per record", TWEAK)):
            enc = lambda: L.uaes_ff3_encrypt_batch(128, key, 10, DEC, p_t, stride, n, DIGITS, p_r, p_o, None)
            dec = lambda: L.uaes_ff3_decrypt_batch(128, key, 10, DEC, p_t, stride, n, DIGITS, p_o, p_b, None)
            assert enc() == 0 and dec() == 0 and torch.equal(back, recs) and not torch.equal(out, recs)
            for name, fn in (("encrypt", enc), ("decrypt", dec)):
                us = reps_of(fn, calls)
                emit("| 2^%d | FF3-1 | %s | %s | %s %d x %d | %s | %.3g |" % (lg, label, name, plan[0], plan[2], plan[3], cell(us),
                                                                             n / statistics.median(us) * 1e6))
        plan = uaes.ff1_plan(DIGITS, n)                         # the yardstick, same records, same run
        ff1 = lambda: L.uaes_ff1_encrypt_batch(128, key, 10, DEC, p_t, FF1_TWEAK, 0, n, DIGITS, p_r, p_o, None)
        assert ff1() == 0
        us = reps_of(ff1, calls)
        emit("| 2^%d | FF1 | shared | encrypt | %s %d x %d | %s | %.3g |" % (lg, plan[0], plan[2], plan[3], cell(us),
                                                                            n / statistics.median(us) * 1e6))
    emit("")
    text = bytes(48 + (7 * i + 3) % 10 for i in range(DIGITS))
    tweak = (C.c_uint8 * TWEAK).from_buffer_copy(bytes(range(TWEAK)))
    h_in, h_out = (C.c_uint8 * DIGITS).from_buffer_copy(text), (C.c_uint8 * DIGITS)()
    d_in = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda")
    d_out = torch.zeros(DIGITS, dtype=torch.uint8, device="cuda")
    emit("## Latency of one call\n")
    emit("| call | data | plan | us per call |\n|---|---|---|---|")
    calls = 100 if quick else 400
    emit("| uaes_ff3_encrypt, %d digits | host | %s | %s |" % (DIGITS, uaes.ff3_plan(DIGITS)[0], cell(reps_of(
        lambda: L.uaes_ff3_encrypt(128, key, 10, DEC, tweak, h_in, DIGITS, h_out), calls))))
    emit("| uaes_ff3_encrypt, %d digits | device | %s | %s |" % (DIGITS, uaes.ff3_plan(DIGITS)[0], cell(reps_of(
        lambda: L.uaes_ff3_encrypt(128, key, 10, DEC, tweak, C.c_void_p(d_in.data_ptr()), DIGITS,
                                   C.c_void_p(d_out.data_ptr())), calls))))
    assert bytes(d_out.cpu().numpy()) == bytes(h_out)
    emit("")
    emit("## One host core of the same machine, %d-digit records\n" % DIGITS)
    emit("| call | us per call | records per second (median) |\n|---|---|---|")
    loops = 2000 if quick else 20000
    prev = uaes.host_policy(max_bytes=1 << 20, chains=1)
    g_out = (C.c_uint8 * DIGITS)()
    fn = lambda: L.uaes_ff3_encrypt(128, key, 10, DEC, tweak, h_in, DIGITS, g_out)
    fn()
    assert bytes(g_out) == bytes(h_out)                        # the host path and the GPU agree
    us = []
    for _ in range(REPS + 1):
        t0 = time.perf_counter()
        for _ in range(loops):
            fn()
        us.append((time.perf_counter() - t0) / loops * 1e6)
    us = us[1:]
    emit("| uaes_ff3_encrypt on the host path | %s | %.3g |" % (cell(us), 1e6 / statistics.median(us)))
    uaes.host_policy(*prev)
    emit("\n(Looped through ctypes: the call overhead of about a microsecond is inside these figures.)\n")
    text_out = "\n".join(rows) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
