#!/usr/bin/env python3
"""Poly1305-AES rates on device-resident data (uaes_poly1305_dev / uaes_poly1305_batch, device pointers):
  size sweep   one message of 4 KiB .. 1 GiB: arrangement, us per call (stream time of `reps` back-to-back calls),
               GiB/s and the fraction of 8 TB/s of read traffic
  latency      one 1 KiB message through the synchronous call (host round trip included) and through _dev
  batch sweep  nmsg x msg_bytes (64 B .. 4 KiB), one wave per message
  cpu          the compiled reference's AES_Poly1305 on one core over 64 MiB (oracle/_ref, when it is there)
Usage: poly1305_rate.py [--quick]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import micro_aes_amd as uaes

L = uaes.engine()
KEYS, NONCE = bytes(range(16)) + b"\xff" * 16, bytes(range(16))
HBM = 8e12


def dev_time(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3         # us


def main():
    quick = "--quick" in sys.argv
    top = 1 << (28 if quick else 30)
    src = torch.randint(0, 256, (top,), dtype=torch.uint8, device="cuda")
    mac = torch.zeros(64, dtype=torch.uint8, device="cuda")
    a, m = C.c_void_p(src.data_ptr()), C.c_void_p(mac.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("size sweep (uaes_poly1305_dev, AES-128, device data)")
    n = 4096
    while n <= top:
        name = uaes.poly1305_plan(n)
        reps = 200 if n <= (16 << 20) else 20
        us = dev_time(lambda: L.uaes_poly1305_dev(128, KEYS, NONCE, a, n, m, st), reps)
        print("  %11d B  %-12s grid %5d steps %6d  %10.2f us  %8.2f GiB/s  %.3f of 8 TB/s" %
              (n, name[0], name[2], name[3], us, n / us / 1e3 / 1.073741824, n / us * 1e6 / HBM), flush=True)
        n *= 2
    # the arrangement boundary from both sides (the planner's answer on this device)
    for n in (64 << 10, 96 << 10, 128 << 10, (128 << 10) + 16, 192 << 10, 256 << 10):
        us = dev_time(lambda: L.uaes_poly1305_dev(128, KEYS, NONCE, a, n, m, st), 200)
        print("  boundary %9d B  %-12s %8.2f us" % (n, uaes.poly1305_plan(n)[0], us), flush=True)
    print("latency, one 1 KiB message")
    out = (C.c_uint8 * 16)()
    host = bytes(1024)
    for label, fn in (("uaes_poly1305, host data", lambda: L.uaes_poly1305(128, KEYS, NONCE, host, 1024, out)),
                      ("uaes_poly1305, device data", lambda: L.uaes_poly1305(128, KEYS, NONCE, a, 1024, out))):
        for _ in range(20):
            fn()
        t0 = time.perf_counter()
        for _ in range(500):
            fn()
        print("  %-30s %8.2f us per call" % (label, (time.perf_counter() - t0) / 500 * 1e6), flush=True)
    us = dev_time(lambda: L.uaes_poly1305_dev(128, KEYS, NONCE, a, 1024, m, st), 500)
    print("  %-30s %8.2f us per call (stream time, back to back)" % ("uaes_poly1305_dev", us), flush=True)
    print("batch sweep (uaes_poly1305_batch, device nonces / data / macs)")
    nmax = 81919
    nonces = torch.randint(0, 256, (nmax * 16,), dtype=torch.uint8, device="cuda")
    macs = torch.zeros(nmax * 16, dtype=torch.uint8, device="cuda")
    pn, pm = C.c_void_p(nonces.data_ptr()), C.c_void_p(macs.data_ptr())
    for nmsg in (1000, 81919):
        for size in (64, 256, 1024, 4096):
            us = dev_time(lambda: L.uaes_poly1305_batch(128, KEYS, pn, nmsg, size, a, pm), 20)
            print("  %6d x %5d B  %10.2f us  %8.2f GiB/s  %10.0f msgs/s" %
                  (nmsg, size, us, nmsg * size / us / 1e3 / 1.073741824, nmsg / us * 1e6), flush=True)
    ref = os.path.join(ROOT, "oracle", "_ref", "libmicroaes_ref_128.so")
    if os.path.exists(ref):
        R = C.CDLL(ref)
        R.AES_Poly1305.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        n = 64 << 20
        buf = (C.c_uint8 * n)()
        t0 = time.perf_counter()
        R.AES_Poly1305(KEYS, NONCE, buf, n, out)
        dt = time.perf_counter() - t0
        print("cpu: reference AES_Poly1305, one core, 64 MiB: %.2f s, %.1f MiB/s" % (dt, n / dt / 2**20), flush=True)


if __name__ == "__main__":
    main()
