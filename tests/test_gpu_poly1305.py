"""Poly1305-AES on the GPU (csrc/uaes_poly1305.hip) against the big-integer restatement of tests/test_poly1305_host.py
(itself checked against the reference's vectors and the compiled reference): the vector file and the paper's KATs
through the C ABI and the drop-in library, every short length at every key size, both sides of the planner's
boundaries, tags whose h sits at the edges of the reduction, messages too long for a Python Horner (closed forms), the
device-pointer, stream, graph and batch forms, and the argument errors."""
import ctypes as C
import random

import pytest

import micro_aes_amd as uaes
from tests.test_gpu_plan import boundaries, around
from tests.test_poly1305_host import P, clamp, block, poly_h, tag, aes_s, poly1305_aes, tv_vectors, kats

pytestmark = pytest.mark.gpu


def _keys(rng, bits, r=None):
    return rng.randbytes(bits // 8) + (r if r is not None else rng.randbytes(16))


def _dev(data):
    import torch
    t = torch.empty(max(len(data), 1), dtype=torch.uint8, device="cuda:0")
    if data:
        t[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def test_vectors_and_kats_through_the_abi_and_the_drop_in_library(orc, golden_dir):
    D = C.CDLL(uaes.lib_path("libmicro_aes_hip_128.so"))
    D.AES_Poly1305.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    D.AES_Poly1305.restype = None
    vs = tv_vectors(golden_dir) + kats(golden_dir)
    assert len(vs) == 82
    for keys, nonce, msg, mac in vs:
        assert uaes.AES_Poly1305(keys, nonce, msg) == mac, len(msg)
        out = (C.c_uint8 * 16)()
        D.AES_Poly1305(keys, nonce, msg, len(msg), out)
        assert bytes(out) == mac, len(msg)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_every_short_length_and_the_block_edges_to_64k(orc, bits):
    rng = random.Random(bits)
    keys = _keys(rng, bits, b"\xff" * 16 if bits == 192 else None)
    nonce = rng.randbytes(16)
    buf = rng.randbytes(65536 + 16)
    if bits == 256:
        buf = b"\xff" * len(buf)                           # all-0xff blocks: the largest c_i
    r, s = clamp(keys[-16:]), aes_s(orc, keys, nonce)
    for n in range(81):
        assert uaes.AES_Poly1305(keys, nonce, buf[:n]) == tag(poly_h(r, buf[:n]), s), (bits, n)
    h = 0                                                  # Horner over whole blocks, k of them so far
    for k in range(1, 4097):
        prev, h = h, (h + block(buf[16 * k - 16:16 * k])) * r % P
        for n, want in ((16 * k - 1, (prev + block(buf[16 * k - 16:16 * k - 1])) * r % P), (16 * k, h),
                        (16 * k + 1, (h + block(buf[16 * k:16 * k + 1])) * r % P)):
            if n > 80 and (k % 16 == 0 or k < 64 or k > 4090):
                assert uaes.AES_Poly1305(keys, nonce, buf[:n]) == tag(want, s), (bits, n)


def test_both_sides_of_every_planner_boundary(orc):
    bs = boundaries(lambda n: uaes.poly1305_plan(n)[0], 0, 64 << 20)
    assert [b[1:] for b in bs] == [("poly.small", "poly.chunks")], bs
    rng = random.Random(5)
    keys = _keys(rng, 128)
    nonce = bytes(16)
    for b, _, _ in bs:
        for n in around(b):
            msg = rng.randbytes(n)
            assert uaes.AES_Poly1305(keys, nonce, msg) == poly1305_aes(orc, keys, nonce, msg), n


def _message_with_h(rng, r, target, nblocks):
    """nblocks (>= 2) blocks whose h mod p is `target`: random blocks, then the last one solved for,
    c_q = target r^-1 - h_(q-1) (h = (h_(q-1) + c_q) r), until c_q is a full block (2^128 <= c_q < 2^129)"""
    rinv = pow(r, P - 2, P)
    while True:
        head = rng.randbytes(16 * (nblocks - 1))
        c = (target * rinv - poly_h(r, head)) % P
        if (1 << 128) <= c < (1 << 129):
            return head + (c - (1 << 128)).to_bytes(16, "little")


def test_edge_tags(orc):
    """h mod p = 0..4, p-5..p-1, 2^128-1, 2^128, 2^128+1, with nonces whose s wraps h + s past 2^128: where a lazy
    reduction or the final canonicalisation goes wrong"""
    rng = random.Random(11)
    targets = list(range(5)) + [P - k for k in range(5, 0, -1)] + [(1 << 128) - 1, 1 << 128, (1 << 128) + 1]
    for bits in (128, 256):
        for rbytes in (b"\xff" * 16, None):
            keys = _keys(rng, bits, rbytes)
            r = clamp(keys[-16:])
            for t in targets:
                for nblocks in (2, 3, 300, 9000):          # poly.small (one and several blocks per lane), poly.chunks
                    msg = _message_with_h(rng, r, t, nblocks)
                    assert poly_h(r, msg) == t
                    for nonce in (bytes(16), b"\xff" * 16, rng.randbytes(16)):
                        s = aes_s(orc, keys, nonce)
                        assert uaes.AES_Poly1305(keys, nonce, msg) == tag(t, s), (bits, t, nblocks)
    # all-0xff messages under the largest clamped r
    keys = _keys(rng, 128, b"\xff" * 16)
    for n in (16, 4096, (256 << 10) + 15):
        msg = b"\xff" * n
        assert uaes.AES_Poly1305(keys, bytes(16), msg) == poly1305_aes(orc, keys, bytes(16), msg), n


def _repeated(c16, q, tail):
    """h of q copies of the block c16 followed by the partial block `tail`: C r^2 (r^q - 1)/(r - 1) + T r"""
    def h(r):
        C_ = block(c16)
        geo = (pow(r, q, P) - 1) * pow(r - 1, P - 2, P) % P
        if not tail:
            return C_ * r % P * geo % P
        return (C_ * r * r % P * geo + block(tail) * r) % P
    return h


@pytest.mark.parametrize("q,tail", [(1 << 26, b""), ((4 << 30) // 16, b"\x01\x02\x03\x04\x05")])
def test_one_gib_and_past_four_gib_in_closed_form(orc, q, tail):
    import torch
    rng = random.Random(q)
    keys, nonce = _keys(rng, 256, b"\xff" * 16), rng.randbytes(16)
    c16 = rng.randbytes(16)
    n = 16 * q + len(tail)
    src = torch.tensor(list(c16), dtype=torch.uint8, device="cuda:0").repeat(q + (1 if tail else 0))
    if tail:
        src[16 * q:n].copy_(torch.tensor(list(tail), dtype=torch.uint8))
    mac = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    uaes.poly1305_dev(keys, nonce, src, n, mac)
    torch.cuda.synchronize()
    r = clamp(keys[-16:])
    want = tag(_repeated(c16, q, tail)(r), aes_s(orc, keys, nonce))
    assert bytes(mac.cpu().numpy()) == want
    del src
    torch.cuda.empty_cache()


def test_period_k_pattern_and_a_64_mib_random_message(orc):
    import torch
    rng = random.Random(3)
    keys, nonce = _keys(rng, 128), rng.randbytes(16)
    r, s = clamp(keys[-16:]), aes_s(orc, keys, nonce)
    k, m = 777, 20011                                      # 777 distinct blocks, 20011 times over (~237 MiB)
    period = rng.randbytes(16 * k)
    src = torch.frombuffer(bytearray(period), dtype=torch.uint8).to("cuda:0").repeat(m)
    mac = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    uaes.poly1305_dev(keys, nonce, src, src.numel(), mac)
    torch.cuda.synchronize()
    hk, rk = poly_h(r, period), pow(r, k, P)
    want = hk * (pow(rk, m, P) - 1) * pow(rk - 1, P - 2, P) % P
    assert bytes(mac.cpu().numpy()) == tag(want, s)
    data = orc.splitmix(64, 64 << 20)
    assert uaes.AES_Poly1305(keys, nonce, data) == tag(poly_h(r, data), s)


def test_device_pointers_streams_and_a_graph(orc):
    import torch
    rng = random.Random(9)
    keys, nonce = _keys(rng, 192), rng.randbytes(16)
    # the synchronous call on device memory (producer: the default stream)
    for n in (0, 33, 1 << 20):
        data = rng.randbytes(n)
        mac = (C.c_uint8 * 16)()
        t = _dev(data)
        rc = uaes.engine().uaes_poly1305(192, keys, nonce, C.c_void_p(t.data_ptr()), n, mac)
        assert rc == 0 and bytes(mac) == poly1305_aes(orc, keys, nonce, data), n
    # _dev on four non-default streams at once, a chunked and a small message each
    streams = [torch.cuda.Stream() for _ in range(4)]
    jobs = []
    for i, st in enumerate(streams):
        for n in (3 << 20, 5000 + i):
            data = rng.randbytes(n)
            src, mac = _dev(data), torch.zeros(16, dtype=torch.uint8, device="cuda:0")
            with torch.cuda.stream(st):
                uaes.poly1305_dev(keys, nonce, src, n, mac, stream=st)
            jobs.append((data, src, mac))
    torch.cuda.synchronize()
    for data, _, mac in jobs:
        assert bytes(mac.cpu().numpy()) == poly1305_aes(orc, keys, nonce, data), len(data)
    for st in streams:
        assert uaes.engine().uaes_stream_release(C.c_void_p(st.cuda_stream)) == 0
    # captured on one stream (both arrangements), replayed with fresh data
    side = torch.cuda.Stream()
    nbig, nsmall = (2 << 20) + 7, 1000
    big, small = torch.zeros(nbig, dtype=torch.uint8, device="cuda:0"), torch.zeros(nsmall, dtype=torch.uint8, device="cuda:0")
    macs = torch.zeros(2, 16, dtype=torch.uint8, device="cuda:0")

    def seq(st):
        uaes.poly1305_dev(keys, nonce, big, nbig, macs[0], stream=st)
        uaes.poly1305_dev(keys, nonce, small, nsmall, macs[1], stream=st)

    with torch.cuda.stream(side):
        seq(side)                                          # warm-up: this stream's scratch slot
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        seq(torch.cuda.current_stream())
    for rep in range(10):
        d = orc.splitmix(500 + rep, nbig + nsmall)
        big.copy_(torch.frombuffer(bytearray(d[:nbig]), dtype=torch.uint8))
        small.copy_(torch.frombuffer(bytearray(d[nbig:]), dtype=torch.uint8))
        macs.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert bytes(macs[0].cpu().numpy()) == poly1305_aes(orc, keys, nonce, d[:nbig]), rep
        assert bytes(macs[1].cpu().numpy()) == poly1305_aes(orc, keys, nonce, d[nbig:]), rep
    del g
    torch.cuda.synchronize()
    assert uaes.engine().uaes_stream_release(C.c_void_p(side.cuda_stream)) == 0


def _host_macs(keys, nonces, msgs):
    """the library's host path (checked against the restatement in tests/test_poly1305_host.py), for the largest
    batches where a Python Horner per message would take minutes -- run after the GPU results are in"""
    prev = uaes.host_policy(1 << 62, 0, 0)
    try:
        return [uaes.AES_Poly1305(keys, n, m) for n, m in zip(nonces, msgs)]
    finally:
        uaes.host_policy(*prev)


@pytest.mark.parametrize("nmsg", [1, 7, 1000, 81919])
def test_batch(orc, nmsg):
    import torch
    rng = random.Random(nmsg)
    for size in (0, 1, 16, 17, 1500, 4096):
        keys = _keys(rng, (128, 192, 256)[size % 3])
        nonces = [rng.randbytes(16) for _ in range(nmsg)]
        blob = orc.splitmix(nmsg + size, nmsg * size) if size else b""
        msgs = [blob[i * size:(i + 1) * size] for i in range(nmsg)]
        got = uaes.poly1305_batch(keys, nonces, msgs)
        # device data and device nonces, device macs
        d_data, d_non = _dev(blob), _dev(b"".join(nonces))
        d_mac = torch.zeros(nmsg * 16, dtype=torch.uint8, device="cuda:0")
        bits = (len(keys) - 16) * 8
        rc = uaes.engine().uaes_poly1305_batch(bits, keys, C.c_void_p(d_non.data_ptr()), nmsg, size,
                                               C.c_void_p(d_data.data_ptr()), C.c_void_p(d_mac.data_ptr()))
        assert rc == 0
        raw = bytes(d_mac.cpu().numpy())
        assert [raw[16 * i:16 * i + 16] for i in range(nmsg)] == got, (nmsg, size)
        if nmsg * size <= 8 << 20:
            for i in (range(nmsg) if nmsg <= 1000 else range(0, nmsg, 97)):
                assert got[i] == poly1305_aes(orc, keys, nonces[i], msgs[i]), (nmsg, size, i)
        else:
            assert got == _host_macs(keys, nonces, msgs), (nmsg, size)


def test_errors_and_the_empty_message(orc):
    L = uaes.engine()
    keys, nonce = bytes(range(32)), bytes(range(16))
    mac = (C.c_uint8 * 16)()
    assert L.uaes_poly1305(100, keys, nonce, b"x", 1, mac) == -2
    assert L.uaes_poly1305(128, keys, nonce, None, 1, mac) == -2
    assert L.uaes_poly1305(128, keys, nonce, None, 0, mac) == 0
    assert bytes(mac) == orc.encrypt_block(keys[:16], nonce)
    d_mac = _dev(bytes(16))
    assert L.uaes_poly1305_dev(128, keys, nonce, None, 0, C.c_void_p(d_mac.data_ptr()), None) == 0
    import torch
    torch.cuda.synchronize()
    assert bytes(d_mac[:16].cpu().numpy()) == orc.encrypt_block(keys[:16], nonce)
    assert L.uaes_poly1305_dev(128, keys, nonce, None, 16, C.c_void_p(d_mac.data_ptr()), None) == -2
