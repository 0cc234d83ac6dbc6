"""OCB on the GPU (csrc/uaes_ocb.hip) where the rest of the suite does not reach: every run length of k_ocb at the size
that really has it, texts past 2^32 bytes, long associated data on the second walk, associated data that is not
aligned, every chunk count and pair of edge-chunk owners, every shift of the nonce, every nonce and tag length, and
guard bytes around the results.

No size here is a literal: they come from walking uaes.plan_ocb (the launcher's own arithmetic, uaesk_plan_ocb_shape)
on the device at hand, so the file holds on a device with another number of CUs.  Texts of 256 MiB and more are out of
the CPU oracle's reach (about 25 MiB/s), so they are held against tests/ocb_ref.py -- RFC 7253 in pieces, proved against
the vectors, the oracle and the RFC's chained offsets by tests/test_ocb_ref_host.py -- evaluated slice by slice with
torch on the device, its block cipher being uaes.ecb_dev: another kernel, pinned to the oracle elsewhere.  All
comparisons are byte for byte, and every failing case prints the tuple that reproduces it."""
import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

import micro_aes_amd as uaes
from tests import ocb_ref as R
from tests.guarded_mem import Mem
from tests.test_gpu_plan import boundaries

pytestmark = pytest.mark.gpu

MIB, GIB = 1 << 20, 1 << 30
CHUNK = 256 * 16                        # bytes of a chunk: 256 blocks, one wave x four blocks per lane
SLICE = 256 * MIB                       # what the torch reference works on at once: 65536 chunks, no multiple of
                                        # run x waves chunks at any grid that is not a power of two, and never aligned
                                        # with the chunks themselves (block i sits at byte 16 (i - 1))
NONCE = bytes(range(50, 62))


def note(test, n, a, shape):
    """what plan_ocb answered for a long case (shown with a failure and by pytest -s; profiles/ocb_long_texts.md keeps one run's)"""
    print("plan_ocb %s len=%d aad=%d -> %s" % (test, n, a, shape))


def key_of(bits):
    return bytes(range(7, 7 + bits // 8))


def first_length(pred, lo=CHUNK * 4 + 16, hi=1 << 40, unit=16):
    """the first multiple of `unit` in (lo, hi] with pred true; pred is monotone (false, then true)"""
    assert not pred(lo) and pred(hi)
    while hi - lo > unit:
        mid = (lo + hi) // 2 // unit * unit
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


@functools.lru_cache(None)
def first_with_run(run, aad=False):
    """the first text (aad: the first associated data behind 100 bytes of text) whose walk takes `run` chunks at once"""
    at = (lambda n: uaes.plan_ocb(100, n)[1]) if aad else (lambda n: uaes.plan_ocb(n)[0])
    n = first_length(lambda n: at(n) >= run, lo=MIB)
    assert at(n) == run and at(n - 16) == run // 2, (run, n, at(n), at(n - 16))
    return n


def device_stream(seed, nbytes):
    """nbytes of splitmix64 output made on the device (64-bit word i = mix(seed + (i + 1) * golden))"""
    import torch

    def s64(v):
        return v - (1 << 64) if v >> 63 else v

    def shr(z, k):
        return (z >> k) & ((1 << (64 - k)) - 1)

    out = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda:0")
    step = 1 << 24
    for lo in range(0, out.numel(), step):
        i = torch.arange(lo + 1, min(lo + step, out.numel()) + 1, dtype=torch.int64, device="cuda:0")
        z = i * s64(0x9E3779B97F4A7C15) + s64(seed)
        z = (z ^ shr(z, 30)) * s64(0xBF58476D1CE4E5B9)
        z = (z ^ shr(z, 27)) * s64(0x94D049BB133111EB)
        out[lo:lo + i.numel()] = z ^ shr(z, 31)
    return out.view(torch.uint8)[:nbytes]


def need_memory(nbytes, what):
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes:
        pytest.skip("%s needs %d MiB of device memory, %d MiB are free" % (what, nbytes >> 20, free >> 20))


def device_ecb(key):
    import torch

    def ecb(t):
        out = torch.empty_like(t)
        uaes.ecb_dev(key, t, out)
        return out
    return ecb


def dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0") if b else None


def host(t):
    return bytes(t.cpu().numpy())


def compare_slices(o, off0, src, got, n, info):
    """got[:16 m] against text_by_blocks over src, slice by slice; returns the checksum of the m whole blocks"""
    import torch
    m, ck, ecb = n // 16, R.ZERO, device_ecb(o.key)
    for lo in range(0, 16 * m, SLICE):
        hi = min(lo + SLICE, 16 * m)
        want, s = R.text_by_blocks(o, off0, lo // 16, src[lo:hi], ecb, torch)
        if not torch.equal(want, got[lo:hi]):
            bad = int(torch.nonzero(want != got[lo:hi])[0]) + lo
            raise AssertionError("%r: first wrong byte %d = block %d (1-based) of chunk %d" % (info, bad, bad // 16 + 1, (bad // 16 + 1) // 256))
        ck = R.xor(ck, s)
        del want
    return ck


def long_text(orc, n, bits, in_place, test, flip=True):
    """one text of n bytes on the device: ciphertext against the slices, tag from the folded checksum, the way back,
    and a flipped byte in the second chunk of a run in the middle of the text"""
    import torch
    info = (test, n, bits, in_place)
    shape = uaes.plan_ocb(n)
    note(test, n, 21, shape)
    need_memory(3 * n + 6 * SLICE, repr(info))
    key, aad = key_of(bits), bytes(range(21))
    o = R.Ocb(orc, key)
    off0 = o.offset0(NONCE)
    src = device_stream(n, n)
    out = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
    if in_place:
        out[:n] = src
    uaes.ocb_dev(key, NONCE, dev(aad), out if in_place else src, n, out)
    ck = compare_slices(o, off0, src, out, n, info)
    m = n // 16
    tail, tag = o.finish(off0, m, ck, host(src[16 * m:]), o.hash_aad(aad))
    assert host(out[16 * m:]) == tail + tag, info
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    back = out if in_place else torch.full((n,), 0xCC, dtype=torch.uint8, device="cuda:0")
    keep = out.clone() if in_place and flip else out
    uaes.ocb_dev(key, NONCE, dev(aad), out, n, back, decrypt=True, status=status)
    assert int(status.item()) == 0 and torch.equal(back[:n], src), info
    if not flip:
        return
    # chunk c = f + 1 is the second of its run when f = q * run + 1 (chunk_of: a run is `run` consecutive chunks)
    run = shape[0]
    c = (n // CHUNK // run // 2) * run + (1 if run > 1 else 0) + 1
    pos = 16 * (256 * c + 100 - 1) + 5
    assert pos < n
    keep[pos] ^= 0x04
    del src
    scratch = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    uaes.ocb_dev(key, NONCE, dev(aad), keep, n, scratch, decrypt=True, status=status)
    assert int(status.item()) == 0x1A, info


# ---- a. every run length at its real size --------------------------------------------------------------------------
EXTRA = 3 * CHUNK + 5 * 16 + 7


def test_the_last_text_with_runs_of_one(orc):
    n = first_with_run(2) - 16
    assert uaes.plan_ocb(n)[0] == 1 and uaes.plan_ocb(n + 16)[0] == 2
    long_text(orc, n, 128, False, "a.run1")


@pytest.mark.parametrize("run,bits,in_place", [(2, 128, False), (2, 256, False), (2, 128, True), (4, 128, False),
                                               (8, 128, False), (16, 128, False)])
def test_every_run_length_at_its_real_size(orc, run, bits, in_place):
    n = first_with_run(run) + EXTRA
    assert uaes.plan_ocb(n)[0] == run
    long_text(orc, n, bits, in_place, "a.run%d" % run)


def test_a_text_beyond_4_gib(orc):
    """byte offsets past 2^32: encryption, the slices, the tag, and the verdict of the way back"""
    long_text(orc, 4 * GIB + 3 * CHUNK + 7, 128, False, "a.4gib", flip=False)


# ---- b. long associated data: the second walk with runs of 2 and of 16 ---------------------------------------------
@pytest.mark.parametrize("run_aad", [2, 16])
def test_long_associated_data(orc, run_aad):
    """tag = the oracle's tag of the same text without associated data ^ HASH(K, A): HASH over the whole blocks from the
    torch slices, its ragged block from ocb_ref.  Both directions (decryption swaps the tables between the walks), a
    text of none, of 6 blocks and of 1 MiB, and a flipped byte in the second chunk of a run of the associated data."""
    import torch
    alen = first_with_run(run_aad, aad=True) + 3 * CHUNK + 5
    need_memory(alen + 5 * SLICE, "associated data of %d bytes" % alen)
    key = key_of(128)
    o = R.Ocb(orc, key)
    aad = device_stream(alen + 1, alen)
    ma, h, ecb = alen // 16, R.ZERO, device_ecb(key)
    for lo in range(0, 16 * ma, SLICE):
        h = R.xor(h, R.text_by_blocks(o, R.ZERO, lo // 16, aad[lo:min(lo + SLICE, 16 * ma)], ecb, torch, hash=True)[1])
    h = R.xor(h, o.aad_tail(ma, host(aad[16 * ma:])))
    c = (alen // CHUNK // run_aad // 2) * run_aad + 2
    pos = 16 * (256 * c + 77 - 1) + 9
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    for n in (0, 100, MIB):
        info = (run_aad, alen, n)
        shape = uaes.plan_ocb(n, alen)
        note("b.run_aad%d" % run_aad, n, alen, shape)
        assert shape[1] == run_aad and shape[4] == ma, info
        pt = orc.splitmix(n + 3, n)
        bare = orc.ocb_encrypt(key, NONCE, b"", pt)
        want = bare[:n] + R.xor(bare[n:], h)
        src = dev(pt) if n else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        out = torch.full((n + 16,), 0xCC, dtype=torch.uint8, device="cuda:0")
        uaes.ocb_dev(key, NONCE, aad, src, n, out)
        assert host(out) == want, info
        back = torch.full((max(n, 16),), 0xCC, dtype=torch.uint8, device="cuda:0")
        status.fill_(-1)
        uaes.ocb_dev(key, NONCE, aad, out, n, back, decrypt=True, status=status)
        assert int(status.item()) == 0 and host(back[:n]) == pt, info
        aad[pos] ^= 0x80
        uaes.ocb_dev(key, NONCE, aad, out, n, back, decrypt=True, status=status)
        assert int(status.item()) == 0x1A, info
        aad[pos] ^= 0x80


# ---- c. associated data that is not aligned ------------------------------------------------------------------------
def test_unaligned_associated_data_on_device_pointers(orc):
    """from 8192 blocks on, aligned associated data is hashed by all workgroups and unaligned data by the finishing
    one alone, through byte loads: the same tag either way, the oracle's"""
    import torch
    key, pt = key_of(192), orc.splitmix(9, 100)
    spread = first_length(lambda a: uaes.plan_ocb(100, a)[4] > 0, lo=65536 + 16, hi=GIB)
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    for alen in (spread - 1, spread, spread + 19):
        a = orc.splitmix(alen, alen)
        want = orc.ocb_encrypt(key, NONCE, a, pt)
        for off in (0, 1, 8):
            info = (alen, off)
            base = torch.zeros(alen + 32, dtype=torch.uint8, device="cuda:0")
            assert base.data_ptr() % 16 == 0
            base[off:off + alen] = dev(a)
            aad = base[off:off + alen]
            shape = uaes.plan_ocb(100, alen, aad_aligned=off % 16 == 0)
            note("c", 100, alen, shape)
            assert shape[4] == (alen // 16 if off == 0 and alen >= spread else 0), info
            out = torch.full((116,), 0xCC, dtype=torch.uint8, device="cuda:0")
            uaes.ocb_dev(key, NONCE, aad, dev(pt), 100, out)
            assert host(out) == want, info
            back = torch.full((100,), 0xCC, dtype=torch.uint8, device="cuda:0")
            uaes.ocb_dev(key, NONCE, aad, out, 100, back, decrypt=True, status=status)
            assert int(status.item()) == 0 and host(back) == pt, info
            base[off + alen // 2] ^= 1
            uaes.ocb_dev(key, NONCE, aad, out, 100, back, decrypt=True, status=status)
            assert int(status.item()) == 0x1A, info


# ---- d. every chunk count, every pair of edge owners ---------------------------------------------------------------
def owners(n):
    """(wave of the first chunk, wave of the last chunk, waves per workgroup) as ocb_main_body computes them"""
    shape = uaes.plan_ocb(n)
    if shape is None:
        return None
    run, _, wg, grid, _ = shape
    nchunks = ((n >> 4) >> 8) + 1
    runs = -(-max(nchunks - 2, 0) // run)
    nwaves = grid * wg // 64
    return runs % nwaves, (runs + 1) % nwaves, wg // 64


def chunk_count_lengths(ks=range(4, 73)):
    out = []
    for k in ks:
        for j, b in enumerate((16 * (256 * k - 1), 16 * 256 * k, 16 * (256 * k + 1))):
            out.append(b + (0, 1, 15)[(k + j) % 3])
    return out


def check_host(orc, bits, n, tag_len=16):
    key, pt, aad = key_of(bits), orc.splitmix(n, n), b"header"
    want = orc.ocb_encrypt(key, NONCE, aad, pt, tag_len=tag_len)
    assert uaes.AES_OCB_encrypt(key, NONCE, aad, pt, tag_len) == want, (bits, n, tag_len)
    assert uaes.AES_OCB_decrypt(key, NONCE, aad, want, 0xCC, tag_len) == (0, pt), (bits, n, tag_len)
    bad = want[:-1] + bytes([want[-1] ^ 0x20])
    assert uaes.AES_OCB_decrypt(key, NONCE, aad, bad, 0xCC, tag_len) == (0x1A, pt), (bits, n, tag_len)


def test_every_chunk_count(orc):
    """4 .. 72 chunks, a block below, at and above each count, ragged tails of 0, 1 and 15 bytes; the key sizes in turn"""
    for i, n in enumerate(chunk_count_lengths()):
        check_host(orc, (128, 192, 256)[i % 3], n)


@functools.lru_cache(None)
def shape_changes():
    """both sides of every length between 16 KiB and 24 MiB at which the threads per workgroup or the workgroups change,
    and the first lengths at which an edge chunk's owner wraps round to wave 0"""
    lens = set()
    for b, _, _ in boundaries(lambda n: (uaes.plan_ocb(n) or (0,) * 5)[2:4], 16384, 24 * MIB):
        lens.update((b - 16, b))
    # a text of c chunks starts at CHUNK * (c - 1) bytes; one chunk more and the first chunk's owner has wrapped as well
    edge = {c: owners(CHUNK * (c - 1)) for c in range(6, 24 * MIB // CHUNK)}
    for c in [c for c, (e0, e1, _) in edge.items() if e1 < e0][:3]:
        lens.update((CHUNK * (c - 1), CHUNK * (c - 1) + 16 * 3 + 5, CHUNK * c + 16))
    return sorted(lens)


def test_the_sweep_meets_every_placement_of_the_edge_owners():
    """the two masked chunks go to the waves runs % nwaves and (runs + 1) % nwaves: the lengths of this section put
    them in one workgroup, in two, and on either side of the wrap to wave 0"""
    seen = set()
    for n in chunk_count_lengths() + shape_changes():
        o = owners(n)
        if o is not None:
            e0, e1, w = o
            seen.add("wrap" if e1 < e0 else "two workgroups" if e0 // w != e1 // w else "one workgroup")
    assert seen == {"wrap", "two workgroups", "one workgroup"}, seen
    assert any(owners(n) is None for n in chunk_count_lengths()) and len(shape_changes()) > 8


BANDS = 8


@pytest.mark.parametrize("band", range(BANDS))
def test_both_sides_of_every_shape_change(orc, band):
    """device-resident, prefixes of one stream; the oracle's answers are computed on all the CPUs there are while the
    GPU works.  The lengths are cut into bands of about equal bytes so that none takes long."""
    import torch
    lens = shape_changes()
    total, acc, mine = sum(lens), 0, []
    for n in lens:
        if band * total <= acc * BANDS < (band + 1) * total:
            mine.append(n)
        acc += n
    key = key_of(128)
    src = device_stream(4, max(lens))
    pt = host(src)
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        for n, want in zip(mine, pool.map(lambda n: orc.ocb_encrypt(key, NONCE, b"", pt[:n]), mine)):
            info = (n, uaes.plan_ocb(n), owners(n))
            out = torch.full((n + 16,), 0xCC, dtype=torch.uint8, device="cuda:0")
            uaes.ocb_dev(key, NONCE, None, src, n, out)
            assert torch.equal(out, dev(want)), info
            back = torch.full((n,), 0xCC, dtype=torch.uint8, device="cuda:0")
            uaes.ocb_dev(key, NONCE, None, out, n, back, decrypt=True, status=status)
            assert int(status.item()) == 0 and torch.equal(back, src[:n]), info
            out[n + 3] ^= 1
            uaes.ocb_dev(key, NONCE, None, out, n, back, decrypt=True, status=status)
            assert int(status.item()) == 0x1A and torch.equal(back, src[:n]), info


# ---- e. nonce and tag edges ----------------------------------------------------------------------------------------
def check_ref(o, nonce, aad, pt, tag_len):
    info = (len(o.key) * 8, nonce.hex(), tag_len, len(pt))
    want = o.encrypt(nonce, aad, pt, tag_len)
    assert uaes.AES_OCB_encrypt(o.key, nonce, aad, pt, tag_len) == want, info
    assert uaes.AES_OCB_decrypt(o.key, nonce, aad, want, 0xCC, tag_len) == (0, pt), info
    bad = want[:-1] + bytes([want[-1] ^ 1])
    assert uaes.AES_OCB_decrypt(o.key, nonce, aad, bad, 0xCC, tag_len) == (0x1A, pt), info


def test_every_bottom_of_the_nonce(orc):
    """the last six bits of the nonce shift Ktop by 0 .. 63 (0 has a branch of its own): one workgroup's kernel at 40
    bytes and k_ocb at 1025 blocks + 3 bytes"""
    o = R.Ocb(orc, key_of(128))
    small, runs = 40, 16 * 1025 + 3
    assert uaes.plan("ocb", small)[0] == "ocb.small" and uaes.plan("ocb", runs)[0] == "ocb.runs"
    texts = {n: orc.splitmix(n, n) for n in (small, runs)}
    for b in range(64):
        for n in (small, runs):
            check_ref(o, bytes(range(11)) + bytes([0x40 | b]), b"bottom", texts[n], 16)


def test_every_nonce_and_tag_length(orc):
    o = R.Ocb(orc, key_of(256))
    pt = orc.splitmix(40, 40)
    for nlen in range(1, 16):
        for tlen in range(1, 17):
            for b in (0, 1, 63):
                check_ref(o, bytes(range(200, 200 + nlen - 1)) + bytes([0x40 | b]), b"lengths", pt, tlen)


# ---- f. nothing outside the result is written ----------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_nothing_is_written_outside_the_result(orc, device):
    """guard bytes in front of the result and behind len + tag_len (encryption) / len (decryption)"""
    L = uaes.engine()
    key, aad, off = key_of(128), b"guarded", 16 if device else 3
    kb = (C.c_uint8 * 16).from_buffer_copy(key)
    for n in chunk_count_lengths(range(4, 6)):
        pt = orc.splitmix(n + 1, n)
        for tlen in (1, 12, 16):
            info = (device, n, tlen)
            want = orc.ocb_encrypt(key, NONCE, aad, pt, tag_len=tlen)
            src, dst = Mem(pt, device, off), Mem(b"", device, off, size=n + tlen)
            assert L.uaes_ocb_encrypt_ex(128, kb, NONCE, 12, tlen, aad, len(aad), src.ptr, n, dst.ptr) == 0, info
            assert dst.get() == want and dst.intact() and src.get() == pt and src.intact(), info
            src, dst = Mem(want, device, off), Mem(b"", device, off, size=n)
            assert L.uaes_ocb_decrypt_ex(128, kb, NONCE, 12, tlen, aad, len(aad), src.ptr, n, dst.ptr) == 0, info
            assert dst.get() == pt and dst.intact() and src.get() == want and src.intact(), info

