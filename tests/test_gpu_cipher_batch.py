"""The cipher batches on the GPU (k_cipher_batch, uaes_cipher_batch.hip) -- CBC decrypt with the CS3 swap, CBC over whole
blocks in both directions, CFB in both directions, OFB and CTR -- against the CPU oracle's cbc / cbc_nocts / cfb / ofb /
ctr_xcrypt_at, one call per record, bit for bit: every short shape, block counts on both sides of row_walk's look-ahead in
and out of place, record counts read from the plan, CTR's carries, per-record lengths, placements, the one-message
calls, round trips, a seeded fuzz and two threads.  Every failing case prints the tuple that reproduces it."""
import random
import threading

import pytest

import micro_aes_amd as uaes
from tests.guarded_mem import FILL, Mem, ptr

pytestmark = pytest.mark.gpu

KEYS = {bits: bytes((bits // 8 + 7 * i) & 0xff for i in range(bits // 8)) for bits in (128, 192, 256)}

E_ARG = -2                                      # UAES_E_ARG (include/uaes_hip.h)
ROW_CH = 16                                     # row_walk's look-ahead in blocks (csrc/uaes_aes.hip.h)

# mode -> (C entry point, takes lens, the oracle's answer for one record, the Python wrapper)
MODES = {
    "cbc_decrypt": ("uaes_cbc_decrypt_batch", False, lambda o, k, v, t: o.cbc(k, v, t, encrypt=False)[1],
                    lambda k, v, t: uaes.cbc_decrypt_batch(k, v, t)),
    "cbc_decrypt_blocks": ("uaes_cbc_decrypt_blocks_batch", False, lambda o, k, v, t: o.cbc_nocts(k, v, t, encrypt=False)[1],
                           lambda k, v, t: uaes.cbc_blocks_batch(k, v, t, decrypt=True)),
    "cbc_encrypt_blocks": ("uaes_cbc_encrypt_blocks_batch", False, lambda o, k, v, t: o.cbc_nocts(k, v, t, encrypt=True)[1],
                           lambda k, v, t: uaes.cbc_blocks_batch(k, v, t)),
    "cfb_encrypt": ("uaes_cfb_encrypt_batch", True, lambda o, k, v, t: o.cfb(k, v, t, True),
                    lambda k, v, t: uaes.cfb_batch(k, v, t)),
    "cfb_decrypt": ("uaes_cfb_decrypt_batch", True, lambda o, k, v, t: o.cfb(k, v, t, False),
                    lambda k, v, t: uaes.cfb_batch(k, v, t, decrypt=True)),
    "ofb": ("uaes_ofb_xcrypt_batch", True, lambda o, k, v, t: o.ofb(k, v, t), lambda k, v, t: uaes.ofb_batch(k, v, t)),
    "ctr": ("uaes_ctr_xcrypt_batch", True, lambda o, k, v, t: o.ctr_xcrypt_at(k, v, 0, t), lambda k, v, t: uaes.ctr_batch(k, v, t)),
}
assert tuple(MODES) == uaes.CIPHER_BATCH_MODES
ALL = list(MODES)
WITH_LENS = [m for m in ALL if MODES[m][1]]
CBC = [m for m in ALL if not MODES[m][1]]


def batch(mode, key, ivs, nmsg, ml, lens, src, dst):
    """the entry point itself; every array bytes, None or Mem"""
    name, has_lens = MODES[mode][:2]
    a = (len(key) * 8, key, ptr(ivs), nmsg, ml) + ((ptr(lens),) if has_lens else ()) + (ptr(src), ptr(dst))
    return getattr(uaes.engine(), name)(*a)


def expected(orc, mode, key, ivs, texts):
    """the oracle's answers, one call per record (a record of no bytes is no call)"""
    f = MODES[mode][2]
    return [f(orc, key, v, t) if t else b"" for v, t in zip(ivs, texts)]


def records(rng, n, ml):
    return [rng.randbytes(16) for _ in range(n)], [rng.randbytes(ml) for _ in range(n)]


def check(orc, mode, key, ivs, texts, info):
    want = expected(orc, mode, key, ivs, texts)
    got = MODES[mode][3](key, ivs, texts)
    if got != want:
        bad = [m for m in range(len(texts)) if got[m] != want[m]]
        raise AssertionError("%s %r: records %r differ" % (mode, info, bad[:8]))
    return got


# ---- 1. every short shape ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("mode", ALL)
def test_every_short_shape(orc, mode, bits):
    """65 records per call: a second 16-wave workgroup's worth.  The lens modes at every slot size 0..49, and once with
    every length 0..49 in one call (lens); the CBC forms at one block (no swap), two (the swap alone), three to five (odd
    and even counts for the pairing)"""
    rng = random.Random(bits + len(mode))
    key = KEYS[bits]
    for ml in (range(50) if MODES[mode][1] else (16, 32, 48, 64, 80)):
        ivs, texts = records(rng, 65, ml)
        check(orc, mode, key, ivs, texts, (bits, ml))
    if MODES[mode][1]:
        ivs, texts = records(rng, 65, 49)
        check(orc, mode, key, ivs, [t[:m % 50] for m, t in enumerate(texts)], (bits, "ragged"))


# ---- 2. the depth of the walk, in place and out of place --------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL)
def test_walk_depth_in_and_out_of_place(orc, mode):
    """block counts on both sides of row_walk's look-ahead and of twice it; device memory.  In place is where a
    decrypt that overwrote a ciphertext block it still needs would show"""
    rng = random.Random(len(mode))
    key, n = KEYS[256], 6
    sizes = [16 * b for b in (ROW_CH - 1, ROW_CH, ROW_CH + 1, 2 * ROW_CH, 2 * ROW_CH + 1)]
    if MODES[mode][1]:
        sizes.append(16 * (2 * ROW_CH + 1) + 5)
    for ml in sizes:
        ivs, texts = records(rng, n, ml)
        want = b"".join(expected(orc, mode, key, ivs, texts))
        mv = Mem(b"".join(ivs), True)
        src, dst = Mem(b"".join(texts), True), Mem(b"", True, size=n * ml)
        assert batch(mode, key, mv, n, ml, None, src, dst) == 0, (mode, ml)
        assert dst.get() == want and dst.intact(n * ml) and src.get() == b"".join(texts), (mode, ml, "out of place")
        io = Mem(b"".join(texts), True)
        assert batch(mode, key, mv, n, ml, None, io, io) == 0, (mode, ml)
        assert io.get() == want and io.intact(n * ml), (mode, ml, "in place")
        assert mv.get() == b"".join(ivs) and mv.intact(16 * n)


# ---- 3. record counts from the plan -----------------------------------------------------------------------------------
def shape_change():
    """the last count of the 4-wave workgroups, found by walking the plan"""
    threads = lambda n: uaes.cipher_batch_plan(n, "ctr", 48)[3]                              # noqa: E731
    lo, hi = 1, 1 << 20
    assert threads(lo) == 256 and threads(hi) == 1024
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if threads(mid) == 256 else (lo, mid)
    return lo


def second_pass():
    """the first count at which the grid-stride loop of the largest launch runs a second time"""
    name, launches, grid, threads = uaes.cipher_batch_plan(1 << 20, "ctr", 48)
    assert name == "cipher.batch" and launches == 1 and threads % 16 == 0
    return grid * threads // 16 + 1


COUNTS = ["1", "3", "4", "5", "63", "64", "65", "shape-change", "shape-change+1", "second-pass"]


@pytest.mark.parametrize("which", COUNTS)
@pytest.mark.parametrize("mode", ALL)
def test_record_counts_from_the_plan(orc, mode, which):
    nmsg = {"shape-change": shape_change(), "shape-change+1": shape_change() + 1, "second-pass": second_pass()}.get(which) or int(which)
    plan = uaes.cipher_batch_plan(nmsg, mode, 48)
    assert plan[:2] == ("cipher.batch", 1)
    if which == "shape-change":
        assert plan[3] == 256 and uaes.cipher_batch_plan(nmsg + 1, mode, 48)[3] == 1024
    if which == "second-pass":
        assert nmsg > plan[2] * plan[3] // 16 >= nmsg - 1                                       # it does run a second time
    rng = random.Random(nmsg)
    ivs, texts = records(rng, nmsg, 48)
    check(orc, mode, KEYS[128], ivs, texts, ("count", nmsg))                                    # every record is compared


# ---- 4. CTR's carries -------------------------------------------------------------------------------------------------
CARRIES = ["00ffffffffffffff", "0000000000ffffff", "fffffffffffffffe", "ffffffffffffffff"]


@pytest.mark.parametrize("bits", [128, 256])
def test_ctr_carries(orc, bits):
    """bytes 9..15 are the counter: a carry through three bytes, the 56-bit wrap after one block and at once; bytes 0..8
    never move, whether byte 8 is as the pattern writes it or ff like bytes 0..7.  Checked against the oracle and against
    counter blocks built here"""
    rng = random.Random(bits)
    key = KEYS[bits]
    ctrs = []
    for c in CARRIES:                                                   # the pattern = bytes 8..15; then byte 8 = ff, too
        tail = bytes.fromhex(c)
        for b8 in (tail[:1], b"\xff"):
            if b"\xff" * 8 + b8 + tail[1:] not in ctrs:
                ctrs.append(b"\xff" * 8 + b8 + tail[1:])
    assert len(ctrs) == 5 and all(len(c) == 16 for c in ctrs)
    for blocks in (3, 40):
        texts = [rng.randbytes(16 * blocks) for _ in ctrs]
        got = check(orc, "ctr", key, ctrs, texts, ("carries", bits, blocks))
        for c0, t, g in zip(ctrs, texts, got):
            v0 = int.from_bytes(c0[9:], "big")
            for i in range(blocks):
                blk = c0[:9] + ((v0 + i) % (1 << 56)).to_bytes(7, "big")
                ks = orc.encrypt_block(key, blk)
                assert bytes(a ^ b for a, b in zip(ks, t[16 * i:16 * i + 16])) == g[16 * i:16 * i + 16], (c0.hex(), blocks, i)


# ---- 5. variable lengths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_on_device", [False, True], ids=["host-lens", "device-lens"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", WITH_LENS)
def test_variable_lengths(orc, mode, device, lens_on_device):
    """entries 0, msg_bytes and msg_bytes + 7 (taken as msg_bytes); what lies behind a record's end stays the caller's"""
    rng = random.Random(48)
    key, n, ml = KEYS[128], 37, 48
    lens = [rng.randrange(49) for _ in range(n)]
    lens[3], lens[20], lens[36], lens[11] = 0, 48, 17, 48 + 7
    eff = [min(k, ml) for k in lens]
    ivs, slots = records(rng, n, ml)
    want = expected(orc, mode, key, ivs, [s[:k] for s, k in zip(slots, eff)])
    lv = Mem(b"".join(k.to_bytes(4, "little") for k in lens), lens_on_device)
    src, dst, mv = Mem(b"".join(slots), device), Mem(b"", device, size=n * ml), Mem(b"".join(ivs), device)
    assert batch(mode, key, mv, n, ml, lv, src, dst) == 0
    out = dst.get()
    for m in range(n):
        info = (mode, device, lens_on_device, m, lens[m])
        assert out[m * ml:m * ml + eff[m]] == want[m], info
        assert set(out[m * ml + eff[m]:(m + 1) * ml]) <= {FILL}, info                           # beyond lens[m]: not written
    assert dst.intact(n * ml) and src.get() == b"".join(slots) and lv.intact(4 * n)
    # in place: the rest of a slot stays the input's
    io = Mem(b"".join(slots), device)
    assert batch(mode, key, mv, n, ml, lv, io, io) == 0
    got = io.get()
    for m in range(n):
        assert got[m * ml:(m + 1) * ml] == want[m] + slots[m][eff[m]:], (mode, device, lens_on_device, m, "in place")
    assert io.intact(n * ml)


def test_device_lens_must_be_aligned():
    lv = Mem(bytes(4 * 4), True, off=2)
    src, dst, mv = Mem(bytes(64), True), Mem(b"", True, size=64), Mem(bytes(64), True)
    for mode in WITH_LENS:
        assert batch(mode, KEYS[128], mv, 4, 16, lv, src, dst) == E_ARG, mode
        assert dst.intact(0)


# ---- 6. placement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", ["host", "device", "device+1", "device+3"])
@pytest.mark.parametrize("mode", ALL)
def test_placement(orc, mode, place):
    """offsets 1 and 3: the byte-wise path (33-byte records where the mode takes them); IVs on the device at offsets 0 and 5"""
    device, off = place != "host", int(place[-1]) if "+" in place else 0
    rng = random.Random(33 + off)
    key, n = KEYS[192], 21
    ml = 48 if not MODES[mode][1] else 33 if off else 32
    ivs, texts = records(rng, n, ml)
    want = b"".join(expected(orc, mode, key, ivs, texts))
    for iv_off in (0, 5):
        info = (mode, place, iv_off)
        mv = Mem(b"".join(ivs), True, iv_off)
        src, dst = Mem(b"".join(texts), device, off), Mem(b"", device, off, size=n * ml)
        assert batch(mode, key, mv, n, ml, None, src, dst) == 0, info
        assert dst.get() == want and dst.intact(n * ml) and src.get() == b"".join(texts) and src.intact(n * ml), info
        io = Mem(b"".join(texts), device, off)
        assert batch(mode, key, mv, n, ml, None, io, io) == 0, info
        assert io.get() == want and io.intact(n * ml), (info, "in place")
        assert mv.get() == b"".join(ivs) and mv.intact(16 * n), info
    # the IVs in host memory, the texts where they are
    src, dst = Mem(b"".join(texts), device, off), Mem(b"", device, off, size=n * ml)
    assert batch(mode, key, Mem(b"".join(ivs), False, 1), n, ml, None, src, dst) == 0
    assert dst.get() == want and dst.intact(n * ml)


# ---- 7. one call at a time --------------------------------------------------------------------------------------------
ONE = {
    "cbc_decrypt": lambda k, v, t: uaes.AES_CBC_decrypt(k, v, t)[1],
    "cbc_decrypt_blocks": lambda k, v, t: uaes.AES_CBC_decrypt(k, v, t, cts=False)[1],
    "cbc_encrypt_blocks": lambda k, v, t: uaes.AES_CBC_encrypt(k, v, t, cts=False, padding=0)[1],
    "cfb_encrypt": uaes.AES_CFB_encrypt,
    "cfb_decrypt": uaes.AES_CFB_decrypt,
    "ofb": uaes.AES_OFB_encrypt,
    "ctr": lambda k, v, t: uaes.ctr_xcrypt_at(k, v, 0, t),
}


@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("mode", ALL)
def test_equals_the_one_message_calls(mode, bits):
    rng = random.Random(bits)
    key = KEYS[bits]
    for ml in ((16, 32, 112, 1008) if not MODES[mode][1] else (1, 16, 100, 257, 1000)):
        ivs, texts = records(rng, 7, ml)
        got = MODES[mode][3](key, ivs, texts)
        for m in range(7):
            assert got[m] == ONE[mode](key, ivs[m], texts[m]), (mode, bits, ml, m)


# ---- 8. round trips ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_round_trips(bits):
    rng = random.Random(bits + 1)
    key = KEYS[bits]
    for n, ml in ((1, 16), (5, 32), (70, 48), (9, 1024)):
        ivs, texts = records(rng, n, ml)
        assert uaes.cbc_decrypt_batch(key, ivs, uaes.cbc_encrypt_batch(key, ivs, texts)) == texts, (bits, n, ml)
        assert uaes.cbc_blocks_batch(key, ivs, uaes.cbc_blocks_batch(key, ivs, texts), decrypt=True) == texts, (bits, n, ml)
        if ml > 16:                                                                           # the two forms differ by the swap alone
            cs3, plain = uaes.cbc_encrypt_batch(key, ivs, texts), uaes.cbc_blocks_batch(key, ivs, texts)
            assert [c[:-32] + c[-16:] + c[-32:-16] for c in cs3] == plain, (bits, n, ml)
    ivs, texts = records(rng, 40, 77)
    ragged = [t[:rng.randrange(78)] for t in texts]
    assert uaes.cfb_batch(key, ivs, uaes.cfb_batch(key, ivs, ragged), decrypt=True) == ragged
    assert uaes.ofb_batch(key, ivs, uaes.ofb_batch(key, ivs, ragged)) == ragged
    assert uaes.ctr_batch(key, ivs, uaes.ctr_batch(key, ivs, ragged)) == ragged


# ---- 9. fuzz ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(orc, seed):
    rng = random.Random(9000 + seed)
    mode = rng.choice(ALL)
    bits = rng.choice((128, 192, 256))
    key = rng.randbytes(bits // 8)
    n = rng.randrange(1, 301)
    ml = rng.randrange(601) if MODES[mode][1] else 16 * rng.randrange(1, 38)
    lens = [rng.randrange(ml + 9) for _ in range(n)] if MODES[mode][1] and rng.randrange(2) else None
    device, off, in_place = rng.randrange(2) == 1, rng.choice((0, 0, 1, 2, 3)), rng.randrange(3) == 0
    info = ("fuzz", seed, mode, bits, n, ml, lens is not None, device, off, in_place)
    ivs, slots = records(rng, n, ml)
    eff = [ml] * n if lens is None else [min(k, ml) for k in lens]
    want = expected(orc, mode, key, ivs, [s[:k] for s, k in zip(slots, eff)])
    lv = None if lens is None else Mem(b"".join(k.to_bytes(4, "little") for k in lens), rng.randrange(2) == 1)
    mv = Mem(b"".join(ivs), rng.randrange(2) == 1, rng.randrange(4))
    src = Mem(b"".join(slots), device, off)
    dst = src if in_place else Mem(b"", device, off, size=n * ml)
    assert batch(mode, key, mv, n, ml, lv, src, dst) == 0, info
    out = dst.get()
    for m in range(n):
        rest = slots[m][eff[m]:] if in_place else bytes([FILL]) * (ml - eff[m])
        assert out[m * ml:(m + 1) * ml] == want[m] + rest, (info, m)
    assert dst.intact(n * ml), info


# ---- 10. threads ------------------------------------------------------------------------------------------------------
def test_two_threads_with_different_keys(orc):
    """the expected values are made first; the threads only call the engine"""
    cases = {}
    for seed in (10, 20):
        rng = random.Random(seed)
        key = rng.randbytes(16 if seed == 10 else 32)
        cases[seed] = []
        for mode in ALL:
            for n, ml in ((1, 16), (70, 64), (300, 48), (9, 1008)):
                ivs, texts = records(rng, n, ml)
                cases[seed].append((mode, key, ivs, texts, expected(orc, mode, key, ivs, texts)))
    errors = []

    def worker(seed):
        try:
            for _ in range(3):
                for mode, key, ivs, texts, want in cases[seed]:
                    assert MODES[mode][3](key, ivs, texts) == want, (seed, mode, len(texts), len(texts[0]))
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(s,)) for s in (10, 20)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
