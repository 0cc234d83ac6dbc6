"""AES key wrap (RFC 3394) on the GPU (uaes_kw.hip) against the compiled reference: the RFC's six parameter sets, every
short length, the lengths where the step counter grows a byte, the LDS / in-place boundary read from the planner at
byte offsets 0..3, every residue of the chain's length against the look-ahead chunk, forgeries, a wrapping of the other
mode (key wrap with padding runs the same kernels), the wipe switch and error lengths on device pointers, the in-place form, batches whose
shapes come from the planner (with forged records in the first workgroup and in the stride loop's second turn) and a
seeded fuzz of round trips.  Every failing case prints the tuple that reproduces it."""
import ctypes as C
import functools
import random

import pytest

import micro_aes_amd as uaes
from tests import kw_ref as R
from tests import kwp_ref as P
from tests.guarded_mem import Mem

pytestmark = pytest.mark.gpu

E_ARG = -2
CHUNK = 16                                      # KW_CH: the steps kw.global's loads run ahead (uaes_kw.hip)


def kbuf(kek):
    return (C.c_uint8 * len(kek)).from_buffer_copy(kek)


def wrap(kek, secret, device=False, soff=0, doff=0):
    """uaes_kw_wrap through host or device buffers at the given byte offsets: (code, the output buffer)"""
    src, dst = Mem(secret, device, soff), Mem(b"", device, doff, size=len(secret) + 8)
    rc = uaes.engine().uaes_kw_wrap(len(kek) * 8, kbuf(kek), src.ptr, len(secret), dst.ptr)
    assert dst.intact() and src.get() == secret
    return rc, dst.get()


def unwrap(kek, wrapped, device=False, soff=0, doff=0):
    src, dst = Mem(wrapped, device, soff), Mem(b"", device, doff, size=max(len(wrapped) - 8, 0))
    rc = uaes.engine().uaes_kw_unwrap(len(kek) * 8, kbuf(kek), src.ptr, len(wrapped), dst.ptr)
    assert dst.intact() and src.get() == wrapped
    return rc, dst.get()


@functools.lru_cache(None)
def lds_max():
    """the longest secret whose semiblocks live in LDS, found by walking the planner"""
    b = [n for n in range(16, 1 << 17, 8) if uaes.kw_plan(n)[0] != uaes.kw_plan(n + 8)[0]]
    assert len(b) == 1 and uaes.kw_plan(b[0])[0] == "kw.lds" and uaes.kw_plan(b[0] + 8)[0] == "kw.global"
    return b[0]


@functools.lru_cache(None)
def batch_max():
    top = max(n for n in range(16, 1 << 13, 8) if uaes.kw_plan(n, 2) is not None)
    assert top >= 64 and uaes.kw_plan(top + 8, 2) is None
    return top


def check(kek, secret, device=False, soff=0, doff=0):
    info = (len(kek) * 8, len(secret), device, soff, doff)
    want = R.wrap(kek, secret)
    assert want[0] == 0
    assert wrap(kek, secret, device, soff, doff) == want, info
    assert unwrap(kek, want[1], device, soff, doff) == (0, secret), info


def test_rfc3394_vectors(golden_dir):
    for c in R.rfc3394(golden_dir):
        for device in (False, True):
            assert wrap(c["kek"], c["secret"], device) == (0, c["wrapped"]), (c["kek_bits"], c["data_bits"], device)
            assert unwrap(c["kek"], c["wrapped"], device) == (0, c["secret"]), (c["kek_bits"], c["data_bits"], device)


@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("unwrapping", [False, True])
def test_every_short_length(bits, unwrapping):
    """n = 2 .. 48 semiblocks: 6 n passes 255 between n = 42 and 43; host pointers for odd n, device pointers for even"""
    rng = random.Random(bits + unwrapping)
    for n in range(2, 49):
        kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
        w = R.wrap(kek, s)[1]
        if unwrapping:
            assert unwrap(kek, w, device=n % 2 == 0) == (0, s), (bits, n)
        else:
            assert wrap(kek, s, device=n % 2 == 0) == (0, w), (bits, n)


@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("unwrapping", [False, True])
def test_third_counter_byte(bits, unwrapping):
    """n = 10923: 6 n = 65538 steps, the step counter's third byte, in the in-place arrangement"""
    rng = random.Random(3 * bits + unwrapping)
    kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * 10923)
    assert uaes.kw_plan(len(s), unwrap=unwrapping)[0] == "kw.global"
    w = R.wrap(kek, s)[1]
    if unwrapping:
        assert unwrap(kek, w, device=True) == (0, s)
    else:
        assert wrap(kek, s, device=True) == (0, w)


@pytest.mark.parametrize("bits", [128, 192, 256])
@pytest.mark.parametrize("unwrapping", [False, True])
def test_lds_boundary_at_every_offset(bits, unwrapping):
    """the last two lengths of kw.lds and the first of kw.global, source and destination 0..3 bytes off an aligned base"""
    rng = random.Random(5 * bits + unwrapping)
    for size in (lds_max() - 8, lds_max(), lds_max() + 8):
        kek, s = rng.randbytes(bits // 8), rng.randbytes(size)
        w = R.wrap(kek, s)[1]
        for soff in range(4):
            for doff in range(4):
                if unwrapping:
                    assert unwrap(kek, w, True, soff, doff) == (0, s), (bits, size, soff, doff)
                else:
                    assert wrap(kek, s, True, soff, doff) == (0, w), (bits, size, soff, doff)
        if unwrapping:
            assert unwrap(kek, w, False, 1, 2) == (0, s), (bits, size)
        else:
            assert wrap(kek, s, False, 1, 2) == (0, w), (bits, size)


@pytest.mark.parametrize("unwrapping", [False, True])
def test_global_chunk_edges(unwrapping):
    """kw.global's loads run CHUNK steps ahead of the chain and its last chunk is short unless 6 n is a multiple of
    CHUNK.  6 n is even, so the residues 1 and 15 do not exist: the eight n above the boundary give every residue that
    does (0, 2, .. 14; 0, 2 and 14 are asserted to be among them); host and device memory in turn"""
    n0 = lds_max() // 8 + 1
    assert {0, 2, CHUNK - 2} <= {6 * n % CHUNK for n in range(n0, n0 + 8)}
    rng = random.Random(16 + unwrapping)
    for k, n in enumerate(range(n0, n0 + 8)):
        bits = (128, 192, 256)[k % 3]
        kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
        assert uaes.kw_plan(8 * n, unwrap=unwrapping)[0] == "kw.global"
        w = R.wrap(kek, s)[1]
        if unwrapping:
            assert unwrap(kek, w, device=k % 2 == 0) == (0, s), (bits, n)
        else:
            assert wrap(kek, s, device=k % 2 == 0) == (0, w), (bits, n)


def unwrap_padded(kek, wrapped, device):
    """uaes_kwp_unwrap: (code, the output buffer, *secretLen)"""
    src, dst, ln = Mem(wrapped, device), Mem(b"", device, size=len(wrapped) - 8), C.c_size_t(77)
    rc = uaes.engine().uaes_kwp_unwrap(len(kek) * 8, kbuf(kek), src.ptr, len(wrapped), dst.ptr, C.byref(ln))
    assert dst.intact() and src.get() == wrapped
    return rc, dst.get(), ln.value


@pytest.mark.parametrize("wipe", [0, 1])
def test_one_mode_does_not_unwrap_the_other(wipe):
    """Both modes run the same two kernels and differ in a template argument: a key wrap does not unwrap as a key wrap
    with padding, nor the padded wrap of a whole-semiblock secret as a key wrap -- 0x1A, and the output is what the chain
    made (zeros under the wipe switch), as in test_forgeries_and_the_wipe_switch.  One secret in LDS, one in place, and
    batches of five records of the shortest and the longest size"""
    rng = random.Random(3394 + 5649)
    eng = uaes.engine()
    kek = rng.randbytes(24)
    left = (lambda text: bytes(len(text))) if wipe else (lambda text: text)
    eng.uaes_set_wipe_on_auth_failure(wipe)
    try:
        for size, name in ((16, "lds"), (lds_max() + 8, "global")):
            assert uaes.kw_plan(size, unwrap=True)[0] == "kw." + name and uaes.kwp_plan(size, unwrap=True)[0] == "kwp." + name
            s = rng.randbytes(size)
            plain, padded = R.wrap(kek, s)[1], P.wrap(kek, s)
            assert len(plain) == len(padded) == size + 8
            as_padded, as_plain = P.unwrap(kek, plain), R.unwrap(kek, padded)
            assert as_padded[0] == as_plain[0] == 0x1A
            for device in (False, True):
                assert unwrap_padded(kek, plain, device) == (0x1A, left(as_padded[1]), 0), (size, device)
                assert unwrap(kek, padded, device) == (0x1A, left(as_plain[1])), (size, device)
        for size in (16, batch_max()):
            assert batch_max() == 256
            secrets = [rng.randbytes(size) for _ in range(5)]
            plain, padded = [R.wrap(kek, s)[1] for s in secrets], [P.wrap(kek, s) for s in secrets]
            assert uaes.kwp_batch(kek, plain, unwrap=True) == (0x1A, [left(P.unwrap(kek, w)[1]) for w in plain], [0] * 5, [0] * 5), size
            assert uaes.kw_batch(kek, padded, unwrap=True) == (0x1A, [left(R.unwrap(kek, w)[1]) for w in padded], [0] * 5), size
    finally:
        eng.uaes_set_wipe_on_auth_failure(0)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_forgeries_and_the_wipe_switch(bits):
    rng = random.Random(40 + bits)
    eng = uaes.engine()
    for n in (2, 3, 32, lds_max() // 8 + 1):
        kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
        w = R.wrap(kek, s)[1]
        for k2, w2 in R.forgeries(kek, w):
            rc, text = R.unwrap(k2, w2)
            assert rc == 0x1A
            assert unwrap(k2, w2, device=True) == (0x1A, text), (bits, n)
            assert unwrap(k2, w2, device=False, soff=1) == (0x1A, text), (bits, n)
            eng.uaes_set_wipe_on_auth_failure(1)
            try:
                assert unwrap(k2, w2, device=True, doff=3) == (0x1A, bytes(8 * n)), (bits, n)
                assert unwrap(k2, w2, device=False) == (0x1A, bytes(8 * n)), (bits, n)
                assert unwrap(kek, w, device=True) == (0, s)
            finally:
                eng.uaes_set_wipe_on_auth_failure(0)


def test_error_lengths_leave_the_buffer():
    rng = random.Random(6)
    for bits in (128, 192, 256):
        kek = rng.randbytes(bits // 8)
        for device in (False, True):
            for n in (0, 8, 12, 20):
                assert wrap(kek, rng.randbytes(n), device) == (1, b"\x5c" * (n + 8)) == R.wrap(kek, bytes(n), 0x5C)
            for n in (8, 16, 20):
                assert unwrap(kek, rng.randbytes(n), device) == (1, b"\x5c" * (n - 8)) == R.unwrap(kek, bytes(n), 0x5C)


@pytest.mark.parametrize("device", [False, True])
def test_in_place(device):
    """secret == wrapped + 8 in both arrangements and both directions"""
    rng = random.Random(7)
    L = uaes.engine()
    for bits in (128, 192, 256):
        for n in (2, 48, lds_max() // 8, lds_max() // 8 + 1, 2000):
            kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
            w = R.wrap(kek, s)[1]
            for off in (0, 3):
                m = Mem(b"\x5c" * 8 + s, device, off)
                assert L.uaes_kw_wrap(bits, kbuf(kek), C.c_void_p(m.ptr.value + 8), 8 * n, m.ptr) == 0
                assert m.get() == w and m.intact(), (bits, n, device, off)
                assert L.uaes_kw_unwrap(bits, kbuf(kek), m.ptr, 8 * n + 8, C.c_void_p(m.ptr.value + 8)) == 0
                assert m.get()[8:] == s and m.intact(), (bits, n, device, off)


@functools.lru_cache(None)
def batch_case(bits, size, nkeys):
    """one key, nkeys secrets of `size` bytes and the reference's wrap of each by itself (computed once, shared)"""
    rng = random.Random(1000 * bits + size)
    kek = rng.randbytes(bits // 8)
    secrets = [rng.randbytes(size) for _ in range(nkeys)]
    return kek, secrets, [R.wrap(kek, s)[1] for s in secrets]


def batch_shapes(size):
    """the record counts to test, from the planner: 1, 2, around one workgroup's rows, and one more than one turn of
    the stride loop of a full grid"""
    name, _, grid1, threads = uaes.kw_plan(size, 1)
    assert name == "kw.batch" and grid1 == 1 and threads % 16 == 0
    rows = threads // 16
    _, _, grid, threads = uaes.kw_plan(size, 1 << 22)                 # as many workgroups as the planner ever asks for
    full = grid * (threads // 16) + 1
    _, _, g, t = uaes.kw_plan(size, full)
    assert g * (t // 16) < full                                       # the stride loop takes a second turn
    return [1, 2, rows - 1, rows, rows + 1, full]


# (secret bytes, key size): every length of the list under one key size, the key sizes in turn
BATCH_SIZES = [(16, 128), (24, 192), (32, 256), (40, 128), (64, 192), (None, 256)]


@pytest.mark.parametrize("size,bits", BATCH_SIZES)
def test_wrap_batches(size, bits):
    size = size or batch_max()
    shapes = batch_shapes(size)
    kek, secrets, wrapped = batch_case(bits, size, shapes[-1])
    L = uaes.engine()
    for nkeys in shapes:
        device = nkeys != 2
        off = 0 if nkeys == shapes[-1] else nkeys % 4
        src, dst = Mem(b"".join(secrets[:nkeys]), device, off), Mem(b"", device, (off + 1) % 4, size=nkeys * (size + 8))
        assert L.uaes_kw_wrap_batch(bits, kbuf(kek), nkeys, size, src.ptr, dst.ptr) == 0, (size, nkeys)
        got = dst.get()
        for m in range(nkeys):
            assert got[m * (size + 8):(m + 1) * (size + 8)] == wrapped[m], (size, bits, nkeys, m)
        assert dst.intact()
    assert uaes.kw_batch(kek, secrets[:5]) == (0, wrapped[:5])                 # the Python mirror of the two calls
    assert uaes.kw_batch(kek, wrapped[:5], unwrap=True) == (0, secrets[:5], [1] * 5)
    bad = [wrapped[0], R.flip(wrapped[1], 70), wrapped[2]]
    assert uaes.kw_batch(kek, bad, unwrap=True) == (0x1A, [secrets[0], R.unwrap(kek, bad[1])[1], secrets[2]], [1, 0, 1])


@pytest.mark.parametrize("size,bits", BATCH_SIZES)
def test_unwrap_batches_with_forged_records(size, bits):
    size = size or batch_max()
    shapes = batch_shapes(size)
    kek, secrets, wrapped = batch_case(bits, size, shapes[-1])
    L = uaes.engine()
    for nkeys in shapes:
        device = nkeys != 2
        off = 0 if nkeys == shapes[-1] else nkeys % 4
        forged = sorted({0, nkeys // 2, nkeys - 1})                     # the last of a full grid + 1: the second turn
        recs = list(wrapped[:nkeys])
        for k, m in enumerate(forged):
            recs[m] = R.flip(recs[m], (13, 64 + 5, 8 * size + 60)[k % 3])
        ref_text = {m: R.unwrap(kek, recs[m]) for m in forged}
        assert all(rc == 0x1A for rc, _ in ref_text.values())
        for wipe in (0, 1):
            src, dst, ver = Mem(b"".join(recs), device, off), Mem(b"", device, (off + 2) % 4, size=nkeys * size), Mem(b"", device, size=nkeys)
            L.uaes_set_wipe_on_auth_failure(wipe)
            try:
                rc = L.uaes_kw_unwrap_batch(bits, kbuf(kek), nkeys, size + 8, src.ptr, dst.ptr, ver.ptr)
            finally:
                L.uaes_set_wipe_on_auth_failure(0)
            assert rc == 0x1A, (size, nkeys)
            assert ver.get() == bytes(0 if m in forged else 1 for m in range(nkeys)), (size, bits, nkeys)
            got = dst.get()
            for m in range(nkeys):
                want = secrets[m] if m not in forged else bytes(size) if wipe else ref_text[m][1]
                assert got[m * size:(m + 1) * size] == want, (size, bits, nkeys, m, wipe)
            assert dst.intact() and ver.intact()
    # nothing forged: 0, every verdict 1
    nkeys = shapes[4]
    src, dst, ver = Mem(b"".join(wrapped[:nkeys]), True), Mem(b"", True, size=nkeys * size), Mem(b"", False, size=nkeys)
    assert L.uaes_kw_unwrap_batch(bits, kbuf(kek), nkeys, size + 8, src.ptr, dst.ptr, ver.ptr) == 0
    assert ver.get() == b"\x01" * nkeys and dst.get() == b"".join(secrets[:nkeys])


def test_batch_limits():
    L = uaes.engine()
    kek = bytes(range(16))
    big = batch_max() + 8
    src, dst, ver = Mem(bytes(4 * (big + 8)), True), Mem(b"", True, size=4 * (big + 8)), Mem(b"", True, size=4)
    assert L.uaes_kw_wrap_batch(128, kbuf(kek), 4, big, src.ptr, dst.ptr) == E_ARG
    assert b"at most" in L.uaes_last_error()
    assert L.uaes_kw_unwrap_batch(128, kbuf(kek), 4, big + 8, src.ptr, dst.ptr, ver.ptr) == E_ARG
    for n in (0, 8, 12, 20):
        assert L.uaes_kw_wrap_batch(128, kbuf(kek), 4, n, src.ptr, dst.ptr) == 1
    for n in (8, 16, 20):
        assert L.uaes_kw_unwrap_batch(128, kbuf(kek), 4, n, src.ptr, dst.ptr, ver.ptr) == 1
    assert set(dst.get()) == {0x5C} and set(ver.get()) == {0x5C} and dst.intact()
    assert L.uaes_kw_wrap_batch(128, kbuf(kek), 0, 32, src.ptr, dst.ptr) == 0


def test_fuzz_round_trips():
    """200 wrap-then-unwrap round trips: random key size, length up to 4 KiB, pointer kind and offsets"""
    rng = random.Random(20240)
    for it in range(200):
        bits = rng.choice((128, 192, 256))
        n = rng.randrange(2, 513) if it % 4 else rng.randrange(2, 12)
        kek, s = rng.randbytes(bits // 8), rng.randbytes(8 * n)
        device, soff, doff = rng.random() < 0.5, rng.randrange(4), rng.randrange(4)
        info = (it, bits, n, device, soff, doff)
        want = R.wrap(kek, s)
        assert wrap(kek, s, device, soff, doff) == want, info
        assert unwrap(kek, want[1], device, doff, soff) == (0, s) == R.unwrap(kek, want[1]), info
