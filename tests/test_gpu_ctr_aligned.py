"""The striped CTR kernel (k_ctr_shared2) with its lanes pinned to the stream: stripes of 2048 blocks counted from
block 0 of the text whatever the first counter's byte 15 (c0) is, nine counter groups per stripe, a lane whose
position carries into the next group (uaes_ctr.hip.h).  Every case against the CPU oracle, byte for byte.

The kernel needs one grid of stripes (32 KiB per workgroup: 8 MiB on 256 CUs), so that is the size of a case.  CTR of a
prefix is the prefix of the CTR: one oracle run per key and counter serves every length."""
import functools

import pytest

import micro_aes_amd as uaes

pytestmark = pytest.mark.gpu

STRIPE = 2048 * 16                                  # bytes
KEYS = {bits: bytes(range(3, 3 + bits // 8)) for bits in (128, 192, 256)}
HEAD = bytes(range(0xB0, 0xB9))                     # bytes 0..8 of the counter block
GUARD = 64


def _counter(v):
    return HEAD + (v & ((1 << 56) - 1)).to_bytes(7, "big")


@functools.lru_cache(maxsize=None)
def _grid():
    """workgroups of the striped kernel = stripes of one round"""
    name, _launches, grid, _ = uaes.plan("ctr", 1 << 30)
    assert name == "ctr.striped"
    return grid


def _tail_split(grid):
    """r stripes of a last partial round stay stripes from r * 100 >= grid * 80 on (CTR_TAIL_PCT): (just under, just over)"""
    over = (grid * 80 + 99) // 100
    return over - 1, over


@functools.lru_cache(maxsize=3)
def _text(n):
    from oracle.pyoracle import Oracle
    return Oracle().splitmix(808, n)


@functools.lru_cache(maxsize=4)
def _expect(bits, v, n):
    from oracle.pyoracle import Oracle
    return Oracle().ctr_xcrypt_at(KEYS[bits], _counter(v), 0, _text(n))


def _aligned(torch, nbytes, offset):
    """a device buffer of nbytes that starts `offset` bytes behind a 1 KiB boundary, filled with 0xEE"""
    raw = torch.full((nbytes + 2048,), 0xEE, dtype=torch.uint8, device="cuda:0")
    skip = (-raw.data_ptr()) % 1024 + offset
    view = raw[skip:skip + nbytes]
    assert view.data_ptr() % 1024 == offset % 1024
    return view


def _run(torch, bits, v, n, want, in_off=0, out_off=0, inplace=False, what=()):
    src = _aligned(torch, n + GUARD, in_off)
    src[:n].copy_(torch.frombuffer(bytearray(_text(n)), dtype=torch.uint8))
    dst = src if inplace else _aligned(torch, n + GUARD, out_off)
    uaes.ctr_xcrypt_dev(KEYS[bits], _counter(v), 0, src, dst, nbytes=n)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().tobytes()
    if got[:n] != want[:n]:
        bad = next(i for i in range(0, n, 16) if got[i:i + 16] != want[i:i + 16])
        raise AssertionError(("first wrong block", bad // 16, "of", n // 16, "bytes", n) + tuple(what))
    assert got[n:] == b"\xEE" * GUARD, ("bytes behind the text were written", n) + tuple(what)
    if not inplace:
        assert src[:n].cpu().numpy().tobytes() == _text(n), ("the input changed", n) + tuple(what)


def _is_striped(v, n):
    return uaes.plan("ctr", n, counter=_counter(v))[0] == "ctr.striped"


@pytest.mark.parametrize("c0", [0, 1, 2, 63, 64, 65, 191, 192, 255])
def test_every_length_at_every_first_position(c0):
    """one grid of stripes exactly, + one block, + 2047 blocks (one short of another stripe), + 5 bytes, and a last
    partial round of stripes just under (handed to the edge path) and just over the 80 % rule (kept as stripes, with a
    ragged end behind them).  c0 = 1 also takes two whole rounds, where a text that does not start a counter group is
    certain to be striped at the exact size."""
    import torch
    grid = _grid()
    G = grid * STRIPE
    under, over = _tail_split(grid)
    sizes = [G, G + 16, G + 2047 * 16, G + 5, G + under * STRIPE, G + over * STRIPE + 7 * 16 + 3]
    if c0 == 1:
        sizes += [2 * G, 2 * G + 16]
    v = 0x5A1234567800 + c0
    nmax = max(sizes)
    want = _expect(128, v, nmax)
    assert _text(nmax)[:G] == _text(G)
    # from one group behind a whole grid of stripes on the planner answers ctr.striped for every c0
    assert all(_is_striped(v, n) for n in sizes if n >= G + 4096), c0
    assert _is_striped(v, G) == (c0 == 0)
    for n in sizes:
        _run(torch, 128, v, n, want, what=(c0,))


@pytest.mark.parametrize("bits", [192, 256])
def test_the_longer_keys(bits):
    import torch
    n = _grid() * STRIPE + 2047 * 16 + 5
    for c0 in (0, 1, 255):
        v = 0x77000000AB00 + c0
        assert _is_striped(v, n)
        _run(torch, bits, v, n, _expect(bits, v, n), what=(bits, c0))


@pytest.mark.parametrize("c0", [1, 192])
def test_placement(c0):
    """in == out, and in and out each 16 and 1008 bytes behind a 1 KiB boundary"""
    import torch
    n = _grid() * STRIPE + 2047 * 16 + 5
    v = 0x3300000C0D00 + c0
    assert _is_striped(v, n)
    want = _expect(128, v, n)
    for in_off, out_off in ((16, 0), (1008, 0), (0, 16), (0, 1008), (16, 1008), (1008, 16)):
        _run(torch, 128, v, n, want, in_off, out_off, what=(c0, in_off, out_off))
    for off in (0, 16, 1008):
        _run(torch, 128, v, n, want, off, off, inplace=True, what=(c0, off, "in place"))


def _move_targets(grid):
    """blocks at which counter bits 40..47 are made to move, in a text of two rounds of stripes + 2047 blocks + 5 bytes:
    the first striped block, the last striped block, and a block in the middle of a wave's 64 (lane 37 of wave 1 of the
    third run of the first stripe of the second round: that lane and the ones above it carry, the ones below do not)"""
    return {"first": 0, "last": 2 * grid * 2048 - 1, "carry": grid * 2048 + 2 * 256 + 64 + 37}


@pytest.mark.parametrize("top", [0x12, 0xFFFF], ids=["bits40", "wrap56"])
@pytest.mark.parametrize("where", ["first", "last", "carry"])
def test_counter_bits_40_47_move(where, top):
    """the move (top = ffff: the wrap at 2^56) at the chosen block, one block before it and one block after it.  The
    lane constants of the striped kernel hold for one value of bits 40..47, so a move inside the stripes costs a second
    launch and a move behind them -- the block after the last striped one -- does not."""
    import torch
    grid = _grid()
    n = 2 * grid * STRIPE + 2047 * 16 + 5
    t = _move_targets(grid)[where]
    for k in (t - 1, t, t + 1):
        v = ((top << 40) | ((-k) % (1 << 40))) & ((1 << 56) - 1)    # block k is the first with the new bits 40..47
        name, launches = uaes.plan("ctr", n, counter=_counter(v))[:2]
        assert name == "ctr.striped", (where, top, k)
        inside = 0 < k <= 2 * grid * 2048 - 1
        assert launches == (2 if inside else 1), (where, top, k, launches)
        if where == "carry":
            c0 = v & 0xFF
            assert (c0 + 64 + 37 + (k - t)) == 256                  # the first lane that carries sits at block k
        _run(torch, 128, v, n, _expect(128, v, n), what=(where, top, k))
