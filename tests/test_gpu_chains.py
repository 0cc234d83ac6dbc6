"""CBC / CFB / OFB, CMAC, CCM and the batches of chains (uaes_chain.hip, uaes_mac.hip) at every boundary, every short
length and every buffer placement, bit-exact against the oracle through the run-time C ABI.

Every boundary comes from uaes.chain_plan() (uaes_debug_plan_chain: the rows the launchers themselves switch on) and
from the device's CU count; tests/chain_cases.py walks them.  Buffers are placed by `Place` below: FRONT guard bytes in
front of and behind the payload, both checked (tests/test_gpu_fuzz.py's Buffers checks the 16 bytes behind only and
draws its placement at random; here the placement is the case).

What the placements reach: the host layer (plan_io, uaes_engine.c) hands the kernels a 16-byte aligned copy of any
text that is not 16-byte aligned device memory, so the (in, out) offsets exercise that staging and the copy back;
inside the kernels the unaligned branches (A4 = false, cbcmac_absorb's byte walk, the lane kernel's block loads off
alignment) are reached by CMAC batches whose message size is no multiple of 4 / 16 and by CCM associated data, whose
first block is 14 or 10 bytes so that the rest starts 2 or 6 bytes into an aligned array.
"""
import ctypes as C
import hashlib

import pytest

import micro_aes_amd as uaes
from tests import chain_cases as K

pytestmark = pytest.mark.gpu

G = 0xA5
FRONT = 64
MIB = K.MIB
KEYS = {128: bytes(range(0x10, 0x20)), 192: bytes(range(0x30, 0x48)), 256: bytes(range(0x60, 0x80))}
IV = bytes(range(0xE0, 0xF0))
# (input offset, output offset, in place) from a 16-byte boundary
PLACEMENTS = [(0, 0, False), (4, 8, False), (1, 0, False), (0, 3, False), (2, 2, True)]
PLACEMENT_IDS = ["in0-out0", "in4-out8", "in1-out0", "in0-out3", "inplace2"]
E_ARG = -2                                       # UAES_E_ARG (include/uaes_hip.h)


class Place:
    """len(data) bytes of input and room for n_out bytes of output, each `off` bytes from a 16-byte boundary, in device
    (dev=True) or host memory, FRONT guard bytes in front of and behind either; in place: one buffer for both"""

    def __init__(self, data, n_out, off_in=0, off_out=0, inplace=False, dev=True):
        self.dev, self.inplace, self.data, self.n_out = dev, inplace, bytes(data), n_out
        self.s_in = FRONT + off_in
        self.s_out = self.s_in if inplace else FRONT + off_out
        span = max(len(data), n_out) if inplace else len(data)
        self.b_in = self._buf(self.s_in + span + FRONT)
        self._put(self.b_in, self.s_in, self.data)
        self.b_out = self.b_in if inplace else self._buf(self.s_out + n_out + FRONT)
        self.pin = C.c_void_p(self._addr(self.b_in) + self.s_in)
        self.pout = C.c_void_p(self._addr(self.b_out) + self.s_out)

    def _buf(self, n):
        if self.dev:
            import torch
            t = torch.full((n,), G, dtype=torch.uint8, device="cuda:0")
            assert t.data_ptr() % 16 == 0
            return t
        b = (C.c_uint8 * n)()
        C.memset(b, G, n)
        return b

    def _addr(self, b):
        return b.data_ptr() if self.dev else C.addressof(b)

    def _put(self, b, at, data):
        if not data:
            return
        if self.dev:
            import torch
            b[at:at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
        else:
            C.memmove(C.addressof(b) + at, data, len(data))

    def _raw(self, b):
        if self.dev:
            import torch
            torch.cuda.synchronize()
            return b.cpu().numpy().tobytes()
        return bytes(b)

    def result(self, n=None):
        """(the n output bytes, every byte in front of and behind the payload still the guard value?)"""
        n = self.n_out if n is None else n
        raw = self._raw(self.b_out)
        end = self.s_out + (max(n, len(self.data)) if self.inplace else n)
        intact = raw[:self.s_out] == bytes([G]) * self.s_out and raw[end:] == bytes([G]) * (len(raw) - end)
        return raw[self.s_out:self.s_out + n], intact

    def input_intact(self):
        """out of place: the input and its guards are as they were"""
        if self.inplace:
            return True
        raw = self._raw(self.b_in)
        return raw == bytes([G]) * self.s_in + self.data + bytes([G]) * FRONT


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


_STREAM = {}


def _stream(orc, n, seed=5):
    """the first n bytes of one splitmix stream per seed (made once, grown on demand)"""
    if seed not in _STREAM or len(_STREAM[seed]) < n:
        _STREAM[seed] = orc.splitmix(seed, (max(n, MIB) + 7) // 8 * 8)
    return _STREAM[seed][:n]


def _same(got, want):
    if len(want) > 8 * MIB:
        return len(got) == len(want) and hashlib.sha256(got).digest() == hashlib.sha256(want).digest()
    return got == want


# ---------------------------------------------------------------------------------------------------------------------
# a. the parallel decrypt (k_fb_dec<U=1> / <U=4>) at and beyond every boundary
# ---------------------------------------------------------------------------------------------------------------------
FB_MODES = [("cbc", 0), ("cbc", 1), ("cbc", 7), ("cbc", 15), ("cbc_nocts", 0), ("cfb", 0), ("cfb", 1), ("cfb", 15)]
# The oracle's own time for a 24 MiB CBC decryption is 1.3 s in one call and 0.2 s cut into pieces on eight cores
# (K.oracle_decrypt), so every mode runs the largest size; the other key sizes run one tail per mode.
FB_KEY_MODES = [("cbc", 7), ("cbc_nocts", 0), ("cfb", 15)]


def _fb_fn(mode):
    L = uaes.engine()
    return {"cbc": L.uaes_cbc_decrypt, "cbc_nocts": L.uaes_cbc_decrypt_blocks, "cfb": L.uaes_cfb_decrypt}[mode]


def _fb_sizes(mode, tail):
    """bytes of parallel blocks: both sides of single -> tiled, the second pass of the grid-stride loop with one block,
    with a full tile and a block, an exact full grid, and a last pass that half the workgroups take (1.5 full grids)"""
    b, (g1, t1), (g4, t4), _ = K.fbdec_marks(_cus())
    ps = [b - 16, b, b + 16, g1 + 16, g1 + t1 + 16, g4, g4 + 16, g4 + t4 + 16]
    if (mode, tail) == ("cbc", 0):                  # the CS3 pair right behind a full grid (b, g1, g4) and a full tile
        ps += [g1, g1 + t1, g4 + t4]
    ps.append(g4 * 3 // 2 + 16 * 1001)
    return b, ps


def _fb_case(orc, mode, tail, p, bits, placements):
    b = K.fbdec_marks()[0]
    n = K.fbdec_len(mode, tail, p)
    plan = uaes.chain_plan(mode, n, decrypt=True)
    assert plan == uaes.chain_plan("cfb", p, decrypt=True) and plan[0] == ("fbdec.single" if p <= b else "fbdec.tiled"), (mode, tail, p, plan)
    key, data = KEYS[bits], _stream(orc, n)
    want = K.oracle_decrypt(orc, mode, key, IV, data)
    for dev, inplace in placements:
        pl = Place(data, n, inplace=inplace, dev=dev)
        info = (mode, tail, p, n, bits, plan, "device" if dev else "host", "in place" if inplace else "")
        assert _fb_fn(mode)(bits, key, IV, pl.pin, n, pl.pout) == 0, info
        got, intact = pl.result()
        assert _same(got, want), info
        assert intact, info + ("guard bytes",)


@pytest.mark.parametrize("mode,tail", FB_MODES, ids=["%s+%d" % m for m in FB_MODES])
def test_parallel_decrypt_at_every_boundary(orc, mode, tail):
    """CBC-CS3 decrypt (tail = bytes of the short last block; 0: whole blocks, the last two swapped), CBC decrypt of
    whole blocks and CFB decrypt (tail = bytes behind the last block), AES-128, device -> device and device in place
    (the private copy of feedback_common), input = any bytes.  The stolen pair / the tail is one lane's work behind the
    parallel blocks in the same launch."""
    b, ps = _fb_sizes(mode, tail)
    for p in ps:
        _fb_case(orc, mode, tail, p, 128, [(True, False), (True, True)])


@pytest.mark.parametrize("bits", [192, 256])
def test_parallel_decrypt_key_sizes(orc, bits):
    b, (g1, t1), (g4, t4), _ = K.fbdec_marks(_cus())
    for mode, tail in FB_KEY_MODES:
        for p in (b + 16, g4 + 16):
            _fb_case(orc, mode, tail, p, bits, [(True, False)])


def test_parallel_decrypt_host_to_host(orc):
    b = K.fbdec_marks(_cus())[0]
    for mode, tail in FB_KEY_MODES:
        _fb_case(orc, mode, tail, b + 16, 128, [(False, False)])


# ---------------------------------------------------------------------------------------------------------------------
# b. the serial chains (k_chain_serial), every short length
# ---------------------------------------------------------------------------------------------------------------------
def _serial_ops(orc):
    L = uaes.engine()

    def padded(p):
        return dict(lo=0,
                    enc=lambda bits, key, pin, n, pout: L.uaes_cbc_encrypt_padded(bits, key, IV, p, pin, n, pout),
                    want=lambda key, d: orc.cbc_nocts(key, IV, d, True, padding=p)[1],
                    dec=lambda bits, key, pin, n, pout: L.uaes_cbc_decrypt_blocks(bits, key, IV, pin, n, pout),
                    back=lambda key, ct, d: orc.cbc_nocts(key, IV, ct, False)[1])
    return {
        "cbc": dict(lo=16, enc=lambda bits, key, pin, n, pout: L.uaes_cbc_encrypt(bits, key, IV, pin, n, pout),
                    want=lambda key, d: orc.cbc(key, IV, d, True)[1],
                    dec=lambda bits, key, pin, n, pout: L.uaes_cbc_decrypt(bits, key, IV, pin, n, pout),
                    back=lambda key, ct, d: d),
        "cbc_pad0": padded(0), "cbc_pad1": padded(1), "cbc_pad2": padded(2),
        "cfb": dict(lo=0, enc=lambda bits, key, pin, n, pout: L.uaes_cfb_encrypt(bits, key, IV, pin, n, pout),
                    want=lambda key, d: orc.cfb(key, IV, d, True),
                    dec=lambda bits, key, pin, n, pout: L.uaes_cfb_decrypt(bits, key, IV, pin, n, pout),
                    back=lambda key, ct, d: d),
        "ofb": dict(lo=0, enc=lambda bits, key, pin, n, pout: L.uaes_ofb_xcrypt(bits, key, IV, pin, n, pout),
                    want=lambda key, d: orc.ofb(key, IV, d),
                    dec=lambda bits, key, pin, n, pout: L.uaes_ofb_xcrypt(bits, key, IV, pin, n, pout),
                    back=lambda key, ct, d: d),
    }


SERIAL_OPS = ["cbc", "cbc_pad0", "cbc_pad1", "cbc_pad2", "cfb", "ofb"]
SERIAL_PLACES = [("host", (0, 0, False))] + list(zip(PLACEMENT_IDS, PLACEMENTS))
_SERIAL_WANT = {}


def _serial_want(orc, op, bits, n):
    """the oracle's ciphertext of the first n stream bytes, computed once for every placement"""
    k = (op, bits, n)
    if k not in _SERIAL_WANT:
        _SERIAL_WANT[k] = _serial_ops(orc)[op]["want"](KEYS[bits], _stream(orc, n, 11))
    return _SERIAL_WANT[k]


def _serial_case(orc, o, op, bits, n, where, place):
    key, data = KEYS[bits], _stream(orc, n, 11)
    want = _serial_want(orc, op, bits, n)
    off_in, off_out, inplace = place
    dev = where != "host"
    info = (op, bits, n, where)
    assert uaes.chain_plan("cbc_nocts" if op.startswith("cbc_pad") else op, n)[0] == "chain.serial"
    pl = Place(data, len(want), off_in, off_out, inplace, dev)
    assert o["enc"](bits, key, pl.pin, n, pl.pout) == 0, info
    got, intact = pl.result()
    assert got == want and intact and pl.input_intact(), info
    if not want:
        return
    pl = Place(want, len(want), off_in, off_out, inplace, dev)            # back through the parallel direction
    assert o["dec"](bits, key, pl.pin, len(want), pl.pout) == 0, info
    got, intact = pl.result()
    assert got == o["back"](key, want, data) and got[:n] == data and intact and pl.input_intact(), info + ("decrypt",)


@pytest.mark.parametrize("where,place", SERIAL_PLACES, ids=[w for w, _ in SERIAL_PLACES])
@pytest.mark.parametrize("op", SERIAL_OPS)
def test_serial_chains_every_short_length(orc, op, where, place):
    """CBC-CS3 encrypt (from 16 bytes), CBC encrypt without stealing with padding 0 / 1 / 2 (from 0), CFB encrypt and
    OFB at every length up to 300, AES-128; host buffers and device buffers in five placements"""
    o = _serial_ops(orc)[op]
    for n in range(o["lo"], 301):
        _serial_case(orc, o, op, 128, n, where, place)


@pytest.mark.parametrize("bits", [192, 256])
@pytest.mark.parametrize("op", SERIAL_OPS)
def test_serial_chains_key_sizes(orc, op, bits):
    o = _serial_ops(orc)[op]
    for n in (16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257):
        for where, place in SERIAL_PLACES:
            _serial_case(orc, o, op, bits, n, where, place)


# ---------------------------------------------------------------------------------------------------------------------
# c. CMAC (k_cmac)
# ---------------------------------------------------------------------------------------------------------------------
def _cmac(bits, pin, n):
    mac = (C.c_uint8 * 48)()
    C.memset(mac, G, 48)
    assert uaes.engine().uaes_cmac(bits, KEYS[bits], pin, n, C.c_void_p(C.addressof(mac) + 16)) == 0, (bits, n)
    raw = bytes(mac)
    assert raw[:16] == raw[32:] == bytes([G]) * 16, (bits, n, "guard bytes")
    return raw[16:32]


def test_cmac_every_short_length(orc):
    assert uaes.chain_plan("cmac", 600) == ("chain.serial", 1, 1, 64)
    for n in range(601):
        data = _stream(orc, n, 13)
        pl = Place(data, 0, dev=False)
        assert _cmac(128, pl.pin, n) == orc.cmac(KEYS[128], data), n


def test_cmac_device_pointers_and_key_sizes(orc):
    edges = (0, 1, 15, 16, 17, 4095, 4096, 4097, 16400)
    for bits in (128, 192, 256):
        for n in edges:
            data = _stream(orc, n, 13)
            want = orc.cmac(KEYS[bits], data)
            for off in (0, 1, 2, 3, 16):
                pl = Place(data, 0, off_in=off)
                assert _cmac(bits, pl.pin, n) == want, (bits, n, off)
                assert pl.input_intact(), (bits, n, off)
            assert _cmac(bits, Place(data, 0, dev=False).pin, n) == want, (bits, n, "host")


# ---------------------------------------------------------------------------------------------------------------------
# d. CCM around the one-wave kernel (k_ccm) and the two-kernel form (k_ccm_tag + CTR)
# ---------------------------------------------------------------------------------------------------------------------
NONCE13 = bytes(range(0xA0, 0xAD))


def _aad_arg(aad, base=None):
    """host bytes, or (base given) device memory `base` bytes from a 16-byte boundary; returns (argument, keep-alive)"""
    if base is None or not aad:
        return aad, None
    pl = Place(aad, 0, off_in=base)
    return pl.pin, pl


def _ccm_enc(bits, nonce, tl, aad_arg, alen, pl, n):
    return uaes.engine().uaes_ccm_encrypt_ex(bits, KEYS[bits], nonce, len(nonce), tl, aad_arg, alen, pl.pin, n, pl.pout)


def _ccm_dec(bits, nonce, tl, aad_arg, alen, pl, n):
    return uaes.engine().uaes_ccm_decrypt_ex(bits, KEYS[bits], nonce, len(nonce), tl, aad_arg, alen, pl.pin, n, pl.pout)


def _ccm_round_trip(orc, bits, nonce, tl, aad, pt, place, dev, aad_base=None, want=None, info=()):
    """encrypt == the oracle (nothing written behind len + tag_len), decrypt returns the text"""
    n = len(pt)
    off_in, off_out, inplace = place
    want = orc.ccm_encrypt(KEYS[bits], nonce, aad, pt, tag_len=tl) if want is None else want
    a, keep = _aad_arg(aad, aad_base)
    info = (bits, len(nonce), tl, len(aad), aad_base, n, place, "device" if dev else "host") + tuple(info)
    pl = Place(pt, n + tl, off_in, off_out, inplace, dev)
    assert _ccm_enc(bits, nonce, tl, a, len(aad), pl, n) == 0, info
    got, intact = pl.result()
    assert got == want and intact and pl.input_intact(), info + ("encrypt",)
    pl = Place(want, n, off_in, off_out, inplace, dev)
    assert _ccm_dec(bits, nonce, tl, a, len(aad), pl, n) == 0, info
    got, intact = pl.result()
    assert got == pt and intact and pl.input_intact(), info + ("decrypt",)
    assert keep is None or keep.input_intact(), info + ("aad",)
    return want


def test_ccm_every_short_length(orc):
    """every text length up to 600 (both sides of the fused kernel's limit and far into the two-kernel form), host
    buffers, 11-byte nonce, 16-byte tag, with and without associated data"""
    b = K.ccm_fused_max()
    assert 0 < b < 600
    for n in range(601):
        assert uaes.chain_plan("ccm", n)[0] == ("ccm.fused" if n <= b else "ccm.split")
        _ccm_round_trip(orc, 128, NONCE13[:11], 16, b"" if n % 3 == 0 else b"header %d" % n, _stream(orc, n, 17),
                        (0, 0, False), dev=False)


@pytest.mark.parametrize("place", PLACEMENTS, ids=PLACEMENT_IDS)
def test_ccm_around_the_fused_limit_on_device_buffers(orc, place):
    b = K.ccm_fused_max()
    assert uaes.chain_plan("ccm", b)[0] == "ccm.fused" and uaes.chain_plan("ccm", b + 1)[0] == "ccm.split"
    for bits in (128, 192, 256):
        for n in range(b - 17, b + 18):
            _ccm_round_trip(orc, bits, NONCE13[:11], 16, b"hdr", _stream(orc, n, 17), place, dev=True)


@pytest.mark.parametrize("n", [61, 1000])
def test_ccm_nonce_and_tag_lengths_and_forgeries(orc, n):
    """the 7 x 7 matrix of nonce lengths 7..13 and tag lengths 4..16 on device pointers at one fused and one split
    size; a forged tag (last byte, first byte) and a flipped ciphertext byte give 0x1A with the decrypted text left in
    place, which is what the reference's default build does (orc.ccm_decrypt)"""
    b = K.ccm_fused_max()
    assert uaes.chain_plan("ccm", n)[0] == ("ccm.fused" if n <= b else "ccm.split") and (n <= b) == (n == 61)
    pt, aad = _stream(orc, n, 19), b"associated"
    for nl in range(7, 14):
        for tl in range(4, 17, 2):
            nonce = NONCE13[:nl]
            want = _ccm_round_trip(orc, 128, nonce, tl, aad, pt, (0, 0, False), dev=True)
            for where in (n + tl - 1, n, n // 2):
                bad = bytearray(want)
                bad[where] ^= 0x20
                rc, text = orc.ccm_decrypt(KEYS[128], nonce, aad, bytes(bad), tag_len=tl)
                assert rc == 0x1A and (text == pt) == (where >= n)
                pl = Place(bytes(bad), n)
                assert _ccm_dec(128, nonce, tl, aad, len(aad), pl, n) == 0x1A, (nl, tl, n, where)
                got, intact = pl.result()
                assert got == text and intact and pl.input_intact(), (nl, tl, n, where)


AAD_LENS = list(range(49)) + [0xFEFE, 0xFEFF, 0xFF00, 0xFF01, 0xFF00 + 9, 0xFF00 + 10, 0xFF00 + 11]


@pytest.mark.parametrize("base", [None, 0, 1, 2], ids=["host", "dev0", "dev1", "dev2"])
@pytest.mark.parametrize("n", [33, 300])
def test_ccm_associated_data(orc, n, base):
    """every AAD length up to 48 (13 / 14 / 15: the two-byte header's first block fills at 14), the switch to the
    six-byte header (0xFEFF / 0xFF00) and its first block filling at 10 bytes, in host memory and in device memory 0,
    1 and 2 bytes from a 16-byte boundary (base 2: what follows the 14-byte first block is 4-byte aligned, the only way
    cbcmac_absorb's aligned branch sees AAD), in the fused kernel and in k_ccm_tag"""
    assert uaes.chain_plan("ccm", 33)[0] == "ccm.fused" and uaes.chain_plan("ccm", 300)[0] == "ccm.split"
    pt, stream = _stream(orc, n, 23), _stream(orc, 0x10000, 29)
    for alen in AAD_LENS:
        _ccm_round_trip(orc, 128, NONCE13[:11], 16, stream[:alen], pt, (0, 0, False), dev=True, aad_base=base)


# ---------------------------------------------------------------------------------------------------------------------
# e. CCM at chosen counters
# ---------------------------------------------------------------------------------------------------------------------
def _ccm_blocks(nonce):
    """(iv = {14 - nl, nonce, 0...}, the first keystream counter block = iv + 1 in bytes 9..15)"""
    iv = bytes([14 - len(nonce)]) + nonce + bytes(15 - len(nonce))
    v = (int.from_bytes(iv[9:], "big") + 1) & ((1 << 56) - 1)
    return iv, iv[:9] + v.to_bytes(7, "big")


def _ccm_counter_expect(orc, bits, nonce, n):
    """(orc.ccm_encrypt, CTR from {14 - nl, nonce, 0...} + 1 by the oracle) as two jobs on the pool"""
    key, pt = KEYS[bits], _stream(orc, n, 31)
    return (K.POOL.submit(orc.ccm_encrypt, key, nonce, b"counter", pt),
            K.POOL.submit(orc.ctr_xcrypt_at, key, _ccm_blocks(nonce)[0], 1, pt))


def _ccm_counter_case(orc, bits, nonce, n, info, expect=None):
    pt, aad = _stream(orc, n, 31), b"counter"
    want, body = [j.result() for j in (expect or _ccm_counter_expect(orc, bits, nonce, n))]
    assert want[:n] == body, info                                         # (the oracle with itself)
    pl = Place(pt, n + 16)
    assert _ccm_enc(bits, nonce, 16, aad, len(aad), pl, n) == 0, info
    got, intact = pl.result()
    assert got[:n] == body, info + ("keystream",)
    assert got == want and intact, info + ("encrypt",)
    pl = Place(want, n)
    assert _ccm_dec(bits, nonce, 16, aad, len(aad), pl, n) == 0, info + ("decrypt",)
    got, intact = pl.result()
    assert got == pt and intact, info + ("decrypt",)
    return want


@pytest.mark.parametrize("bits", [128, 256])
def test_ccm_counter_wraps_at_2_to_56_without_touching_byte_8(orc, bits):
    """13-byte nonce ending in ff ff ff ff ff: the counter (bytes 9..15 of the block) starts at ff ff ff ff ff 00 01
    and wraps to zero at block 65 535; bytes 0..8, nonce bytes among them, stay"""
    nonce = NONCE13[:8] + b"\xff" * 5
    n = MIB + 4096 + 5
    iv, first = _ccm_blocks(nonce)
    wrap = (1 << 56) - int.from_bytes(first[9:], "big")
    assert wrap == 65535 and 16 * wrap + 16 <= n
    want = _ccm_counter_case(orc, bits, nonce, n, (bits, "wrap"))
    pt = _stream(orc, n, 31)
    ks = bytes(x ^ y for x, y in zip(want[16 * wrap:16 * wrap + 16], pt[16 * wrap:16 * wrap + 16]))
    assert ks == orc.encrypt_block(KEYS[bits], iv[:9] + bytes(7)), "byte 8 moved"


def _striped_size():
    """the first size at which the CTR planner answers ctr.striped for a counter that does not carry"""
    return K.first(lambda m: uaes.plan("ctr", m)[0] == "ctr.striped", 16, 1 << 30)


def _ccm_counter_sizes(orc, bits, nonce, launches):
    n = _striped_size()
    first = _ccm_blocks(nonce)[1]
    expect = {m: _ccm_counter_expect(orc, bits, nonce, m) for m in (n, n - 4096)}
    assert uaes.plan("ctr", n, counter=first)[:2] == ("ctr.striped", launches), uaes.plan("ctr", n, counter=first)
    assert uaes.plan("ctr", n - 4096, counter=first)[0] != "ctr.striped"
    for m in (n, n - 4096):
        _ccm_counter_case(orc, bits, nonce, m, (bits, len(nonce), m), expect[m])


@pytest.mark.parametrize("bits", [128, 256])
def test_ccm_counter_bits_40_to_47_move_inside_the_text(orc, bits):
    """13-byte nonce ending in ff ff ff: counter bits 40..47 (a nonce byte) move at block 65 535.  At the first size
    the CTR planner gives ctr.striped, that text cannot be one striped launch (two launches), and one group of 256
    counters below that size it is not striped at all."""
    nonce = NONCE13[:10] + b"\xff" * 3
    assert int.from_bytes(_ccm_blocks(nonce)[1][11:], "big") + 65535 == 1 << 40 and 65535 * 16 < _striped_size() - 4096
    _ccm_counter_sizes(orc, bits, nonce, 2)


@pytest.mark.parametrize("bits", [128, 256])
def test_ccm_12_byte_nonce_keeps_one_striped_launch(orc, bits):
    """With a 12-byte nonce the three low counter bytes start at zero: bits 40..47 would move after 2^24 blocks
    (256 MiB, a serial CBC-MAC of seconds) and the CCM calls take no start counter.  The same two sizes run with ff ff
    at the nonce's end and the planner is asserted to keep one launch."""
    nonce = NONCE13[:10] + b"\xff" * 2
    assert int.from_bytes(_ccm_blocks(nonce)[1][11:], "big") + _striped_size() // 16 < 1 << 40
    _ccm_counter_sizes(orc, bits, nonce, 1)


@pytest.mark.parametrize("bits", [128, 256])
def test_ctr_at_the_counter_a_12_byte_ccm_nonce_reaches_after_2_to_24_blocks(orc, bits):
    """the keystream a CCM text under that 12-byte nonce would have from block 2^24 - 65 535 on, where counter bits
    40..47 do move, through the CTR call at that counter (without the MAC): ctr.striped in two launches"""
    n = _striped_size()
    iv, key, pt = _ccm_blocks(NONCE13[:10] + b"\xff" * 2)[0], KEYS[bits], _stream(orc, n, 31)
    off = (1 << 24) - 65535
    at = iv[:9] + ((int.from_bytes(iv[9:], "big") + off) & ((1 << 56) - 1)).to_bytes(7, "big")
    assert int.from_bytes(at[11:], "big") + 65535 == 1 << 40
    assert uaes.plan("ctr", n, counter=at)[:2] == ("ctr.striped", 2), uaes.plan("ctr", n, counter=at)
    pl = Place(pt, n)
    assert uaes.engine().uaes_ctr_xcrypt_at(bits, key, iv, off, pl.pin, n, pl.pout) == 0
    got, intact = pl.result()
    assert got == orc.ctr_xcrypt_at(key, iv, off, pt) and intact, (bits, "keystream from block 2^24 - 65535")


# ---------------------------------------------------------------------------------------------------------------------
# f. batches of chains (k_chain_batch_row, k_chain_batch)
# ---------------------------------------------------------------------------------------------------------------------
BATCH_CAP = 16 * MIB
SMALL_COUNTS = [1, 15, 16, 17, 63, 64, 65]
CHECK_ALL = 20000                                # up to here the oracle checks every message
BATCH_PLACES = [("host", 0, False, False), ("dev", 0, False, True), ("dev-odd", 1, False, True), ("dev-inplace", 0, True, True)]


def _batch_counts():
    """1 .. 65 and both sides of every change the hook reports (workgroup shape, first strided count, row -> lane)"""
    marks = K.batch_marks()
    assert [m[1].split(" -> ")[1] for m in marks[:4]] == ["batch.row/256 strided", "batch.row/1024", "batch.row/1024 strided",
                                                          "batch.lane/1024"], marks
    return SMALL_COUNTS + [k + d for k, _ in marks for d in (-1, 0)]


_BATCH_WANT = {}


def _batch_want(orc, what, bits, nmsg, size, idx):
    """{message index: the oracle's CBC-CS3 ciphertext / CMAC of that message alone}, kept for every placement"""
    have = _BATCH_WANT.setdefault((what, bits, nmsg, size), {})
    key, data, ivs = KEYS[bits], _stream(orc, nmsg * size, 37), _stream(orc, nmsg * 16, 41)
    for i in idx:
        if i not in have:
            m = data[i * size:(i + 1) * size]
            have[i] = orc.cbc(key, ivs[16 * i:16 * i + 16], m, True)[1] if what == "cbc_batch" else orc.cmac(key, m)
    return have


def _batch_run(orc, what, bits, nmsg, size, off, inplace, dev, iv_dev=False):
    L, key = uaes.engine(), KEYS[bits]
    data = _stream(orc, nmsg * size, 37)
    if what == "cbc_batch":
        pl = Place(data, nmsg * size, off, off, inplace, dev)
        ivs = _stream(orc, nmsg * 16, 41)
        ivp = Place(ivs, 0) if iv_dev else None
        rc = L.uaes_cbc_encrypt_batch(bits, key, ivp.pin if iv_dev else ivs, nmsg, size, pl.pin, pl.pout)
        assert ivp is None or ivp.input_intact()
    else:
        pl = Place(data, nmsg * 16, off, off, False, dev)
        rc = L.uaes_cmac_batch(bits, key, nmsg, size, pl.pin, pl.pout)
    assert rc == 0, (what, bits, nmsg, size, off, inplace, dev)
    got, intact = pl.result()
    assert intact and pl.input_intact(), (what, bits, nmsg, size, off, inplace, dev, "guard bytes")
    return got


def _batch_case(orc, what, bits, nmsg, size, places=BATCH_PLACES):
    plan = uaes.chain_plan(what, size, nmsg)
    idx = range(nmsg) if nmsg <= CHECK_ALL else K.batch_samples(nmsg, plan)
    want = _batch_want(orc, what, bits, nmsg, size, idx)
    osz = size if what == "cbc_batch" else 16
    for name, off, inplace, dev in places:
        if inplace and what != "cbc_batch":
            continue
        got = _batch_run(orc, what, bits, nmsg, size, off, inplace, dev, iv_dev=dev and off == 0)
        if nmsg <= CHECK_ALL:
            assert got == b"".join(want[i] for i in range(nmsg)), (what, bits, nmsg, size, name, plan)
        else:
            for i in idx:
                assert got[i * osz:(i + 1) * osz] == want[i], (what, bits, nmsg, size, name, plan, i)
    return plan


@pytest.mark.parametrize("size", [16, 32, 48, 80, 96, 112, 144, 160])
def test_cbc_batch_counts_and_placements(orc, size):
    """1, 2, 3, 5, 6, 7, 9 and 10 blocks per message (the lane kernel's groups of four start at 6) at every count, in
    host memory, device memory (aligned, with device IVs; at an odd offset) and in place"""
    seen = set()
    for nmsg in _batch_counts():
        if nmsg * size <= BATCH_CAP:
            plan = _batch_case(orc, "cbc_batch", 128, nmsg, size)
            seen.add(plan[0])
    assert seen == {"batch.row", "batch.lane"}


CMAC_SIZES = [33, 63, 64, 65, 79, 80, 81, 128, 4101]          # (33: short enough for the lane kernel's strided counts)


@pytest.mark.parametrize("size", CMAC_SIZES)
def test_cmac_batch_counts_and_placements(orc, size):
    """3, 4 and 5 whole blocks in front of the last one (the lane kernel's groups of four start at 4, and only for a
    16-byte aligned message), sizes that are no multiple of 4 (the row kernel's A4 = false) and 4101 bytes"""
    ran = 0
    for nmsg in _batch_counts():
        if nmsg * size <= BATCH_CAP:
            _batch_case(orc, "cmac_batch", 128, nmsg, size)
            ran += 1
    assert ran >= len(SMALL_COUNTS)


@pytest.mark.parametrize("lane", [False, True], ids=["65", "lane"])
def test_cmac_batch_every_short_message(orc, lane):
    """messages of 0..40 bytes at 65 messages and at the first count of the lane kernel: host, device aligned, device odd"""
    nmsg = [k for k, what in K.batch_marks() if "-> batch.lane/" in what and "batch.row" in what][0] if lane else 65
    assert uaes.chain_plan("cmac_batch", 16, nmsg)[0] == ("batch.lane" if lane else "batch.row")
    for size in range(41):
        _batch_case(orc, "cmac_batch", 128, nmsg, size, BATCH_PLACES[:3])


@pytest.mark.parametrize("what,size", [("cbc_batch", 16), ("cbc_batch", 96), ("cbc_batch", 144), ("cmac_batch", 5), ("cmac_batch", 64),
                                       ("cmac_batch", 81)])
def test_batch_row_form_equals_lane_form(orc, what, size):
    """the last count of the row kernel and the first of the lane kernel, same messages: the two outputs agree on all
    of the row form's messages"""
    lane = [k for k, w in K.batch_marks() if "-> batch.lane/" in w and "batch.row" in w][0]
    assert uaes.chain_plan(what, size, lane - 1)[0] == "batch.row" and uaes.chain_plan(what, size, lane)[0] == "batch.lane"
    osz = size if what == "cbc_batch" else 16
    for off in (0, 1):
        row = _batch_run(orc, what, 128, lane - 1, size, off, False, True)
        ln = _batch_run(orc, what, 128, lane, size, off, False, True)
        assert row == ln[:(lane - 1) * osz], (what, size, off)


@pytest.mark.parametrize("bits", [192, 256])
def test_batch_key_sizes(orc, bits):
    lane = [k for k, w in K.batch_marks() if "-> batch.lane/" in w and "batch.row" in w][0]
    for nmsg in (65, lane):
        _batch_case(orc, "cbc_batch", bits, nmsg, 112, BATCH_PLACES[1:2])
        _batch_case(orc, "cmac_batch", bits, nmsg, 81, BATCH_PLACES[1:2])


def test_cbc_batch_device_ivs_must_be_aligned(orc):
    """a device IV array works when it is 16-byte aligned (checked in every aligned device placement above) and is
    refused with UAES_E_ARG otherwise, nothing written"""
    L, nmsg, size = uaes.engine(), 17, 48
    data, ivs = _stream(orc, nmsg * size, 37), _stream(orc, nmsg * 16, 41)
    for off in (1, 4, 8):
        pl, ivp = Place(data, nmsg * size), Place(ivs, 0, off_in=off)
        assert L.uaes_cbc_encrypt_batch(128, KEYS[128], ivp.pin, nmsg, size, pl.pin, pl.pout) == E_ARG, off
        got, intact = pl.result()
        assert got == bytes([G]) * (nmsg * size) and intact and pl.input_intact(), off
