"""Counter-solving helpers: inputs whose keystream starts at a CHOSEN counter (a plain module, like tests/rsp.py).

Every GCM kernel builds its keystream from the 56-bit big-endian counter in bytes 9..15 of J0 (+ 1, N4); where a
text's groups of 256 counters, its stripes and its head blocks fall depends on the low byte of the first counter.
A 12-byte nonce always gives J0 = nonce || 00000001, so the one-shot calls only reach other counters through a nonce
of another length, whose J0 = GHASH_H(nonce) (H = E_K(0)).  GHASH is linear in each nonce block, so any J0 can be
reached by choosing the other blocks and solving one.  GCM-SIV's counter is the tag (byte 15 |= 0x80, a little-endian
32-bit word in bytes 0..3): its POLYVAL input is solved the same way for a tag whose low word is chosen.

Built on the C oracle (oracle/pyoracle.py) only: orc.gf128_mul (GCM's bit order; 0x80 00.. is 1), orc.ghash,
orc.encrypt_block.
"""
import random

ONE = bytes([0x80]) + bytes(15)          # 1 in GCM's bit order
X = bytes([0x40]) + bytes(15)            # the element x
MASK56 = (1 << 56) - 1


def xor(a, b):
    return bytes(p ^ q for p, q in zip(a, b))


def gf_pow(orc, h, e):
    """h^e by square and multiply"""
    r, s = ONE, h
    while e:
        if e & 1:
            r = orc.gf128_mul(r, s)
        s = orc.gf128_mul(s, s)
        e >>= 1
    return r


def gf_inv(orc, h):
    """h^-1 = h^(2^128 - 2)"""
    return gf_pow(orc, h, (1 << 128) - 2)


def gcm_h(orc, key):
    return orc.encrypt_block(key, bytes(16))


def j0_bytes(prefix9, v):
    """J0 = 9 fixed bytes || the 56-bit counter v (big-endian)"""
    assert len(prefix9) == 9 and 0 <= v <= MASK56
    return bytes(prefix9) + v.to_bytes(7, "big")


def j0_counter(j0):
    return int.from_bytes(j0[9:], "big")


def gcm_nonce_for_j0(orc, key, j0, nonce_len, seed=0, solve_at=None):
    """a nonce of nonce_len >= 16 bytes with GHASH_H(nonce) == j0.  The blocks other than block `solve_at` (default:
    the last whole one) are random; J0 = XOR_i X_i * H^(m-i+1) ^ L * H over the m = ceil(len/16) nonce blocks X_i
    and the length block L, so X_solve = (j0 ^ J0 with X_solve = 0) * H^-(m - solve_at + 1)."""
    assert nonce_len >= 16 and len(j0) == 16
    rnd = random.Random((seed, nonce_len, j0).__repr__())
    m = (nonce_len + 15) // 16
    t = nonce_len // 16 - 1 if solve_at is None else solve_at
    assert 0 <= t and 16 * (t + 1) <= nonce_len
    nonce = bytearray(rnd.randbytes(nonce_len))
    nonce[16 * t:16 * t + 16] = bytes(16)
    H = gcm_h(orc, key)
    rest = orc.ghash(H, b"", bytes(nonce))
    nonce[16 * t:16 * t + 16] = orc.gf128_mul(xor(j0, rest), gf_inv(orc, gf_pow(orc, H, m - t + 1)))
    nonce = bytes(nonce)
    assert orc.ghash(H, b"", nonce) == bytes(j0), "J0 solver self-check"
    return nonce


def gcm_expect(orc, key, j0, aad, pt, tag_len=16):
    """GCM by its definition at a given J0: CTR from J0 + 1 (56-bit, bytes 9..15), tag = E(J0) ^ GHASH(aad, ct).
    The same as orc.gcm_encrypt for a nonce with that J0 (tests/test_counter_helpers.py), and about twice as fast."""
    ct = orc.ctr_xcrypt_at(key, j0, 1, pt)
    tag = xor(orc.encrypt_block(key, j0), orc.ghash(gcm_h(orc, key), aad, ct))
    return ct + tag[:tag_len]


# ---- GCM-SIV (RFC 8452) -------------------------------------------------------------------------------------------
def siv_keys(orc, key, nonce):
    """(message-authentication key, message-encryption key), RFC 8452 section 4: the first 8 bytes of
    E_K(LE32(i) || nonce) for i = 0, 1 and for the len(key) / 8 blocks after them"""
    blocks = [orc.encrypt_block(key, i.to_bytes(4, "little") + bytes(nonce))[:8] for i in range(2 + len(key) // 8)]
    return b"".join(blocks[:2]), b"".join(blocks[2:])


def _rev_blocks(data):
    """every 16-byte block byte-reversed (POLYVAL's order <-> GHASH's, RFC 8452 appendix A)"""
    import numpy as np
    a = np.frombuffer(bytes(data), dtype=np.uint8).reshape(-1, 16)
    return a[:, ::-1].tobytes()


def _pad16(b):
    return bytes(b) + bytes(-len(b) % 16)


def polyval(orc, h, data):
    """POLYVAL_h over whole blocks: ByteReverse(GHASH(mulX_GHASH(ByteReverse(h)), ByteReverse(X_1), ...)) (RFC 8452
    appendix A).  orc.ghash appends its own length block L: its result is (Y ^ L) * Hg, so Y = result * Hg^-1 ^ L."""
    assert len(data) % 16 == 0
    hg = orc.gf128_mul(h[::-1], X)
    g = orc.ghash(hg, b"", _rev_blocks(data))
    lens = bytes(8) + (len(data) * 8).to_bytes(8, "big")
    return xor(orc.gf128_mul(g, gf_inv(orc, hg)), lens)[::-1]


def siv_message_for_counter(orc, key, nonce, aad, nblocks, le32_start, solve_at=None, tail=0, fill="zero", seed=0):
    """a GCM-SIV plaintext of 16 * nblocks + tail bytes whose tag's bytes 0..3 are le32_start (little-endian): the
    keystream of block i then uses the counter word le32_start + i (mod 2^32).  A tag T with that low word and random
    other bytes is drawn until D_encKey(T) has byte 15's top bit clear (the tag is E(S) with S[15] &= 0x7f); S = D(T)
    with bytes 0..11 XOR the nonce is then the POLYVAL value to reach, and the plaintext block `solve_at` (default:
    the middle one) is solved for it: POLYVAL = XOR_j X_j * H'^(m-j+1), H' = H * x^-128.  fill = "zero": every other
    plaintext byte is zero; "random": random bytes.  Returns the plaintext."""
    assert len(nonce) == 12 and nblocks >= 1 and 0 <= tail < 16
    rnd = random.Random(repr((seed, key, nonce, nblocks, tail, le32_start, fill)))
    t = nblocks // 2 if solve_at is None else solve_at
    assert 0 <= t < nblocks
    auth, enc = siv_keys(orc, key, nonce)
    while True:
        T = (le32_start & 0xffffffff).to_bytes(4, "little") + rnd.randbytes(12)
        S = orc.encrypt_block(enc, T, decrypt=True)
        if not S[15] & 0x80:
            break
    target = xor(S, bytes(nonce) + bytes(4))
    n = 16 * nblocks + tail
    pt = bytearray(rnd.randbytes(n) if fill == "random" else bytes(n))
    pt[16 * t:16 * t + 16] = bytes(16)
    lens = (len(aad) * 8).to_bytes(8, "little") + (n * 8).to_bytes(8, "little")
    stream = _pad16(aad) + _pad16(pt) + lens
    m = len(stream) // 16
    j = len(_pad16(aad)) // 16 + t                        # 0-based position of the solved block
    rest = polyval(orc, auth, stream)
    # in GHASH's order the block at 0-based position j carries the weight Hg^(m - j)
    hg = orc.gf128_mul(auth[::-1], X)
    blk = orc.gf128_mul(xor(target, rest)[::-1], gf_inv(orc, gf_pow(orc, hg, m - j)))[::-1]
    pt[16 * t:16 * t + 16] = blk
    pt = bytes(pt)
    assert polyval(orc, auth, _pad16(aad) + _pad16(pt) + lens) == target, "POLYVAL solver self-check"
    return pt


def siv_counter_check(orc, key, nonce, aad, pt, le32_start):
    """the solver's end-to-end self-check: the oracle's tag starts with le32_start"""
    tag = orc.gcmsiv_encrypt(key, nonce, aad, pt)[-16:]
    assert int.from_bytes(tag[:4], "little") == le32_start & 0xffffffff, "GCM-SIV counter self-check"
    return tag


# ---- the named J0 targets ------------------------------------------------------------------------------------------
def v_for_first(c):
    """J0's counter v whose first keystream block uses counter c (v + 1 = c, mod 2^56)"""
    return (c - 1) & MASK56


def v_carry32_at(i, hi=0x5a3c17):
    """v such that block i's counter is hi * 2^32 (bits 0..31 zero: the carry into byte 11 happens at block i);
    hi's low byte must not be 0 (that would move bits 40..47 as well)"""
    assert hi & 0xff
    return ((hi << 32) - 1 - i) & MASK56


def v_bits40_at(i, hi=0x3b):
    """v such that block i's counter is hi * 2^40: counter bits 40..47 move at block i"""
    return ((hi << 40) - 1 - i) & MASK56


def v_wrap56_at(i):
    """v such that block i's counter is 0 after 2^56 - 1: the 56-bit counter wraps at block i"""
    return (-1 - i) & MASK56


def gcm_targets(nfull, rem, cus=None, seed=0):
    """[(name, v, byte 8)]: the J0 counters of the GPU tests for a text of nfull whole blocks and rem tail bytes.
    A carry into byte 11 at block i makes block i a group start (its counter's low byte is 0), so the head is i % 256
    blocks long.  cus = the workgroups of a striped arrangement: the carries then go into its first and last round of
    stripes (of the c0 = 0x80 geometry, stripe_geometry) and the blocks behind the stripes; None = the chunk
    arrangements, whose units are spread evenly over the text."""
    rnd = random.Random(repr((seed, nfull, rem, cus)))
    out = [("c0=00", v_for_first(0x7c00), 0x11), ("c0=01", v_for_first(0x31201), 0x22),
           ("c0=ff", v_for_first(0x5ff), 0x33), ("c0=80", v_for_first(0x180), 0x44)]
    if cus:
        h0, _g_lo, n8, h1 = stripe_geometry(0x80, nfull, cus)
        last_round = h0 + 2048 * cus * ((n8 - 1) // cus)
        spots = [("carry@head", 0), ("carry@first-group", h0), ("carry@first-round", h0 + 2048 * min(n8, cus) - 256 * 3),
                 ("carry@last-round", last_round + 256 * 5), ("carry@tail", h1 + 256)]
    else:
        spots = [("carry@head", 0), ("carry@first-group", 255), ("carry@first-unit", nfull // 16 + 7),
                 ("carry@middle", nfull // 2), ("carry@last-unit", nfull - nfull // 16 - 3), ("carry@tail", nfull - 1)]
    for name, i in spots:
        if 0 <= i < nfull:
            out.append((name, v_carry32_at(i), 0x55))
    if rem:
        out.append(("carry@byte-tail", v_carry32_at(nfull), 0x66))
    out.append(("bits40@middle", v_bits40_at(nfull // 2 + 256), 0x77))
    out.append(("wrap56@middle", v_wrap56_at(nfull // 3), 0xff))
    out.append(("random", rnd.getrandbits(56), rnd.getrandbits(8)))
    return out


def stripe_geometry(c0, nfull, cus):
    """the striped region of a text whose first counter has low byte c0 (gcm_stripes, csrc/uaes_gcm.hip): head h0, first
    group g_lo, stripes n8 (2048 blocks each, dealt round-robin over `cus` workgroups), tail from h1"""
    h0 = (256 - c0) & 255
    g_lo = 1 if c0 else 0
    groups = (c0 + nfull) // 256
    n8 = (groups - g_lo) // 8 if groups > g_lo else 0
    return h0, g_lo, n8, h0 + 2048 * n8
