"""OCB (RFC 7253) in pieces, plain Python / numpy over the oracle's block cipher (oracle/pyoracle.py: encrypt_block,
ecb_encrypt, ecb_decrypt).  Shared by tests/test_ocb_ref_host.py, which proves it against the RFC's vectors, the oracle's
own OCB and the RFC's chained offsets, and tests/test_gpu_ocb.py, which holds k_ocb against it at the sizes the oracle
cannot reach in seconds.

    Ocb(orc, key)       L_*, L_$, L_j; offset0(nonce, tag_len); hash_aad; encrypt / decrypt for a nonce of 1..15 bytes
                        and a tag of 1..16 -- offsets chained as the RFC defines them, Offset_i = Offset_{i-1} ^ L_ntz(i)
    offsets             the same offsets NOT chained: Offset_i = Offset_0 ^ XOR{ L_j : bit j of i ^ (i >> 1) } for a
                        range of indices at once, as pairs of int64 -- numpy arrays, or torch tensors on a device
    text_by_blocks      C_i = ECB_K(P_i ^ Offset_i) ^ Offset_i for a slice of whole blocks, with the XOR-fold of the
                        plaintext (the checksum); with Offset_0 = 0 and hash=True the fold of the cipher's outputs,
                        HASH(K, A) over whole blocks
    Ocb.finish          the ragged block and the tag from a folded checksum; Ocb.aad_tail: HASH's ragged-block term

A block is 16 bytes; where it is a pair of int64 the two are its bytes 0..7 and 8..15 read in the machine's byte order
(XOR does not care, and both the data and the L_j are read the same way)."""
import numpy as np

ZERO = bytes(16)


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def dbl(b):
    """double(S) of RFC 7253 section 2: the block as a big-endian number, << 1, ^ 0x87 on a carry"""
    v = int.from_bytes(b, "big") << 1
    if v >> 128:
        v = (v ^ 0x87) & ((1 << 128) - 1)
    return v.to_bytes(16, "big")


def ntz(i):
    return (i & -i).bit_length() - 1


def _xor_buffers(a, b):
    return (int.from_bytes(a, "big") ^ int.from_bytes(b, "big")).to_bytes(len(a), "big") if a else b""


class Ocb:
    """the key-dependent pieces (RFC 7253 section 4.1) and the calls built from them"""

    def __init__(self, orc, key):
        self.orc, self.key = orc, bytes(key)
        self.l_star = self.enc(ZERO)
        self.l_dollar = dbl(self.l_star)
        self._l = [dbl(self.l_dollar)]

    def enc(self, block):
        return self.orc.encrypt_block(self.key, block)

    def ecb(self, data, decrypt=False):
        """whole blocks through the oracle's ECB"""
        assert len(data) % 16 == 0
        if not data:
            return b""
        if decrypt:
            rc, out = self.orc.ecb_decrypt(self.key, data)
            assert rc == 0
            return out
        return self.orc.ecb_encrypt(self.key, data)

    def L(self, j):
        while len(self._l) <= j:
            self._l.append(dbl(self._l[-1]))
        return self._l[j]

    def offset0(self, nonce, tag_len=16):
        """Offset_0 of section 4.2: Nonce = num2str(TAGLEN mod 128, 7) || 0.. || 1 || N, bottom = its last six bits,
        Ktop = ENCIPHER(K, Nonce with those bits cleared), Stretch = Ktop || (Ktop[1..64] ^ Ktop[9..72])"""
        assert 1 <= len(nonce) <= 15 and 1 <= tag_len <= 16
        n = bytearray(16 - len(nonce)) + bytearray(nonce)
        n[0] |= ((tag_len * 8) % 128) << 1
        n[15 - len(nonce)] |= 1
        bottom = n[15] & 63
        n[15] &= 0xC0
        ktop = self.enc(bytes(n))
        stretch = int.from_bytes(ktop + xor(ktop[:8], ktop[1:9]), "big")
        return ((stretch >> (64 - bottom)) & ((1 << 128) - 1)).to_bytes(16, "big")

    def chained(self, off0, count):
        """Offset_1 .. Offset_count by the RFC's recurrence, back to back"""
        off, out = off0, bytearray()
        for i in range(1, count + 1):
            off = xor(off, self.L(ntz(i)))
            out += off
        return bytes(out)

    def delta(self, i):
        """Offset_i ^ Offset_0 without the chain: the L_j of the set bits of i ^ (i >> 1)"""
        g, d, j = i ^ (i >> 1), ZERO, 0
        while g:
            if g & 1:
                d = xor(d, self.L(j))
            g, j = g >> 1, j + 1
        return d

    def aad_tail(self, m, tail):
        """HASH's term for the ragged block behind m whole blocks: ENCIPHER(K, (A_* || 1 || 0..) ^ Offset_m ^ L_*)"""
        if not tail:
            return ZERO
        assert len(tail) < 16
        return self.enc(xor(xor((bytes(tail) + b"\x80").ljust(16, b"\0"), self.delta(m)), self.l_star))

    def hash_aad(self, aad):
        """HASH(K, A) of section 4.1, offsets chained from zero"""
        m = len(aad) // 16
        offs = self.chained(ZERO, m)
        out = self.ecb(_xor_buffers(aad[:16 * m], offs))
        s = ZERO
        for i in range(m):
            s = xor(s, out[16 * i:16 * i + 16])
        assert (offs[-16:] if m else ZERO) == self.delta(m)
        return xor(s, self.aad_tail(m, aad[16 * m:]))

    def finish(self, off0, m, checksum, tail, hashed=ZERO, decrypt=False):
        """behind m whole blocks whose plaintext folds to `checksum`: the ragged block `tail` (plaintext, or ciphertext
        with decrypt) and the tag.  Returns (the other form of the tail, the 16-byte tag)."""
        off = xor(off0, self.delta(m))
        other = b""
        if tail:
            off = xor(off, self.l_star)
            pad = self.enc(off)
            other = xor(tail, pad)
            checksum = xor(checksum, ((other if decrypt else bytes(tail)) + b"\x80").ljust(16, b"\0"))
        return other, xor(self.enc(xor(xor(checksum, off), self.l_dollar)), hashed)

    def _text(self, off0, data, decrypt):
        """whole blocks with chained offsets: (output, checksum of the plaintext)"""
        m = len(data) // 16
        offs = self.chained(off0, m)
        out = _xor_buffers(self.ecb(_xor_buffers(data, offs), decrypt), offs)
        pt, s = (out if decrypt else data), ZERO
        for i in range(m):
            s = xor(s, pt[16 * i:16 * i + 16])
        return out, s

    def encrypt(self, nonce, aad, pt, tag_len=16):
        """ciphertext || tag[:tag_len]"""
        pt, m = bytes(pt), len(pt) // 16
        off0 = self.offset0(nonce, tag_len)
        ct, s = self._text(off0, pt[:16 * m], False)
        tail, tag = self.finish(off0, m, s, pt[16 * m:], self.hash_aad(bytes(aad)))
        return ct + tail + tag[:tag_len]

    def decrypt(self, nonce, aad, ct_and_tag, tag_len=16):
        """(0 or 0x1A, the text -- written either way, as the reference does)"""
        ct = bytes(ct_and_tag[:len(ct_and_tag) - tag_len])
        m = len(ct) // 16
        off0 = self.offset0(nonce, tag_len)
        pt, s = self._text(off0, ct[:16 * m], True)
        tail, tag = self.finish(off0, m, s, ct[16 * m:], self.hash_aad(bytes(aad)), decrypt=True)
        return (0 if tag[:tag_len] == bytes(ct_and_tag[len(ct):]) else 0x1A), pt + tail


# ---- the offsets of many blocks at once, numpy or torch ------------------------------------------------------------
def pair(block):
    """a 16-byte block as two Python ints that fit int64: its halves in the machine's byte order"""
    a = np.frombuffer(bytes(block), dtype=np.int64)
    return int(a[0]), int(a[1])


def unpair(hi, lo):
    return np.array([hi, lo], dtype=np.int64).tobytes()


def _arange(xp, lo, hi, like):
    if xp is np:
        return np.arange(lo, hi, dtype=np.int64)
    return xp.arange(lo, hi, dtype=xp.int64, device=like.device)


def offsets(ocb, off0, first, count, xp=np, like=None):
    """Offset_i for i = first + 1 .. first + count, not chained: (hi, lo), two int64 arrays of `count` elements.
    xp = numpy, or torch with `like` a tensor on the device the offsets are wanted on."""
    i = _arange(xp, first + 1, first + count + 1, like)
    g = i ^ (i >> 1)
    h0, l0 = pair(off0)
    hi, lo = xp.zeros_like(i) + h0, xp.zeros_like(i) + l0
    for j in range((first + count).bit_length()):
        lh, ll = pair(ocb.L(j))
        mask = -((g >> j) & 1)                          # all ones where bit j of gray(i) is set
        hi ^= mask & lh
        lo ^= mask & ll
    return hi, lo


def fold(blocks):
    """XOR of the rows of an (n, 2) int64 array (numpy or torch): 16 bytes"""
    x = blocks
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        y = x[:h] ^ x[h:2 * h]
        if x.shape[0] & 1:
            y[0] ^= x[2 * h]
        x = y
    return unpair(int(x[0, 0]), int(x[0, 1])) if x.shape[0] else ZERO


def text_by_blocks(ocb, off0, first, data, ecb, xp=np, hash=False):
    """The whole blocks first + 1 .. first + n of a text, n = len(data) / 16.  data: a contiguous uint8 array (numpy)
    or tensor (torch); ecb: whole blocks in such an array -> their ECB encryption in a new one.
    Returns (C, checksum): C_i = ECB_K(P_i ^ Offset_i) ^ Offset_i and the XOR of the P_i.  With hash=True (and
    off0 = ZERO) returns (None, XOR of the ECB_K(A_i ^ Offset_i)): this slice's share of HASH(K, A)."""
    n = data.shape[0] // 16
    assert data.shape[0] == 16 * n
    if not n:
        return data[:0], ZERO
    p = data.view(xp.int64).reshape(n, 2)
    hi, lo = offsets(ocb, off0, first, n, xp, data)
    w = xp.empty_like(p)
    w[:, 0] = p[:, 0] ^ hi
    w[:, 1] = p[:, 1] ^ lo
    e = ecb(w.reshape(-1).view(xp.uint8)).view(xp.int64).reshape(n, 2)
    if hash:
        return None, fold(e)
    e[:, 0] ^= hi
    e[:, 1] ^= lo
    return e.reshape(-1).view(xp.uint8), fold(p)


def numpy_ecb(ocb):
    """the `ecb` of text_by_blocks over the oracle"""
    return lambda a: np.frombuffer(bytearray(ocb.ecb(a.tobytes())), dtype=np.uint8)
