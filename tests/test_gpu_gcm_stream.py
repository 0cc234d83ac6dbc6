"""Streamed GCM (uaes_gcm_stream_begin / _update / _finish) at every piece arrangement, position and table state.

The cases are made by tests/gcm_stream_cases.py from uaes.plan_gcm_piece (the function uaesk_gcm_stream_piece switches
on) and tests/counters.py stripe_geometry; tests/test_gcm_stream_cases.py proves without a device that they cover what
they claim.  Every case runs in both directions: the stream's bytes and tag against the oracle's answer for the case's
message (orc.gcm_encrypt once per message; the tag of a prefix from orc.ghash by GCM's definition), the decrypting
stream back to the text with the tag accepted, and after every piece GcmStream.tables() against the cache word the
case file restates.  Groups B and C are also held against uaes.AES_GCM_encrypt of the same bytes; the first case of every
item decrypts once more with a forged tag.  A: every boundary of the piece planner; B: the striped piece at its
smallest; C: table-cache transitions; D: host, device and in-place buffers; E: streams side by side and on a recycled
scratch; F: past the oracle (the striped piece the table picks by itself, and the B table twice)."""
import pytest

import micro_aes_amd as uaes
from tests import gcm_stream_cases as G

pytestmark = pytest.mark.gpu

LOOK_DEFAULT = 100000
GUARD = 32
_REFS, _ONE_SHOT = {}, {}


def ref(orc, name):
    if name not in _REFS:
        _REFS[name] = G.Reference(orc, G.messages()[name])
    return _REFS[name]


def one_shot(r, n):
    """uaes.AES_GCM_encrypt of the message's first n bytes, once"""
    if (r.m.name, n) not in _ONE_SHOT:
        _ONE_SHOT[(r.m.name, n)] = uaes.AES_GCM_encrypt(r.key, r.nonce, r.aad, r.text[:n])
    return _ONE_SHOT[(r.m.name, n)]


class Feeder:
    """one stream of a case: pieces in, bytes out, tables() after every step"""

    def __init__(self, c, r, decrypt):
        import torch
        self.c, self.n, self.off = c, sum(c.pieces), 0
        self.src = (r.ct if decrypt else r.text)[:self.n]
        self.st = uaes.GcmStream(r.key, r.nonce, r.aad, decrypt=decrypt)
        self.seq = [self.st.tables()]
        self.out = bytearray()
        if c.place != "host":
            # the source 16 bytes into its allocation; a buffer of its own for the output, or none
            self.alloc = torch.empty(16 + self.n + GUARD, dtype=torch.uint8, device="cuda:0")
            self.alloc[16 + self.n:] = 0xCC
            self.d_src = self.alloc[16:16 + self.n]
            self.d_src.copy_(torch.frombuffer(bytearray(self.src), dtype=torch.uint8))
            self.d_all = self.alloc[16:] if c.place == "inplace" else torch.full((self.n + GUARD,), 0xCC, dtype=torch.uint8, device="cuda:0")
            self.d_dst = self.d_all[:self.n]

    def step(self, k):
        p = self.c.pieces[k]
        if self.c.place == "host":
            self.out += self.st.update(self.src[self.off:self.off + p])
        else:
            self.st.update_dev(self.d_src.data_ptr() + self.off, p, self.d_dst.data_ptr() + self.off)
        self.off += p
        self.seq.append(self.st.tables())

    def finish(self, tag=None):
        res = self.st.finish(tag)
        if self.c.place != "host":
            self.out = self.d_dst.cpu().numpy().tobytes()
            assert self.d_all[self.n:].cpu().numpy().tobytes() == b"\xCC" * GUARD, "a write behind the piece"
        return bytes(self.out), res


def feed(c, r, decrypt, tag=None):
    L = uaes.engine()
    try:
        L.uaes_debug_plan_disable(c.mask)
        L.uaes_debug_gcm_look(0 if c.look == 0 else LOOK_DEFAULT)
        f = Feeder(c, r, decrypt)
        for k in range(len(c.pieces)):
            f.step(k)
        out, res = f.finish(tag)
    finally:
        L.uaes_debug_plan_disable(0)
        L.uaes_debug_gcm_look(LOOK_DEFAULT)
    return out, res, f.seq


def flipped(tag):
    return bytes([tag[0] ^ 1]) + tag[1:]


def check(orc, c, forge=False):
    r = ref(orc, c.msg)
    n = sum(c.pieces)
    want_ct, want_tag = r.ct[:n], r.prefix_tag(n)
    what = (c.group, c.msg, c.pieces, hex(c.mask), c.place, c.look, c.note)
    out, tag, seq = feed(c, r, False)
    assert out == want_ct, what
    assert tag == want_tag, what
    assert seq == G.simulate(c)[0], (what, seq)
    back, rc, seq = feed(c, r, True, want_tag)
    assert rc == 0 and back == r.text[:n], what
    assert seq == G.simulate(c, True)[0], (what, seq)
    if c.group in "BC" and r.m.oracle:              # (a message past the oracle's cap already has the one-shot call as its reference)
        assert one_shot(r, n) == want_ct + want_tag, what
    if forge:
        assert feed(c, r, True, flipped(want_tag))[1] == 0x1A, what


@pytest.mark.parametrize("item", list(G.items()))
def test_gcm_stream_cases(orc, item):
    """groups A to D and the single streams of E, an item at a time (tests/gcm_stream_cases.py: items)"""
    for k, c in enumerate(G.items()[item]):
        check(orc, c, forge=k == 0)


def test_two_streams_side_by_side(orc):
    """E: two streams under different keys, one encrypting and one decrypting, advanced in turn from one thread through
    d, c1, d, c2 pieces and what is left: each has its own scratch, running value, counter position and done word"""
    ca, cb = [c for c in G.group_e() if c.note == "side by side"]
    ra, rb = ref(orc, ca.msg), ref(orc, cb.msg)
    assert ra.key != rb.key and len(ca.pieces) == len(cb.pieces) and G.kinds(ca)[:4] == ["d", "c1", "d", "c2"] == G.kinds(cb, True)[:4]
    L = uaes.engine()
    try:
        L.uaes_debug_gcm_look(LOOK_DEFAULT)
        fa, fb = Feeder(ca, ra, False), Feeder(cb, rb, True)
        for k in range(len(ca.pieces)):
            fa.step(k)
            fb.step(k)
        back, rc = fb.finish(rb.tag)
        out, tag = fa.finish()
    finally:
        L.uaes_debug_gcm_look(LOOK_DEFAULT)
    assert out == ra.ct and tag == ra.tag
    assert rc == 0 and back == rb.text
    assert fa.seq == G.simulate(ca)[0] and fb.seq == G.simulate(cb, True)[0]
    fb = Feeder(cb, rb, True)
    fa = Feeder(ca, ra, False)
    for k in range(len(ca.pieces)):
        fb.step(k)
        fa.step(k)
    assert fa.finish() == (ra.ct, ra.tag)
    assert fb.finish(flipped(rb.tag))[1] == 0x1A


def test_a_stream_on_a_recycled_scratch(orc):
    """E: one stream after another.  A stream that built striped tables and a bulk table is finished: finish() wipes its
    scratch and keeps it for the next begin.  The streams that follow, under other keys -- one right after it, one after
    a stream aborted behind a chunk piece (abort frees its scratch, so that one takes a kept scratch if there is one,
    else a new one) -- give the oracle's bytes and tag, and tables() read from the new stream right after begin is what
    that begin's own absorb set up: nothing of an earlier stream's cache word (check() compares every step).  Whether a
    begin took a kept scratch or a fresh one cannot be seen from outside; the test runs the sequence in which it does."""
    full = [c for c in G.group_e() if c.note.startswith("leaves")][0]
    after = [c for c in G.group_e() if c.note == "on a recycled scratch"]
    r = ref(orc, full.msg)
    out, tag, seq = feed(full, r, False)
    assert (out, tag) == (r.ct, r.tag) and seq == G.simulate(full)[0]
    assert seq[-1][3] and any(s[1] for s in seq), seq               # the scratch it gives back held both
    check(orc, after[0])
    c = after[1]
    r8 = ref(orc, "m8")
    st = uaes.GcmStream(r8.key, r8.nonce, r8.aad)
    assert G.kinds(c)[1] == "c1"
    got = st.update(r8.text[:c.pieces[0]]) + st.update(r8.text[c.pieces[0]:c.pieces[0] + c.pieces[1]])
    assert got == r8.ct[:c.pieces[0] + c.pieces[1]]
    st.abort()
    check(orc, c, forge=True)


def _dev_stream(key, nonce, pieces, mask, src, dst, decrypt, tag=None):
    L = uaes.engine()
    try:
        L.uaes_debug_plan_disable(mask)
        st = uaes.GcmStream(key, nonce, b"", decrypt=decrypt)
        seq, off = [st.tables()], 0
        for p in pieces:
            st.update_dev(src.data_ptr() + off, p, dst.data_ptr() + off)
            off += p
            seq.append(st.tables())
        return st.finish(tag), seq
    finally:
        L.uaes_debug_plan_disable(0)


@pytest.mark.parametrize("which", [0, 1])
def test_past_the_oracle(orc, which):
    """F: a message made on the device.
    0: [128 MiB + a stripe, a block, 128 MiB + a stripe, two blocks] with no mask.  Both long pieces are the striped
    arrangement by the table, and the counter position crosses 2^23 blocks inside the first and 2^24 inside the second.
    1: two absorbs of 32 MiB + 16 under a mask that leaves only the absorb path: the second reuses logA = 16 and the B
    table.
    Text and tag against uaes.gcm_encrypt_dev over the same buffer (an independent planner path, pinned to the
    reference's digest by the C4 test), the first 64 KiB against the oracle; then decrypted by a stream in place, and
    a tag with one bit flipped returns 0x1A."""
    import torch
    pieces, mask = G.group_f()[which]
    n = sum(pieces)
    key, nonce = bytes(range(0x40, 0x50)), bytes(range(0x70, 0x7C))
    want_seq, events = G.simulate_pieces(0, pieces, mask)
    if which == 0:
        for k in (0, 2):
            for dec in (False, True):
                assert uaes.plan_gcm_piece(pieces[k], sum(pieces[:k]), dec)[0] == "gcm.striped"
        assert 2 < (1 << 23) < 2 + pieces[0] // 16 and 2 + sum(pieces[:2]) // 16 < (1 << 24) < 2 + sum(pieces[:3]) // 16
    else:
        assert G.kinds(G.Case("F", None, pieces, mask, "dev", None, "")) == ["a16", "d", "a16", "d"]
        assert [e for e in events if e[0] == "B"] == [("B", "rebuilt"), ("B", "reused")]
    torch.manual_seed(77 + which)
    src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0")
    want = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
    uaes.gcm_encrypt_dev(key, nonce, None, src, n, want)
    torch.cuda.synchronize()
    head = src[:G.HEAD].cpu().numpy().tobytes()
    assert want[:G.HEAD].cpu().numpy().tobytes() == orc.gcm_encrypt(key, nonce, b"", head)[:G.HEAD]
    want_tag = want[n:].cpu().numpy().tobytes()
    work = torch.full((n + GUARD,), 0xCC, dtype=torch.uint8, device="cuda:0")
    tag, seq = _dev_stream(key, nonce, pieces, mask, src, work, False)
    assert tag == want_tag and torch.equal(work[:n], want[:n]) and seq == want_seq, seq
    assert bool((work[n:] == 0xCC).all())
    rc, seq = _dev_stream(key, nonce, pieces, mask, work, work, True, want_tag)          # in place
    assert rc == 0 and torch.equal(work[:n], src) and seq == want_seq, seq
    assert bool((work[n:] == 0xCC).all())
    work[:n].copy_(want[:n])
    rc, _seq = _dev_stream(key, nonce, pieces, mask, work, work, True, flipped(want_tag))
    assert rc == 0x1A
