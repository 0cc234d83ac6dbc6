"""The cases of tests/test_gpu_gcm_stream.py, made without a device, and their reference.

A streamed GCM message (uaes_gcm_stream_begin / _update / _finish) carries state no other mode has: a running GHASH
value stepped by H^m, a counter position, a per-stream table cache (plan_state), a done word and a recycled scratch.
Which kernels a piece runs is decided by uaes.plan_gcm_piece (the function uaesk_gcm_stream_piece switches on), where
its stripes fall by tests/counters.py stripe_geometry; both answer without a device, for a 256-CU MI355X.  Every length
below is derived from those two and from the level rule of plan_for (level_plan, stated once); the one size typed in is
TOP, the 17 MiB at which the walk over the piece planner ends and which the longest message has.
tests/test_gcm_stream_cases.py proves that the lists hold what they claim and that the oracle is handed at most
ITEM_CAP bytes per test item and FILE_CAP bytes in all.

A case is (message, pieces, mask, placement): the message's associated data goes in at begin, the pieces are fed in
order under the plan-disable mask (one mask per stream), from host memory, from device memory into another buffer, or
in place in device memory.  The messages are few and fixed, so one oracle call serves every splitting of a message in
both directions.  A splitting whose last piece has to be ragged at a chosen length cannot also add up to a fixed
message: it covers a PREFIX of its message.  The text of a prefix is the prefix of the oracle's ciphertext (CTR); its
tag is made from the oracle's own primitives by GCM's definition, tag = E(J0) ^ GHASH_H(aad, ct[:n]), with GHASH's
Horner form cut into segments, raw(A || B) = raw(A) * H^blocks(B) ^ raw(B).  A prefix in the front half of its message
is hashed from the front; one in the back half is taken out of the oracle's tag of the whole message, which needs only
the ciphertext behind the prefix.  Either way one pass of orc.ghash serves every prefix on its side (Reference.prefix_tag;
the CPU test holds both ways equal to orc.gcm_encrypt of the prefix)."""
import collections
import contextlib

import micro_aes_amd as uaes
from tests.counters import gcm_h, gf_inv, gf_pow, stripe_geometry, xor
from tests.test_gpu_plan import boundaries

MIB = 1 << 20
ITEM_CAP, FILE_CAP = 40 * MIB, 110 * MIB     # bytes handed to the oracle: per test item, for the whole file
SEG = 1 << 16                                # bytes per segment of the prefix-tag pass
HEAD = 1 << 16                               # what a message past the oracle compares with it
GH_DIRECT, GH_LOGB, GH_MAXLOG = 32768, 14, 18    # csrc/uaes_ghash.hip.h
PLACES = ("host", "dev", "inplace")

Message = collections.namedtuple("Message", "name bits aad_len text_len seed oracle")
Case = collections.namedtuple("Case", "group msg pieces mask place look note")


# ---- the planner, asked under a mask ----------------------------------------------------------------------------------
_BITS = {}


def mask_of(*names):
    m = 0
    for n in names:
        if n not in _BITS:
            _BITS[n] = 1 << uaes.arrangement_id(n)
        m |= _BITS[n]
    return m


@contextlib.contextmanager
def masked(mask):
    """uaes_debug_plan_disable is process-wide: set inside try / finally and put back to 0"""
    L = uaes.engine()
    try:
        L.uaes_debug_plan_disable(mask)
        yield
    finally:
        L.uaes_debug_plan_disable(0)


def piece_plan(mask, n, done=0, decrypt=False):
    with masked(mask):
        return uaes.plan_gcm_piece(n, done, decrypt)


def level_plan(nv):
    """plan_for (csrc/uaes_gcm.hip): (logA, needs the B table) of nv GHASH positions -- no bulk level up to GH_DIRECT
    positions, else the smallest stride 2^lg >= 2^GH_LOGB with 64 << lg >= nv (the loop runs while 64 << lg < nv); the B
    table where a stride is too long for the last kernel alone"""
    if nv <= GH_DIRECT:
        return 0, False
    lg = GH_LOGB
    while lg < GH_MAXLOG and (64 << lg) < nv:
        lg += 1
    return lg, (1 << lg) > GH_DIRECT


def kind_of(mask, n, done=0, decrypt=False):
    """d: absorb, direct; a<logA>: absorb with a bulk level; c<steps>: chunk piece; t: two phases; s: striped"""
    name, _launches, _grid, steps = piece_plan(mask, n, done, decrypt)
    if name == "gcm.levels":
        lg = level_plan((n + 15) // 16)[0]
        return "a%d" % lg if lg else "d"
    return {"gcm.chunks": "c%d" % steps, "gcm.twophase": "t", "gcm.striped": "s"}[name]


def cus():
    """the workgroups of a striped piece: the CU count the planner sizes for"""
    name, _launches, grid, _steps = piece_plan(0, 1 << 30)
    assert name == "gcm.striped"
    return grid


STRIPE = stripe_geometry(0, 1 << 16, 1)[3] // stripe_geometry(0, 1 << 16, 1)[2]      # blocks per stripe
GROUP = STRIPE // 8                                                                  # counters per group


def c0_at(done):
    """the low byte of a piece's first counter (a 12-byte nonce: the stream's first is 2)"""
    return (2 + done // 16) & (GROUP - 1)


def fill_for(c0):
    """bytes in front of a piece whose first counter's low byte is to be c0"""
    return 16 * ((c0 - 2) % GROUP)


def striped_len(done, n8, tail_blocks=0, ragged=0):
    """a piece behind `done` bytes with n8 stripes, tail_blocks whole blocks behind them and `ragged` more bytes"""
    h0 = stripe_geometry(c0_at(done), 0, 1)[0]
    return 16 * (h0 + STRIPE * n8 + tail_blocks) + ragged


def geometry_at(done, n):
    return stripe_geometry(c0_at(done), n // 16, cus())


# ---- the fixed messages -----------------------------------------------------------------------------------------------
CH, TP = "gcm.chunks", "gcm.twophase"
TOP = 17 * MIB                                # where the walk over the piece planner ends


def piece_bounds():
    """[(b, kind below, kind from b on)]: every boundary of the piece planner up to TOP"""
    return boundaries(lambda n: kind_of(0, n), 16, TOP)


def _messages():
    c = cus()
    long_aad = 16 * (64 << (GH_LOGB + 1)) + 16            # the first AAD with logA = 16, which needs the B table
    m8 = STRIPE * (c + 1) + STRIPE + 4 * GROUP + 2 * 1024            # blocks

    direct = 16 * GH_DIRECT                               # the longest piece without a bulk level
    ms = [Message("m17", 128, 20, TOP - 3, 17, True),
          Message("m8", 128, 33, 16 * m8 + 5, 8, True), Message("m8.192", 192, 33, 16 * m8 + 1, 81, True),
          Message("m8.256", 256, 33, 16 * m8 + 15, 82, True),
          Message("m1", 128, 7, 2 * (direct + 16) + (1 << 16) + 7, 1, True),
          Message("aad32", 128, long_aad, 16 * 3 + piece_bounds()[0][0] + 5, 32, True),
          # the same associated data in front of a striped piece: past the per-item cap, compared with the one-shot call
          Message("aad32.s", 128, long_aad, striped_len(0, c, 1) + 9, 32, False)]
    for alen in (0, 1, 16, 17, direct, direct + 1):
        ms.append(Message("aad%d" % alen, 128, alen, 16 * 3 + piece_bounds()[0][0] + 5, 100 + alen % 251, True))
    return collections.OrderedDict((m.name, m) for m in ms)


_CACHE = {}


def messages():
    if "messages" not in _CACHE:
        _CACHE["messages"] = _messages()
    return _CACHE["messages"]


def key_of(m):
    return bytes((0x21 + 7 * i + m.bits + m.seed) & 0xff for i in range(m.bits // 8))


def nonce_of(m):
    return bytes((0xA0 + 3 * i + m.seed) & 0xff for i in range(12))


class Reference:
    """a message's oracle answer, computed once: ciphertext || tag of the whole text, and the tag of any prefix"""

    def __init__(self, orc, m, seg=SEG):
        self.orc, self.m, self.seg = orc, m, seg
        self.key, self.nonce = key_of(m), nonce_of(m)
        self.aad, self.text = orc.splitmix(m.seed + 1000, m.aad_len), orc.splitmix(m.seed, m.text_len)
        if m.oracle:
            want = orc.gcm_encrypt(self.key, self.nonce, self.aad, self.text)
        else:
            # past the cap: the one-shot call, an independent planner path; its first HEAD bytes against the oracle (the
            # associated data does not enter the ciphertext, so none is handed over)
            want = uaes.AES_GCM_encrypt(self.key, self.nonce, self.aad, self.text)
            assert want[:HEAD] == orc.gcm_encrypt(self.key, self.nonce, b"", self.text[:HEAD])[:HEAD]
        self.ct, self.tag = want[:m.text_len], want[m.text_len:]
        self._h = self._front = self._back = None

    def _raw(self, data):
        """GHASH's Horner value over data, without the length block: orc.ghash gives (raw ^ L) * H"""
        if not data:
            return bytes(16)
        lens = bytes(8) + (8 * len(data)).to_bytes(8, "big")
        return xor(self.orc.gf128_mul(self.orc.ghash(self._h, b"", data), self._hinv), lens)

    def _behind(self, raw_a, b):
        """raw(A || B) from raw(A) and the bytes B"""
        return xor(self.orc.gf128_mul(raw_a, gf_pow(self.orc, self._h, (len(b) + 15) // 16)), self._raw(b)) if b else raw_a

    def _lens(self, n):
        return (8 * self.m.aad_len).to_bytes(8, "big") + (8 * n).to_bytes(8, "big")

    def _from_front(self, n):
        """raw(aad || ct[:n]), by a pass over the ciphertext from its first byte as far as n"""
        if self._front is None:
            self._front = [self._raw(self.aad)]
        k = n // self.seg
        while len(self._front) <= k:               # the pass goes only as far as the longest prefix asked for
            off = (len(self._front) - 1) * self.seg
            self._front.append(self._behind(self._front[-1], self.ct[off:off + self.seg]))
        return self._behind(self._front[k], self.ct[k * self.seg:n])

    def _from_back(self, n):
        """raw(aad || ct[:n]) out of the oracle's tag of the whole message, by a pass over the ciphertext from its last
        byte back to n: raw(whole) = (tag ^ E(J0)) * H^-1 ^ L; with q whole blocks in the prefix and k blocks behind them,
        raw(aad || ct[:16q]) = (raw(whole) ^ raw(ct[16q:])) * H^-k; one more step brings in the padded partial block"""
        orc, seg, total = self.orc, self.seg, self.m.text_len
        nseg = -(-total // seg)
        if self._back is None:
            self._back = [bytes(16)]               # [i] = raw(ct[(nseg - i) * seg:])
        q16 = n // 16 * 16
        j = -(-q16 // seg)
        while len(self._back) <= nseg - j:         # the pass goes only as far back as the shortest prefix asked for
            off = (nseg - len(self._back)) * seg
            behind = (max(total - off - seg, 0) + 15) // 16
            here = orc.gf128_mul(self._raw(self.ct[off:off + seg]), gf_pow(orc, self._h, behind))
            self._back.append(xor(here, self._back[-1]))
        mid = self.ct[q16:j * seg]
        behind = (max(total - j * seg, 0) + 15) // 16
        tail = xor(orc.gf128_mul(self._raw(mid), gf_pow(orc, self._h, behind)), self._back[nseg - j])
        whole = xor(orc.gf128_mul(xor(self.tag, self._ej0), self._hinv), self._lens(total))
        y = orc.gf128_mul(xor(whole, tail), gf_pow(orc, self._hinv, (total - q16 + 15) // 16))
        return self._behind(y, self.ct[q16:n])

    def prefix_tag(self, n, back=None):
        """the tag of the message's first n bytes, from the end of the message that is nearer to n (or the one asked for)"""
        if n == self.m.text_len and back is None:
            return self.tag
        assert self.m.oracle and 0 <= n <= self.m.text_len
        if self._h is None:
            self._h = gcm_h(self.orc, self.key)
            self._hinv = gf_inv(self.orc, self._h)
            self._ej0 = self.orc.encrypt_block(self.key, self.nonce + b"\0\0\0\1")
        if back is None:
            back = from_back(self.m, n)
        y = self._from_back(n) if back else self._from_front(n)
        return xor(self._ej0, self.orc.gf128_mul(xor(y, self._lens(n)), self._h))


def from_back(m, n):
    """whether the tag of m's first n bytes is made from the back of the message: the nearer end"""
    return m.text_len - n < n


def is_prefix(c):
    return sum(c.pieces) < messages()[c.msg].text_len


def prefix_bytes(m, prefixes, seg=SEG):
    """what Reference hands to orc.ghash for the tags of these prefixes of m.  From the front: the associated data, the
    ciphertext in whole segments as far as the longest such prefix reaches, and each prefix's last partial segment.  From
    the back: the whole segments behind the longest such prefix (the last may be short), and for each prefix the blocks
    between its last whole block and the next segment, and its partial block"""
    front = [n for n in prefixes if not from_back(m, n)]
    back = [n for n in prefixes if from_back(m, n)]
    total = 0
    if front:
        total += m.aad_len + max(front) // seg * seg + sum(n % seg for n in front)
    if back:
        ends = [min(-(-(n // 16 * 16) // seg) * seg, m.text_len) for n in back]
        total += m.text_len - min(ends) + sum(e - n // 16 * 16 + n % 16 for e, n in zip(ends, back))
    return total


def oracle_bytes(cases):
    """what a test item that runs `cases` alone hands to the oracle: every message once (HEAD bytes of one past the cap),
    and what the tags of its prefixes take (prefix_bytes)"""
    total, per_msg = 0, collections.defaultdict(set)
    for c in cases:
        per_msg[c.msg].add(sum(c.pieces))
    for name, ends in per_msg.items():
        m = messages()[name]
        total += (m.aad_len + m.text_len) if m.oracle else HEAD
        total += prefix_bytes(m, [n for n in ends if n < m.text_len])
    return total


# ---- the table cache, restated ----------------------------------------------------------------------------------------
INVALID = (False, 0, False, False)


def simulate(c, decrypt=False):
    """([tables() after begin and after every piece], [(table, "rebuilt" | "reused")]): the cache word as
    uaesk_gcm_stream_absorb and uaesk_gcm_stream_piece keep it.  An absorb sets the tables up anew when the word is not
    valid or its level plan (level_plan) asks for a bulk table that is not there, and keeps the striped bit; a chunk or
    two-phase piece leaves the word alone; a striped piece takes its tables as they are when the striped bit is set and
    the level plan of [T][tail] is met, else it sets up and writes that plan with the striped bit."""
    return simulate_pieces(messages()[c.msg].aad_len, c.pieces, c.mask, decrypt)


def simulate_pieces(aad_len, pieces, mask, decrypt=False):
    """simulate() for pieces that are no case of a fixed message (Group F)"""
    state, seq, events = INVALID, [], []

    def absorb(nv):
        nonlocal state
        lg, nb = level_plan(max(nv, 1))
        ok = state[0] and (not lg or state[1] == lg) and (not nb or state[2])
        if lg:
            events.append(("logA", "reused" if ok else "rebuilt"))
        if nb:
            events.append(("B", "reused" if ok else "rebuilt"))
        if not ok:
            state = (True, lg, nb, state[3])

    absorb((aad_len + 15) // 16)
    seq.append(state)
    done = 0
    for n in pieces:
        kind = kind_of(mask, n, done, decrypt)
        if kind == "s":
            _h0, _g_lo, _n8, h1 = geometry_at(done, n)
            lg, nb = level_plan(1 + (n - 16 * h1 + 15) // 16)
            ok = state[0] and state[3] and (not lg or state[1] == lg) and (not nb or state[2])
            events.append(("striped", "reused" if ok else "rebuilt"))
            if not ok:
                state = (True, lg, nb, True)
        elif kind[0] in "da":
            absorb((n + 15) // 16)
        seq.append(state)
        done += n
    return seq, events


def kinds(c, decrypt=False):
    out, done = [], 0
    for n in c.pieces:
        out.append(kind_of(c.mask, n, done, decrypt))
        done += n
    return out


def split_rest(m, pieces):
    """the pieces and what is left of the message behind them"""
    rest = messages()[m].text_len - sum(pieces)
    assert rest > 0 and all(p % 16 == 0 for p in pieces), (m, pieces)
    return list(pieces) + [rest]


# ---- A. every boundary of the piece planner -------------------------------------------------------------------------
def message_for(n, bits=128):
    """the smallest message of that key size that holds a piece of n bytes between two others"""
    fit = [m for m in messages().values() if m.name.startswith("m") and m.bits == bits and n + 16 * 8 < m.text_len]
    return min(fit, key=lambda m: m.text_len).name


def group_a():
    """each boundary b of the piece planner as a middle piece (b - 16, b, b + 16), as the stream's first piece and as
    its last (b - 3, b + 1: prefixes), with the look of the chunk kernel's preparing workgroup at its default and at 0;
    the first boundary (absorb path -> one chunk workgroup and the finisher) at all three key sizes"""
    out = []
    bs = piece_bounds()
    for look in (None, 0):
        for i, (b, below, above) in enumerate(bs):
            for bits in (128, 192, 256) if i == 0 else (128,):
                m = message_for(b + 16, bits)
                note = "%s->%s" % (below, above)
                for n in (b - 16, b, b + 16):
                    out.append(Case("A", m, split_rest(m, [16 * 3, n]), 0, "host", look, note + " middle"))
                out.append(Case("A", m, split_rest(m, [b]), 0, "host", look, note + " first"))
                for n in (b - 3, b + 1):
                    out.append(Case("A", m, [16 * 3, n], 0, "host", look, note + " last"))
    return out


# ---- B. the striped piece at its smallest ---------------------------------------------------------------------------
C0S = (2, GROUP - 1, 0, 1)                   # no fill (h0 = GROUP - 2), h0 = 1, h0 = 0 and g_lo = 0, h0 = GROUP - 1
TAILS = (0, 1, STRIPE - 1)
RAGGED = (0, 1, 15)


def n8s():
    c = cus()
    return (c - 1, c, c + 1, 2 * c - 1)


def _striped_case(group, bits, c0, n8, tail, ragged, mask, place="dev", note=""):
    fill = fill_for(c0)
    n = striped_len(fill, n8, tail, ragged)
    m = message_for(fill + n, bits)
    front = [fill] if fill else []
    pieces = front + [n] if ragged else split_rest(m, front + [n])
    return Case(group, m, pieces, mask, place, None, note or "n8=%d c0=%d tail=%d+%d" % (n8, c0, tail, ragged))


def group_b():
    """mask gcm.chunks | gcm.twophase: a piece is striped from one stripe per workgroup on.  Stripes n8 x first counter
    c0 x tail x ragged end (the ragged ones are last pieces: prefixes), and the whole n8 = CUs row at all three key
    sizes; mask gcm.twophase alone: the first two-phase length goes chunks -> striped."""
    mask = mask_of(CH, TP)
    out = []
    for n8 in n8s():
        for c0 in C0S:
            for tail in TAILS:
                for ragged in RAGGED:
                    out.append(_striped_case("B", 128, c0, n8, tail, ragged, mask, "host" if n8 == cus() and tail == 1 else "dev"))
                    if n8 == cus():
                        out += [_striped_case("B", bits, c0, n8, tail, ragged, mask) for bits in (192, 256)]
    two = [b for b, _below, above in piece_bounds() if above == "t"][0]
    for front in ([16], [piece_bounds()[0][0]]):
        out.append(Case("B", "m17", split_rest("m17", front + [two]), mask_of(TP), "dev", None, "chunks -> striped"))
    return out


# ---- C. table-cache transitions -------------------------------------------------------------------------------------
C_MASKS = ((), (CH,), (CH, TP), (TP,))


def first_lengths(mask, top):
    """{kind: the first length at which a stream's first piece is of that kind} under a mask"""
    out = collections.OrderedDict([(kind_of(mask, 16), 16)])
    for b, _below, above in boundaries(lambda n: kind_of(mask, n), 16, top):
        out.setdefault(above, b)
    return out


def _len_at(mask, kind, done, first):
    return striped_len(done, cus(), 1) if kind == "s" and kind_of(mask, first[kind], done) != "s" else first[kind]


def feasible_pairs(mask, total):
    """the ordered pairs of kinds that fit one message of `total` bytes under a mask"""
    first = first_lengths(mask, total)
    worst = {k: max(_len_at(mask, k, fill_for(c0), first) for c0 in C0S) for k in first}
    return [(x, y) for x in first for y in first if worst[x] + worst[y] + 16 <= total]


def pair_streams(names, msg="m17"):
    """streams over one message in which every feasible ordered pair of kinds stands side by side somewhere: each walks
    on from its last kind to a pair not yet seen while the message has room, and ends with what is left of it"""
    mask, total = mask_of(*names), messages()[msg].text_len
    first = first_lengths(mask, total)
    todo = feasible_pairs(mask, total)
    out = []
    while todo:
        seq, pieces = [todo[0][0]], [_len_at(mask, todo[0][0], 0, first)]
        while True:
            done = sum(pieces)
            step = [p for p in todo if p[0] == seq[-1] and done + _len_at(mask, p[1], done, first) + 16 <= total]
            if not step:
                break
            todo.remove(step[0])
            seq.append(step[0][1])
            pieces.append(_len_at(mask, step[0][1], done, first))
        assert len(seq) > 1, (names, seq, todo)
        c = Case("C", msg, split_rest(msg, pieces), mask, "dev", None, "pairs " + ",".join(seq))
        assert kinds(c)[:len(seq)] == seq, (kinds(c), seq)
        out.append(c)
    return out


def named_stream(seq, names, msg, note):
    mask = mask_of(*names)
    first = first_lengths(mask, messages()[msg].text_len)
    pieces = []
    for kind in seq:
        pieces.append(_len_at(mask, kind, sum(pieces), first))
    c = Case("C", msg, split_rest(msg, pieces), mask, "dev", None, note)
    assert kinds(c)[:len(seq)] == list(seq), (kinds(c), seq)
    return c


def group_c():
    out = []
    for names in C_MASKS:
        out += pair_streams(names)
    out.append(named_stream(("s", "d", "s"), (CH, TP), "m17", "s,d,s: the second s takes the Enc(J0)-only branch"))
    out.append(named_stream(("s", "a14", "s"), (CH, TP), "m17", "s,a14,s: the rebuild keeps the striped bit"))
    out.append(named_stream(("a14", "d", "a14"), (CH,), "m1", "a14,d,a14: the second a14 without a rebuild"))
    for m in messages().values():
        if m.name.startswith("aad") and m.oracle:
            out.append(Case("C", m.name, split_rest(m.name, [16 * 3]), 0, "host", None, "aad %d: d, chunk" % m.aad_len))
    out.append(Case("C", "aad32.s", split_rest("aad32.s", [striped_len(0, cus(), 1)]), mask_of(CH, TP), "dev", None,
                    "aad with the B table, then s: the striped setup writes logA = 0"))
    return out


# ---- D. placements --------------------------------------------------------------------------------------------------
def group_d():
    """every Group A boundary piece (b as a middle piece, b + 1 as the last) and every Group B n8 = CUs case at AES-128,
    in all three placements"""
    bs = {b for b, _below, _above in piece_bounds()}
    base = [c for c in group_a() if c.look is None and messages()[c.msg].bits == 128 and
            ((c.note.endswith("middle") and c.pieces[1] in bs) or (c.note.endswith("last") and c.pieces[1] - 1 in bs))]
    base += [c for c in group_b() if "n8=%d " % cus() in c.note and messages()[c.msg].bits == 128]
    return [c._replace(group="D", place=p) for c in base for p in PLACES]


# ---- E. streams side by side and one after another ------------------------------------------------------------------
def group_e():
    """side by side: d, c1, d, c2 pieces (and what is left) of two messages under different keys; one after another:
    a stream that leaves a scratch with every table in it, and the short streams that follow it and an aborted one"""
    bs = piece_bounds()
    c1, c2 = bs[0][0], bs[1][0]
    side = [Case("E", m, split_rest(m, [16 * 3, c1, 16 * 2, c2]), 0, "host", None, "side by side") for m in ("m8", "m8.192")]
    full = named_stream(("s", "a14"), (CH, TP), "m17", "leaves striped and logA tables behind")._replace(group="E")
    after = [Case("E", m, split_rest(m, [16, c1]), 0, "host", None, "on a recycled scratch") for m in ("m1", "aad17")]
    return side + [full] + after


# ---- F. past the oracle ---------------------------------------------------------------------------------------------
def group_f():
    """(pieces, mask): the natural striped piece -- the first length past the two phases and a stripe more, twice, with a
    block between them, so that the counter position crosses 2^23 blocks --, and two absorbs that need the B table"""
    hi = TOP
    while kind_of(0, hi) != "s":
        hi *= 2
    top = [b for b, _below, above in boundaries(lambda n: kind_of(0, n), TOP, hi) if above == "s"][0] - 16
    long_piece = top + 16 * STRIPE
    with_b = 16 * (64 << (GH_LOGB + 1)) + 16
    return [([long_piece, 16, long_piece, 32], 0), ([with_b, 16, with_b, 5], mask_of(CH, TP, "gcm.striped"))]


# ---- the test items ---------------------------------------------------------------------------------------------------
def items():
    """{item id: [cases]}: what one test of tests/test_gpu_gcm_stream.py runs"""
    if "items" in _CACHE:
        return _CACHE["items"]
    out = collections.OrderedDict()
    for c in group_a():
        out.setdefault("A-%s-%s" % (c.msg, "look0" if c.look == 0 else "look"), []).append(c)
    for c in group_b():
        out.setdefault("B-%s" % c.msg, []).append(c)
    for c in group_c():
        off = "+".join(n[4:] for n in (CH, TP) if c.mask & mask_of(n)) or "none"
        out.setdefault("C-aad32.s" if c.msg == "aad32.s" else "C-aad" if c.msg.startswith("aad") else "C-%s-%s" % (c.msg, off), []).append(c)
    for c in group_d():
        out.setdefault("D-%s-%s" % (c.msg, c.place), []).append(c)
    out["E"] = group_e()
    _CACHE["items"] = out
    return out
