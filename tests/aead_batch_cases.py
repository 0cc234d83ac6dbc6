"""One frame for the GPU tests of the AEAD record batches (CCM, OCB, GCM-SIV, multi-key GCM, XAES-256-GCM): a `Mode`
says what a mode is, and every check that the five tests/test_gpu_*.py files share is written here once, taking the Mode
and the data of the case.  tests/test_aead_batch_cases.py runs the frame without a device: the cases are the intended
ones, and every check fails when the engine is wrong in the way it looks for.  A case draws from its rng in one order:
the keys (where every record has its own), the nonces, the AADs, the texts."""
import functools
import hashlib
import random
import threading
from typing import Any, Callable, NamedTuple, Optional

import micro_aes_amd as uaes
from tests.guarded_mem import FILL, Mem, ptr

E_AUTH = 0x1A                                   # UAES_E_AUTHENTICATION


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def engine_wipe_switch(on):
    uaes.engine().uaes_set_wipe_on_auth_failure(on)


class Mode(NamedTuple):
    name: str
    plan: Callable                  # (msg_bytes, nmsg, decrypt) -> (arrangement, launches, workgroups, threads)
    arrangement: str                # the name the plan must answer
    wrapper: Callable               # uaes.<mode>_batch
    raw: Callable                   # (decrypt, bits, key(s), nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts)
    #                                 onto the two C entry points; the arrays are pointers, bytes or None by then
    key_bits: tuple
    fixed_keys: dict                # bits -> the one key of a call; empty where every record has a key of its own
    nonce_lens: tuple
    tag_lens: Optional[tuple]       # None: always 16, and the wrapper takes no tag_len
    enc: Callable                   # the reference: (key, nonce, aad, text, tl) -> ciphertext || tag
    dec: Callable                   # the reference: (key, nonce, aad, ciphertext || tag, tl) -> (code, text)
    one: Callable                   # the product's one-message call: (decrypt, key, nonce, aad, data, tl) -> what enc / dec give
    forged: tuple                   # a forged record's slot with the wipe switch off, on: "released" (what the reference
    #                                 leaves), "zeros" or "untouched"
    short_shapes: Callable          # bits -> [(records, tl, al, ml, lens or None)]
    short_nls: tuple                # the nonce lengths the short shapes run at
    short_seed: Callable            # (bits, nl) -> the seed of that run
    count_shape: tuple              # (nl, al, ml, tl) of the record-count test
    count_sampled: bool             # at the second-pass count: 70 + 70 + 200 records go to the reference, not all
    lengths_shape: tuple            # (nl, tl, n): n lengths drawn below 49, or n = None for GIVEN
    placement_shape: tuple          # (nl, tl)
    placement_offsets: tuple
    forgery_shape: tuple            # (records, nl, tl, lens or None)
    forgery_parts: tuple            # "<what> of <m>" for forgery(), or what the mode's own forge takes
    forge: Optional[Callable] = None    # part -> Forged, where the mode flips in a way of its own
    wipe_switch: Callable = engine_wipe_switch

    @property
    def per_record_keys(self):
        return not self.fixed_keys

    def bits(self, want):
        return want if want in self.key_bits else self.key_bits[-1]


class Case(NamedTuple):
    bits: int
    key: Any                        # the key, or the list of the records' keys
    nonces: list
    aads: list
    texts: list                     # the slots, all of one size
    tl: int = 16
    lens: Optional[list] = None     # as handed over: an entry above the slot size means the slot size


class Forged(NamedTuple):
    case: Case                      # AAD, nonce or key of record m may be the flipped one
    cts: list
    tags: list
    m: int


def join(items):
    return b"".join(items)


def le32(values):
    return join(v.to_bytes(4, "little") for v in values)


def flip(b, i):
    b = bytearray(b)
    b[i % len(b)] ^= 1 << (i % 8)
    return bytes(b)


def records(mode, rng, n, bits, nl, al, ml):
    """(keys or None, nonces, aads, texts)"""
    keys = [rng.randbytes(bits // 8) for _ in range(n)] if mode.per_record_keys else None
    return keys, [rng.randbytes(nl) for _ in range(n)], [rng.randbytes(al) for _ in range(n)], [rng.randbytes(ml) for _ in range(n)]


def draw(mode, rng, bits, n, nl, al, ml, tl=16, lens=None, key=None):
    assert bits in mode.key_bits and nl in mode.nonce_lens and (tl == 16 if mode.tag_lens is None else tl in mode.tag_lens)
    keys, nonces, aads, texts = records(mode, rng, n, bits, nl, al, ml)
    return Case(bits, keys if mode.per_record_keys else (key or mode.fixed_keys[bits]), nonces, aads, texts, tl, lens)


def key_of(mode, c, m):
    return c.key[m] if mode.per_record_keys else c.key


def cut(c):
    """the records themselves: the first lens[m] bytes of every slot"""
    return c.texts if c.lens is None else [t[:k] for t, k in zip(c.texts, c.lens)]


def expected(mode, c, only=None):
    """the reference's (ciphertexts, tags), one call per record (only: of these records)"""
    cts, tags = [], []
    texts = cut(c)
    for m in range(len(texts)) if only is None else only:
        ct = mode.enc(key_of(mode, c, m), c.nonces[m], c.aads[m], texts[m], c.tl)
        cts.append(ct[:len(texts[m])])
        tags.append(ct[len(texts[m]):])
    return cts, tags


def call(mode, c, texts, **kw):
    if mode.tag_lens is not None:
        kw["tag_len"] = c.tl
    return mode.wrapper(c.key, c.nonces, c.aads, texts, lens=c.lens, **kw)


def check_against(mode, want, c, info):
    """encrypt == want per record and nothing beyond lens[m]; decrypt returns 0, all verdicts 1 and the plaintext into a
    prefilled buffer, again with nothing beyond lens[m]"""
    texts = cut(c)
    cts, tags = call(mode, c, c.texts, prefill=0x33)
    bad = [m for m, t in enumerate(texts) if (cts[m][:len(t)], tags[m]) != (want[0][m], want[1][m])]
    if bad:
        raise AssertionError("encrypt %r: records %r differ" % (info, bad[:8]))
    assert all(set(ct[len(t):]) <= {0x33} for ct, t in zip(cts, texts)), ("encrypt wrote beyond lens", info)
    rc, pts, verdicts = call(mode, c, cts, decrypt=True, tags=tags, prefill=0x77)
    assert rc == 0 and verdicts == [1] * len(texts), ("decrypt", info, rc, verdicts)
    assert [p[:len(t)] for p, t in zip(pts, texts)] == texts, ("decrypt", info)
    assert all(set(p[len(t):]) <= {0x77} for p, t in zip(pts, texts)), ("decrypt wrote beyond lens", info)


def check_both(mode, c, info):
    check_against(mode, expected(mode, c), c, info)


# ---- every short shape ------------------------------------------------------------------------------------------------
def short_cases(mode, bits, nl, seed=None, key=None):
    rng = random.Random(mode.short_seed(bits, nl) if seed is None else seed)
    return [draw(mode, rng, bits, n, nl, al, ml, tl, lens, key) for n, tl, al, ml, lens in mode.short_shapes(bits)]


def check_short_shapes(mode, bits, nl):
    for c in short_cases(mode, bits, nl):
        check_both(mode, c, (mode.name, bits, nl, c.tl, len(c.aads[0]), len(c.texts[0])))


# ---- record counts from the plan --------------------------------------------------------------------------------------
def second_pass(mode):
    """the first count at which the grid-stride loop of the largest launch runs a second time, + 3"""
    name, launches, grid, threads = mode.plan(16, 1 << 20, False)
    assert name == mode.arrangement and launches == 1 and threads % 16 == 0
    return grid * threads // 16 + 3


def count_case(mode, nmsg):
    """(the case, its rng as the draws left it)"""
    rng = random.Random(nmsg)
    nl, al, ml, tl = mode.count_shape
    c = draw(mode, rng, mode.key_bits[0], nmsg, nl, al, ml, tl)
    assert len(set(c.nonces)) == nmsg                                           # every record has its own nonce
    assert not mode.per_record_keys or len(set(c.key)) == nmsg                  # and its own key
    return c, rng


def check_count(mode, nmsg, second=False):
    """second: nmsg is second_pass(mode), and the modes that sample compare 70 + 70 + 200 records there"""
    if second:
        for dec in (False, True):
            name, _, grid, threads = mode.plan(16, nmsg, dec)
            assert name == mode.arrangement and nmsg > grid * threads // 16     # it does run a second time
    c, rng = count_case(mode, nmsg)
    if not (second and mode.count_sampled):
        check_both(mode, c, ("count", nmsg))                                    # every record is compared
        return
    look = sorted(set(range(70)) | set(range(nmsg - 70, nmsg)) | set(rng.sample(range(nmsg), 200)))
    cts, tags = call(mode, c, c.texts)
    want = expected(mode, c, look)
    bad = [m for k, m in enumerate(look) if (cts[m], tags[m]) != (want[0][k], want[1][k])]
    assert not bad, ("count", nmsg, bad[:8])
    rc, pts, verdicts = call(mode, c, cts, decrypt=True, tags=tags, prefill=0x77)
    assert rc == 0 and verdicts == [1] * nmsg and pts == c.texts, ("count", nmsg, rc)


# ---- the raw entry points ---------------------------------------------------------------------------------------------
def run(mode, c, decrypt, key, lens, nonces, aads, src, dst, tags, verdicts=None):
    """one call of an entry point for case c; every array bytes, None or Mem"""
    return mode.raw(decrypt, c.bits, ptr(key), len(c.nonces[0]), c.tl, len(c.texts), len(c.texts[0]), ptr(lens), ptr(nonces),
                    ptr(aads), len(c.aads[0]), ptr(src), ptr(dst), ptr(tags), ptr(verdicts))


def keys_in(mode, c, device=False, off=0):
    """the key argument of a raw call: the records' keys as an array in memory, or the one key as it is"""
    return Mem(join(c.key), device, off) if mode.per_record_keys else c.key


def ones(n):
    return b"\1" * n


# ---- per-record lengths -----------------------------------------------------------------------------------------------
GIVEN = [0, 1, 15, 16, 17, 33, 48, 1000, 48, 0, 31]                             # 1000: taken as msg_bytes


def lengths_case(mode):
    """lengths_shape's n lengths below 49 drawn before the records, or GIVEN; 48-byte slots, 9 bytes of AAD"""
    rng = random.Random(48)
    nl, tl, n = mode.lengths_shape
    lens = list(GIVEN)
    if n is not None:
        lens = [rng.randrange(49) for _ in range(n)]
        lens[3], lens[20], lens[36] = 0, 48, 17
        assert min(lens) == 0 and max(lens) == 48
    return draw(mode, rng, mode.key_bits[0], len(lens), nl, 9, 48, tl, lens)


def check_lengths(mode, c, device, lens_on_device):
    """over raw pointers: record m is lens[m] bytes, the rest of its slot is not written, and an entry above msg_bytes is
    taken as msg_bytes"""
    n, ml, tl = len(c.texts), len(c.texts[0]), c.tl
    lens = [min(k, ml) for k in c.lens]
    want = expected(mode, c)
    slot = lambda buf, m: (buf[m * ml:m * ml + lens[m]], buf[m * ml + lens[m]:(m + 1) * ml])        # noqa: E731
    lv, mk = Mem(le32(c.lens), lens_on_device), keys_in(mode, c, device)
    src, dst, tags = Mem(join(c.texts), device), Mem(size=n * ml, device=device), Mem(size=n * tl, device=device)
    mn, ma = Mem(join(c.nonces), device), Mem(join(c.aads), device)
    assert run(mode, c, False, mk, lv, mn, ma, src, dst, tags) == 0
    out, tg = dst.get(), tags.get()
    for m in range(n):
        info = (device, lens_on_device, m, c.lens[m])
        assert slot(out, m)[0] == want[0][m] and tg[m * tl:(m + 1) * tl] == want[1][m], info
        assert set(slot(out, m)[1]) <= {FILL}, info                              # beyond lens[m]: not written
    assert dst.intact(n * ml) and tags.intact(n * tl) and src.get() == join(c.texts)
    back, ver = Mem(size=n * ml, device=device), Mem(size=n, device=device)
    assert run(mode, c, True, mk, lv, mn, ma, dst, back, tags, ver) == 0
    got = back.get()
    for m in range(n):
        assert slot(got, m)[0] == c.texts[m][:lens[m]] and set(slot(got, m)[1]) <= {FILL}, m
    assert ver.get() == ones(n) and back.intact(n * ml) and ver.intact(n)
    clamp = Mem(le32(k if k < ml else 1000 + k for k in c.lens), lens_on_device)
    dst2, tags2 = Mem(size=n * ml, device=device), Mem(size=n * tl, device=device)
    assert run(mode, c, False, mk, clamp, mn, ma, src, dst2, tags2) == 0
    assert dst2.get() == out and tags2.get() == tg and dst2.intact(n * ml)


# ---- placement --------------------------------------------------------------------------------------------------------
ARRAYS = ("keys", "nonces", "aad", "texts", "tags", "verdicts")


def arrays(mode):
    return ARRAYS if mode.per_record_keys else ARRAYS[1:]


def places(mode):
    """masks over arrays(mode), bit k: array k is in device memory -- none, all, each alone, all but each"""
    k, full = len(arrays(mode)), (1 << len(arrays(mode))) - 1
    return [0, full] + [1 << i for i in range(k)] + [full ^ (1 << i) for i in range(k)]


def place_id(mode, mask):
    return "+".join(a for k, a in enumerate(arrays(mode)) if mask >> k & 1) or "host"


def placement_case(mode, off):
    """21 records at key size 192 (or the mode's only one), 17 bytes of AAD; offsets other than 0 with 33-byte records:
    the byte-wise path; offset 0 with 32: the 4-byte-aligned one"""
    nl, tl = mode.placement_shape
    return draw(mode, random.Random(33 + off), mode.bits(192), 21, nl, 17, 33 if off else 32, tl)


def check_placement(mode, c, mask, off):
    """every array `off` bytes behind an aligned address, in device memory where its bit of mask says so: out of place
    and in place, both directions; only the outputs are written, and those inside their bounds"""
    n, ml, tl = len(c.texts), len(c.texts[0]), c.tl
    on = {a: bool(mask >> k & 1) for k, a in enumerate(arrays(mode))}
    on.setdefault("keys", False)
    text, (wct, wtag) = join(c.texts), map(join, expected(mode, c))
    info = (place_id(mode, mask), off)
    mk, mn, ma = keys_in(mode, c, on["keys"], off), Mem(join(c.nonces), on["nonces"], off), Mem(join(c.aads), on["aad"], off)
    src, dst = Mem(text, on["texts"], off), Mem(size=n * ml, device=on["texts"], off=off)
    tags = Mem(size=n * tl, device=on["tags"], off=off)
    assert run(mode, c, False, mk, None, mn, ma, src, dst, tags) == 0, info
    assert dst.get() == wct and tags.get() == wtag, info
    assert dst.intact(n * ml) and tags.intact(n * tl) and src.get() == text, info
    back, ver = Mem(size=n * ml, device=on["texts"], off=off), Mem(size=n, device=on["verdicts"], off=off)
    assert run(mode, c, True, mk, None, mn, ma, dst, back, tags, ver) == 0, info
    assert back.get() == text and ver.get() == ones(n) and back.intact(n * ml) and ver.intact(n), info
    # crtxt == pntxt
    io, tags2 = Mem(text, on["texts"], off), Mem(size=n * tl, device=on["tags"], off=off)
    assert run(mode, c, False, mk, None, mn, ma, io, io, tags2) == 0, info
    assert io.get() == wct and tags2.get() == wtag and io.intact(n * ml) and tags2.intact(n * tl), info
    ver2 = Mem(size=n, device=on["verdicts"], off=off)
    assert run(mode, c, True, mk, None, mn, ma, io, io, tags2, ver2) == 0, info
    assert io.get() == text and io.intact(n * ml) and ver2.get() == ones(n) and ver2.intact(n), info
    for given, was in ((mn, c.nonces), (ma, c.aads)) + (((mk, c.key),) if mode.per_record_keys else ()):
        assert given.get() == join(was) and given.intact(len(join(was))), info


def check_in_place(mode, seed, ml, nl, nonces_at_off=False):
    """row_walk requests a chunk of blocks ahead: six records of more blocks than that in place, in device memory, at
    offsets 0 and 2, without AAD"""
    c = draw(mode, random.Random(seed), mode.bits(256), 6, nl, 0, ml)
    n, tl = 6, c.tl
    text, (wct, wtag) = join(c.texts), map(join, expected(mode, c))
    for off in (0, 2):
        io, tags, ver = Mem(text, True, off), Mem(size=n * tl, device=True), Mem(size=n, device=True)
        mk, mn = keys_in(mode, c, True, off), Mem(join(c.nonces), True, off if nonces_at_off else 0)
        assert run(mode, c, False, mk, None, mn, None, io, io, tags) == 0
        assert io.get() == wct and tags.get() == wtag and io.intact(n * ml), (ml, off)
        assert run(mode, c, True, mk, None, mn, None, io, io, tags, ver) == 0
        assert io.get() == text and ver.get() == ones(n) and io.intact(n * ml), (ml, off)


# ---- forgeries --------------------------------------------------------------------------------------------------------
def forgery_case(mode):
    """(the case, its rng as the draws left it): key size 128 (or the mode's only one), 40-byte slots, 13 bytes of AAD"""
    rng = random.Random(9)
    n, nl, tl, lens = mode.forgery_shape
    return draw(mode, rng, mode.key_bits[0], n, nl, 13, 40, tl, lens), rng


def forged(mode, c, what, m, flipped=None):
    """case c with one part ("text", "tag", "AAD", "nonce" or "key") of record m replaced by flipped(part)"""
    cts, tags = expected(mode, c)
    c = c._replace(nonces=list(c.nonces), aads=list(c.aads), key=list(c.key) if mode.per_record_keys else c.key)
    part = {"text": cts, "tag": tags, "AAD": c.aads, "nonce": c.nonces, "key": c.key}[what]
    part[m] = flipped(part[m])
    return Forged(c, cts, tags, m)


def forgery(mode, part):
    """part = "<what> of <m>": one bit of it flipped, the bit drawn after the records"""
    if mode.forge is not None:
        return mode.forge(part)
    c, rng = forgery_case(mode)
    bit = rng.randrange(1 << 16)
    return forged(mode, c, part.split()[0], int(part.split()[-1]), lambda b: flip(b, bit))


def check_forgery(mode, f, in_place=False, device=True):
    """one forged record among authentic ones, the wipe switch off and on: the reference rejects it too, the call answers
    0x1A, the verdicts name that record alone, its slot holds what mode.forged says, every other record is authentic and
    correct, and nothing beyond lens[m] moves.  in_place: over the raw entry point, the ciphertext as the output"""
    c, m = f.case, f.m
    n, ml = len(c.texts), len(c.texts[0])
    lens, texts = [ml] * n if c.lens is None else [min(k, ml) for k in c.lens], cut(c)
    orc_rc, left = mode.dec(key_of(mode, c, m), c.nonces[m], c.aads[m], f.cts[m] + f.tags[m], c.tl)
    assert orc_rc == E_AUTH and len(left) == lens[m]
    padded = [ct + bytes(ml - len(ct)) for ct in f.cts]
    for wipe in (0, 1):
        info = (mode.name, m, in_place, wipe)
        mode.wipe_switch(wipe)
        try:
            if in_place:
                io, ver = Mem(join(padded), device), Mem(size=n, device=device)
                key = join(c.key) if mode.per_record_keys else c.key
                rc = run(mode, c, True, key, None if c.lens is None else le32(c.lens), join(c.nonces), join(c.aads), io, io,
                         join(f.tags), ver)
                out, before = io.get(), padded                                   # an untouched slot stays ciphertext
                pts, verdicts = [out[k * ml:(k + 1) * ml] for k in range(n)], list(ver.get())
                assert io.intact(n * ml) and ver.intact(n), info
            else:
                rc, pts, verdicts = call(mode, c, padded, decrypt=True, tags=f.tags, prefill=0x5A)
                before = [bytes([0x5A]) * ml] * n                                # an untouched slot stays the prefill
        finally:
            mode.wipe_switch(0)
        assert rc == E_AUTH and verdicts == [0 if k == m else 1 for k in range(n)], (info, rc, verdicts)
        holds = {"released": left, "zeros": bytes(lens[m]), "untouched": before[m][:lens[m]]}[mode.forged[wipe]]
        assert pts[m][:lens[m]] == holds, info
        for k in range(n):
            assert pts[k][lens[k]:] == before[k][lens[k]:], (info, k)             # nothing else moves
            assert k == m or pts[k][:lens[k]] == texts[k], (info, k)


# ---- one call at a time -----------------------------------------------------------------------------------------------
def check_one_message_calls(mode, bits, seed, shapes, n, look=None):
    """shapes of (nl, tl, al, ml), n records each: the batch equals the product's one-message calls and the reference,
    record by record (look: these records only).  Returns [(case, ciphertexts, tags)]"""
    rng = random.Random(seed)
    done = []
    for nl, tl, al, ml in shapes:
        c = draw(mode, rng, bits, n, nl, al, ml, tl)
        cts, tags = call(mode, c, c.texts)
        for m in range(n) if look is None else look:
            info = (mode.name, bits, nl, tl, al, ml, m)
            key, args = key_of(mode, c, m), (c.nonces[m], c.aads[m])
            assert mode.one(False, key, *args, c.texts[m], tl) == cts[m] + tags[m] == mode.enc(key, *args, c.texts[m], tl), info
            assert mode.one(True, key, *args, cts[m] + tags[m], tl) == (0, c.texts[m]), info
        done.append((c, cts, tags))
    return done


# ---- threads ----------------------------------------------------------------------------------------------------------
def keyed_thread_jobs(mode, nl):
    """jobs for two threads with a random 128-bit key each: five shapes, tags of 8 bytes"""
    jobs = {}
    for seed in (10, 20):
        rng = random.Random(seed)
        key = rng.randbytes(16)
        jobs[seed] = [draw(mode, rng, 128, n, nl, ml % 31, ml, 8, key=key) for n, ml in ((1, 0), (5, 17), (70, 64), (300, 33), (9, 1000))]
    return jobs


def check_two_threads(mode, jobs, repeats=1):
    """jobs: {thread: its cases}.  The expected values are made first; the threads only call the engine"""
    wants = {t: [expected(mode, c) for c in cases] for t, cases in jobs.items()}
    errors = []

    def worker(t):
        try:
            for _ in range(repeats):
                for c, want in zip(jobs[t], wants[t]):
                    check_against(mode, want, c, (mode.name, t, len(c.texts), len(c.texts[0])))
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(t,)) for t in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---- what tests/test_aead_batch_cases.py pins -------------------------------------------------------------------------
def digest(cases):
    """SHA-256 over the inputs of the cases: key size, tag length, key(s), nonces, AADs, texts and lens, each with its length"""
    h = hashlib.sha256()
    for c in cases:
        keys = c.key if isinstance(c.key, list) else [c.key]
        h.update(b"%d %d %d|" % (c.bits, c.tl, len(c.texts)))
        for items in (keys, c.nonces, c.aads, c.texts):
            h.update(b"%d:%d:" % (len(items), len(items[0])) + join(items))
        h.update(b"-" if c.lens is None else le32(c.lens))
    return h.hexdigest()
