"""The GCM record kernel (k_gcm_records, csrc/uaes_gcm_records.hip) behind uaes_gcm_key_{en,de}crypt_records, their _v
and _dev forms and uaes_gcm_record_max: every live count of every arrangement in records of different lengths, equally
long records at every arrangement limit, more turns than workgroups, the variable-length device call with forgeries in
every place of a turn, every placement of the five arrays through the synchronous calls, what an in-place call leaves in
the slots, AAD-only records and the argument limits.

The reference is orc.gcm_encrypt of each record alone; decryption is checked against the known plaintext.  Every record
of every batch is compared.  A failure prints the tuple that reproduces it: (S, steps), nrec, max_len or rec_len, aad_len,
the record's index and its length.  The lengths and counts come from tests/gcm_records_cases.py, whose own test shows
what they reach."""
import functools
import random
import struct

import pytest

import micro_aes_amd as uaes
from tests import gcm_records_cases as GC
from tests.guarded_mem import FILL, Mem

pytestmark = pytest.mark.gpu

E_AUTH, E_ARG = 0x1A, -2
ALL_BITS = (128, 192, 256)


def key_of(bits):
    return random.Random(bits).randbytes(bits // 8)


@functools.lru_cache(maxsize=None)
def gkey(bits):
    return uaes.GcmKey(key_of(bits))


def r16(n):
    return (n + 15) // 16 * 16


def flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def slots(parts, stride, fill=FILL):
    """the parts at the start of a slot of `stride` bytes each, the rest of a slot filled"""
    return b"".join(p + bytes([fill]) * (stride - len(p)) for p in parts)


def u32s(values):
    return struct.pack("<%dI" % len(values), *values)


def call(bits, decrypt, nrec, nonces, aad, aad_len, aad_stride, src, lens, rec_len, in_stride, dst, out_stride,
         verdicts=None, status=None, dev=False, v=None):
    """one of the eight record calls of the C ABI; Mem or None for every array"""
    p = lambda m: m.ptr if isinstance(m, Mem) else m
    v = lens is not None if v is None else v
    name = "uaes_gcm_key_%s_records%s%s" % ("decrypt" if decrypt else "encrypt", "_v" if v else "", "_dev" if dev else "")
    args = [gkey(bits)._h if bits else None, nrec, p(nonces), p(aad), aad_len, aad_stride, p(src)]
    if v:
        args.append(p(lens))
    args += [rec_len, in_stride, p(dst), out_stride]
    if decrypt:
        args.append(p(verdicts))
    if dev:
        if decrypt:
            args.append(p(status))
        args.append(uaes._stream(None))
    return getattr(uaes.engine(), name)(*args)


def check_records(got, want, what, case, lens):
    """got == want, record by record; case = ((S, steps), nrec, max_len or rec_len, aad_len)"""
    bad = [r for r in range(len(want)) if got[r] != want[r]]
    if bad:
        raise AssertionError("%s: %d of %d records differ, the first: %r" % (what, len(bad), len(want), case + (bad[0], lens[bad[0]])))


def check_slots(after, before, stride, heads, span, what, case, lens):
    """slot r of `after` starts with heads[r]; behind that, up to span[r] bytes, it holds what it held `before` or zeros
    (the synchronous variable-length calls return zeros there), and from span[r] on what it held before.  heads[r] None:
    the whole slot is as it was."""
    assert len(after) == len(before) == stride * len(heads)
    for r, head in enumerate(heads):
        a, b = after[r * stride:(r + 1) * stride], before[r * stride:(r + 1) * stride]
        if head is None:
            ok = a == b
        else:
            n, e = len(head), max(span[r], len(head))
            ok = a[:n] == head and a[e:] == b[e:] and all(x == y or x == 0 for x, y in zip(a[n:e], b[n:e]))
        if not ok:
            raise AssertionError("%s: slot %r is wrong (%s)" % (what, case + (r, lens[r]), "touched" if head is None else
                                 "head" if a[:len(head)] != head else "tail"))


def case_of(aad_len, max_len, nrec):
    return (GC.arrangement(aad_len, max_len), nrec, max_len, aad_len)


def status_mem():
    return Mem(struct.pack("<i", 0x55555555), True)


def status_of(m):
    return struct.unpack("<i", m.get())[0]


# ---- the restated rule ------------------------------------------------------------------------------------------------
def test_record_max_and_the_six_arrangements():
    for a in (0, 1, 16, 17, 33, 16 * 2044, 16 * 2045):
        assert uaes.GcmKey.record_max(a) == GC.record_max(a), a
    assert uaes.GcmKey.record_max(16 * 2045 + 1) == 0
    seen = []
    for n in range(0, GC.record_max(0) + 1):
        a = GC.arrangement(0, n)
        if not seen or seen[-1] != a:
            seen.append(a)
    assert tuple(seen) == GC.ARRANGEMENTS and len(seen) == 6


# ---- 1. every live count of each arrangement, records of different lengths ----------------------------------------------
V_CASES = [(t, form, bits) for t in GC.TARGETS for form in GC.AAD_FORMS if form == "none" or t in GC.UPPER_TARGETS
           for bits in (ALL_BITS if t <= 512 else (128, 256))]


@pytest.mark.parametrize("target,form,bits", V_CASES)
def test_every_live_count_in_records_of_different_lengths(orc, target, form, bits):
    aad_len, each = GC.AAD_FORMS[form]
    max_len = GC.max_len_for(target, aad_len)
    rng = random.Random(target * 1000 + bits + aad_len)
    lens = GC.lengths_for(aad_len, max_len, rng)
    n = len(lens)
    case = case_of(aad_len, max_len, n)
    texts, nonces = [rng.randbytes(m) for m in lens], [rng.randbytes(12) for _ in lens]
    aads = [rng.randbytes(aad_len) for _ in lens] if each else rng.randbytes(aad_len)
    key, k = key_of(bits), gkey(bits)
    want = [orc.gcm_encrypt(key, nonces[r], aads[r] if each else aads, texts[r]) for r in range(n)]
    check_records(k.encrypt_records_v(nonces, aads, texts, max_len=max_len), want, "encrypt_records_v", case, lens)
    rc, ver, back = k.decrypt_records_v(nonces, aads, want, prefill=FILL, max_len=max_len)
    check_records(back, texts, "decrypt_records_v", case, lens)
    check_records(ver, [0] * n, "decrypt_records_v verdicts", case, lens)
    assert rc == 0, case


# ---- 2. equally long records at every boundary length --------------------------------------------------------------------
@pytest.mark.parametrize("bits", ALL_BITS)
@pytest.mark.parametrize("form", list(GC.AAD_FORMS))
def test_equally_long_records_at_every_boundary_length(orc, form, bits):
    aad_len, each = GC.AAD_FORMS[form]
    rng = random.Random(bits + aad_len)
    key, k = key_of(bits), gkey(bits)
    for rec_len, nrec in GC.fixed_lengths(aad_len):
        case, lens = case_of(aad_len, rec_len, nrec), [rec_len] * nrec
        assert nrec == GC.groups(case[0][0]) + 1
        texts, nonces = [rng.randbytes(rec_len) for _ in lens], [rng.randbytes(12) for _ in lens]
        aads = [rng.randbytes(aad_len) for _ in lens] if each else rng.randbytes(aad_len)
        want = [orc.gcm_encrypt(key, nonces[r], aads[r] if each else aads, texts[r]) for r in range(nrec)]
        check_records(k.encrypt_records(nonces, aads, texts), want, "encrypt_records", case, lens)
        rc, ver, back = k.decrypt_records(nonces, aads, want, prefill=FILL)
        check_records(back, texts, "decrypt_records", case, lens)
        assert rc == 0 and ver == [0] * nrec, case
        # the first record and the one alone in the last turn forged: they keep the prefill, the others decrypt
        forged = list(want)
        forged[0] = flip(want[0], rng.randrange(8 * rec_len) if rec_len else 5)
        forged[-1] = flip(want[-1], 8 * rec_len + rng.randrange(128))
        rc, ver, back = k.decrypt_records(nonces, aads, forged, prefill=FILL)
        left = bytes([FILL]) * rec_len
        check_records(back, [left] + texts[1:-1] + [left], "decrypt_records, two forged", case, lens)
        check_records(ver, [E_AUTH] + [0] * (nrec - 2) + [E_AUTH], "verdicts, two forged", case, lens)
        assert rc == E_AUTH, case


# ---- 3. more turns than workgroups ---------------------------------------------------------------------------------------
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


_turns = {}


def turn_reference(orc, S, steps, rec_len, bits):
    """nonces, texts and the reference's answers for the largest count of a form, made once for its four counts; the
    variable-length form takes a prefix of each text and shares the answers of the records that stay whole"""
    if (S, steps, bits) not in _turns:
        n = GC.turn_counts(cus(), GC.groups(S))[-1]
        rng = random.Random(S * 8 + steps + bits)
        key = key_of(bits)
        nonces, texts = [rng.randbytes(12) for _ in range(n)], [rng.randbytes(rec_len) for _ in range(n)]
        want = [orc.gcm_encrypt(key, nonces[r], b"", texts[r]) for r in range(n)]
        lens = GC.turn_lengths(rec_len, n, S + steps)
        want_v = [want[r] if lens[r] == rec_len else orc.gcm_encrypt(key, nonces[r], b"", texts[r][:lens[r]]) for r in range(n)]
        _turns[S, steps, bits] = nonces, texts, want, lens, want_v
    return _turns[S, steps, bits]


TURN_CASES = [(S, steps, n, which, bits) for S, steps, n in GC.turn_forms() for which in range(4)
              for bits in (ALL_BITS if S < 1024 else (128, 256))]


@pytest.mark.parametrize("S,steps,rec_len,which,bits", TURN_CASES)
def test_more_turns_than_workgroups(orc, S, steps, rec_len, which, bits):
    assert GC.arrangement(0, rec_len) == (S, steps)
    nrec = GC.turn_counts(cus(), GC.groups(S))[which]
    nonces, texts, want, lens_v, want_v = (x[:nrec] for x in turn_reference(orc, S, steps, rec_len, bits))
    stride = r16(rec_len + 16)
    case = case_of(0, rec_len, nrec)
    # the nonces of the fixed calls at an odd address (the kernel reads them byte by byte), of the _v calls word aligned
    for lens, answers, noff in ((None, want, 1), (lens_v, want_v, 0)):
        what = "records_v_dev" if lens else "records_dev"
        ll = lens or [rec_len] * nrec
        dn = Mem(b"".join(nonces), True, noff)
        dl = Mem(u32s(lens), True, 4) if lens else None
        plain = slots([t[:m] for t, m in zip(texts, ll)], stride)
        src, before = Mem(plain, True, 16), bytes([FILL]) * (nrec * stride)
        dst = Mem(before, True, 32)
        assert call(bits, 0, nrec, dn, None, 0, 0, src, dl, rec_len, stride, dst, stride, dev=True) == 0, case
        check_slots(dst.get(), before, stride, answers, [0] * nrec, "encrypt_" + what, case, ll)
        assert dst.intact() and src.get() == plain, case
        src, dst, ver, st = Mem(slots(answers, stride), True, 16), Mem(before, True, 32), Mem(size=nrec, fill=7, device=True), status_mem()
        assert call(bits, 1, nrec, dn, None, 0, 0, src, dl, rec_len, stride, dst, stride, ver, st, dev=True) == 0, case
        check_slots(dst.get(), before, stride, [t[:m] for t, m in zip(texts, ll)], [0] * nrec, "decrypt_" + what, case, ll)
        check_records(list(ver.get()), [0] * nrec, "verdicts of decrypt_" + what, case, ll)
        assert status_of(st) == 0 and dst.intact() and ver.intact() and st.intact(), case


# ---- 4. uaes_gcm_key_decrypt_records_v_dev ---------------------------------------------------------------------------------
AAD_EACH = 13
_vdev = {}


def vdev_reference(orc, max_len, bits):
    """2 G + a part of G records with 13 bytes of AAD each; record 1 is max_len bytes, record 2 empty"""
    if (max_len, bits) not in _vdev:
        G = GC.groups(GC.arrangement(AAD_EACH, max_len)[0])
        nrec = 2 * G + max(2, G // 3)
        rng = random.Random(max_len + bits)
        lens = [rng.randrange(2, max_len + 1) for _ in range(nrec)]
        lens[1], lens[2] = max_len, 0
        nonces, aads = [rng.randbytes(12) for _ in lens], [rng.randbytes(AAD_EACH) for _ in lens]
        texts = [rng.randbytes(m) for m in lens]
        want = [orc.gcm_encrypt(key_of(bits), nonces[r], aads[r], texts[r]) for r in range(nrec)]
        _vdev[max_len, bits] = G, nrec, lens, nonces, aads, texts, want
    return _vdev[max_len, bits]


def forge(kind, r, nonces, aads, cts, lens, rng):
    """record r made a forgery of the given kind, in place in the four lists"""
    if kind == "text":
        cts[r] = flip(cts[r], rng.randrange(8 * (len(cts[r]) - 16)))
    elif kind == "tag":
        cts[r] = flip(cts[r], 8 * (len(cts[r]) - 16) + rng.randrange(128))
    elif kind == "aad":
        aads[r] = flip(aads[r], rng.randrange(8 * AAD_EACH))
    elif kind == "nonce":
        nonces[r] = nonces[r - 1]
    else:
        lens[r] -= 1


@pytest.mark.parametrize("bits", ALL_BITS)
@pytest.mark.parametrize("max_len", [100, 2040], ids=["G16", "G4"])
@pytest.mark.parametrize("which", ["none", "places", "a-whole-turn"])
def test_decrypt_records_v_dev(orc, which, max_len, bits):
    G, nrec, true_lens, nonces, aads, texts, want = vdev_reference(orc, max_len, bits)
    assert GC.arrangement(AAD_EACH, max_len) == (1024 // G, 1) and 2 * G < nrec < 3 * G
    kinds = ["text", "tag", "aad", "nonce", "lens"]
    # the first and the last group of a turn, the first and the last record of the last (partial) turn, one in between
    places = {0: "text", G - 1: "tag", 2 * G: "aad", nrec - 1: "nonce", G + 1: "lens"}
    forged = {"none": {}, "places": places, "a-whole-turn": {G + q: kinds[q % 5] for q in range(G)}}[which]
    rng = random.Random(max_len)
    fn, fa, fc, fl = list(nonces), list(aads), list(want), list(true_lens)
    for r, kind in forged.items():
        forge(kind, r, fn, fa, fc, fl, rng)
    fl[1] = max_len + 4096                                    # above max_len: clamped, the tag is read behind max_len
    in_stride, out_stride = r16(max_len + 16), r16(max_len + 16) + 32
    case = case_of(AAD_EACH, max_len, nrec)
    dn, da, dl = Mem(b"".join(fn), True, 1), Mem(b"".join(fa), True, 3), Mem(u32s(fl), True, 4)
    cts = slots(fc, in_stride)
    verdicts = bytes(E_AUTH if r in forged else 0 for r in range(nrec))
    for with_verdicts in (True, False):
        src, before = Mem(cts, True, 16), bytes([FILL]) * (nrec * out_stride)
        dst, st = Mem(before, True, 32), status_mem()
        ver = Mem(size=nrec, fill=7, device=True) if with_verdicts else None
        rc = call(bits, 1, nrec, dn, da, AAD_EACH, AAD_EACH, src, dl, max_len, in_stride, dst, out_stride, ver, st, dev=True)
        assert rc == 0, case
        heads = [None if r in forged else texts[r] for r in range(nrec)]
        check_slots(dst.get(), before, out_stride, heads, [0] * nrec, "decrypt_records_v_dev (%s)" % which, case, true_lens)
        assert status_of(st) == (E_AUTH if forged else 0) and st.intact() and dst.intact() and src.get() == cts, case
        if ver:
            check_records(list(ver.get()), list(verdicts), "verdicts (%s)" % which, case, true_lens)
            assert ver.intact()
    # in place: a forged record keeps its ciphertext, its neighbours hold their plaintext in front of what was there
    buf, st = Mem(cts, True, 16), status_mem()
    assert call(bits, 1, nrec, dn, da, AAD_EACH, AAD_EACH, buf, dl, max_len, in_stride, buf, in_stride, None, st, dev=True) == 0
    check_slots(buf.get(), cts, in_stride, heads, [0] * nrec, "decrypt_records_v_dev in place (%s)" % which, case, true_lens)
    assert status_of(st) == (E_AUTH if forged else 0) and buf.intact(), case


# ---- 5. placement through the synchronous calls ------------------------------------------------------------------------------
PLACEMENTS = {
    "all-host": set(),
    "all-device": {"nonces", "aad", "in", "out", "lens"},
    "records-device": {"in", "out"},
    "sides-device": {"nonces", "aad", "lens"},
    "lens-device": {"lens"},
}
P_N, P_LEN, P_IN, P_OUT, P_FORGED = 5, 45, 64, 96, 3
P_LENS = [45, 0, 17, 32, 45]


@pytest.mark.parametrize("bits", ALL_BITS)
@pytest.mark.parametrize("variable", [False, True], ids=["fixed", "v"])
@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_placement_through_the_synchronous_calls(orc, placement, variable, bits):
    on = PLACEMENTS[placement]
    rng = random.Random(bits + len(placement))
    lens = P_LENS if variable else [P_LEN] * P_N
    nonces, aads = [rng.randbytes(12) for _ in lens], [rng.randbytes(AAD_EACH) for _ in lens]
    texts = [rng.randbytes(m) for m in lens]
    want = [orc.gcm_encrypt(key_of(bits), nonces[r], aads[r], texts[r]) for r in range(P_N)]
    case = case_of(AAD_EACH, P_LEN, P_N) + (placement,)
    # device arrays at odd addresses where the call takes them (the records: a multiple of 16, as the strides)
    dn, da = Mem(b"".join(nonces), "nonces" in on, 1), Mem(slots(aads, 16), "aad" in on, 3)
    dl = Mem(u32s(lens), "lens" in on, 4) if variable else None
    before = bytes([FILL]) * (P_N * P_OUT)

    plain = slots(texts, P_IN)
    src, dst = Mem(plain, "in" in on, 16), Mem(before, "out" in on, 16)
    assert call(bits, 0, P_N, dn, da, AAD_EACH, 16, src, dl, P_LEN, P_IN, dst, P_OUT) == 0, case
    check_slots(dst.get(), before, P_OUT, want, [P_LEN + 16] * P_N, "encrypt", case, lens)
    assert dst.intact() and src.get() == plain and dn.intact() and da.intact(), case

    for forged in (False, True):
        cts = list(want)
        if forged:
            cts[P_FORGED] = flip(cts[P_FORGED], 8 * lens[P_FORGED] + 77)
        heads = [None if forged and r == P_FORGED else texts[r] for r in range(P_N)]
        for with_verdicts in (True, False):
            src, dst = Mem(slots(cts, P_IN), "in" in on, 16), Mem(before, "out" in on, 16)
            ver = Mem(size=P_N, fill=7) if with_verdicts else None
            rc = call(bits, 1, P_N, dn, da, AAD_EACH, 16, src, dl, P_LEN, P_IN, dst, P_OUT, ver)
            what = "decrypt%s%s" % (", one forged" if forged else "", "" if with_verdicts else ", no verdicts")
            assert rc == (E_AUTH if forged else 0), case + (what,)
            check_slots(dst.get(), before, P_OUT, heads, [P_LEN] * P_N, what, case, lens)
            assert dst.intact(), case + (what,)
            if ver:
                assert ver.get() == bytes(E_AUTH if forged and r == P_FORGED else 0 for r in range(P_N)) and ver.intact(), case


@pytest.mark.parametrize("bits", ALL_BITS)
def test_fixed_records_in_place_on_the_host(orc, bits):
    rng = random.Random(bits)
    nonces, aad = [rng.randbytes(12) for _ in range(P_N)], rng.randbytes(33)
    texts = [rng.randbytes(P_LEN) for _ in range(P_N)]
    want = [orc.gcm_encrypt(key_of(bits), nonces[r], aad, texts[r]) for r in range(P_N)]
    case, lens = case_of(33, P_LEN, P_N), [P_LEN] * P_N
    dn, da = Mem(b"".join(nonces)), Mem(aad)
    plain = slots(texts, P_IN)
    buf = Mem(plain, False, 16)
    assert call(bits, 0, P_N, dn, da, 33, 0, buf, None, P_LEN, P_IN, buf, P_IN) == 0
    check_slots(buf.get(), plain, P_IN, want, [0] * P_N, "encrypt in place", case, lens)
    assert buf.intact()
    for forged in (False, True):
        cts = list(want)
        if forged:
            cts[P_FORGED] = flip(cts[P_FORGED], 9)
        buf, ver = Mem(slots(cts, P_IN), False, 16), Mem(size=P_N, fill=7)
        assert call(bits, 1, P_N, dn, da, 33, 0, buf, None, P_LEN, P_IN, buf, P_IN, ver) == (E_AUTH if forged else 0)
        heads = [None if forged and r == P_FORGED else texts[r] for r in range(P_N)]
        check_slots(buf.get(), slots(cts, P_IN), P_IN, heads, [0] * P_N, "decrypt in place", case, lens)
        assert buf.intact() and ver.get() == bytes(E_AUTH if forged and r == P_FORGED else 0 for r in range(P_N))


# ---- 6. an in-place _v encrypt on the host leaves no earlier call's bytes ----------------------------------------------------
@pytest.mark.parametrize("short", ["last", "first", "middle"])
def test_in_place_v_encrypt_leaves_no_earlier_bytes(orc, short):
    """The synchronous calls stage the records in a per-thread buffer that the next call uses again.  An in-place
    encryption writes its output into the staged input and copies max_len + 16 bytes of every slot back: whatever the
    call did not write itself -- the sixteen bytes behind max_len of the last slot when the last record is short -- must
    not be what an earlier call staged there."""
    bits, nrec, max_len, stride = 128, 6, 1024, 1040
    marker = b"\xA5SECRET\x5A" * (stride // 8)                # a whole slot of it: the bytes behind a record as well
    rng = random.Random(6)
    nonces = [rng.randbytes(12) for _ in range(nrec + 1)]
    dn = Mem(b"".join(nonces))
    # a longer batch of the marker, not in place: what the caller had in its slots stays in the input staging
    src, dst = Mem(slots([marker] * (nrec + 1), stride)), Mem(size=(nrec + 1) * stride)
    assert call(bits, 0, nrec + 1, dn, None, 0, 0, src, None, max_len, stride, dst, stride) == 0
    lens = [max_len] * nrec
    lens[{"last": nrec - 1, "first": 0, "middle": 3}[short]] = 5
    texts = [rng.randbytes(m) for m in lens]
    plain = slots(texts, stride)
    buf = Mem(plain, False, 16)
    assert call(bits, 0, nrec, dn, None, 0, 0, buf, Mem(u32s(lens)), max_len, stride, buf, stride) == 0
    want = [orc.gcm_encrypt(key_of(bits), nonces[r], b"", texts[r]) for r in range(nrec)]
    case = case_of(0, max_len, nrec)
    after = buf.get()
    check_slots(after, plain, stride, want, [max_len + 16] * nrec, "encrypt_records_v in place", case, lens)
    assert b"SECRET" not in buf.raw(), "an earlier call's plaintext in the caller's buffer: %r" % (case + (short,),)
    assert buf.intact()


# ---- 7. AAD-only records and the limits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", ALL_BITS)
@pytest.mark.parametrize("aad_len", [1, 16, 17, 1008, 16 * 2045])
def test_aad_only_records(orc, aad_len, bits):
    """rec_len == 0: a batch of GMACs; 16 * 2045 bytes of AAD are nv == 2046 positions, the most there are"""
    S, steps = GC.arrangement(aad_len, 0)
    assert (S, steps) == {1008: (64, 2), 16 * 2045: (1024, 2)}.get(aad_len, (64, 1)) and GC.positions(aad_len, 0) <= GC.MAXNV
    nrec = GC.groups(S) + 2
    rng = random.Random(aad_len + bits)
    key, k = key_of(bits), gkey(bits)
    nonces, lens = [rng.randbytes(12) for _ in range(nrec)], [0] * nrec
    case = case_of(aad_len, 0, nrec)
    for each in (False, True):
        aads = [rng.randbytes(aad_len) for _ in range(nrec)] if each else rng.randbytes(aad_len)
        want = [orc.gcm_encrypt(key, nonces[r], aads[r] if each else aads, b"") for r in range(nrec)]
        forged = list(want)
        forged[nrec - 2] = flip(want[nrec - 2], 100)
        verdicts = [0] * (nrec - 2) + [E_AUTH, 0]
        check_records(k.encrypt_records(nonces, aads, [b""] * nrec), want, "encrypt_records (each: %r)" % each, case, lens)
        check_records(k.encrypt_records_v(nonces, aads, [b""] * nrec, max_len=0), want, "encrypt_records_v (each: %r)" % each, case, lens)
        assert k.decrypt_records(nonces, aads, want) == (0, [0] * nrec, [b""] * nrec), case
        assert k.decrypt_records_v(nonces, aads, want, max_len=0) == (0, [0] * nrec, [b""] * nrec), case
        assert k.decrypt_records(nonces, aads, forged) == (E_AUTH, verdicts, [b""] * nrec), case
        assert k.decrypt_records_v(nonces, aads, forged, max_len=0) == (E_AUTH, verdicts, [b""] * nrec), case


def refused(decrypt, v, dev, nrec=2, rec_len=32, aad_len=AAD_EACH, aad_stride=AAD_EACH, in_stride=None, out_stride=None,
            lens="good", status=True, room=None):
    """the call returns UAES_E_ARG and has written nothing: output, verdicts and status as they were, guards intact"""
    in_stride = r16(rec_len + 16) if in_stride is None else in_stride
    out_stride = r16(rec_len + 16) if out_stride is None else out_stride
    room = nrec * r16(rec_len + 16) if room is None else room
    dn, da = Mem(size=12 * nrec, device=dev), Mem(size=max(aad_len, aad_stride) * nrec, device=dev)
    src, dst, ver = Mem(size=room, device=dev, off=16), Mem(size=room, device=dev, off=16), Mem(size=nrec, fill=7, device=dev)
    st = status_mem() if dev and decrypt and status else None
    dl = None
    if v and lens is not None:
        dl = Mem(u32s([rec_len + 1 if lens == "long" and r == nrec - 1 else rec_len for r in range(nrec)]), dev)
    rc = call(128, decrypt, nrec, dn, da, aad_len, aad_stride, src, dl, rec_len, in_stride, dst, out_stride, ver, st, dev=dev, v=v)
    what = (decrypt, v, dev, nrec, rec_len, aad_len, aad_stride, in_stride, out_stride, lens, status)
    assert rc == E_ARG, (rc,) + what
    assert dst.get() == bytes([FILL]) * room and dst.intact() and ver.get() == bytes([7]) * nrec and ver.intact(), what
    assert st is None or (status_of(st) == 0x55555555 and st.intact()), what


ALL_CALLS = [(d, v, dev) for d in (0, 1) for v in (False, True) for dev in (False, True)]


def test_argument_errors_write_nothing():
    for d, v, dev in ALL_CALLS:
        # one AAD block more than fits beside an empty record
        refused(d, v, dev, nrec=1, rec_len=0, aad_len=16 * 2045 + 1, aad_stride=0)
        for a in (0, 17, 16 * 2044):
            refused(d, v, dev, nrec=1, rec_len=GC.record_max(a) + 1, aad_len=a, aad_stride=0)
        refused(d, v, dev, in_stride=72, out_stride=72, room=160)
        refused(d, v, dev, in_stride=48, out_stride=56, room=160)
        refused(d, v, dev, nrec=1, in_stride=(1 << 22) + 16, out_stride=(1 << 22) + 16)
        refused(d, v, dev, nrec=1, in_stride=48, out_stride=(1 << 22) + 16)
    for d in (0, 1):
        refused(d, True, True, lens=None)                     # NULL lens in the _v_dev calls
        refused(d, True, False, lens=None)
        refused(d, True, False, lens="long")                  # a host lens[r] above max_len
        for v in (False, True):
            refused(d, v, False, aad_stride=AAD_EACH - 1)     # an AAD stride shorter than the AAD
    for v in (False, True):
        refused(1, v, True, status=False)                     # NULL d_status in the decrypting _dev calls


def test_no_records_is_no_work():
    for d, v, dev in ALL_CALLS:
        assert call(128, d, 0, None, None, 0, 0, None, None, 0, 0, None, 0, dev=dev, v=v) == 0, (d, v, dev)
        assert call(128, d, 0, None, None, 13, 13, None, None, 32, 48, None, 48, dev=dev, v=v) == 0, (d, v, dev)
