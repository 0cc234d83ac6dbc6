"""GCM and GCM-SIV at CHOSEN starting counters, in every arrangement and direction.

Where a GCM text's head, groups of 256 counters and stripes fall depends on the low byte c0 of its first counter
(J0 + 1), and a 12-byte nonce always gives c0 = 2.  Here the nonce is 16 or 60 bytes (some 17 / 4096 / 70 000) and
solved for a chosen J0 (tests/counters.py): c0 = 0, 1, 0x80, 0xff, a carry into byte 11 at a chosen block (first
block, first group boundary, first and last round of stripes or chunk units, blocks behind the stripes, byte tail),
counter bits 40..47 moving inside the text (no striped launch may take it), the 2^56 wrap with byte 8 = 0xff, and a
random J0.  Each case runs encryption, the tag-first decryption (N7), the one-pass decryption and a 12-byte tag (the
tag-only direction), on host and device pointers, against GCM by its definition at that J0 (counters.gcm_expect, the
same as the oracle's GCM: tests/test_counter_helpers.py).  The arrangement is asserted from uaes.plan(..., counter=J0)
before each run.  GCM-SIV's counter wraps mod 2^32 in bytes 0..3 of the tag: plaintexts are solved for tags that put
the wrap at chosen blocks of siv.small, siv.chunks and siv.levels.

Every assertion message carries (bits, nonce_len, J0 hex, n, arrangement, direction).
"""
import ctypes as C
import os
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import micro_aes_amd as uaes
from tests import counters as K
from tests.test_gpu_plan import around, boundaries

pytestmark = pytest.mark.gpu

MIB = 1 << 20
ORACLE_CAP = 10 * MIB                # boundaries checked in full up to here (the CPU oracle is the slow part)
POOL = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))   # the oracle's ctypes calls release the GIL


def _ids(*names):
    m = 0
    for n in names:
        m |= 1 << uaes.arrangement_id(n)
    return m


def _t(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0") if len(b) else torch.empty(1, dtype=torch.uint8, device="cuda:0")


def _bytes(t, n):
    return bytes(t[:n].cpu().numpy()) if n else b""


def _dev_encrypt(key, nonce, aad, src, n, dst):
    import torch
    rc = uaes.engine().uaes_gcm_encrypt_ex(len(key) * 8, uaes._in(key), uaes._in(nonce), len(nonce), 16, uaes._in(aad),
                                           len(aad), C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()))
    torch.cuda.synchronize()
    return rc


def _dev_decrypt(key, nonce, aad, src, n, dst, tag_len=16):
    import torch
    rc = uaes.engine().uaes_gcm_decrypt_ex(len(key) * 8, uaes._in(key), uaes._in(nonce), len(nonce), tag_len, uaes._in(aad),
                                           len(aad), C.c_void_p(src.data_ptr()), n, C.c_void_p(dst.data_ptr()))
    torch.cuda.synchronize()
    return rc


def _untouched_or_zeroed(back, direction):
    """after a forged tag (N7): the tag-first decryption never wrote the output; the one-pass decryption (opted in)
    either did not write it either (one workgroup) or zeroed what it wrote"""
    untouched = int((back != 0xCC).sum()) == 0
    return untouched or (direction == 2 and int((back != 0).sum()) == 0)


def _what(key, nonce, j0, n, arr, direction, name=""):
    return (len(key) * 8, len(nonce), j0.hex(), n, arr, direction, name)


def _plan(n, alen, direction, j0):
    return uaes.plan("gcm", n, alen, direction, counter=j0)[0]


def run_gcm_case(orc, key, nonce, j0, aad, pt, want, ran, name="", dev=True, forge=False):
    """encrypt (host, device), tag-first decrypt (device), one-pass decrypt (host; device with the switch), 12-byte tag
    (host) -- each direction's arrangement from the plan, recorded in `ran`"""
    import torch
    L = uaes.engine()
    n, alen = len(pt), len(aad)
    arr = {d: _plan(n, alen, d, j0) for d in (0, 1, 2, 3)}
    for d in arr:
        ran.add((arr[d], d))
    assert uaes.AES_GCM_encrypt(key, nonce, aad, pt) == want, _what(key, nonce, j0, n, arr[0], 0, name)
    assert uaes.AES_GCM_decrypt(key, nonce, aad, want) == (0, pt), _what(key, nonce, j0, n, arr[2], 2, name)
    assert uaes.AES_GCM_decrypt(key, nonce, aad, want[:n + 12], tag_len=12) == (0, pt), _what(key, nonce, j0, n, arr[3], 3, name)
    if dev:
        src, ct = _t(pt), torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
        assert _dev_encrypt(key, nonce, aad, src, n, ct) == 0
        assert _bytes(ct, n + 16) == want, _what(key, nonce, j0, n, arr[0], 0, name + " dev")
        back = torch.full((max(n, 1),), 0xCC, dtype=torch.uint8, device="cuda:0")
        for one_pass, d in ((0, 1), (1, 2)):
            L.uaes_set_gcm_one_pass_decrypt(one_pass)
            try:
                back.fill_(0xCC)
                assert _dev_decrypt(key, nonce, aad, ct, n, back) == 0, _what(key, nonce, j0, n, arr[d], d, name + " dev")
                assert _bytes(back, n) == pt, _what(key, nonce, j0, n, arr[d], d, name + " dev")
                if forge:
                    ct[n + 5] ^= 0x40
                    back.fill_(0xCC)
                    assert _dev_decrypt(key, nonce, aad, ct, n, back) == 0x1A, _what(key, nonce, j0, n, arr[d], d, "forged")
                    assert _untouched_or_zeroed(back, d), _what(key, nonce, j0, n, arr[d], d, "forged: output released")
                    ct[n + 5] ^= 0x40
            finally:
                L.uaes_set_gcm_one_pass_decrypt(0)
        back.fill_(0xCC)
        assert _dev_decrypt(key, nonce, aad, ct, n, back, tag_len=12) == 0, _what(key, nonce, j0, n, arr[3], 3, name + " dev")
        assert _bytes(back, n) == pt, _what(key, nonce, j0, n, arr[3], 3, name + " dev")
        del src, ct, back
    if forge:
        bad = bytearray(want)
        bad[n // 2 if n else -1] ^= 1
        assert uaes.AES_GCM_decrypt(key, nonce, aad, bytes(bad), prefill=0xCC) == (0x1A, b"\xcc" * n), \
            _what(key, nonce, j0, n, arr[2], 2, "forged")
    return arr


def _cases(orc, key, aad, n, targets, seed):
    """[(name, j0, nonce, pt, future of the expected ciphertext || tag)]"""
    rnd = random.Random(seed)
    pt = orc.splitmix(seed, n)
    out = []
    for k, (name, v, b8) in enumerate(targets):
        j0 = K.j0_bytes(rnd.randbytes(8) + bytes([b8]), v)
        nonce = K.gcm_nonce_for_j0(orc, key, j0, 60 if k % 4 == 3 else 16, seed=seed)
        out.append((name, j0, nonce, pt, POOL.submit(K.gcm_expect, orc, key, j0, aad, pt)))
    return out


# (arrangement for an encryption, mask of arrangements switched off, n) -- the chunk sizes double as the ones of the
# one-pass decryption's two-launch chunks form and of the tag-first decryption's chunks + CTR
SCENARIOS = [("gcm.small", 0, 20000 + 5),
             ("gcm.chunks", 0, 2 * MIB + 5),
             ("gcm.levels", "gcm.chunks", 100 * 1024 + 5),
             ("gcm.twophase", 0, 17 * MIB + 5),
             ("gcm.striped", "gcm.chunks", 9 * MIB + 5),
             ("gcm.levels", "gcm.chunks gcm.striped", 9 * MIB + 5)]


def test_gcm_every_arrangement_at_chosen_counters(orc):
    L = uaes.engine()
    ran = set()
    expect = {}
    try:
        for si, (arr, mask, n) in enumerate(SCENARIOS):
            bits = (128, 256, 192)[si % 3]
            rnd = random.Random(700 + si)
            key, aad = random.Random(bits).randbytes(bits // 8), rnd.randbytes((37, 0, 5)[si % 3])
            L.uaes_debug_plan_disable(_ids(*mask.split()) if mask else 0)
            nfull, rem = n // 16, n % 16
            cus = uaes.plan("gcm", 9 * MIB + 5, 0, 0)[2] if arr == "gcm.striped" else None
            targets = K.gcm_targets(nfull, rem, cus)
            if arr == "gcm.twophase":          # (17 MiB per case: the named c0 forms and the carries at the ends)
                targets = [t for t in targets if t[0] in ("c0=00", "c0=ff", "carry@first-unit", "carry@last-unit",
                                                          "carry@byte-tail", "bits40@middle", "wrap56@middle")]
            key_of = (bits, n, len(aad))
            if key_of not in expect:
                expect[key_of] = _cases(orc, key, aad, n, targets, 710 + si)
            for name, j0, nonce, pt, fut in expect[key_of]:
                got = _plan(n, len(aad), 0, j0)
                if arr == "gcm.striped" and name.startswith(("bits40", "wrap56")):
                    assert got != "gcm.striped", _what(key, nonce, j0, n, got, 0, name)
                else:
                    assert got == arr, _what(key, nonce, j0, n, got, 0, name)
                run_gcm_case(orc, key, nonce, j0, aad, pt, fut.result(), ran, name, dev=True, forge=(name == "random"))
    finally:
        L.uaes_debug_plan_disable(0)
    for want in [("gcm.small", 0), ("gcm.small", 1), ("gcm.small", 2), ("gcm.chunks", 0), ("gcm.chunks", 1),
                 ("gcm.chunks", 2), ("gcm.twophase", 0), ("gcm.twophase", 2), ("gcm.striped", 0), ("gcm.striped", 2),
                 ("gcm.levels", 0), ("gcm.levels", 1), ("gcm.levels", 2), ("gcm.levels", 3)]:
        assert want in ran, (want, sorted(ran))


def test_gcm_boundaries_at_each_c0(orc):
    """every boundary of the encryption's and the tag-first decryption's table, derived with the counter, up to
    ORACLE_CAP: b - 16, b - 3, b, b + 16 for c0 = 0, 1, 0x80, 0xff"""
    ran = set()
    rnd = random.Random(720)
    key = rnd.randbytes(16)
    for c0 in (0, 1, 0x80, 0xff):
        j0 = K.j0_bytes(rnd.randbytes(9), K.v_for_first((rnd.getrandbits(40) << 8) | c0))
        sizes = set()
        for direction in (0, 1):
            found = boundaries(lambda n: (_plan(n, 0, direction, j0), uaes.plan("gcm", n, 0, direction, counter=j0)[3]),
                               0, ORACLE_CAP)
            assert len(found) >= 3, (c0, direction, found)
            for b, _below, _above in found:
                sizes.update(around(b))
        nonce = K.gcm_nonce_for_j0(orc, key, j0, 16)
        data = {n: orc.splitmix(n + c0, n) for n in sizes}
        futs = {n: POOL.submit(K.gcm_expect, orc, key, j0, b"", data[n]) for n in sorted(sizes)}
        for n in sorted(sizes):
            run_gcm_case(orc, key, nonce, j0, b"", data[n], futs[n].result(), ran, "c0=%02x" % c0, dev=n % 3 == 0)


def _striped_only():
    """gcm.chunks and gcm.twophase off: gcm.striped takes a text from its own first size on (n8 >= CUs)"""
    return _ids("gcm.chunks", "gcm.twophase")


def test_gcm_striped_start_moves_with_c0(orc):
    """the boundary that moves with c0: gcm.striped starts at 256 * (8 * CUs + g_lo) - c0 whole blocks, where n8 = CUs
    exactly (c0 = 0: no head and g_lo = 0, the text ends at the last stripe; c0 = 1: a 255-block head).  Derived from
    the plan with the counter for the encryption and the one-pass decryption, b - 16 / b - 3 / b / b + 16 against GCM
    at that J0"""
    L = uaes.engine()
    ran = set()
    rnd = random.Random(725)
    key = rnd.randbytes(16)
    cus = uaes.plan("gcm", 200 * MIB)[2]
    try:
        L.uaes_debug_plan_disable(_striped_only())
        for c0 in (0, 1, 2, 0x80, 0xff):
            j0 = K.j0_bytes(rnd.randbytes(9), K.v_for_first((rnd.getrandbits(40) << 8) | c0))
            want_b = 16 * (256 * (8 * cus + (1 if c0 else 0)) - c0)
            for direction in (0, 2):
                found = [f for f in boundaries(lambda n: _plan(n, 0, direction, j0), 0, ORACLE_CAP) if f[2] == "gcm.striped"]
                assert [f[0] for f in found] == [want_b], (128, 16, j0.hex(), want_b, found, direction)
                assert _plan(want_b, 0, direction, j0) == "gcm.striped" and _plan(want_b - 16, 0, direction, j0) != "gcm.striped"
            nonce = K.gcm_nonce_for_j0(orc, key, j0, 16 if c0 & 1 else 60)
            sizes = around(want_b)
            data = {n: orc.splitmix(n + c0, n) for n in sizes}
            futs = {n: POOL.submit(K.gcm_expect, orc, key, j0, b"", data[n]) for n in sizes}
            for n in sizes:
                run_gcm_case(orc, key, nonce, j0, b"", data[n], futs[n].result(), ran, "striped start c0=%02x" % c0,
                             forge=(n == want_b))
    finally:
        L.uaes_debug_plan_disable(0)
    assert ("gcm.striped", 0) in ran and ("gcm.striped", 2) in ran, sorted(ran)


def test_gcm_striped_aad_limit_at_each_head(orc):
    """gcm_stripes' `ablk + h0 <= Sl` (Sl = 2048 * CUs lanes): the AAD and the head blocks fill the lanes in front of the
    stripes.  At h0 = 255 (c0 = 1) and h0 = 0 (c0 = 0) an AAD of exactly Sl - h0 blocks is striped, one block more is
    not; each against GCM at that J0"""
    rnd = random.Random(727)
    key = rnd.randbytes(32)
    cus = uaes.plan("gcm", 200 * MIB)[2]
    Sl = 2048 * cus
    n = 9 * MIB + 5
    pt = orc.splitmix(727, n)
    cases = []
    for c0, extra in ((1, 0), (1, 1), (0, 0), (0, 1)):
        h0 = (256 - c0) & 255
        ablk = Sl - h0 + extra
        aad = rnd.randbytes(16 * ablk - 7)
        j0 = K.j0_bytes(rnd.randbytes(9), K.v_for_first((rnd.getrandbits(40) << 8) | c0))
        cases.append((c0, extra, aad, j0, POOL.submit(K.gcm_expect, orc, key, j0, aad, pt)))
    L = uaes.engine()
    ran = set()
    try:
        L.uaes_debug_plan_disable(_striped_only())
        for c0, extra, aad, j0, fut in cases:
            nonce = K.gcm_nonce_for_j0(orc, key, j0, 16)
            for direction in (0, 2):
                got = _plan(n, len(aad), direction, j0)
                assert (got == "gcm.striped") == (extra == 0), _what(key, nonce, j0, n, got, direction, "aad %d" % len(aad))
            run_gcm_case(orc, key, nonce, j0, aad, pt, fut.result(), ran, "aad limit c0=%02x +%d" % (c0, extra), dev=False)
    finally:
        L.uaes_debug_plan_disable(0)


def test_gcm_striped_beyond_128_mib_at_c0(orc):
    """one natural gcm.striped encryption per c0 in (0, 1, 0xff), with a carry into byte 11 inside its last round of
    stripes: the ciphertext around the carry and the first / last 64 KiB against the oracle's keystream, the tag
    against the gcm.levels run of the same call and against E(J0) ^ GHASH; both decryptions and a forged tag"""
    import torch
    L = uaes.engine()
    rnd = random.Random(730)
    key = rnd.randbytes(32)
    n = 136 * MIB + 5
    nfull = n // 16
    cus = uaes.plan("gcm", n)[2]
    H = K.gcm_h(orc, key)
    for c0 in (0, 1, 0xff):
        h0, _g, n8, h1 = K.stripe_geometry(c0, nfull, cus)
        carry = h0 + 2048 * cus * ((n8 - 1) // cus) + 256 * 9          # a group start in the last round of stripes
        j0 = K.j0_bytes(rnd.randbytes(9), K.v_carry32_at(carry))
        assert (K.j0_counter(j0) + 1) & 0xff == c0
        nonce = K.gcm_nonce_for_j0(orc, key, j0, 16)
        arr = _plan(n, 0, 0, j0)
        assert arr == "gcm.striped", _what(key, nonce, j0, n, arr, 0)
        src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda:0")
        ct = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
        assert _dev_encrypt(key, nonce, b"", src, n, ct) == 0
        ct_host = _bytes(ct, n + 16)
        tag_fut = POOL.submit(lambda c=ct_host[:n], j=j0: K.xor(orc.encrypt_block(key, j), orc.ghash(H, b"", c)))
        windows = [(0, 1 << 12), (carry - 128, carry + 128), (h1 - 64, min(h1 + 64, nfull)), (nfull - (1 << 12), nfull)]
        src_host = _bytes(src, n)
        for lo, hi in windows:
            a, b = 16 * lo, min(16 * hi, n) if hi < nfull else n
            assert ct_host[a:b] == orc.ctr_xcrypt_at(key, j0, 1 + lo, src_host[a:b]), _what(key, nonce, j0, n, arr, 0, (lo, hi))
        try:
            L.uaes_debug_plan_disable(_ids("gcm.striped"))
            other = _plan(n, 0, 0, j0)
            assert other == "gcm.levels", _what(key, nonce, j0, n, other, 0)
            ct2 = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
            assert _dev_encrypt(key, nonce, b"", src, n, ct2) == 0
            assert torch.equal(ct, ct2), _what(key, nonce, j0, n, other, 0, "striped != levels")
            del ct2
        finally:
            L.uaes_debug_plan_disable(0)
        back = torch.full((n,), 0xCC, dtype=torch.uint8, device="cuda:0")
        for one_pass, d in ((0, 1), (1, 2)):
            L.uaes_set_gcm_one_pass_decrypt(one_pass)
            try:
                back.fill_(0xCC)
                assert _dev_decrypt(key, nonce, b"", ct, n, back) == 0 and torch.equal(back, src), \
                    _what(key, nonce, j0, n, _plan(n, 0, d, j0), d)
                ct[carry * 16 + 3] ^= 4
                back.fill_(0xCC)
                assert _dev_decrypt(key, nonce, b"", ct, n, back) == 0x1A, _what(key, nonce, j0, n, _plan(n, 0, d, j0), d, "forged")
                assert _untouched_or_zeroed(back, d), _what(key, nonce, j0, n, _plan(n, 0, d, j0), d, "forged: output released")
                ct[carry * 16 + 3] ^= 4
            finally:
                L.uaes_set_gcm_one_pass_decrypt(0)
        assert ct_host[n:] == tag_fut.result(), _what(key, nonce, j0, n, arr, 0, "tag vs E(J0) ^ GHASH")
        del src, ct, back


def test_gcmsiv_counter_wraps(orc):
    """the tag's LE32 word wraps at chosen blocks (the first block after the wrap: 1, 2, the middle, the last whole
    block, the byte tail) in siv.small, siv.chunks and siv.levels, both directions against the oracle; and a forged
    tag chosen directly (no solving) whose wrap falls in the middle of a longer text: (rc, text) as the oracle's"""
    L = uaes.engine()
    rnd = random.Random(740)
    for arr, mask, nfull, rem, alen in (("siv.small", 0, 1000, 7, 9), ("siv.chunks", 0, 65536, 5, 0),
                                        ("siv.levels", "siv.chunks", 65536, 11, 40)):
        bits = {"siv.small": 128, "siv.chunks": 256, "siv.levels": 192}[arr]
        key, nonce, aad = rnd.randbytes(bits // 8), rnd.randbytes(12), rnd.randbytes(alen)
        n = 16 * nfull + rem
        try:
            L.uaes_debug_plan_disable(_ids(*mask.split()) if mask else 0)
            assert uaes.plan("siv", n, alen)[0] == arr, (bits, 12, None, n, arr)
            for d in (0, 1):
                assert uaes.plan("siv", n, alen, d)[0] == arr
            for wrap in (1, 2, nfull // 2, nfull - 1, nfull):
                pt = K.siv_message_for_counter(orc, key, nonce, aad, nfull, -wrap, tail=rem, fill="random", seed=wrap)
                want = orc.gcmsiv_encrypt(key, nonce, aad, pt)
                what = (bits, 12, want[-16:].hex(), n, arr, "wrap@%d" % wrap)
                assert int.from_bytes(want[-16:-12], "little") == (-wrap) & 0xffffffff, what
                assert uaes.GCM_SIV_encrypt(key, nonce, aad, pt) == want, what + (0,)
                assert uaes.GCM_SIV_decrypt(key, nonce, aad, want) == (0, pt), what + (1,)
            for n2 in (n, 6 * MIB + 3) if arr != "siv.small" else (n,):
                nb = (n2 + 15) // 16
                tag = ((-(nb // 2)) & 0xffffffff).to_bytes(4, "little") + rnd.randbytes(12)
                ct = rnd.randbytes(n2) + tag
                got = uaes.GCM_SIV_decrypt(key, nonce, aad, ct, prefill=0xCC)
                assert got == orc.gcmsiv_decrypt(key, nonce, aad, ct, prefill=0xCC), (bits, 12, tag.hex(), n2, arr, "forged")
                assert got[0] == 0x1A
        finally:
            L.uaes_debug_plan_disable(0)


def test_key_cache_across_nonce_lengths_and_long_nonces(orc):
    """under one key on one thread: 12-byte nonce calls long enough to turn the key cache on, then 12- and 16-byte
    nonces alternating across small -> chunks -> striped -> small (each 16-byte call redoes the one-shot setup and
    clobbers the cached tables); then nonces of 17, 4096, 70 000 and 600 000 bytes -- the last one is more than GH_DIRECT
    (32768) GHASH positions long, so uaesk_gcm_j0 runs a k_ghash_pass level in front of its last kernel"""
    L = uaes.engine()
    rnd = random.Random(750)
    key = rnd.randbytes(16)
    ran = set()
    for i in range(9):
        nonce, pt = rnd.randbytes(12), rnd.randbytes(300 + i)
        assert uaes.AES_GCM_encrypt(key, nonce, b"a", pt) == orc.gcm_encrypt(key, nonce, b"a", pt), ("warm-up", i)
    try:
        for arr, mask, n in (("gcm.small", 0, 5000 + 3), ("gcm.chunks", 0, MIB + 9), ("gcm.striped", "gcm.chunks", 9 * MIB + 1),
                             ("gcm.small", 0, 7000 + 1)):
            L.uaes_debug_plan_disable(_ids(*mask.split()) if mask else 0)
            pt = orc.splitmix(n, n)
            for nlen in (12, 16, 12, 16, 12):
                if nlen == 12:
                    nonce = rnd.randbytes(12)
                    j0 = nonce + b"\0\0\0\1"
                else:
                    j0 = K.j0_bytes(rnd.randbytes(9), K.v_for_first(rnd.getrandbits(48) << 8))
                    nonce = K.gcm_nonce_for_j0(orc, key, j0, 16)
                assert _plan(n, 3, 0, j0) == arr, _what(key, nonce, j0, n, _plan(n, 3, 0, j0), 0)
                want = K.gcm_expect(orc, key, j0, b"hdr", pt)
                run_gcm_case(orc, key, nonce, j0, b"hdr", pt, want, ran, "cache", dev=False)
    finally:
        L.uaes_debug_plan_disable(0)
    pt = orc.splitmix(3, MIB + 7)
    for nlen in (17, 4096, 70000, 600000):
        j0 = K.j0_bytes(rnd.randbytes(8) + b"\xff", K.v_wrap56_at(nlen))
        nonce = K.gcm_nonce_for_j0(orc, key, j0, nlen)
        run_gcm_case(orc, key, nonce, j0, b"", pt, K.gcm_expect(orc, key, j0, b"", pt), ran, "long nonce", dev=nlen >= 70000)
        nonce = rnd.randbytes(nlen)                  # unsolved: the oracle's own J0
        assert uaes.AES_GCM_encrypt(key, nonce, b"z", pt[:5000]) == orc.gcm_encrypt(key, nonce, b"z", pt[:5000]), nlen
