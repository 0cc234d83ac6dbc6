"""tests/aead_batch_cases.py without a device: (a) the cases of the five record-batch files are the intended ones, by
count and by a digest of the generated inputs; (b) the reference alone accepts its own records and rejects every forged
part; (c) the frame's checks pass on a stand-in engine made of the reference, and each of them raises when that engine is
broken in the way the check looks for."""
import ctypes as C
import random

import pytest

from tests import aead_batch_cases as F
from tests import test_gpu_ccm_batch, test_gpu_gcm_multikey, test_gpu_gcmsiv_batch, test_gpu_ocb_batch, test_gpu_xaes
from tests.guarded_mem import FILL, GUARD, Mem

FILES = (test_gpu_ccm_batch, test_gpu_ocb_batch, test_gpu_gcmsiv_batch, test_gpu_gcm_multikey, test_gpu_xaes)
MODES = {f.MODE.name: f.MODE for f in FILES}

# ---- (a) the cases ----------------------------------------------------------------------------------------------------
SHORT_COUNTS = {"ccm": (1050, 105, 105), "ocb": (1050, 168, 168), "gcmsiv": (300, 30, 30), "gcm_multikey": (300, 30, 30),
                "xaes256gcm": (6,)}            # shape tuples per parametrized test, by key size
# SHA-256 of the inputs (F.digest) that the five files generated before they ran on the frame
DIGESTS = {
    "ccm": {"short": "a24bb4d5fcba2a2ccb5dce0f808f4e763f88700c5278fb78edc6f22839a0524c",
            "forgery": "cae1e26e8c12edbe66540a8fafba505082c35f6c7d6bfe8b014699c98e934a97",
            "placement": "5b19e6d83298cc85264d1eb7706c41c626e79ac3787bc338173d0268672e4a60",
            "lengths": "1f76c8c989c07b30c53bdfebf5b6ad395e5dc7706e0ca9380a27471189f338d7"},
    "ocb": {"short": "c9f09a5a2fc8388020c4879b0648abdbf88e99ea6f7230a5704461f735ab05f2",
            "forgery": "13fffe21f14879666f927079c2629ba3a0a8e51f970557b29bd93325a9821bf3",
            "placement": "5b19e6d83298cc85264d1eb7706c41c626e79ac3787bc338173d0268672e4a60",
            "lengths": "1f76c8c989c07b30c53bdfebf5b6ad395e5dc7706e0ca9380a27471189f338d7"},
    "gcmsiv": {"short": "2d1c71559cfde37767b98a6fc27532b87633748081093982f1ae5f3a6614614f",
               "forgery": "08b5890ddefdde4dc0d275dc92547481d2b4b78f5b223c7272cc7e93c8f05fa6",
               "placement": "01d99c0b00f88ff15ea1a1fc3308a0e0b4b7f88d430478b144a7824f4d0f46a8",
               "lengths": "fc7200b12f58fd76f7317bfb46ddbbfaaeb40867d56664709ca164291df01543"},
    "gcm_multikey": {"short": "3edcc13ef0f01a8d5604e6ec55dbbc1db738befe6149e71dffd6cc6e0fd018e4",
                     "forgery": "a23cb81095f77a63538546cab3071aaf4f3144320e92e3750286c33175e54ba1",
                     "placement": "725d02fb09f53b774206ae1acb1f13926618a65d7eb348b50479c85fc7a87cfa",
                     "lengths": "8cc8c7c9db64d1e7e1768e111dff9d60e7bb8a22932275cfa615cae70c13f5dc"},
    "xaes256gcm": {"short": "fe40f23bc01c9383e8c3268f6d8ab211ed443633ae4435de2526b11acdf0659e",
                   "forgery": "e25fb8fd4c1d69154f9c2b4500fd1c94be593dc8012f6b480c1c9182162466e5",
                   "placement": "063a7ad3fdc4c1400cf1345767117af2f606ccbfbedc06069f19cf5d53703aaf",
                   "lengths": "7df97bd720f208567ade7b0cd63cd7095f7de478899720213dc346755f97c789"},
}


@pytest.mark.parametrize("name", MODES)
def test_the_short_shapes_are_the_intended_ones(name):
    mode = MODES[name]
    assert tuple(len(mode.short_shapes(bits)) for bits in mode.key_bits) == SHORT_COUNTS[name]
    cases = [c for bits in mode.key_bits for nl in mode.short_nls for c in F.short_cases(mode, bits, nl)]
    assert len(cases) == len(mode.short_nls) * sum(SHORT_COUNTS[name])
    assert F.digest(cases) == DIGESTS[name]["short"]


@pytest.mark.parametrize("name", MODES)
def test_the_forgery_placement_and_length_cases_are_the_intended_ones(name):
    mode = MODES[name]
    assert F.digest([F.forgery(mode, part).case for part in mode.forgery_parts]) == DIGESTS[name]["forgery"]
    assert F.digest([F.placement_case(mode, off) for off in mode.placement_offsets]) == DIGESTS[name]["placement"]
    assert F.digest([F.lengths_case(mode)]) == DIGESTS[name]["lengths"]


def test_modes_say_what_they_are():
    assert [m.arrangement for m in MODES.values()] == ["ccm.batch", "ocb.batch", "gcmsiv.batch", "gcm.multikey", "xaes.gcm"]
    assert [m.per_record_keys for m in MODES.values()] == [False, False, False, True, False]
    assert [m.count_sampled for m in MODES.values()] == [False, False, True, True, True]
    assert [len(F.places(m)) for m in MODES.values()] == [12, 12, 12, 14, 12]
    assert F.place_id(MODES["gcm_multikey"], 1) == "keys" and F.place_id(MODES["gcmsiv"], 1) == "nonces" and F.place_id(MODES["ocb"], 0) == "host"


@pytest.mark.parametrize("name", MODES)
def test_every_record_of_a_count_case_has_its_own_nonce_and_key(name):
    """count_case asserts it; the plan answers here for a 256-CU MI355X"""
    mode, module = MODES[name], FILES[list(MODES).index(name)]
    for dec in (False, True):
        assert mode.plan(16, 1 << 20, dec)[0] == mode.arrangement
    for nmsg in module.COUNTS + (F.second_pass(mode),):
        assert len(F.count_case(mode, nmsg)[0].texts) == nmsg


# ---- (b) the reference alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODES)
def test_the_reference_accepts_its_own_records_and_rejects_every_forged_part(name):
    mode = MODES[name]
    c, _ = F.forgery_case(mode)
    texts, (cts, tags) = F.cut(c), F.expected(mode, c)
    for m in range(len(texts)):
        assert mode.dec(F.key_of(mode, c, m), c.nonces[m], c.aads[m], cts[m] + tags[m], c.tl) == (0, texts[m])
    whats = set()
    for part in mode.forgery_parts:
        f = F.forgery(mode, part)
        changed = [k for k in ("key", "nonces", "aads") if getattr(f.case, k) != getattr(c, k)] + \
                  [k for k, a, b in (("cts", f.cts, cts), ("tags", f.tags, tags)) if a != b]
        assert len(changed) == 1, (part, changed)
        whats.add(changed[0])
        assert mode.dec(F.key_of(mode, f.case, f.m), f.case.nonces[f.m], f.case.aads[f.m], f.cts[f.m] + f.tags[f.m], c.tl)[0] == F.E_AUTH
    assert whats == {"nonces", "aads", "cts", "tags"} | ({"key"} if mode.per_record_keys else set())


# ---- (c) the checks can fail ------------------------------------------------------------------------------------------
class StandIn:
    """an engine made of the mode's reference, over the wrapper's lists and over raw pointers into host memory (Mem,
    bytes or None); `broken` names the one thing it does wrong"""

    def __init__(self, mode, broken=None):
        self.ref, self.broken, self.wipe = mode, broken, 0
        self.mode = mode._replace(wrapper=self.wrapper, raw=self.raw, wipe_switch=self.wipe_switch)

    def wipe_switch(self, on):
        self.wipe = on

    def records(self, decrypt, keys, nonces, aads, slots, lens, tags, tl, outs):
        """the records one by one into outs (bytearrays): (code, tags or verdicts)"""
        rc, res = 0, []
        for m, slot in enumerate(slots):
            k = len(slot) if lens is None else min(lens[m], len(slot))
            if not decrypt:
                ct = self.ref.enc(keys[m], nonces[m], aads[m], slot[:k], tl)
                outs[m][:k] = ct[:k]
                res.append(ct[k:])
                continue
            code, text = self.ref.dec(keys[m], nonces[m], aads[m], slot[:k] + tags[m], tl)
            res.append(int(code == 0))
            if code == 0:
                outs[m][:k] = text
            else:
                rc = F.E_AUTH
                left = {"released": text, "zeros": bytes(k), "untouched": outs[m][:k]}[self.ref.forged[self.wipe]]
                outs[m][:k] = left
                if self.broken == "verdict":
                    rc, res[m] = 0, 1
        if not decrypt and self.broken == "ciphertext":
            outs[1][0] ^= 0x10
        if not decrypt and self.broken == "tag":
            res[0] = F.flip(res[0], 3)
        if self.broken == "beyond lens" and lens is not None:
            m = [len(s) > k for s, k in zip(slots, lens)].index(True)
            outs[m][min(lens[m], len(slots[m]))] ^= 0xFF
        return rc, res

    def wrapper(self, key, nonces, aads, texts, tag_len=16, decrypt=False, tags=None, prefill=0, lens=None):
        n = len(texts)
        keys = key if self.ref.per_record_keys else [key] * n
        outs = [bytearray([prefill]) * len(t) for t in texts]
        rc, res = self.records(decrypt, keys, nonces, aads, texts, lens, tags, tag_len, outs)
        return (rc, [bytes(o) for o in outs], res) if decrypt else ([bytes(o) for o in outs], res)

    def raw(self, decrypt, bits, key, nl, tl, nmsg, ml, lens, nonces, aads, al, src, dst, tags, verdicts):
        def read(p, size):
            return bytes(p[:size]) if isinstance(p, bytes) else C.string_at(p, size)

        def split(p, size):
            return [read(p, nmsg * size)[m * size:(m + 1) * size] for m in range(nmsg)] if size else [b""] * nmsg
        keys = split(key, bits // 8) if self.ref.per_record_keys else [key] * nmsg
        lv = None if lens is None else [int.from_bytes(x, "little") for x in split(lens, 4)]
        outs = [bytearray(x) for x in split(dst, ml)]
        rc, res = self.records(decrypt, keys, split(nonces, nl), split(aads, al), split(src, ml), lv,
                               split(tags, tl) if decrypt else None, tl, outs)
        C.memmove(dst, bytes(b"".join(outs)), nmsg * ml)
        if decrypt:
            C.memmove(verdicts, bytes(res), nmsg)
        else:
            C.memmove(tags, b"".join(res), nmsg * tl)
        if self.broken == "past the output":
            C.memmove(dst.value + nmsg * ml, b"\0", 1)
        if self.broken == "before the output":
            C.memmove(dst.value - 1, b"\0", 1)
        return rc


def all_checks(mode):
    """what the frame checks with no device in it: {check: a call of it}"""
    n, tl, al, ml, lens = mode.short_shapes(mode.key_bits[0])[-1]
    c = F.draw(mode, random.Random(1), mode.key_bits[0], n, mode.short_nls[0], al, ml, tl, lens)
    forgeries = [F.forgery(mode, part) for part in mode.forgery_parts]
    return {
        "check_both": lambda: F.check_both(mode, c, "stand-in"),
        "check_forgery": lambda: [F.check_forgery(mode, f, in_place, device=False) for f in forgeries for in_place in (False, True)],
        "check_lengths": lambda: F.check_lengths(mode, F.lengths_case(mode), False, False),
        "check_placement": lambda: [F.check_placement(mode, F.placement_case(mode, off), 0, off) for off in mode.placement_offsets],
    }


@pytest.mark.parametrize("name", MODES)
def test_the_checks_pass_on_the_stand_in(name):
    for check in all_checks(StandIn(MODES[name]).mode).values():
        check()
    F.check_count(StandIn(MODES[name]).mode, 65)
    F.check_two_threads(StandIn(MODES[name]).mode, {1: F.short_cases(MODES[name], MODES[name].key_bits[-1], MODES[name].short_nls[0])[:7]})


SABOTAGE = {"ciphertext": "check_both", "tag": "check_both", "verdict": "check_forgery", "beyond lens": "check_lengths",
            "past the output": "check_placement", "before the output": "check_placement"}


@pytest.mark.parametrize("broken", SABOTAGE)
@pytest.mark.parametrize("name", ["ccm", "gcm_multikey"])
def test_a_broken_stand_in_fails_the_check_that_looks_for_it(name, broken):
    checks = all_checks(StandIn(MODES[name], broken).mode)
    with pytest.raises(AssertionError):
        checks[SABOTAGE[broken]]()


def test_a_byte_before_an_aligned_output_is_seen():
    """offset 0: the byte in front of the buffer is a guard byte of its own"""
    m = Mem(size=8)
    assert m.intact() and m.intact(0) and m.get() == bytes([FILL]) * 8
    C.memmove(m.ptr.value - 1, b"\0", 1)
    assert not m.intact() and not m.intact(8) and m.raw()[m.at - 1] == 0 and m.raw()[m.at - 2] == GUARD
    m = Mem(b"ab", size=4, fill=7)
    assert m.intact(2) and m.get() == b"ab\7\7"
    C.memmove(m.ptr.value + 3, b"\0", 1)
    assert m.intact() and m.intact(4) and not m.intact(3) and not m.intact(2)
