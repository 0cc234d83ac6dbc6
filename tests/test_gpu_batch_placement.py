"""The row batches with their side outputs in the other kind of memory than their texts: host texts and host side inputs
with the tags / IVs / verdicts in device memory, and the reverse.  EAX, SIV, CCM and key unwrap, five records each,
against the references the neighbouring tests use; one record of every decryption is forged, so the verdicts and the
return code come through the placement under test."""
import random

import pytest

import micro_aes_amd as uaes
from tests import eax_siv_ref as ES
from tests import kw_ref as KW
from tests.guarded_mem import Mem, ptr
from tests.test_gpu_ccm_batch import raw as ccm_raw
from tests.test_gpu_eax_siv import batch as eax_siv_batch

pytestmark = pytest.mark.gpu

N, ML, AL, FORGED = 5, 33, 8, 3
VERDICTS = bytes(0 if m == FORGED else 1 for m in range(N))
_ref = {}


def pointers(args):
    return [ptr(a) for a in args]


def eax_siv_call(*args):
    return eax_siv_batch(*pointers(args))


def ccm_call(decrypt, key, *args):
    """tests/test_gpu_ccm_batch.py's raw(): the arguments from nl on, without verdicts when encrypting"""
    return ccm_raw(decrypt, len(key) * 8, key, *pointers(args), *[None] * (12 - len(args)))


def flip_record(parts, bit):
    """the records joined, with one bit of record FORGED changed"""
    parts = list(parts)
    parts[FORGED] = KW.flip(parts[FORGED], bit)
    return b"".join(parts)


def reference(orc):
    """inputs and expected outputs, made once for both placements"""
    if _ref:
        return _ref
    rng = random.Random(533)
    rb = lambda n: [rng.randbytes(n) for _ in range(N)]
    r = _ref
    r["key"], r["keys"] = rng.randbytes(16), rng.randbytes(32)
    r["texts"], r["aads"], r["nonces16"], r["nonces13"], r["secrets"] = rb(ML), rb(AL), rb(16), rb(13), rb(24)
    eax = ES.eax_encrypt_records(128, r["key"], r["nonces16"], r["aads"], r["texts"])
    r["eax"] = [x[:-16] for x in eax], [x[-16:] for x in eax]
    siv = ES.siv_encrypt_records(128, r["keys"], r["aads"], r["texts"])
    r["siv"] = [c for _, c in siv], [v for v, _ in siv]
    ccm = [orc.ccm_encrypt(r["key"], n, a, t, tag_len=8) for n, a, t in zip(r["nonces13"], r["aads"], r["texts"])]
    r["ccm"] = [x[:ML] for x in ccm], [x[ML:] for x in ccm]
    r["wrapped"] = [KW.wrap(r["key"], s)[1] for s in r["secrets"]]
    return r


@pytest.mark.parametrize("outputs_on_device", [True, False], ids=["host-texts-device-outputs", "device-texts-host-outputs"])
def test_side_outputs_in_the_other_memory(orc, outputs_on_device):
    r = reference(orc)
    od, td = outputs_on_device, not outputs_on_device
    key, aads, texts = r["key"], r["aads"], r["texts"]
    da, plain = Mem(b"".join(aads), td), b"".join(texts)

    def decrypted(dst, forged_text):
        got = dst.get(N * ML)
        return [got[m * ML:(m + 1) * ML] for m in range(N)] == [forged_text if m == FORGED else texts[m] for m in range(N)]

    # EAX: tags out of the encryption, verdicts out of the decryption; a forged record's output stays as it was
    cts, tags = r["eax"]
    dn = Mem(b"".join(r["nonces16"]), td)
    dst, dt = Mem(size=N * ML, device=td), Mem(size=16 * N, device=od)
    assert eax_siv_call(False, False, 128, key, N, ML, dn, 16, da, AL, Mem(plain, td), dst, dt) == 0
    assert dst.get() == b"".join(cts) and dt.get() == b"".join(tags) and dst.intact(N * ML) and dt.intact(16 * N)
    dst, dv = Mem(b"\x77" * (N * ML), td), Mem(size=N, device=od)
    rc = eax_siv_call(False, True, 128, key, N, ML, dn, 16, da, AL, Mem(b"".join(cts), td), dst, Mem(flip_record(tags, 77), td), dv)
    assert rc == 0x1A and dv.get() == VERDICTS and dv.intact(N) and decrypted(dst, b"\x77" * ML) and dst.intact(N * ML)

    # SIV: IVs and verdicts; a forged record is left as the reference leaves it
    cts, ivs = r["siv"]
    dst, dt = Mem(size=N * ML, device=td), Mem(size=16 * N, device=od)
    assert eax_siv_call(True, False, 128, r["keys"], N, ML, None, 0, da, AL, Mem(plain, td), dst, dt) == 0
    assert dst.get() == b"".join(cts) and dt.get() == b"".join(ivs) and dst.intact(N * ML) and dt.intact(16 * N)
    fivs = flip_record(ivs, 41)
    orc_rc, left = ES.siv_decrypt_rc(128, r["keys"], fivs[16 * FORGED:16 * FORGED + 16], aads[FORGED], cts[FORGED])
    assert orc_rc == 0x1A
    dst, dv = Mem(size=N * ML, device=td), Mem(size=N, device=od)
    rc = eax_siv_call(True, True, 128, r["keys"], N, ML, None, 0, da, AL, Mem(b"".join(cts), td), dst, Mem(fivs, td), dv)
    assert rc == 0x1A and dv.get() == VERDICTS and dv.intact(N) and decrypted(dst, left) and dst.intact(N * ML)

    # CCM, 13-byte nonces and 8-byte tags
    cts, tags = r["ccm"]
    dn = Mem(b"".join(r["nonces13"]), td)
    dst, dt = Mem(size=N * ML, device=td), Mem(size=8 * N, device=od)
    assert ccm_call(False, key, 13, 8, N, ML, None, dn, da, AL, Mem(plain, td), dst, dt) == 0
    assert dst.get() == b"".join(cts) and dt.get() == b"".join(tags) and dst.intact(N * ML) and dt.intact(8 * N)
    ftags = flip_record(tags, 13)
    orc_rc, left = orc.ccm_decrypt(key, r["nonces13"][FORGED], aads[FORGED], cts[FORGED] + ftags[8 * FORGED:8 * FORGED + 8], tag_len=8)
    assert orc_rc == 0x1A
    dst, dv = Mem(size=N * ML, device=td), Mem(size=N, device=od)
    rc = ccm_call(True, key, 13, 8, N, ML, None, dn, da, AL, Mem(b"".join(cts), td), dst, Mem(ftags, td), dv)
    assert rc == 0x1A and dv.get() == VERDICTS and dv.intact(N) and decrypted(dst, left) and dst.intact(N * ML)

    # key unwrap, 24-byte secrets
    fw = flip_record(r["wrapped"], 64 + 9)
    orc_rc, left = KW.unwrap(key, fw[32 * FORGED:32 * FORGED + 32])
    assert orc_rc == 0x1A
    src, dst, dv = Mem(fw, td), Mem(size=N * 24, device=td), Mem(size=N, device=od)
    rc = uaes.engine().uaes_kw_unwrap_batch(128, key, N, 32, src.ptr, dst.ptr, dv.ptr)
    got = dst.get()
    assert rc == 0x1A and dv.get() == VERDICTS and dv.intact(N) and dst.intact(N * 24)
    assert [got[24 * m:24 * m + 24] for m in range(N)] == [left if m == FORGED else r["secrets"][m] for m in range(N)]
