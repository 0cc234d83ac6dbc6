"""The CBC / CFB / OFB / CMAC / CCM / batch rows of csrc/uaes_plan.h without a device (uaes_debug_plan_chain answers for
a 256-CU MI355X then), and the helpers tests/test_gpu_chains.py takes its cases from."""

import micro_aes_amd as uaes
from tests import chain_cases as K

MIB = K.MIB


def test_the_chain_rows_restate_the_launchers_constants():
    """the boundaries for 256 CUs are the constants the launchers held before the rows existed: 8 MiB of parallel
    blocks (fb-dec), 256 B (CCM), 8192 messages (workgroup shape) and 81 919 messages (row -> lane)"""
    b, (g1, tile1), (g4, tile4), full = K.fbdec_marks()
    assert (b, g1, tile1, g4, tile4, full) == (8 * MIB, 4 * MIB, 16 * 1024, 16 * MIB, 16 * 4096, 256)
    for mode, tail in (("cbc", 0), ("cbc", 1), ("cbc", 15), ("cbc_nocts", 0), ("cfb", 0), ("cfb", 15)):
        for p in (16, b - 16, b, b + 16, g1, g1 + 16, g4, g4 + 16, 3 * g4):
            n = K.fbdec_len(mode, tail, p)
            assert uaes.chain_plan(mode, n, decrypt=True) == uaes.chain_plan("cfb", p, decrypt=True), (mode, tail, p)
    assert uaes.chain_plan("cfb", 5, decrypt=True) == ("fbdec.single", 1, 1, 1024)          # no whole block: the tail's lane
    assert uaes.chain_plan("cbc", 16, decrypt=True)[:3] == uaes.chain_plan("cbc", 31, decrypt=True)[:3] == ("fbdec.single", 1, 1)
    assert K.ccm_fused_max() == 256
    assert uaes.chain_plan("ccm", 257)[1] == 1 + uaes.plan("ctr", 257)[1] and uaes.chain_plan("ccm", 64 * MIB)[1] == 1 + uaes.plan("ctr", 64 * MIB)[1]
    for what in ("cbc", "cfb", "ofb", "cmac", "cbc_nocts"):
        for n in (16, 300, 64 * MIB):
            assert uaes.chain_plan(what, n) == ("chain.serial", 1, 1, 64), (what, n)
    assert uaes.chain_plan("ofb", 64 * MIB, decrypt=True) == ("chain.serial", 1, 1, 64)
    marks = K.batch_marks()
    assert [k for k, _ in marks] == [4097, 8193, 16385, 81920, 262145], marks
    assert "batch.row/256 -> batch.row/256 strided" in marks[0][1] and "batch.row/256 strided -> batch.row/1024" in marks[1][1]
    assert "batch.row/1024 strided -> batch.lane/1024" in marks[3][1] and marks[4][1].endswith("batch.lane/1024 strided")
    for what in ("cbc_batch", "cmac_batch"):
        assert uaes.chain_plan(what, 16, 8192) == ("batch.row", 1, 256, 256) and uaes.chain_plan(what, 16, 8193) == ("batch.row", 1, 129, 1024)
        assert uaes.chain_plan(what, 16, 81919) == ("batch.row", 1, 256, 1024) and uaes.chain_plan(what, 16, 81920) == ("batch.lane", 1, 80, 1024)
        assert uaes.chain_plan(what, 16, 1) == ("batch.row", 1, 1, 256) and uaes.chain_plan(what, 16, 1 << 24) == ("batch.lane", 1, 256, 1024)
    # arguments that make no sense have no plan
    hook = uaes.engine().uaes_debug_plan_chain
    for what, direction, a in ((8, 0, 16), (-1, 0, 16), (0, 2, 16), (0, 1, 15), (0, 0, 15), (7, 1, 17), (5, 0, 24), (5, 0, 0),
                               (5, 1, 16), (6, 1, 16), (3, 1, 16)):
        assert hook(what, direction, a, 4, None) is None, (what, direction, a)
    assert hook(4, 1, 100, 0, None) == b"ccm.fused"


def test_the_piecewise_oracle_is_the_oracle(orc):
    """tests/chain_cases.py oracle_decrypt (pieces on a thread pool) == the oracle's one call, for every mode and tail
    the GPU tests use, at a size of several pieces that is no multiple of the piece"""
    key, iv = bytes(range(40, 56)), bytes(range(200, 216))
    base = 5 * K.PIECE // 2 + 48
    data = orc.splitmix(77, base + 32)
    for mode, tails, ref in (("cbc", (0, 1, 7, 15), lambda d: orc.cbc(key, iv, d, False)[1]),
                             ("cbc_nocts", (0,), lambda d: orc.cbc_nocts(key, iv, d, False)[1]),
                             ("cfb", (0, 1, 15), lambda d: orc.cfb(key, iv, d, False))):
        for tail in tails:
            d = data[:K.fbdec_len(mode, tail, base)]
            assert K.oracle_decrypt(orc, mode, key, iv, d) == ref(d), (mode, tail)
        for n in (16, 17, 32, 33, 2 * K.PIECE, 2 * K.PIECE + 16):
            if mode == "cbc_nocts" and n % 16:
                continue
            assert K.oracle_decrypt(orc, mode, key, iv, data[:n]) == ref(data[:n]), (mode, n)


def test_batch_samples_cover_the_ends_and_every_pass():
    for nmsg in (81919, 81920, 262145):
        plan = uaes.chain_plan("cbc_batch", 16, nmsg)
        s = K.batch_samples(nmsg, plan)
        per_pass = plan[2] * K.batch_rows(plan)
        assert 2048 <= len(s) == len(set(s)) and s[0] == 0 and s[-1] == nmsg - 1 and set(range(64)) <= set(s)
        assert set(range(nmsg - 64, nmsg)) <= set(s)
        for k in range(1, nmsg // per_pass + 1):
            assert {k * per_pass - 1, k * per_pass, k * per_pass + 1} & set(range(nmsg)) <= set(s), (nmsg, k)
    assert K.batch_samples(100, uaes.chain_plan("cbc_batch", 16, 100)) == list(range(100))


def test_every_row_batch_takes_one_launch_shape():
    """the row batches (CBC / CMAC up to 81 919 messages, CCM, key wrap, FF1, EAX / SIV) answer with the same grid
    and, where the hook reports them, the same threads per workgroup, at every number of records; the values are
    those for 256 CUs"""
    pinned = {1: (1, 256), 64: (4, 256), 65: (5, 256), 4096: (256, 256), 8192: (256, 256), 8193: (129, 1024),
              16384: (256, 1024), 81919: (256, 1024), 1 << 24: (256, 1024)}
    for n in (1, 2, 63, 64, 65, 4096, 4097, 8192, 8193, 16384, 16385, 81919, 81920, 1 << 20, 1 << 24):
        shapes = {("ccm_batch", d): uaes.chain_plan("ccm_batch", 16, n, decrypt=d)[2:] for d in (False, True)}
        shapes.update({("kw", d): uaes.kw_plan(16, n, unwrap=d)[2:] for d in (False, True)})
        shapes["ff1"] = uaes.ff1_plan(6, n)[2:]
        if n <= 81919:
            shapes.update({what: uaes.chain_plan(what, 16, n)[2:] for what in ("cbc_batch", "cmac_batch")})
        assert len(set(shapes.values())) == 1, (n, shapes)
        shape = shapes["ff1"]
        if n >= 2:
            for siv in (False, True):
                assert uaes.eax_siv_plan(siv, 16, n)[2] == shape[0], (n, siv)
        if n in pinned:
            assert shape == pinned[n], n
