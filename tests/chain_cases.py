"""Shared by tests/test_chain_plan.py (no GPU) and tests/test_gpu_chains.py: the boundaries of the CBC / CFB / OFB /
CMAC / CCM / batch rows of csrc/uaes_plan.h, found by walking uaes.chain_plan() (nothing here is a literal size), and
the oracle's block-parallel decryptions cut into pieces so that the CPU's cores share them."""
import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import micro_aes_amd as uaes

MIB = 1 << 20
POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))   # the oracle's ctypes calls release the GIL
PIECE = 1 << 18


def first(pred, lo, hi, unit=16):
    """the smallest lo + k * unit <= hi at which pred holds; pred is false at lo, true at hi and changes once"""
    assert not pred(lo) and pred(hi), (lo, hi)
    while hi - lo > unit:
        m = lo + (hi - lo) // 2 // unit * unit
        if pred(m):
            hi = m
        else:
            lo = m
    return hi


def fbdec_marks(cus=None):
    """The parallel decrypt (k_fb_dec) in bytes of PARALLEL blocks, from the CFB row (n = bytes / 16): b = the largest
    size of fbdec.single; for either arrangement the tile (bytes one workgroup takes per pass) and g = the largest size
    of one pass (every workgroup of the capped grid one full tile: the kernel's grid-stride loop runs beyond it).
    Returns (b, (g1, tile1), (g4, tile4), workgroups of a full grid); cus (the device's) is asserted if given."""
    def plan(n):
        return uaes.chain_plan("cfb", n, decrypt=True)
    top = 1 << 32
    name, launches, full, threads = plan(top)
    assert name == "fbdec.tiled" and launches == 1 and (cus is None or full == cus), (plan(top), cus)
    b = first(lambda n: plan(n)[0] == "fbdec.tiled", 16, top) - 16
    assert plan(b)[0] == "fbdec.single" and plan(b + 16)[0] == "fbdec.tiled"
    marks = []
    for lo, hi in ((16, b), (b + 16, top)):
        assert plan(lo)[2] < full - 1 and plan(hi)[2] == full, (plan(lo), plan(hi))
        f1 = first(lambda n: plan(n)[2] >= full, lo, hi)
        f0 = first(lambda n: plan(n)[2] >= full - 1, lo, hi)
        tile = f1 - f0
        g = f1 - 16 + tile
        assert plan(g)[0] == plan(hi)[0] and plan(g)[2] == full and tile % (16 * threads) == 0, (g, tile, plan(g))
        marks.append((g, tile))
    assert marks[0][1] // (16 * threads) == 1 and marks[1][1] // (16 * threads) == 4       # k_fb_dec<U=1> and <U=4>
    return b, marks[0], marks[1], full


def fbdec_len(mode, tail, p):
    """the text length of `mode` ("cbc": CS3, tail = bytes of the short last block, 0 = whole blocks; "cbc_nocts";
    "cfb": tail = bytes behind the last whole block) that has p bytes of parallel blocks"""
    if mode == "cbc":
        return p + 32 if tail == 0 else p + 16 + tail       # the stolen pair is held back (AES_CBC_decrypt :756-764)
    return p + tail


def ccm_fused_max():
    """the longest text of ccm.fused, from the hook (both directions agree)"""
    top = 1 << 20
    b = first(lambda n: uaes.chain_plan("ccm", n)[0] == "ccm.split", 0, top, 1) - 1
    assert uaes.chain_plan("ccm", b)[:2] == ("ccm.fused", 1) and uaes.chain_plan("ccm", b + 1)[0] == "ccm.split"
    assert uaes.chain_plan("ccm", b, decrypt=True)[0] == "ccm.fused" and uaes.chain_plan("ccm", b + 1, decrypt=True)[0] == "ccm.split"
    return b


def batch_rows(plan):
    """messages one workgroup takes per pass: sixteen lanes per message in the row kernel, one in the lane kernel"""
    return plan[3] // 16 if plan[0] == "batch.row" else plan[3]


@functools.lru_cache(maxsize=None)
def batch_marks(top=1 << 19):
    """Every message count k <= top at which a batch changes: ((k, what changed), ...) with k the first count of the
    new state.  The state is (arrangement, threads per workgroup, strided?); strided = the capped grid no longer holds
    every message in one pass (k > workgroups * messages per workgroup).  Walked for uaes_cbc_encrypt_batch; the
    answer for uaes_cmac_batch is asserted to be the same on both sides of every change."""
    hook, out = uaes.engine().uaes_debug_plan_chain, (C.c_int * 3)()

    def state(what, k):
        name = hook(uaes.CHAIN_WHAT[what], 0, 16, k, out)
        rows = out[2] // 16 if name == b"batch.row" else out[2]
        return name.decode(), out[2], k > out[1] * rows
    marks, k, prev = [], 1, state("cbc_batch", 1)
    assert prev[2] is False
    while state("cbc_batch", top) != prev:                    # (a state that was left does not come back)
        k = first(lambda x: state("cbc_batch", x) != prev, k, top, 1)
        cur = state("cbc_batch", k)
        assert state("cbc_batch", k - 1) == state("cmac_batch", k - 1) == prev and state("cmac_batch", k) == cur, k
        marks.append((k, "%s/%d%s -> %s/%d%s" % (prev[0], prev[1], " strided" if prev[2] else "",
                                                 cur[0], cur[1], " strided" if cur[2] else "")))
        prev = cur
    return tuple(marks)


def batch_samples(nmsg, plan, least=2048):
    """the messages of a large batch that the oracle checks: the first and last 64, the messages around every pass of
    the grid-stride loop (k * workgroups * messages per workgroup - 1, + 0, + 1) and evenly spread ones, at least
    `least` (or all of them)"""
    per_pass = plan[2] * batch_rows(plan)
    s = set(range(min(64, nmsg))) | set(range(max(0, nmsg - 64), nmsg))
    for k in range(1, nmsg // per_pass + 2):
        s.update(i for i in (k * per_pass - 1, k * per_pass, k * per_pass + 1) if 0 <= i < nmsg)
    s.update(range(7 % nmsg, nmsg, max(1, nmsg // least)))
    assert len(s) >= min(least, nmsg)
    return sorted(s)


def oracle_decrypt(orc, mode, key, iv, data):
    """orc.cbc / orc.cbc_nocts / orc.cfb decryption of the whole text, computed piecewise: the decrypting directions
    are block-parallel (CBC: P_i = Dec(C_i) ^ C_{i-1}; CFB: P_i = Enc(C_{i-1}) ^ C_i), so a piece of whole blocks
    decrypted with the ciphertext block in front of it as its IV is that part of the whole text's decryption.  CBC with
    stealing: the pieces in front run without stealing, the last one (at least two blocks) is the CS3 call.
    tests/test_chain_plan.py checks this identity against the one-call oracle."""
    n = len(data)
    if n <= 2 * PIECE:
        return _oracle_piece(orc, mode, key, iv, data, True)
    cuts = list(range(0, n - PIECE, PIECE)) + [n]           # the last piece: PIECE .. 2 * PIECE bytes and any ragged end
    jobs = []
    for lo, hi in zip(cuts, cuts[1:]):
        piv = iv if lo == 0 else data[lo - 16:lo]
        jobs.append(POOL.submit(_oracle_piece, orc, mode, key, piv, data[lo:hi], hi == n))
    return b"".join(j.result() for j in jobs)


def _oracle_piece(orc, mode, key, iv, piece, last):
    """one oracle call on bytes, straight through its C ABI (orc.cbc's own wrapper spends four times the cipher's time
    on its prefilled output buffer, under the interpreter lock)"""
    out = C.create_string_buffer(max(len(piece), 1))
    if mode == "cfb":
        orc.L.orc_cfb(len(key) * 8, key, iv, 0, piece, len(piece), out)
        return out.raw[:len(piece)]
    fn = orc.L.orc_cbc_decrypt if mode == "cbc" and last else orc.L.orc_cbc_decrypt_nocts
    assert ord(fn(len(key) * 8, key, iv, piece, len(piece), out)) == 0
    return out.raw[:len(piece)]
