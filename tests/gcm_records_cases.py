"""The cases of tests/test_gpu_gcm_records.py, made without a device: the launcher's arrangement rule restated
(launch_records and k_gcm_records, csrc/uaes_gcm_records.hip), and the record lengths and counts that put a record at
every place where that rule, the tree's row skipping or the turn loop changes behaviour.

A record of n bytes with a bytes of AAD has nv = ceil(a / 16) + ceil(n / 16) + 1 GHASH positions (AAD blocks, text blocks,
the length block).  A workgroup of 1024 threads is G = 16, 4 or 1 groups of S = 64, 256 or 1024 threads, a record per group,
chosen by the LONGEST record of the call: S = 64 while nv + 1 <= 128, S = 256 while nv + 1 <= 512, else S = 1024 (the + 1 is
the position that carries Enc(J0)); a thread carries two positions when nv + 1 > S.  tests/test_gcm_records_cases.py proves
that the lists below reach what they are meant to reach and stay small enough for the reference."""
import random

THREADS = 1024
MAXNV = 2046                                                  # GSM_MAXNV: the positions of the longest record
REF_CAP = 20 << 20                                            # bytes one test may hand to the compiled reference (~7 MB/s)

# nv_max + 1 of the variable-length batches: both sides of every arrangement change, and the maximum
TARGETS = (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047)
UPPER_TARGETS = (64, 128, 256, 512, 1024, 2047)               # the upper limit of each of the six arrangements
ARRANGEMENTS = ((64, 1), (64, 2), (256, 1), (256, 2), (1024, 1), (1024, 2))
# (aad_len, per record?) of the batches: none; 13 bytes each (stride 13: every second AAD at an odd address); 33 bytes
# shared (three blocks, the last partial)
AAD_FORMS = {"none": (0, False), "13-each": (13, True), "33-shared": (33, False)}


def blocks(n):
    return (n + 15) // 16


def positions(aad_len, n):
    """nv: the GHASH positions of a record of n bytes"""
    return blocks(aad_len) + blocks(n) + 1


def arrangement(aad_len, max_len):
    """(S, steps): threads per record and positions per thread for a call whose longest record is max_len bytes"""
    nv = positions(aad_len, max_len)
    if nv > MAXNV:
        raise ValueError("%d positions: the record call takes %d" % (nv, MAXNV))
    S = 64 if nv + 1 <= 128 else 256 if nv + 1 <= 512 else 1024
    return S, 2 if nv + 1 > S else 1


def groups(S):
    """G: records per workgroup and turn"""
    return THREADS // S


def record_max(aad_len):
    """uaes_gcm_record_max restated"""
    ablk = blocks(aad_len)
    return 0 if ablk + 2 > MAXNV else (MAXNV - 1 - ablk) * 16


def max_len_for(target, aad_len):
    """the longest record (whole blocks) whose nv + 1 is `target` with this much AAD"""
    return 16 * (target - 2 - blocks(aad_len))


def block_counts_for(aad_len, max_len):
    """the text block counts of one variable-length batch: every count whose nv is at most 130, beyond that every count whose
    nv is within 1 of a multiple of 16, and the two smallest and the two largest"""
    ablk, cmax = blocks(aad_len), blocks(max_len)
    cs = {c for c in range(cmax + 1) if ablk + c + 1 <= 130 or (ablk + c + 1) % 16 in (15, 0, 1)}
    cs |= {c for c in (0, 1, cmax - 1, cmax) if c >= 0}
    return sorted(cs)


def lengths_for(aad_len, max_len, rng):
    """the record lengths of one variable-length batch: each block count of block_counts_for once with whole blocks and
    once with a last block of 15 bytes or of 1 byte (rng decides), shuffled so that the groups of a turn hold unlike
    lengths; the first and the last record are exactly max_len bytes"""
    lens = []
    for c in block_counts_for(aad_len, max_len):
        lens.append(min(16 * c, max_len))
        if c >= 1:
            lens.append(min(16 * c - rng.choice((1, 15)), max_len))
    rng.shuffle(lens)
    lens.remove(max_len)
    return [max_len] + lens + [max_len]


def reference_bytes(lens, aad_len):
    """what the reference reads for records of these lengths"""
    return sum(lens) + aad_len * len(lens)


def fixed_block_counts(aad_len):
    """the text block counts of the equal-length batches: nv + 1 over 2 .. 6, over each arrangement limit minus 1, exactly
    and plus 1, and the longest record"""
    ablk = blocks(aad_len)
    want = set(range(2, 7))
    for b in (64, 128, 256, 512, 1024):
        want |= {b - 1, b, b + 1}
    cs = {t - 2 - ablk for t in want if t - 2 - ablk >= 0}
    cs.add(record_max(aad_len) // 16)
    return sorted(cs)


def fixed_lengths(aad_len):
    """[(rec_len, nrec)]: whole blocks, a last block of 15 bytes and one of 1 byte for each count of fixed_block_counts;
    G + 1 records, so that the last turn has one record and G - 1 groups without one"""
    out = []
    for c in fixed_block_counts(aad_len):
        for n in sorted({16 * c, max(16 * c - 1, 0), max(16 * c - 15, 0)}):
            out.append((n, groups(arrangement(aad_len, n)[0]) + 1))
    return out


def turn_forms():
    """[(S, steps, rec_len)] of the batches with more turns than workgroups: the shortest record of each arrangement (no
    AAD) -- for G = 16 the shortest that has a text, one byte; the two-position form for G = 4 and G = 1 as well"""
    out = []
    for S, steps in ((64, 1), (256, 1), (256, 2), (1024, 1), (1024, 2)):
        n = next(n for n in range(1, record_max(0) + 1, 16) if arrangement(0, n) == (S, steps))
        out.append((S, steps, n))
    return out


def turn_counts(cus, G):
    """one pass of the grid less a record, exactly, a second pass of one record, and a second pass whose last turn is one
    group short"""
    return [cus * G - 1, cus * G, cus * G + 1, 2 * cus * G + G - 1]


def turn_lengths(rec_len, nrec, seed):
    """the lengths of the variable-length form of such a batch: 0, rec_len and a seeded random length in turn"""
    rng = random.Random(seed)
    return [(0, rec_len, rng.randrange(1, rec_len + 1))[r % 3] for r in range(nrec)]
