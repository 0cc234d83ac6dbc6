/*
 * uaes_kw.hip -- AES key wrap, RFC 3394 / SP 800-38F KW, and key wrap with padding, RFC 5649 / SP 800-38F KWP.
 *
 *   k_kw        one secret, one wave: KW <- AES_KEY_wrap :1829-1855, AES_KEY_unwrap :1865-1894; KWP (the reference has none)
 *   k_kw_batch  many secrets under one key-encryption key, sixteen lanes per record
 * Both modes are instances of both kernels; the template argument PAD says which.
 *
 * The wrap of n semiblocks (8 bytes each) is ONE chain of 6 n block operations:
 *     B = AES(A | R_i);  A = MSB64(B) ^ t;  R_i = LSB64(B)         t = 1 .. 6 n, i walking 1 .. n round and round
 * and the unwrap runs it backwards with the inverse cipher, t = 6 n .. 1.  What counts is the latency of one block, so
 * the sixteen lanes of a DPP row share it (row_encrypt / row_decrypt, uaes_aes.hip.h).  The state is a column word per
 * lane: columns 0 and 1 are A, which never leaves the registers; columns 2 and 3 are R_i, which the lanes of those
 * columns fetch and put back.  t is a 64-bit big-endian number ending at byte 7 of A (xorBEint, MIDST): the lanes of
 * column 0 XOR its high word, those of column 1 its low word.  KW: the secret is whole semiblocks, n >= 2, A starts as
 * A6 A6 .. A6 and the unwrap accepts when it ends as that.
 *
 * Where R lives (the plan, uaes_plan.h):
 *   kw.lds     secrets up to UAES_KW_LDS_MAX: in LDS behind the row tables.  R_(i+1) was stored at least one step ago
 *              (n >= 2), so its ds_read is issued before the step's cipher starts and is off the chain.
 *   kw.global  longer secrets: in place in the output buffer.  R_i is stored and not touched again for n - 1 steps, so
 *              the loads run a chunk of KW_CH steps ahead of the chain (the reasoning of row_walk): a load is issued
 *              after the store it must see -- the same wave, program order, at least n - 2 KW_CH steps earlier -- and
 *              first used KW_CH steps later.  The first n steps read the input, the others the output, so the caller's
 *              input is never written unless it is the output (the in-place form secret == wrapped + 8).
 *   kw.batch   the four DPP rows of a wave walk four records (row4 tables); a record's semiblocks sit in a slot of
 *              LDS behind the tables; the slot stride is 8 bytes more than a multiple of 128, meant to put the rows of a
 *              wave on different banks (a design intention: no conflict counter has been read; it decides speed only).
 * Every loop is bounded by the lengths passed in; no workgroup waits for another.
 *
 * What padding adds (PAD; kwp.lds, kwp.global and kwp.batch are the arrangements above by the padded length): a secret
 * of any length m = 1 .. 2^32 - 1 bytes is zero-filled to n = ceil(m / 8) semiblocks and A starts as A6 59 59 A6 || m
 * (big-endian, the MLI).  n = 1 is ONE block AES(A | R_1), no chain (kwp.block).  Unwrap accepts when MSB32(A) is the
 * constant, 8 (n - 1) < MLI <= 8 n and the 8 n - MLI bytes behind the secret are zero: all three are computed and ORed,
 * no branch, and the outcome is the MLI or 0 (an authentic MLI is at least 1).  Only the wrap's input is ever short: it
 * is zero-filled on its way into LDS (kwp.lds, kwp.batch) or handed to the first pass of kw_chain_global as a register
 * (kwp.global); everything written is whole semiblocks.  In a batch the records of a wave have lengths of their own
 * (lens), so the four rows leave the chain loop at different trips and some take the one-block path: the row primitives
 * read within their row only (DPP row rotates, quad permutes, the row's LDS slot), and the verdict takes A from the row's
 * own lanes (a bpermute within the row, whose lanes are active together).
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

#define KW_IV      0xA6A6A6A6u
#define KWP_IV     0xA65959A6u                            /* A6 59 59 A6: the same word in either byte order */
#define KW_CH      16u                                    /* kw.global: steps a load runs ahead of its use */
#define KW_R_AT    UAES_LDS_ROW                           /* kw.lds: LDS byte address of R (+ 8 bytes nobody reads) */
#define KW_LDS     (UAES_LDS_ROW + (unsigned)UAES_KW_LDS_MAX + 8u)
#define KW_SLOT    ((unsigned)UAES_KW_BATCH_MAX + 8u)     /* kw.batch: LDS bytes per record */
#define KW_BATCH_AT UAES_LDS_ROW4
#define KW_BATCH_LDS (UAES_LDS_ROW4 + (UAES_WG / 16u) * KW_SLOT)

static_assert(UAES_KW_LDS_MAX / 8 >= 2 * KW_CH, "kw.global loads two chunks ahead of the oldest store it may meet");
static_assert(KW_LDS <= 160u * 1024u && KW_BATCH_LDS <= 160u * 1024u, "LDS of one CU");
static_assert(UAES_KW_BATCH_MAX >= 64 && UAES_KW_BATCH_MAX % 8 == 0, "a batch record holds at least 64 bytes");
static_assert(KW_SLOT / 64u == 4u && UAES_KW_BATCH_MAX <= 256, "k_kw_batch stages a padded record as four words a lane; the slot is 256 + 8 bytes");

template <bool A4>
__device__ __forceinline__ u32 kw_ld(const unsigned char *p)
{
    if (A4) return *(const u32 *)p;
    return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24);
}

/* the word at p of which only the first `avail` bytes (may be <= 0) exist: zeros behind them, and they are not read */
template <bool A4>
__device__ __forceinline__ u32 kwp_ld(const unsigned char *p, long long avail)
{
    if (avail >= 4) return kw_ld<A4>(p);
    u32 v = 0;
#pragma unroll
    for (u32 k = 0; k < 3; ++k)
        if ((long long)k < avail) v |= (u32)p[k] << (8u * k);
    return v;
}

template <bool A4>
__device__ __forceinline__ void kw_st(unsigned char *p, u32 w)
{
    if (A4) { *(u32 *)p = w; return; }
    p[0] = (unsigned char)w; p[1] = (unsigned char)(w >> 8); p[2] = (unsigned char)(w >> 16); p[3] = (unsigned char)(w >> 24);
}

/* R is read through lds_word's absolute addresses; it is written the same way, so that the compiler sees one kind of
 * pointer and keeps a step's store in front of the later step's load of the same semiblock */
__device__ __forceinline__ void kw_lds_st(u32 byte_addr, u32 v)
{
    *(__attribute__((address_space(3))) u32 *)(uintptr_t)byte_addr = v;
}

/* this lane's word of the step counter inside A (masks instead of selects on the column: the chain loop stays
 * straight-line code) */
__device__ __forceinline__ u32 kw_tword(u64 t, u32 c)
{
    const u32 m0 = c == 0 ? ~0u : 0u, m1 = c == 1 ? ~0u : 0u;
    return (bswap32((u32)(t >> 32)) & m0) | (bswap32((u32)t) & m1);
}

/* one step: a = this lane's word of A (lanes of columns 0, 1), r = its word of R_i (columns 2, 3); returns the word of
 * the cipher's output, which is the new R_i in columns 2, 3; a is updated */
template <int NR, bool DEC>
__device__ __forceinline__ u32 kw_step(u32 &a, u32 r, u64 t, const RowLane<NR> &L)
{
    const u32 tw = kw_tword(t, L.c);
    if (!DEC) {
        const u32 e = row_encrypt<NR>(L.c < 2u ? a : r, L);
        a = e ^ tw;
        return e;
    }
    const u32 e = row_decrypt<NR>(L.c < 2u ? a ^ tw : r, L);
    a = e;
    return e;
}

/* the whole chain over the n semiblocks at LDS byte address `base` (word j at base + 4 j; the 8 bytes behind them take
 * the stores of the lanes that hold A, so that the loop has no branch); returns the final A word */
template <int NR, bool DEC>
__device__ __forceinline__ u32 kw_chain_lds(u32 a, u32 base, u32 n, const RowLane<NR> &L)
{
    const u32 half = 4u * (L.c & 1u);
    const u32 sink = base + 8u * n + half;
    const u64 steps = 6ull * n;
    u32 i = DEC ? n - 1u : 0u;
    u32 r = lds_word(base + 8u * i + half);
    for (u64 k = 0; k < steps; ++k) {
        const u32 nx = DEC ? (i ? i - 1u : n - 1u) : (i + 1u == n ? 0u : i + 1u);
        const u32 rn = lds_word(base + 8u * nx + half);             /* stored at least one step ago: off the chain */
        const u32 e = kw_step<NR, DEC>(a, r, DEC ? steps - k : k + 1, L);
        kw_lds_st(L.c < 2u ? sink : base + 8u * i + half, e);
        i = nx;
        r = rn;
    }
    return a;
}

/* n = 1 (padding only): the semiblock at LDS `base` and A through one block of the cipher, stored as kw_chain_lds stores
 * a step */
template <int NR, bool DEC>
__device__ __forceinline__ u32 kwp_block(u32 a, u32 base, const RowLane<NR> &L)
{
    const u32 half = 4u * (L.c & 1u);
    const u32 x = L.c < 2u ? a : lds_word(base + half);
    const u32 e = DEC ? row_decrypt<NR>(x, L) : row_encrypt<NR>(x, L);
    kw_lds_st(L.c < 2u ? base + 8u + half : base + half, e);
    return e;
}

/* the whole chain in place in global memory (kw.global, above): the first n steps read rin, the others rout, the loads a
 * chunk of KW_CH steps ahead; n >= 2 KW_CH; returns the final A word.  SHORT (the wrap of a padded secret): semiblock
 * n - 1 of rin may be short; this lane's word of it, zero-filled, comes in `lastw`, and rin is not read there */
template <int NR, bool DEC, bool A4, bool SHORT>
__device__ __forceinline__ u32 kw_chain_global(u32 a, const unsigned char *rin, unsigned char *rout, u64 n,
                                               const RowLane<NR> &L, u32 lastw)
{
    const u32 half = 4u * (L.c & 1u);
    const u64 steps = 6 * n;
    u64 kp = 0, ip = 0;                                         /* the step the next load is for, and kp mod n */
    auto fetch = [&]() {
        const u64 e = DEC ? n - 1 - ip : ip;
        const bool part = SHORT && kp == n - 1;                 /* the short semiblock: a whole one is loaded instead */
        const u32 v = kw_ld<A4>((kp < n ? rin : rout) + 8 * (part ? e - 1 : e) + half);
        ++kp;
        if (++ip == n) ip = 0;                                  /* past the last step: a semiblock nobody uses */
        return part ? lastw : v;
    };
    u64 i = DEC ? n - 1 : 0;
    auto step = [&](u64 k, u32 r) {
        const u32 e = kw_step<NR, DEC>(a, r, DEC ? steps - k : k + 1, L);
        if (L.c >= 2u) kw_st<A4>(rout + 8 * i + half, e);
        i = DEC ? (i ? i - 1 : n - 1) : (i + 1 == n ? 0 : i + 1);
    };
    u32 cur[KW_CH], nxt[KW_CH];
#pragma unroll
    for (u32 j = 0; j < KW_CH; ++j) cur[j] = fetch();
    for (u64 k0 = 0; k0 < steps; k0 += KW_CH) {
        /* steps k0 + KW_CH .. k0 + 2 KW_CH - 1: their semiblocks were last stored n steps earlier, before step k0
         * (n >= 2 KW_CH), by this wave: the loads follow those stores in program order */
#pragma unroll
        for (u32 j = 0; j < KW_CH; ++j) nxt[j] = fetch();
        if (k0 + KW_CH <= steps) {
#pragma unroll
            for (u32 j = 0; j < KW_CH; ++j) step(k0 + j, cur[j]);
        } else {
#pragma unroll
            for (u32 j = 0; j < KW_CH; ++j)
                if (k0 + j < steps) step(k0 + j, cur[j]);
        }
#pragma unroll
        for (u32 j = 0; j < KW_CH; ++j) cur[j] = nxt[j];
    }
    return a;
}

/* this lane's word of the initial A of a wrap (padded: of m bytes) */
template <bool PAD>
__device__ __forceinline__ u32 kw_a0(u32 m, u32 c)
{
    return !PAD ? KW_IV : c == 1u ? bswap32(m) : KWP_IV;
}

/* is A the initial value of a wrap without padding?  (one secret per wave: every row holds the same A) */
__device__ __forceinline__ bool kw_forged_wave(u32 a)
{
    return (u32)__builtin_amdgcn_readlane((int)a, 0) != KW_IV || (u32)__builtin_amdgcn_readlane((int)a, 4) != KW_IV;
}

/* padding's verdict.  a0, a1: the words of A after the unwrap; w0, w1: those of the last semiblock R_n.  The MLI, or 0
 * for a forgery */
__device__ __forceinline__ u32 kwp_verdict(u32 a0, u32 a1, u64 n, u32 w0, u32 w1)
{
    const u64 mli = bswap32(a1), top = 8 * n;
    const u32 pad = (u32)(top - mli) & 7u;                              /* meaningful when the MLI is in range */
    const u64 last = (u64)w0 | ((u64)w1 << 32), behind = ~(~0ull >> (8u * pad));   /* the last `pad` bytes of R_n */
    const u32 bad = (a0 ^ KWP_IV) | (u32)(mli + 8 <= top) | (u32)(mli > top) | (u32)((last & behind) != 0);
    return bad ? 0u : (u32)mli;
}

/* One secret, one wave; ARR = enum uaes_kw_arrangement.  len = semiblocks of the secret, or PAD: its bytes (wrap) / the
 * bytes of the wrapped form - 8 (unwrap).  wrap: in = the secret, out = the 8 n + 8 bytes of A || R; unwrap: in = A || R,
 * out = the 8 n bytes the chain makes (the secret and, padded, its zero fill), left there whatever the verdict, like the
 * reference; status[0] = 0 / 0x1A and, PAD, status[1] = the MLI / 0.  in and out are disjoint or the in-place form (the
 * secret at wrapped + 8); what sits in LDS is read whole before anything is written.  A4: both pointers 4-byte aligned. */
template <int NR, bool DEC, int ARR, bool A4, bool PAD>
__global__ __launch_bounds__(64) void k_kw(uaesk_rk rk, uaesk_tables tb, const unsigned char *in, unsigned char *out,
                                           u64 len, int *status)
{
    if (DEC) row_fill_tables_dec(tb.td0, rk); else row_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row_lane<NR>();
    const u32 half = 4u * (L.c & 1u);
    const u64 n = PAD ? (len + 7) / 8 : len;
    const unsigned char *rin = DEC ? in + 8 : in;
    unsigned char *rout = DEC ? out : out + 8;
    u32 a = DEC ? kw_ld<A4>(in + half) : kw_a0<PAD>((u32)len, L.c);
    u32 w0 = 0u, w1 = 0u;
    if (ARR != UAES_KW_GLOBAL) {
        const u32 nw = 2u * (u32)n;
        for (u32 j = threadIdx.x; j < nw; j += 64u)
            kw_lds_st(KW_R_AT + 4u * j, PAD && !DEC ? kwp_ld<A4>(rin + 4u * j, (long long)len - 4ll * j) : kw_ld<A4>(rin + 4u * j));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          /* one wave: its LDS operations complete in order */
        a = ARR == UAES_KW_BLOCK ? kwp_block<NR, DEC>(a, KW_R_AT, L) : kw_chain_lds<NR, DEC>(a, KW_R_AT, (u32)n, L);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (u32 j = threadIdx.x; j < nw; j += 64u) kw_st<A4>(rout + 4u * j, lds_word(KW_R_AT + 4u * j));
        if (PAD && DEC) {
            w0 = lds_word(KW_R_AT + 4u * nw - 8u);
            w1 = lds_word(KW_R_AT + 4u * nw - 4u);
        }
    } else {
        const u64 at = 8 * (n - 1) + half;
        a = kw_chain_global<NR, DEC, A4, PAD && !DEC>(a, rin, rout, n, L,
                                                      PAD && !DEC ? kwp_ld<A4>(rin + at, (long long)(len - at)) : 0u);
        if (PAD && DEC) {                                 /* R_n as this wave stored it, 5 n steps ago or later */
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            w0 = kw_ld<A4>(rout + 8 * (n - 1));
            w1 = kw_ld<A4>(rout + 8 * (n - 1) + 4);
        }
    }
    if (!DEC) {
        if (threadIdx.x < 8u && (threadIdx.x & 3u) == 0) kw_st<A4>(out + half, a);     /* lanes 0 and 4: A */
    } else if (!PAD) {
        const bool forged = kw_forged_wave(a);
        if (threadIdx.x == 0) *status = forged ? 0x1A : 0;
    } else {
        const u32 mli = kwp_verdict((u32)__builtin_amdgcn_readlane((int)a, 0), (u32)__builtin_amdgcn_readlane((int)a, 4),
                                    n, w0, w1);
        if (threadIdx.x == 0) { status[0] = mli ? 0 : 0x1A; status[1] = (int)mli; }
    }
}

/* nkeys records in slots, back to back.  !PAD: rec = semiblocks of every secret; the secret of record m at m * 8 rec, its
 * wrapped form at m * (8 rec + 8); lens and lens_out are not read.  PAD: rec = bytes of a secret's slot (unwrap: the
 * wrapped slot - 8, a multiple of 8).  wrap: secret m at m * rec, `lens[m]` (NULL: rec) of its bytes count, its wrapped
 * form goes to m * (8 ceil(rec / 8) + 8) and is 8 ceil(lens[m] / 8) + 8 bytes; a length of 0 or above rec writes nothing
 * and sets bit 1 of *bad.  unwrap: wrapped record m at m * (rec + 8), lens[m] (NULL: rec + 8) bytes of it count, the 8 n it
 * unwraps to go to m * rec, lens_out[m] = the MLI / 0; a length that is no multiple of 8, below 16 or above rec + 8 fails
 * unwritten.  Either: unwrap writes verdicts[m] = 1 (authentic) / 0 and bit 0 of *bad for a record that fails, and a forged
 * record's output is what the chain made of it, or zeros when wipe != 0.  A4: both arrays and both slot sizes are 4-byte
 * aligned. */
template <int NR, bool DEC, bool A4, bool PAD>
__global__ __launch_bounds__(UAES_WG) void k_kw_batch(uaesk_rk rk, uaesk_tables tb, u64 nkeys, u32 rec, const u32 *lens,
                                                      const unsigned char *in, unsigned char *out, u32 *lens_out,
                                                      unsigned char *verdicts, int *bad, int wipe)
{
    if (DEC) row4_fill_tables_dec(tb.td0, rk); else row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>();
    const u32 row = threadIdx.x >> 4, li = threadIdx.x & 15u, half = 4u * (L.c & 1u);
    const u32 slot = KW_BATCH_AT + row * KW_SLOT;
    const u64 rows = blockDim.x >> 4, sb = PAD ? (u64)rec : 8ull * rec, wb = PAD ? 8ull * ((rec + 7u) / 8u) + 8 : sb + 8;
    for (u64 m = (u64)blockIdx.x * rows + row; m < nkeys; m += (u64)gridDim.x * rows) {
        const unsigned char *src = in + m * (DEC ? wb : sb);
        unsigned char *dst = out + m * (DEC ? sb : wb);
        const u32 given = !PAD ? rec : lens ? lens[m] : DEC ? rec + 8u : rec;
        const bool valid = !PAD || (DEC ? (given & 7u) == 0 && given >= 16u && given <= rec + 8u : given - 1u < rec);
        if (!valid) {
            if (DEC) {
                row_verdict(li == 0, verdicts, m, false, bad);
                if (li == 0) lens_out[m] = 0u;
            } else if (li == 0) {
                atomicOr(bad, 2);
            }
            continue;
        }
        const u32 len = DEC ? given - 8u : given, n = PAD ? (len + 7u) / 8u : rec, nw = 2u * n;
        const unsigned char *rin = DEC ? src + 8 : src;
        unsigned char *rout = DEC ? dst : dst + 8;
        u32 a = DEC ? kw_ld<A4>(src + half) : kw_a0<PAD>(len, L.c);
        if (DEC || !PAD) {
            for (u32 j = li; j < nw; j += 16u) kw_lds_st(slot + 4u * j, kw_ld<A4>(rin + 4u * j));
        } else {
            /* a lane's up to four words (KW_SLOT: 64 words a record) are requested together, clamped to the last whole
             * word instead of branched around -- a load behind a branch is waited for where it is issued, and the
             * record would pay four memory latencies -- and the one short word is fetched bytewise */
            const u32 full = len >> 2, rem = len & 3u;
            u32 v[KW_SLOT / 64u] = { 0u, 0u, 0u, 0u }, part = 0u;
            if (full) {
#pragma unroll
                for (u32 q = 0; q < KW_SLOT / 64u; ++q) v[q] = kw_ld<A4>(rin + 4u * min(li + 16u * q, full - 1u));
            }
            if (rem) part = kwp_ld<A4>(rin + 4u * full, rem);
#pragma unroll
            for (u32 q = 0; q < KW_SLOT / 64u; ++q) {
                const u32 j = li + 16u * q;
                if (j < nw) kw_lds_st(slot + 4u * j, j < full ? v[q] : j == full ? part : 0u);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          /* the record's sixteen lanes are one wave's */
        if (PAD && n == 1u) a = kwp_block<NR, DEC>(a, slot, L);
        else a = kw_chain_lds<NR, DEC>(a, slot, n, L);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bool zero = false;
        if (DEC && !PAD) {
            const bool forged = row_any(L.c < 2u && a != KW_IV);
            row_verdict(li == 0, verdicts, m, !forged, bad);
            zero = forged && wipe;
        } else if (DEC) {
            const int lane0 = (int)(threadIdx.x & 48u);             /* this row's first lane within the wave */
            const u32 mli = kwp_verdict((u32)__shfl((int)a, lane0), (u32)__shfl((int)a, lane0 + 4), n,
                                        lds_word(slot + 4u * nw - 8u), lds_word(slot + 4u * nw - 4u));
            row_verdict(li == 0, verdicts, m, mli != 0u, bad);
            if (li == 0) lens_out[m] = mli;
            zero = !mli && wipe;
        } else if (li < 8u && (li & 3u) == 0) {
            kw_st<A4>(dst + half, a);
        }
        for (u32 j = li; j < nw; j += 16u) kw_st<A4>(rout + 4u * j, zero ? 0u : lds_word(slot + 4u * j));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          /* read out before the next record is staged */
    }
}

/* ---- the plan (uaes_plan.h) ---------------------------------------------------------------------------------------- */
static int plan_kw(bool pad, int dir, size_t len, size_t nkeys, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if (dir != 0 && dir != 1) return (int)hipErrorInvalidValue;
    if (pad ? len == 0 || (dir ? len % 8 != 0 || len > UAES_KWP_MAX + 1 : len > UAES_KWP_MAX) : len % 8 || len < 16)
        return (int)hipErrorInvalidValue;
    p->launches = 1;
    if (nkeys == 0) {                                     /* one wave: sixteen lanes per block, four rows redundantly */
        p->arrangement = len <= 8 ? UAES_KW_BLOCK : (len + 7) / 8 * 8 <= UAES_KW_LDS_MAX ? UAES_KW_LDS : UAES_KW_GLOBAL;
        p->grid = 1;
        p->steps = 64;
        return 0;
    }
    if (len > UAES_KW_BATCH_MAX) return (int)hipErrorInvalidValue;
    const RowShape s = uaesk_row_shape(nkeys);
    p->arrangement = UAES_KW_BATCH;
    p->grid = s.grid;
    p->steps = s.wg;
    return 0;
}

extern "C" int uaesk_plan_kw(int dir, size_t len, size_t nkeys, uaes_plan *p) { return plan_kw(false, dir, len, nkeys, p); }
extern "C" int uaesk_plan_kwp(int dir, size_t len, size_t nkeys, uaes_plan *p) { return plan_kw(true, dir, len, nkeys, p); }

static const char *kw_name(bool pad, int id)
{
    static const char *const names[2][4] = { { "?", "kw.lds", "kw.global", "kw.batch" },
                                             { "kwp.block", "kwp.lds", "kwp.global", "kwp.batch" } };
    return id >= 0 && id < 4 ? names[pad][id] : "?";
}

extern "C" const char *uaesk_kw_arrangement_name(int id) { return kw_name(false, id); }
extern "C" const char *uaesk_kwp_arrangement_name(int id) { return kw_name(true, id); }

/* ---- launchers ------------------------------------------------------------------------------------------------------ */
template <int NR, bool PAD>
static int launch_kw(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k, bool dec, const void *in, size_t len,
                     void *out, int *status)
{
    uaes_plan p;
    const int e = plan_kw(PAD, dec, len, 0, &p);
    if (e) return e;
    return with_bool(dec, [&](auto DEC) {
        return with_bool(uaesk_rows_a4(in, out, 0), [&](auto A4) {
            constexpr bool D = decltype(DEC)::value, A = decltype(A4)::value;
            /* without padding the plan never says block, and no such instance is made */
            auto *kern = p.arrangement == UAES_KW_GLOBAL ? k_kw<NR, D, UAES_KW_GLOBAL, A, PAD>
                         : p.arrangement == UAES_KW_LDS ? k_kw<NR, D, UAES_KW_LDS, A, PAD>
                                                        : k_kw<NR, D, PAD ? UAES_KW_BLOCK : UAES_KW_LDS, A, PAD>;
            return uaesk_launch(kern, p.grid, p.steps, KW_LDS, st, *k, *tb, in, out, PAD ? len : len / 8, status); }); });
}

template <int NR, bool PAD>
static int launch_kw_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k, bool dec, int wipe, size_t nkeys,
                           size_t rec, const void *lens, const void *in, void *out, void *lens_out, void *verdicts, int *bad)
{
    uaes_plan p;
    const int e = plan_kw(PAD, dec, rec, nkeys, &p);
    if (e) return e;
    return with_bool(dec, [&](auto DEC) {
        return with_bool(uaesk_rows_a4(in, out, dec ? 0 : rec), [&](auto A4) {
            return uaesk_launch(k_kw_batch<NR, decltype(DEC)::value, decltype(A4)::value, PAD>, p.grid, p.steps, KW_BATCH_LDS,
                                st, *k, *tb, nkeys, PAD ? rec : rec / 8, lens, in, out, lens_out, verdicts, bad, wipe); }); });
}

extern "C" int uaesk_kw(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk, int pad,
                        int unwrap, const void *in, size_t len, void *out, int *status)
{
    const uaesk_rk *k = unwrap ? dk : ek;
    DISPATCH_NR(nr, return (pad ? launch_kw<NR, true>(S(stream), tb, k, unwrap != 0, in, len, out, status)
                                : launch_kw<NR, false>(S(stream), tb, k, unwrap != 0, in, len, out, status)));
    return 0;
}

extern "C" int uaesk_kw_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk, int pad,
                              int unwrap, int wipe, size_t nkeys, size_t rec, const void *lens, const void *in, void *out,
                              void *lens_out, void *verdicts, int *bad)
{
    const uaesk_rk *k = unwrap ? dk : ek;
    if (nkeys == 0) return 0;
    DISPATCH_NR(nr, return (pad ? launch_kw_batch<NR, true>(S(stream), tb, k, unwrap != 0, wipe, nkeys, rec, lens, in, out,
                                                            lens_out, verdicts, bad)
                                : launch_kw_batch<NR, false>(S(stream), tb, k, unwrap != 0, wipe, nkeys, rec, NULL, in, out,
                                                             NULL, verdicts, bad)));
    return 0;
}
