/*
 * uaes_kw.hip -- AES key wrap, RFC 3394 / SP 800-38F KW.
 *
 *   k_kw        <- AES_KEY_wrap :1829-1855, AES_KEY_unwrap :1865-1894: one secret, one wave
 *   k_kw_batch  many secrets of one length under one key-encryption key, sixteen lanes per record
 *
 * The wrap of n semiblocks (8 bytes each) is ONE chain of 6 n block operations:
 *     B = AES(A | R_i);  A = MSB64(B) ^ t;  R_i = LSB64(B)         t = 1 .. 6 n, i walking 1 .. n round and round
 * and the unwrap runs it backwards with the inverse cipher, t = 6 n .. 1.  What counts is the latency of one block, so
 * the sixteen lanes of a DPP row share it (row_encrypt / row_decrypt, uaes_aes.hip.h).  The state is a column word per
 * lane: columns 0 and 1 are A, which never leaves the registers; columns 2 and 3 are R_i, which the lanes of those
 * columns fetch and put back.  t is a 64-bit big-endian number ending at byte 7 of A (xorBEint, MIDST): the lanes of
 * column 0 XOR its high word, those of column 1 its low word.
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
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

#define KW_IV      0xA6A6A6A6u
#define KW_CH      16u                                    /* kw.global: steps a load runs ahead of its use */
#define KW_R_AT    UAES_LDS_ROW                           /* kw.lds: LDS byte address of R (+ 8 bytes nobody reads) */
#define KW_LDS     (UAES_LDS_ROW + (unsigned)UAES_KW_LDS_MAX + 8u)
#define KW_SLOT    ((unsigned)UAES_KW_BATCH_MAX + 8u)     /* kw.batch: LDS bytes per record */
#define KW_BATCH_AT UAES_LDS_ROW4
#define KW_BATCH_LDS (UAES_LDS_ROW4 + (UAES_WG / 16u) * KW_SLOT)

static_assert(UAES_KW_LDS_MAX / 8 >= 2 * KW_CH, "kw.global loads two chunks ahead of the oldest store it may meet");
static_assert(KW_LDS <= 160u * 1024u && KW_BATCH_LDS <= 160u * 1024u, "LDS of one CU");
static_assert(UAES_KW_BATCH_MAX >= 64 && UAES_KW_BATCH_MAX % 8 == 0, "a batch record holds at least 64 bytes");

template <bool A4>
__device__ __forceinline__ u32 kw_ld(const unsigned char *p)
{
    if (A4) return *(const u32 *)p;
    return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24);
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

/* is A the initial value?  (one secret per wave: every row holds the same A) */
__device__ __forceinline__ bool kw_forged_wave(u32 a)
{
    return (u32)__builtin_amdgcn_readlane((int)a, 0) != KW_IV || (u32)__builtin_amdgcn_readlane((int)a, 4) != KW_IV;
}

/* in: the secret (wrap) / A || R (unwrap); out: A || R / the secret; n = semiblocks of the secret.  in and out are
 * disjoint or the in-place form (the secret at wrapped + 8); unwrap writes *status = 0 / 0x1A and leaves what the
 * chain made in `out` either way, like the reference.  A4: both pointers 4-byte aligned. */
template <int NR, bool DEC, bool GLOBAL, bool A4>
__global__ __launch_bounds__(64) void k_kw(uaesk_rk rk, uaesk_tables tb, const unsigned char *in, unsigned char *out,
                                           u64 n, int *status)
{
    if (DEC) row_fill_tables_dec(tb.td0, rk); else row_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row_lane<NR>();
    const u32 half = 4u * (L.c & 1u);
    const unsigned char *rin = DEC ? in + 8 : in;
    unsigned char *rout = DEC ? out : out + 8;
    u32 a = DEC ? kw_ld<A4>(in + half) : KW_IV;
    if (!GLOBAL) {
        const u32 nw = 2u * (u32)n;
        for (u32 j = threadIdx.x; j < nw; j += 64u) kw_lds_st(KW_R_AT + 4u * j, kw_ld<A4>(rin + 4u * j));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          /* one wave: its LDS operations complete in order */
        a = kw_chain_lds<NR, DEC>(a, KW_R_AT, (u32)n, L);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (u32 j = threadIdx.x; j < nw; j += 64u) kw_st<A4>(rout + 4u * j, lds_word(KW_R_AT + 4u * j));
    } else {
        const u64 steps = 6 * n;
        u64 kp = 0, ip = 0;                                         /* the step the next load is for, and kp mod n */
        auto fetch = [&]() {
            const u64 e = DEC ? n - 1 - ip : ip;
            const u32 v = kw_ld<A4>((kp < n ? rin : rout) + 8 * e + half);
            ++kp;
            if (++ip == n) ip = 0;                                  /* past the last step: a semiblock nobody uses */
            return v;
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
    }
    if (!DEC) {
        if (threadIdx.x < 8u && (threadIdx.x & 3u) == 0) kw_st<A4>(out + half, a);     /* lanes 0 and 4: A */
    } else {
        const bool forged = kw_forged_wave(a);
        if (threadIdx.x == 0) *status = forged ? 0x1A : 0;
    }
}

/* nkeys records of n semiblocks each, back to back: the secret of record m at m * 8 n, its wrapped form at
 * m * (8 n + 8).  Unwrap: verdicts[m] = 1 (authentic) / 0, *bad |= 1 for a forgery, and a forged record's output is
 * what the chain made of it, or zeros when wipe != 0.  A4: both arrays 4-byte aligned. */
template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_kw_batch(uaesk_rk rk, uaesk_tables tb, u64 nkeys, u32 n,
                                                      const unsigned char *in, unsigned char *out,
                                                      unsigned char *verdicts, int *bad, int wipe)
{
    if (DEC) row4_fill_tables_dec(tb.td0, rk); else row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>();
    const u32 row = threadIdx.x >> 4, li = threadIdx.x & 15u, half = 4u * (L.c & 1u), nw = 2u * n;
    const u32 slot = KW_BATCH_AT + row * KW_SLOT;
    const u64 rows = blockDim.x >> 4, sb = 8ull * n, wb = sb + 8;
    for (u64 m = (u64)blockIdx.x * rows + row; m < nkeys; m += (u64)gridDim.x * rows) {
        const unsigned char *src = in + m * (DEC ? wb : sb);
        unsigned char *dst = out + m * (DEC ? sb : wb);
        const unsigned char *rin = DEC ? src + 8 : src;
        unsigned char *rout = DEC ? dst : dst + 8;
        u32 a = DEC ? kw_ld<A4>(src + half) : KW_IV;
        for (u32 j = li; j < nw; j += 16u) kw_lds_st(slot + 4u * j, kw_ld<A4>(rin + 4u * j));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          /* the record's sixteen lanes are one wave's */
        a = kw_chain_lds<NR, DEC>(a, slot, n, L);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        bool zero = false;
        if (DEC) {
            const bool forged = row_any(L.c < 2u && a != KW_IV);
            row_verdict(li == 0, verdicts, m, !forged, bad);
            zero = forged && wipe;
        } else if (li < 8u && (li & 3u) == 0) {
            kw_st<A4>(dst + half, a);
        }
        for (u32 j = li; j < nw; j += 16u) kw_st<A4>(rout + 4u * j, zero ? 0u : lds_word(slot + 4u * j));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          /* read out before the next record is staged */
    }
}

/* ---- the plan (uaes_plan.h) ---------------------------------------------------------------------------------------- */
static int plan_kw(int dir, size_t len, size_t nkeys, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((dir != 0 && dir != 1) || len % 8 || len < 16) return (int)hipErrorInvalidValue;
    p->launches = 1;
    if (nkeys == 0) {                                     /* one wave: sixteen lanes per block, four rows redundantly */
        p->arrangement = len <= UAES_KW_LDS_MAX ? UAES_KW_LDS : UAES_KW_GLOBAL;
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

extern "C" int uaesk_plan_kw(int dir, size_t len, size_t nkeys, uaes_plan *p)
{
    return plan_kw(dir, len, nkeys, p);
}

extern "C" const char *uaesk_kw_arrangement_name(int id)
{
    static const char *const names[] = { "kw.lds", "kw.global", "kw.batch" };
    return id >= 0 && id < 3 ? names[id] : "?";
}

/* ---- launchers ------------------------------------------------------------------------------------------------------ */
template <int NR>
static int launch_kw(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k, bool dec, const void *in, size_t len,
                     void *out, int *status)
{
    uaes_plan p;
    const int e = plan_kw(dec, len, 0, &p);
    if (e) return e;
    return with_bool(dec, [&](auto DEC) {
        return with_bool(p.arrangement == UAES_KW_GLOBAL, [&](auto G) {
            return with_bool(uaesk_rows_a4(in, out, len), [&](auto A4) {
                return uaesk_launch(k_kw<NR, decltype(DEC)::value, decltype(G)::value, decltype(A4)::value>, p.grid, p.steps,
                                    KW_LDS, st, *k, *tb, in, out, len / 8, status); }); }); });
}

template <int NR>
static int launch_kw_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k, bool dec, int wipe, size_t nkeys,
                           size_t len, const void *in, void *out, void *verdicts, int *bad)
{
    uaes_plan p;
    const int e = plan_kw(dec, len, nkeys, &p);
    if (e) return e;
    return with_bool(dec, [&](auto DEC) {
        return with_bool(uaesk_rows_a4(in, out, len), [&](auto A4) {
            return uaesk_launch(k_kw_batch<NR, decltype(DEC)::value, decltype(A4)::value>, p.grid, p.steps, KW_BATCH_LDS, st,
                                *k, *tb, nkeys, len / 8, in, out, verdicts, bad, wipe); }); });
}

extern "C" int uaesk_kw(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk, int unwrap,
                        const void *in, size_t secret_len, void *out, int *status)
{
    DISPATCH_NR(nr, return (launch_kw<NR>(S(stream), tb, unwrap ? dk : ek, unwrap != 0, in, secret_len, out, status)));
    return 0;
}

extern "C" int uaesk_kw_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk,
                              int unwrap, int wipe, size_t nkeys, size_t secret_bytes, const void *in, void *out,
                              void *verdicts, int *bad)
{
    if (nkeys == 0) return 0;
    DISPATCH_NR(nr, return (launch_kw_batch<NR>(S(stream), tb, unwrap ? dk : ek, unwrap != 0, wipe, nkeys, secret_bytes,
                                                in, out, verdicts, bad)));
    return 0;
}
