/*
 * uaes_ctr.hip.h -- the counter-mode core shared by the CTR kernel (uaes_kernels.hip)
 * and the fused GCM encrypt kernel (uaes_gcm.hip).
 *
 *   ctr_words        <- the counter block of stream block i (incBlock, micro_aes.c:421-427)
 *   ctr_edges        <- blocks outside the whole chunks + the byte tail (mixThenXor, :949)
 *   ctr_shared_loop  <- CTR_cipher (:943-949) with rounds 1-2 shared between the 256
 *                       counters of a group
 */
#ifndef UAES_CTR_HIP_H_
#define UAES_CTR_HIP_H_

#include "uaes_aes.hip.h"

/* counter block for stream block i: bytes 0..8 fixed, bytes 9..15 = 56-bit
 * big-endian (v0 + i) mod 2^56 (reference N2)                               */
__device__ __forceinline__ void ctr_words(const uaesk_ctr &c, u64 i, u32 (&w)[4])
{
    if (c.le32) {                              /* GCM-SIV: LE32 counter in bytes 0..3 (wave-uniform branch) */
        w[0] = c.w0 + (u32)i;
        w[1] = c.w1; w[2] = c.w2; w[3] = c.w3;
        return;
    }
    const u64 v = (c.v0 + i) & 0x00FFFFFFFFFFFFFFull;
    w[0] = c.w0;
    w[1] = c.w1;
    w[2] = bswap32((c.b8 << 24) | (u32)(v >> 32));
    w[3] = bswap32((u32)v);
}

/* one block through the plain NR-round path: out[i] = in[i] ^ Enc(counter i); returns the ciphertext */
template <int NR, typename LC>
__device__ __forceinline__ uint4 ctr_one_block(const uaesk_rk &rk, const uaesk_ctr &ctr, const uint4 *in, uint4 *out,
                                               u64 i, const LC &lc)
{
    u32 s1[1][4];
    ctr_words(ctr, i, s1[0]);
    enc_blocks<NR, 1>(s1, rk, lc);
    const uint4 d = in[i];
    const uint4 c = make_uint4(d.x ^ s1[0][0], d.y ^ s1[0][1], d.z ^ s1[0][2], d.w ^ s1[0][3]);
    out[i] = c;
    return c;
}

/* reference N3: len%16 tail bytes use Enc(ctr_final) (mixThenXor, :949); one thread */
template <int NR, typename LC>
__device__ __forceinline__ void ctr_byte_tail(const uaesk_rk &rk, const uaesk_ctr &ctr, const uint4 *in, uint4 *out,
                                              u64 nfull, u32 rem, const LC &lc)
{
    u32 s1[1][4];
    ctr_words(ctr, nfull, s1[0]);
    enc_blocks<NR, 1>(s1, rk, lc);
    const unsigned char *src = (const unsigned char *)(in + nfull);
    unsigned char *dst = (unsigned char *)(out + nfull);
    for (u32 i = 0; i < rem; ++i)
        dst[i] = src[i] ^ (unsigned char)(s1[0][i >> 2] >> (8 * (i & 3)));
}

/* Blocks [0, pre_end) and [suf, nfull) and the byte tail, spread evenly over all
 * workgroups, one block per thread through the plain 10/12/14-round path, so no
 * separate launch (and no second table fill) is needed.                         */
template <int NR, typename LC>
__device__ __forceinline__ void ctr_edge_blocks(const uaesk_rk &rk, const uaesk_ctr &ctr, const uint4 *in, uint4 *out,
                                                u64 pre_end, u64 suf, u64 nfull, u32 rem, const LC &lc)
{
    const u64 nedge = pre_end + (nfull - suf);
    const u64 per = (nedge + gridDim.x - 1) / gridDim.x;
    const u64 lo = (u64)blockIdx.x * per;
    u64 hi = lo + per;
    if (hi > nedge) hi = nedge;
    for (u64 e = lo + threadIdx.x; e < hi; e += UAES_WG)
        (void)ctr_one_block<NR>(rk, ctr, in, out, e < pre_end ? e : suf + (e - pre_end), lc);
    if (rem && blockIdx.x == 0 && threadIdx.x == 0) ctr_byte_tail<NR>(rk, ctr, in, out, nfull, rem, lc);
}

#define CTRS_CHUNK 64u                       /* groups (of 256 counters) per U-buffer refill: one barrier each;
                                                256 measured no faster (profiles/HISTORY.md) */

/* ------------------------------------------------------------------------ */
/* CTR with shared rounds 1-2                                                 */
/* ------------------------------------------------------------------------ */
/* Consecutive counter blocks differ only in their low bytes.  Cut the stream
 * into GROUPS of 256 counters that share bytes 0..14 (group G, position p =
 * counter byte 15), and pin every lane to one p for the whole kernel:
 *
 *   after AddRoundKey(0) only state byte 15 depends on p; after round 1 only
 *   column 0 does:  col0 = A(G) ^ Te3[p ^ rk0.b15],  col1..3 = uniform(G);
 *   after round 2 every column is  Te_k[one byte of col0] ^ U_c(G).
 *
 * A(G) changes only when counter bits 40..47 change, so the four round-2
 * lookups on col0's bytes are per-LANE constants L_c, computed once; the
 * uniform parts U_c(G) cost 27 lookups per GROUP (one lane of wave 0 per group,
 * handed over through LDS).  A block therefore enters round 3 as L ^ U(G):
 * 4 XORs instead of 32 table lookups -- 128 lookups per AES-128 block instead
 * of 160 on a path whose bound is the LDS lookup rate (32 lanes/clk/CU).
 *
 * Workgroup = 16 waves = 4 quads.  One ITERATION of the workgroup covers one STRIPE of 2048 consecutive
 * blocks (32 KiB): quad q takes the two 256-block runs q and q+4 of it, two blocks per lane, half a round
 * out of phase (enc_rounds_skewed), so each wave-level load/store is one contiguous 1 KiB segment.  The
 * stripes are dealt round-robin: iteration `it` of workgroup b takes stripe b + grid*it, so every workgroup
 * gets floor or ceil of stripes/grid stripes.  Two ways to pin the lanes to the stripes (FOLD::aligned):
 *
 *   pinned to the STREAM (the CTR kernel).  Stripe s is blocks [2048 s, 2048 s + 2048) of the text, whatever
 *   the first counter is: lane r = 64*(w&3) + lane of quad q holds block 2048 s + 256 (q + 4u) + r, so a wave's
 *   1 KiB is aligned as the text is (a 12-byte IV starts the counter at 1 or 2: runs cut at the counter's
 *   groups would put every wave access 16 or 32 bytes off its 128-byte lines).  With c0 = byte 15 of the
 *   first counter the lane's position is p = (c0 + r) & 255 and its group is 8 s + q + 4u + carry,
 *   carry = (c0 + r) >> 8, counted from the first counter's own group: a stripe meets NINE groups, the
 *   U-buffer holds nine entries per iteration, and the carry is part of the lane's constant U-buffer address.
 *
 *   pinned to the COUNTER (the fused GCM kernel).  Stripe s is the eight groups g_lo + 8 s ..; lane p = r
 *   holds block 256 (g_lo + 8 s + q + 4u) - c0 + p.  Block (b, it, q, u, p) then sits at  j + S*it  with
 *   the lane index j = 2048 b + 256 (q + 4u) + p and S = 2048 grid: exactly the strided Horner layout of
 *   GHASH, so a lane can fold its own ciphertext blocks as it produces them.
 *
 * U-buffer: the uniform parts of the next 8 iterations (64 or 72 groups), double buffered,
 * one s_barrier per 8 iterations.                                                */
/* A(G) is the same for every group of ONE LAUNCH: it depends on the counter's bits 40..47 only, and the launchers cut
 * a text at the (one in 2^40 blocks) place where those move -- ctr_blocks_cross_a() below, launch_ctr and the
 * GCM launchers -- so the lane constants L are made once per kernel and are loop invariants.  (Until round 5 the loop
 * watched A per block and redefined L under a wave-uniform condition: a loop-carried value with a conditional
 * definition, which cost eight v_mov per trip and a second copy of the flags in the U-buffer.)                   */
/* do counter bits 40..47 differ between the first and the last of the blocks [b_lo, b_hi) of the stream? */
static inline bool ctr_blocks_cross_a(const uaesk_ctr *c, u64 b_lo, u64 b_hi)
{
    if (b_hi <= b_lo) return false;
    const u64 first = c->v0 + b_lo, last = c->v0 + b_hi - 1;                               /* (a wrap at 2^56 counts) */
    return (first >> 40) != (last >> 40);
}
/* the same for n8 stripes of eight groups from group g_lo on (counter pinning) */
static inline bool ctr_stripes_cross_a(const uaesk_ctr *c, u64 g_lo, u64 n8)
{
    if (!n8) return false;
    const u64 vbase = c->v0 - (c->v0 & 0xffu);
    const u64 first = vbase + (g_lo << 8), last = vbase + ((g_lo + 8 * n8) << 8) - 1;     /* (a wrap at 2^56 counts) */
    return (first >> 40) != (last >> 40);
}

struct CtrGeo {
    u64 first;          /* g_lo: first group of the striped region (counter pinning; 0 with stream pinning) */
    u64 iters;          /* iterations (stripes) of THIS workgroup                     */
};

__device__ __forceinline__ u64 ctr_geo_group0(const CtrGeo &g, u64 it)
{
    return g.first + 8ull * ((u64)blockIdx.x + (u64)gridDim.x * it);
}

/* FOLD: functor called once per iteration with two blocks of this lane (u = 0, 1), in stream
 * order per lane; `void operator()(uint4 b0, uint4 b1)`.  FOLD::of_input selects which side of the
 * XOR it sees: the blocks just written (encrypting GCM hashes its output) or the blocks just
 * read (decrypting GCM hashes its input).                                            */
struct CtrNoFold {
    static constexpr bool of_input = false;
    static constexpr int round_prio = 1;       /* wave priority while a round's lookups are issued */
    static constexpr bool expand2 = true;      /* the loop body twice per trip, text buffers swapped (no register moves) */
    static constexpr bool text_ahead = true;   /* the text of iteration it + 1 is requested before the rounds of iteration it */
    static constexpr bool aligned = true;      /* lanes pinned to the stream: stripes start at block 0 of the text */
    static constexpr bool write_through = true; /* the ciphertext leaves L2 as it is stored (sc1): nothing dirty at the kernel's end */
    __device__ __forceinline__ void operator()(const uint4 &, const uint4 &) const {}
};

#define CTRS_SLOTS(aligned) ((aligned) ? CTRS_CHUNK + CTRS_CHUNK / 8u : CTRS_CHUNK)    /* U-buffer entries per refill */

/* first block of the stripe of iteration `it` of this workgroup */
template <typename FOLD>
__device__ __forceinline__ u64 ctr_geo_block0(const uaesk_ctr &ctr, const CtrGeo &g, u64 it)
{
    return (ctr_geo_group0(g, it) << 8) - (FOLD::aligned ? 0u : (u32)ctr.v0 & 0xffu);
}

/* The text of this lane's first iteration (FOLD::text_ahead): a kernel asks for it before it makes its tables and
 * hands it to ctr_shared_loop. */
template <typename FOLD>
__device__ __forceinline__ void ctr_first_text(const uaesk_ctr &ctr, const uint4 *in, const CtrGeo &geo, uint4 (&d)[2])
{
    d[0] = d[1] = make_uint4(0, 0, 0, 0);
    if (FOLD::text_ahead && geo.iters) {
#pragma unroll
        for (int u = 0; u < 2; ++u) d[u] = (in + ctr_geo_block0<FOLD>(ctr, geo, 0) + 1024u * u)[threadIdx.x];
    }
}

/* lds_buf: byte offset of 2 x CTRS_SLOTS x 32 B of LDS for the U-buffer; d0: ctr_first_text() */
template <int NR, typename LC, typename FOLD>
__device__ __forceinline__ void ctr_shared_loop(const uaesk_rk &rk, const uaesk_ctr &ctr, const uint4 *in, uint4 *out,
                                                const CtrGeo &geo, u32 lds_buf, const LC &lc, FOLD &fold,
                                                const uint4 (&d0)[2])
{
    constexpr bool aligned = FOLD::aligned;
    constexpr u32 slots = CTRS_SLOTS(aligned), per_it = slots / 8u;
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u32 r = ((wave & 3u) << 6) | lane;               /* the lane's place in a run of 256 blocks */
    const u32 quad = wave >> 2;
    const u32 c0 = (u32)ctr.v0 & 0xffu;                    /* position of stream block 0   */
    const u32 p = aligned ? (c0 + r) & 0xffu : r;          /* counter byte 15 of this lane */
    const u32 carry = aligned ? (c0 + r) >> 8 : 0u;        /* 1: the lane's blocks belong to the next group */
    const u64 vbase = ctr.v0 - c0;                         /* group-aligned counter        */
    uint4 *buf = (uint4 *)(uaes_lds + lds_buf);
    const u32 lane_blk = (quad << 8) | r;                  /* lane's block offset inside the stripe (= threadIdx.x) */
    /* the lane's U-buffer entry of an iteration's first block: a constant LDS address, the carry in it */
    const u32 lane_u = lds_buf + (quad + carry) * 32u;

    /* byte 15 after AddRoundKey(0), as a Te3 lookup operand in byte 3 */
    const u32 x15 = ((p << 24) ^ rk.w[3]) & 0xff000000u;
    /* round keys 3..NR (wave-uniform: they stay in SGPRs; forcing them into VGPRs to
     * speed up v_bitop3 issue measured 3 % SLOWER -- more VGPRs, lower clock)        */
    struct { u32 w[4 * (NR - 2)]; } rkv;
#pragma unroll
    for (int i = 0; i < 4 * (NR - 2); ++i) rkv.w[i] = rk.w[12 + i];
    u32 L0 = 0, L1 = 0, L2 = 0, L3 = 0;
    u32 parity = 0;

    /* Block index of (it, u, lane) = block0(it) + 1024 u [uniform] + lane_blk [per lane].
     * The plaintext of iteration it+1 is requested before the rounds of iteration it, so
     * HBM latency hides under ~260 table lookups.                                       */
    u64 it = 0;

    /* One iteration = two blocks per lane.  The body is written once and expanded twice per trip with the two text
     * buffers swapped, so that "next becomes current" is a renaming, not eight register moves; the text addresses are a
     * wave-uniform 64-bit base (SGPRs, advanced by scalar instructions) plus the lane's constant 32-bit offset, so no
     * 64-bit vector adds either: the VALU is the second-busiest unit of this kernel.          */
    const u32 lane_byte = lane_blk * 16u;
    /* the text of a stripe through a buffer resource whose base is the stripe (four SGPRs, rebuilt by scalar
     * instructions every iteration) + the lane's constant byte offset + 16 KiB for the second block of the lane */
    typedef u32 u32x4 __attribute__((ext_vector_type(4)));
#define UNIFORM_PTR(p) (((u64)(u32)__builtin_amdgcn_readfirstlane((int)((u64)(p) >> 32)) << 32) | \
                        (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(u64)(p)))
#define STRIPE_RSRC(p) __builtin_amdgcn_make_buffer_rsrc((void *)UNIFORM_PTR(p), 0, 0x7fffffff, 0x00020000)
#define TL(k, b, w) tlook_true<k, b>(w, lc)
    if (geo.iters) {                                        /* the lane constants: A of the launch, then L0..L3 */
        const u64 v = (vbase + (ctr_geo_group0(geo, 0) << 8)) & 0x00FFFFFFFFFFFFFFull;
        const u32 s0 = ctr.w0 ^ rk.w[0], s1 = ctr.w1 ^ rk.w[1];
        const u32 s2 = bswap32((ctr.b8 << 24) | (u32)(v >> 32)) ^ rk.w[2];
        const u32 A = xor3(TL(0, 0, s0), TL(1, 1, s1), TL(2, 2, s2)) ^ rk.w[4];
        const u32 col0 = A ^ TL(3, 3, x15);
        L0 = TL(0, 0, col0);
        L1 = TL(3, 3, col0);
        L2 = TL(2, 2, col0);
        L3 = TL(1, 1, col0);
    }
    /* uniform part of rounds 1 and 2 of group g (counted from vbase) into entry `slot` of the buffer being filled */
    auto u_entry = [&](u64 g, u32 slot) {
        const u64 v = (vbase + (g << 8)) & 0x00FFFFFFFFFFFFFFull;
        const u32 s0 = ctr.w0 ^ rk.w[0], s1 = ctr.w1 ^ rk.w[1];
        const u32 s2 = bswap32((ctr.b8 << 24) | (u32)(v >> 32)) ^ rk.w[2];
        const u32 s3 = (bswap32((u32)v) ^ rk.w[3]) & 0x00ffffffu;      /* byte 15 excluded */
        const u32 c1 = xor3(xor3(TL(0, 0, s1), TL(1, 1, s2), TL(2, 2, s3)), TL(3, 3, s0), rk.w[5]);
        const u32 c2 = xor3(xor3(TL(0, 0, s2), TL(1, 1, s3), TL(2, 2, s0)), TL(3, 3, s1), rk.w[6]);
        const u32 c3 = xor3(xor3(TL(0, 0, s3), TL(1, 1, s0), TL(2, 2, s1)), TL(3, 3, s2), rk.w[7]);
        const u32 u0 = xor3(TL(1, 1, c1), TL(2, 2, c2), TL(3, 3, c3)) ^ rk.w[8];
        const u32 u1 = xor3(TL(0, 0, c1), TL(1, 1, c2), TL(2, 2, c3)) ^ rk.w[9];
        const u32 u2 = xor3(TL(0, 0, c2), TL(1, 1, c3), TL(3, 3, c1)) ^ rk.w[10];
        const u32 u3 = xor3(TL(0, 0, c3), TL(2, 2, c1), TL(3, 3, c2)) ^ rk.w[11];
        buf[(parity * slots + slot) * 2 + 0] = make_uint4(u0, u1, u2, u3);
    };
    auto refill = [&](u64 it) {
        /* the groups of iterations it .. it+7: lane gi of wave 0 handles group group0(it + gi/8) + gi%8; with stream
         * pinning and c0 != 0 a stripe reaches into a ninth group, group0 + 8: lanes 0..7 of wave 1, one iteration each */
        if (wave == 0) u_entry(ctr_geo_group0(geo, it + (lane >> 3)) + (lane & 7u), per_it * (lane >> 3) + (lane & 7u));
        if (aligned && c0 != 0 && wave == 1 && lane < 8u) u_entry(ctr_geo_group0(geo, it + lane) + 8u, per_it * lane + 8u);
        __syncthreads();
    };
    auto body = [&](u64 it, uint4 (&d_cur)[2], uint4 (&d_nxt)[2]) {
        /* request the next iteration's plaintext (clamped to this workgroup's last one) -- or, for a fold that cannot
         * afford a second text buffer (FOLD::text_ahead == false), THIS iteration's: the text is not needed before the
         * rounds are done, and one iteration (~4.7 us per 2048 blocks of a workgroup) hides the load either way */
        const u64 b0 = ctr_geo_block0<FOLD>(ctr, geo, it);
        {
            const u64 bn = FOLD::text_ahead ? ctr_geo_block0<FOLD>(ctr, geo, it + 1 < geo.iters ? it + 1 : it) : b0;
            uint4 (&d_ld)[2] = FOLD::text_ahead ? d_nxt : d_cur;
            const __amdgpu_buffer_rsrc_t rin = STRIPE_RSRC(in + bn);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rin, lane_byte, 16384 * u, 0);
                d_ld[u] = make_uint4(v.x, v.y, v.z, v.w);
            }
        }

        u32 s[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            uint4 uu;
            if constexpr (aligned) {                                           /* slot 9 (it & 7) + quad + 4u + carry */
                uu = *(const uint4 *)(uaes_lds + lane_u + (parity * slots + per_it * ((u32)it & 7u) + 4u * u) * 32u);
            } else {
                const u32 gl = 8u * ((u32)it & 7u) + quad + 4u * u;            /* slot in the U-buffer */
                uu = buf[(parity * slots + gl) * 2 + 0];
            }
            s[u][0] = L0 ^ uu.x; s[u][1] = L1 ^ uu.y; s[u][2] = L2 ^ uu.z; s[u][3] = L3 ^ uu.w;
        }
        enc_rounds_skewed<NR, 3, decltype(rkv), false, LC, FOLD::round_prio>(s[0], s[1], rkv, lc);
        uint4 ct[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            ct[u] = make_uint4(d_cur[u].x ^ s[u][0], d_cur[u].y ^ s[u][1], d_cur[u].z ^ s[u][2], d_cur[u].w ^ s[u][3]);
            /* the ciphertext goes out through a plain global pointer, NOT through a buffer resource like the loads:
             * `buffer_store_dwordx4 v[a:a+3], voff, s[rsrc], s_off offen` followed at once by a VALU write to v[a..a+3]
             * stores garbage for some lanes on gfx950 (seen in the one-pass GCM decrypt, whose GHASH selects reuse the
             * registers of the second store: ~1 % of the blocks came out as the selects' zeros, different ones every run,
             * profiles/r04_buffer_store_hazard.log).  The ISA manuals list that hazard -- store data of more than 64 bits,
             * then a VALU write of the data registers: 1 wait state -- with the exception "not if SOFFSET is an SGPR",
             * and the compiler's hazard recogniser follows them; for global_store it always inserts the wait state.   */
            if constexpr (FOLD::write_through) {
                /* sc1: the line is written through to memory and does not stay dirty in the XCD's L2, which a kernel
                 * that streams would otherwise leave full of ciphertext for the next kernel's start to wait out.  Whole
                 * 128-byte lines only (aligned pinning).  The hazard recogniser does not see into the statement, so the
                 * wait state above is spelled out. */
                const u64 ob = UNIFORM_PTR(out + b0 + 1024u * u);
                const u32x4 cv = { ct[u].x, ct[u].y, ct[u].z, ct[u].w };
                asm volatile("global_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 0" :: "v"(lane_byte), "v"(cv), "s"(ob) : "memory");
            } else {
                (out + b0 + 1024u * u)[lane_blk] = ct[u];
            }
        }
        if (FOLD::of_input) fold(d_cur[0], d_cur[1]); else fold(ct[0], ct[1]);
    };
    uint4 d_a[2], d_b[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) d_a[u] = d0[u];
    constexpr bool twice = FOLD::expand2;
    /* chunk by chunk (8 iterations = one fill of the U-buffer): refill, then the chunk's iterations */
    while (it < geo.iters) {
        const u64 end = it + 8 < geo.iters ? it + 8 : geo.iters;
        refill(it);
        if constexpr (twice) {
            for (; it + 2 <= end; it += 2) {
                body(it, d_a, d_b);
                body(it + 1, d_b, d_a);
            }
            if (it < end) { body(it, d_a, d_b); ++it; }      /* an odd count: only the launch's last stripe */
        } else {                                            /* a fold too big to hold twice (GCM: it would spill) */
            for (; it < end; ++it) {
                body(it, d_a, d_b);
                if (FOLD::text_ahead) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) d_a[u] = d_b[u];
                }
            }
        }
        parity ^= 1u;
    }
#undef TL
#undef STRIPE_RSRC
#undef UNIFORM_PTR
}

template <int NR, typename LC, typename FOLD>
__device__ __forceinline__ void ctr_shared_loop(const uaesk_rk &rk, const uaesk_ctr &ctr, const uint4 *in, uint4 *out,
                                                const CtrGeo &geo, u32 lds_buf, const LC &lc, FOLD &fold)
{
    uint4 d0[2];
    ctr_first_text<FOLD>(ctr, in, geo, d0);
    ctr_shared_loop<NR>(rk, ctr, in, out, geo, lds_buf, lc, fold, d0);
}

#endif
