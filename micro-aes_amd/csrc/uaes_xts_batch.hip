/*
 * uaes_xts_batch.hip -- batches of XTS data units: many short units under one key pair in one launch, a tweak and,
 * optionally, a length per unit (uaes_xts_encrypt_batch, uaes_xts_decrypt_batch, uaes_xts_sector_list).
 *
 * One kernel, k_xts_batch, a row batch (uaes_plan.h): sixteen lanes per unit, four units per wave, the row4 tables of
 * uaes_aes.hip.h, the launch shape of uaesk_row_shape and a grid-stride loop over the units, so any number of units is
 * one launch.  A unit is bit for bit what uaes_xts_encrypt / uaes_xts_decrypt give for it with its tweak
 * (XTS_cipher, micro_aes.c:1008-1053), ciphertext stealing included.  A contiguous run of equal sectors remains the job
 * of uaes_xts_sectors and its kernels (uaes_kernels.hip), which spread one unit's blocks over many lanes.
 */
#include <hip/hip_runtime.h>
#include <type_traits>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

/* LDS: the row4 tables and key 1's round keys (the encryption schedule, or the equivalent-inverse one under the inverse
 * tables), then key 2's encryption schedule, then -- a decrypting launch only -- a plain Te0 for the one forward block a
 * unit needs, T = Enc_key2(tweak): the OCB batch's layout (uaes_ocb.hip) without its L table.
 *   0 .. 128 KiB          row4 tables (Te, or Td and Si)
 *   128 KiB + 0 .. 239    key 1, 4 (NR + 1) words
 *   128 KiB + 256 .. 495  key 2, 4 (NR + 1) words
 *   128 KiB + 512 .. 1535 Te0, 256 words (decrypting) */
#define XTSB_K2      (131072u + 256u)
#define XTSB_TE0     (131072u + 512u)
#define XTSB_LDS_ENC XTSB_TE0
#define XTSB_LDS_DEC (XTSB_TE0 + 1024u)
static_assert(UAES_LDS_ROW4 <= XTSB_K2 && XTSB_K2 + 240u <= XTSB_TE0, "the two schedules and the table do not overlap");
static_assert(XTSB_LDS_DEC <= 160u * 1024u, "one workgroup's LDS");

/* T -> alpha T and T -> alpha^2 T in column words (doubleLblock, micro_aes.c).  T is a little-endian 128-bit number and
 * column word c is its limb c, held by all four lanes of quad c: one DPP row rotation by four lanes brings the limb
 * below, and limb 0 takes limb 3's top bits folded by x^128 = x^7 + x^2 + x + 1 (0x87; two bits: 0x87 and 0x10E). */
__device__ __forceinline__ u32 xtsb_mul_alpha(u32 w, u32 c)
{
    const u32 hi = row_dpp<0x124>(w) >> 31;               /* row_ror:4 = take lane i - 4: the previous column's word */
    return (w << 1) ^ (c ? hi : hi * 0x87u);
}

__device__ __forceinline__ u32 xtsb_mul_alpha2(u32 w, u32 c)
{
    const u32 hi = row_dpp<0x124>(w) >> 30;
    return (w << 2) ^ (c ? hi : ((hi & 1u) * 0x87u) ^ ((hi >> 1) * 0x10eu));
}

/* this lane's column of the tweak block: the n = 16 raw bytes at p, or LE128 of the n = 8 bytes of a sector number (the
 * upper half is zero).  row_load takes an aligned sector number byte by byte; here it is one word load, too */
__device__ __forceinline__ u32 xtsb_load_tweak(const unsigned char *p, u32 n, u32 c)
{
    if (n == 8u && (((uintptr_t)p) & 3u) == 0) return c < 2u ? ((const u32 *)p)[c] : 0u;
    return row_load(p, n, c);
}

/* key 2's lane for T = Enc_key2(tweak): over the row4 tables when they are the forward ones, else over the plain Te0 */
template <int NR, bool DEC>
__device__ __forceinline__ auto xtsb_tweak_lane()
{
    if constexpr (DEC) return row_te0_lane<NR>(XTSB_TE0, XTSB_K2);
    else return row4_lane<NR>(XTSB_K2);
}
template <int NR> __device__ __forceinline__ u32 xtsb_tweak(u32 w, const RowLane<NR> &F) { return row_encrypt<NR>(w, F); }
template <int NR> __device__ __forceinline__ u32 xtsb_tweak(u32 w, const RowTe0<NR> &F) { return row_encrypt_te0<NR>(w, F); }

/* Unit m: text at in / out + m msg_bytes, its first lens[m] <= msg_bytes bytes (lens NULL: all of it); its tweak the
 * tweak_bytes (16, or 8: a sector number, LE128 of which is the tweak) at tweaks + m tweak_bytes, any byte offset.  A
 * length below 16 writes nothing and sets bit 0 of *bad (only a launch with lens can meet one; without lens bad is not
 * touched).  k1 = key 1's encryption schedule, decrypting the equivalent-inverse one; k2 = key 2's encryption schedule.
 * Row steps per unit of b whole blocks and r = 1 for a ragged tail, n = b - r the blocks outside the stealing pair:
 *   1                 T = Enc_key2(tweak)
 *   floor(n / 2)      two blocks per step (row_encrypt2 / row_decrypt2) under T and alpha T; T then moves by alpha^2
 *   n % 2             a last odd block alone
 *   2 r               the stealing pair, one block after the other: encrypting block n under T_n, then the tail with
 *                     the rest of that ciphertext under T_(n+1); decrypting block n under T_(n+1) = alpha T_n, then
 *                     the rebuilt block under T_n
 * so 1 + ceil(b / 2) without a tail.  The tweak arithmetic is column words and one DPP move; a row never reads a lane of
 * another unit.  in == out works: row_walk asks for the text a chunk ahead, a block is in registers before its place is
 * written, and the stealing pair -- block n and the tail -- is read before the unit's first store.  A4: every unit
 * 4-byte aligned in both texts.  The key-2 lane is a second RowLane (encrypting) or a RowTe0 (decrypting) held across
 * the units beside row_walk's full look-ahead: the widest instance takes 122 of the 128 registers a 16-wave workgroup
 * has and none has scratch (profiles/xts_batch_resources.txt); building it per unit saved nothing at the widest. */
template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_xts_batch(uaesk_rk k1, uaesk_rk k2, uaesk_tables tb,
                                                       const unsigned char *tweaks, u32 tweak_bytes, u64 nmsg,
                                                       u64 msg_bytes, const u32 *lens, const unsigned char *in,
                                                       unsigned char *out, int *bad)
{
    for (u32 i = threadIdx.x; i < 60u; i += blockDim.x) ((u32 *)(uaes_lds + XTSB_K2))[i] = k2.w[i];
    if (DEC) {                                        /* row4_fill_tables_dec ends in the barrier these need, too */
        for (u32 i = threadIdx.x; i < 256u; i += blockDim.x) ((u32 *)(uaes_lds + XTSB_TE0))[i] = tb.te0[i];
        row4_fill_tables_dec(tb.td0, k1);
    } else {
        row4_fill_tables(tb.te0, k1);
    }
    const RowLane<NR> L = row4_lane<NR>();
    const u32 c = L.c;
    const auto F = xtsb_tweak_lane<NR, DEC>();
    auto crypt = [&](u32 w) {
        if constexpr (DEC) return row_decrypt<NR>(w, L); else return row_encrypt<NR>(w, L);
    };
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        u64 len = msg_bytes;
        if (lens) { const u64 l = lens[m]; if (l < len) len = l; }
        if (len < 16) {
            if ((threadIdx.x & 15u) == 0) atomicOr(bad, 1);
            continue;
        }
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        const u64 full = len >> 4;
        const u32 rem = (u32)len & 15u;
        const u64 n = rem ? full - 1 : full;              /* the blocks outside the stealing pair */
        /* the stealing pair, before anything is stored */
        const u32 xl = rem ? row_load_full<A4>(src + 16 * n, c) : 0u;
        const u32 l0 = rem ? row_load(src + 16 * full, rem, c) : 0u;
        u32 t = xtsb_tweak<NR>(xtsb_load_tweak(tweaks + m * tweak_bytes, tweak_bytes, c), F);
        u32 px = 0;                                       /* an even block, waiting for its partner */
        row_walk<A4>(src, n, c, [&](u64 i, u32 x) {
            if (!(i & 1u)) {
                px = x;
                if (i + 1 < n) return;
                row_store_full<A4>(dst + 16 * i, crypt(x ^ t) ^ t, c);      /* the last block, alone */
                t = xtsb_mul_alpha(t, c);
                return;
            }
            const u32 t1 = xtsb_mul_alpha(t, c);
            u32 a = px ^ t, b = x ^ t1;
            if (DEC) row_decrypt2<NR>(a, b, L, L); else row_encrypt2<NR>(a, b, L, L);
            row_store_full<A4>(dst + 16 * (i - 1), a ^ t, c);
            row_store_full<A4>(dst + 16 * i, b ^ t1, c);
            t = xtsb_mul_alpha2(t, c);
        });
        if (rem) {                                        /* t = T_n (:1037-1052) */
            const u32 t1 = xtsb_mul_alpha(t, c);
            const u32 ta = DEC ? t1 : t, tb2 = DEC ? t : t1;
            const u32 y = crypt(xl ^ ta) ^ ta;            /* its first rem bytes are the tail's */
            const u32 z = l0 | (y & ~row_keep(rem, c));   /* the tail (zero-filled), filled up with what it steals */
            row_store_full<A4>(dst + 16 * n, crypt(z ^ tb2) ^ tb2, c);
            row_put(dst + 16 * full, y, rem, c);
        }
    }
}

/* ------------------------------------------------------------------------ */
/* plan and launcher                                                          */
/* ------------------------------------------------------------------------ */
/* xts.batch: a row batch at any number of units (uaesk_row_shape) */
extern "C" int uaesk_plan_xts_batch(size_t len, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if (len < 16 || len > 0xffffffffull) return (int)hipErrorInvalidValue;
    uaesk_row_plan(UAES_XTS_BATCH, nmsg, p);
    return 0;
}

extern "C" const char *uaesk_xts_batch_arrangement_name(int id)
{
    return id == UAES_XTS_BATCH ? "xts.batch" : "?";
}

template <int NR>
static int launch_xts_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k1, const uaesk_rk *k2, int decrypt,
                            const void *tweaks, unsigned tweak_bytes, size_t nmsg, size_t msg_bytes, const void *lens,
                            const void *in, void *out, int *bad)
{
    uaes_plan p;
    uaesk_row_plan(UAES_XTS_BATCH, nmsg, &p);
    return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_xts_batch<NR, decltype(DEC)::value, decltype(A4)::value>, p.grid, p.steps,
                            decrypt ? XTSB_LDS_DEC : XTSB_LDS_ENC, st, *k1, *k2, *tb, tweaks, tweak_bytes, nmsg, msg_bytes,
                            lens, in, out, bad); }); });
}

extern "C" int uaesk_xts_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *k1, const uaesk_rk *k2,
                               int decrypt, const void *tweaks, unsigned tweak_bytes, size_t nmsg, size_t msg_bytes,
                               const void *lens, const void *in, void *out, int *bad)
{
    uaes_plan p;
    const int e = uaesk_plan_xts_batch(msg_bytes, nmsg, &p);
    if (e) return e;
    if (tweak_bytes != 8u && tweak_bytes != 16u) return (int)hipErrorInvalidValue;
    if (nmsg == 0) return 0;
    DISPATCH_NR(nr, return (launch_xts_batch<NR>(S(stream), tb, k1, k2, decrypt, tweaks, tweak_bytes, nmsg, msg_bytes, lens,
                                                 in, out, bad)));
    return 0;
}
